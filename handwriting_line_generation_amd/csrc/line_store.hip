// GAN batches from a device-resident line store (data/line_store.py). What AuthorHWDataset.__getitem__ and collate do on the host per line
// read from disk (reference: datasets/author_hw_dataset.py:386-470, utils/augmentation.py:61-72 affine_trans through cv2.warpAffine) - the
// horizontal stretch + shear around the mid-line, 1 - p / 128, padding with -1 to the widest line of the batch, and the same warp of the
// line's foreground mask, padded with 0 - for lines that live in GPU memory as one ragged uint8 pool (the layout of hwg_fg_masks: line k is
// the row-major H x widths[k] picture at pixels + offsets[k], any width >= 1, any byte offset). One launch writes EVERY element of
// out [B,1,H,W] and, with a mask pool, of out_mask [B,1,H,W]; nothing is cleared first.
//
// ARITHMETIC (fp64, no contraction, in exactly this order; tests/_line_store_ref.py restates it in numpy and the kernel's output is compared
// bit for bit). Output row b shows line k = line[b] stretched by strech[b] and sheared by m[b] = tan(skew) (computed on the host), out_w[b]
// columns wide:
//     h  = H / 2.0
//     sx = ((double)x - m * ((double)y - h)) / strech          the reference's matrix [[strech, m, -h m], [0, 1, 0]] inverted in cv2's
//     x0 = floor(sx),  f = sx - x0                              pixel-INDEX convention; y maps to itself: the interpolation is 1-D
//     p0, p1 = the bytes at columns x0, x0 + 1 of row y of the line, or the border value where the column is outside [0, widths[k]):
//              255 for lines, 0 for masks - warpAffine's constant border, blended into the edge pixels
//     v  = p0 + f * (p1 - p0)
//     line: level = clamp(floor(v + 0.5), 0, 255), element = 1 - level / 128 (exact in fp32)
//     mask: p = byte / 255 (the pool holds 0 / 255), element = (float)v
//     columns x >= out_w[b]: -1 in out, 0 in out_mask
// strech = 1, m = 0 gives f = 0 and the line's own bytes.
//
// MAPPING: output-centred, as sheet_compose_kernel. A lane owns 4 consecutive floats of the flat output: it decodes (b, y, x) once (two
// integer divisions), carries across row and image ends without dividing again, and makes one 16-byte store per tensor. W is arbitrary (not
// a multiple of 4): the buffers hold B*H*W rounded up to 4 elements and the surplus of the last word is written as padding. The source
// bytes are gathered with byte loads: the step of sx per column is 1 / strech in [0.71, 1.67], so neighbouring lanes read neighbouring
// bytes of the same row. No atomics, no LDS, no hand-off between workgroups.
//
// The caller validated the tables (ops.store_batch, on the host before the upload); a row whose entry is bad all the same - a line index
// outside [0, n_lines), a line that does not lie inside pixel_bytes, out_w outside [0, W], a strech that is not finite and positive, an m
// that is not finite - becomes padding: nothing is read through it. All stores are inside the rounded-up outputs whatever the tables hold.
#include "hwg_common.h"

constexpr int STORE_BLOCK = 256;

struct StoreRow {
  long long off;       // first byte of the line in the pool(s)
  int w;               // its width
  int ow;              // columns of the output row that show it (0: the whole row is padding)
  double strech, m;
};

__device__ __forceinline__ StoreRow store_row(int b, long long pixel_bytes, const long long* __restrict__ offsets, const int* __restrict__ widths,
                                              int n_lines, const int* __restrict__ line, const int* __restrict__ out_w,
                                              const double* __restrict__ strech, const double* __restrict__ m, int H, int W) {
  StoreRow r;
  r.off = 0; r.w = 1; r.ow = 0; r.strech = 1.0; r.m = 0.0;
  const int k = line[b];
  if (k < 0 || k >= n_lines) return r;
  const int w = widths[k], ow = out_w[b];
  const long long off = offsets[k];
  const double s = strech[b], mm = m[b];
  const bool ok = hwg_line_in_pool(off, w, H, pixel_bytes) && ow >= 0 && ow <= W &&
                  s > 0.0 && fabs(s) < INFINITY && fabs(mm) < INFINITY;      // (comparisons are false for NaN)
  if (!ok) return r;
  r.off = off; r.w = w; r.ow = ow; r.strech = s; r.m = mm;
  return r;
}

// the byte at column xd of the row that starts at `row`, or `border` outside [0, w): xd is an integer-valued double (or +-inf)
__device__ __forceinline__ double store_tap(const unsigned char* __restrict__ row, double xd, int w, double border) {
  if (xd >= 0.0 && xd < (double)w) return (double)row[(int)xd];
  return border;
}

template <bool MASK>
__global__ __launch_bounds__(STORE_BLOCK) void store_batch_kernel(const unsigned char* __restrict__ pixels, const unsigned char* __restrict__ masks,
                                                                   long long pixel_bytes, const long long* __restrict__ offsets,
                                                                   const int* __restrict__ widths, int n_lines, const int* __restrict__ line,
                                                                   const int* __restrict__ out_w, const double* __restrict__ strech,
                                                                   const double* __restrict__ m, int B, int H, int W, long long total,
                                                                   long long words, float* __restrict__ out, float* __restrict__ out_mask) {
#pragma clang fp contract(off)
  const long long word = (long long)blockIdx.x * STORE_BLOCK + threadIdx.x;
  if (word >= words) return;
  const long long first = 4 * word;
  const long long hw = (long long)H * W;
  int b = (int)(first / hw);
  const long long rem = first - (long long)b * hw;
  int y = (int)(rem / W);
  int x = (int)(rem - (long long)y * W);
  const double h = (double)H / 2.0;
  StoreRow r;
  r.off = 0; r.w = 1; r.ow = 0; r.strech = 1.0; r.m = 0.0;
  if (b < B) r = store_row(b, pixel_bytes, offsets, widths, n_lines, line, out_w, strech, m, H, W);
  float vo[4], vm[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float e = -1.0f, em = 0.0f;                        // PADDING_CONSTANT / the mask's padding
    if (first + j < total && x < r.ow) {
      const double t = r.m * ((double)y - h);
      const double num = (double)x - t;
      const double sx = num / r.strech;
      const double x0 = floor(sx);
      const double f = sx - x0;
      const double x1 = x0 + 1.0;
      const long long base = r.off + (long long)y * r.w;
      {
        const double p0 = store_tap(pixels + base, x0, r.w, 255.0), p1 = store_tap(pixels + base, x1, r.w, 255.0);
        const double d = p1 - p0;
        const double fd = f * d;
        const double v = p0 + fd;
        const double q = floor(v + 0.5);
        const float level = (float)fmin(fmax(q, 0.0), 255.0);
        e = 1.0f - level / 128.0f;
      }
      if (MASK) {
        const double p0 = store_tap(masks + base, x0, r.w, 0.0) / 255.0, p1 = store_tap(masks + base, x1, r.w, 0.0) / 255.0;
        const double d = p1 - p0;
        const double fd = f * d;
        const double v = p0 + fd;
        em = (float)v;
      }
    }
    vo[j] = e;
    vm[j] = em;
    if (++x == W) {                                    // carry: next image row, next image (its table entry is read then)
      x = 0;
      if (++y == H) {
        y = 0;
        ++b;
        r.ow = 0;
        if (b < B) r = store_row(b, pixel_bytes, offsets, widths, n_lines, line, out_w, strech, m, H, W);
      }
    }
  }
  const f32x4 o = {vo[0], vo[1], vo[2], vo[3]};
  *(f32x4*)(out + first) = o;
  if (MASK) {
    const f32x4 om = {vm[0], vm[1], vm[2], vm[3]};
    *(f32x4*)(out_mask + first) = om;
  }
}

extern "C" int hwg_store_batch(const unsigned char* pixels, const unsigned char* masks, long long pixel_bytes, const long long* offsets,
                               const int* widths, int n_lines, const int* line, const int* out_w, const double* strech, const double* m, int B,
                               int H, int W, float* out, float* out_mask, long long out_elems, void* stream) {
  HWG_REQUIRE(pixels && offsets && widths && line && out_w && strech && m && out, "store_batch: null argument");
  HWG_REQUIRE((masks == nullptr) == (out_mask == nullptr), "store_batch: masks and out_mask go together, one of them is null");
  HWG_REQUIRE(B > 0 && H > 0 && W > 0, "store_batch: bad sizes B=%d H=%d W=%d", B, H, W);
  HWG_REQUIRE(n_lines > 0 && pixel_bytes > 0, "store_batch: bad sizes n_lines=%d pixel_bytes=%lld", n_lines, pixel_bytes);
  HWG_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)out_mask & 15) == 0, "store_batch: out and out_mask must be 16-byte aligned");
  HWG_REQUIRE(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)strech & 7) == 0 && ((uintptr_t)m & 7) == 0 && ((uintptr_t)widths & 3) == 0 &&
              ((uintptr_t)line & 3) == 0 && ((uintptr_t)out_w & 3) == 0, "store_batch: the tables must be aligned to their element size");
  const long long bh = (long long)B * H;                                 // < 2^62
  HWG_REQUIRE(bh <= (0x7fffffffffffffffll - 3) / W, "store_batch: B*H*W = %d*%d*%d does not fit 64 bits", B, H, W);
  const long long total = bh * W, words = (total + 3) / 4;
  HWG_REQUIRE(out_elems >= 4 * words, "store_batch: out holds %lld elements, B*H*W rounded up to 4 needs %lld", out_elems, 4 * words);
  const long long blocks = (words + STORE_BLOCK - 1) / STORE_BLOCK;
  HWG_REQUIRE(blocks <= 0x7fffffffll, "store_batch: %lld elements are more than one launch covers", total);
  if (masks)
    hipLaunchKernelGGL(store_batch_kernel<true>, dim3((unsigned)blocks), dim3(STORE_BLOCK), 0, (hipStream_t)stream, pixels, masks, pixel_bytes,
                       offsets, widths, n_lines, line, out_w, strech, m, B, H, W, total, words, out, out_mask);
  else
    hipLaunchKernelGGL(store_batch_kernel<false>, dim3((unsigned)blocks), dim3(STORE_BLOCK), 0, (hipStream_t)stream, pixels, masks, pixel_bytes,
                       offsets, widths, n_lines, line, out_w, strech, m, B, H, W, total, words, out, out_mask);
  HWG_LAUNCH_CHECK("store_batch");
  return HWG_OK;
}
