// Recogniser pre-training batches from the device-resident line store (data/line_store.py, `device_store: "warp"`): the brightness + mesh
// warp augmentation of augment.hip executed on the POOL's bytes instead of on an uploaded, collated fp32 batch. What the host path does per
// batch - decode pages, resize, convert to fp32, collate, upload, histogram + Otsu (hwg_augment_stats), warp (hwg_augment_warp) - becomes
//   once, when the pool is built: store_line_stats_kernel, one workgroup per line -> thr [n] (Otsu level) and hist [n][256]: they depend on
//     the stored bytes alone, only the two brightness draws of a batch row change, and with them the LUT and the border level;
//   per batch: store_warp_kernel, one workgroup per row x 64 columns (the mapping of augment_warp_kernel) -> every element of out [B,1,H,W].
//
// ARITHMETIC: none of its own. The Otsu level is augment_stats_kernel's definition (exact integer sums, (s0 w1 - s1 w0)^2 / (w0 w1) with
// the square and the quotient each rounded once in fp64, lowest level on ties; restated here as fg_mask.hip restates it - integers and two
// fp64 roundings leave no freedom). The LUT entry, the border level and the lattice / diagonal / barycentric / bilinear path are the
// functions of augment_warp.h that augment.hip calls too; the only difference is the tap: lut[pool byte] instead of lut[level of a float].
// The border level sum hist[p] * lut[p] is an exact integer reduction (any order gives the same integer), then ONE fp64 division.
//
// Per output row b the tables of ops.LineMesh.tables (lines_i = {w, gy, gx, x_off}, lines_f, draws; see include/hwg.h) plus line[b], the
// pool line it shows. Columns outside [x_off, x_off + w) are -1. The caller validated the tables (ops.store_warp_batch, on the host before
// the upload); a row whose entry is bad all the same - a line index outside [0, n_lines), a line that does not lie inside pixel_bytes, a
// width that is not the pool's, an extent outside [0, W] - becomes padding: nothing is read through it. A lattice that does not fit
// (gy > GY, gx > GX, gy > 16) leaves the LUT alone, as in augment_warp_kernel; the lattice reads stay inside the strides the entry point
// checked whatever the tables hold. Plain vector stores, no atomics, no hand-off between workgroups.
#include "augment_warp.h"

constexpr int SLS_BLOCK = 512;

__global__ __launch_bounds__(SLS_BLOCK) void store_line_stats_kernel(const unsigned char* __restrict__ pixels, long long pixel_bytes,
                                                                     const long long* __restrict__ offsets, const int* __restrict__ widths, int H,
                                                                     int* __restrict__ thr_out, int* __restrict__ hist_out) {
  __shared__ int whist[8][256];          // one histogram per wavefront: only one lane of a wavefront writes at a time, no atomics
  __shared__ int hist[256];
  __shared__ double var[256];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long off = offsets[b];
  const int w = widths[b];
  // a bad table entry (ops.store_line_stats refuses it on the host) reads nothing: threshold -1, empty histogram
  if (!hwg_line_in_pool(off, w, H, pixel_bytes)) {
    if (tid == 0) thr_out[b] = -1;
    if (tid < 256) hist_out[(size_t)b * 256 + tid] = 0;
    return;
  }
  const unsigned char* img = pixels + off;
  for (int i = tid; i < 8 * 256; i += SLS_BLOCK) (&whist[0][0])[i] = 0;
  __syncthreads();
  for (int y = wv; y < H; y += 8) {
    for (int x0 = 0; x0 < w; x0 += 64) {
      const int xl = x0 + lane;
      const bool valid = xl < w;
      const int p = valid ? (int)img[(size_t)y * w + xl] : -1;
      // lines are mostly paper: the lanes that share the first pending lane's level are counted with one ballot and added by that lane
      unsigned long long pending = __ballot(valid);
      while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int lv = __shfl(p, leader, 64);
        const unsigned long long same = __ballot(p == lv) & pending;
        if (lane == leader) whist[wv][lv] += __popcll(same);
        pending &= ~same;
      }
    }
  }
  __syncthreads();
  if (tid < 256) {
    int s = 0;
    for (int k = 0; k < 8; ++k) s += whist[k][tid];
    hist[tid] = s;
    hist_out[(size_t)b * 256 + tid] = s;
  }
  __syncthreads();
  const long long N = (long long)H * w;
  if (tid < 256) {
    long long w0 = 0, s0 = 0, S = 0;
    for (int p = 0; p < 256; ++p) {
      const long long h = hist[p];
      S += h * p;
      if (p <= tid) { w0 += h; s0 += h * p; }
    }
    const long long w1 = N - w0, s1 = S - s0;
    double v = 0.0;
    if (w0 > 0 && w1 > 0) {
      const double d = (double)(s0 * w1 - s1 * w0);
      const double dd = d * d;
      v = dd / (double)(w0 * w1);
    }
    var[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    double best = 0.0;
    for (int p = 0; p < 256; ++p)
      if (var[p] > best) { best = var[p]; t = p; }      // lowest level on ties
    thr_out[b] = t;
  }
}

// the line's pixels as the pool holds them: levels
struct StorePoolTap {
  const unsigned char* img;              // first byte of the line
  int w;
  __device__ __forceinline__ int operator()(int yy, int xx) const { return (int)img[(size_t)yy * w + xx]; }
};

__global__ __launch_bounds__(256) void store_warp_kernel(const unsigned char* __restrict__ pixels, long long pixel_bytes,
                                                         const long long* __restrict__ offsets, const int* __restrict__ widths, int n_lines,
                                                         const int* __restrict__ thr, const int* __restrict__ hist, const int* __restrict__ line,
                                                         const int* __restrict__ lines_i, const float* __restrict__ lines_f, int lf_stride,
                                                         const float* __restrict__ draws, int draw_stride, int H, int W, int GY, int GX,
                                                         float* __restrict__ out, float* __restrict__ map_out) {
  __shared__ AugTileLds s;
  __shared__ long long part[4];
  const int b = blockIdx.y, X0 = blockIdx.x * AUG_TILE, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* yb = out + (size_t)b * H * W;
  float* mb = map_out ? map_out + (size_t)b * 2 * H * W : nullptr;
  const int k = line[b];
  int w = 0, xoff = 0;
  long long off = 0;
  if (k >= 0 && k < n_lines) {
    const int wk = widths[k], xo = lines_i[4 * b + 3];
    const long long o = offsets[k];
    if (lines_i[4 * b] == wk && hwg_line_in_pool(o, wk, H, pixel_bytes) && xo >= 0 && wk <= W && xo <= W - wk) {
      w = wk; xoff = xo; off = o;
    }
  }
  if (max(X0 - xoff, 0) > min(X0 + AUG_TILE - 1 - xoff, w - 1)) {      // padding only (every tile of a bad row: w = 0)
    aug_padding_tile(H, W, X0, yb, mb);
    return;
  }
  const int gy = lines_i[4 * b + 1], gx = lines_i[4 * b + 2];
  const bool warp = gy >= 2 && gx >= 2 && gy <= GY && gx <= GX && gy <= AUG_MAXR && H > 5 && w > 5;
  const float* lf = lines_f + (size_t)b * lf_stride;
  const float* dr = draws + (size_t)b * draw_stride;
  // 1. the row's LUT from the line's stored threshold and the row's two draws; 2. its border level from the stored histogram
  const int q = aug_lut_entry(tid, thr[k], lf, dr);
  s.lut[tid] = (float)q;
  long long v = (long long)hist[(size_t)k * 256 + tid] * q;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) part[wv] = v;
  __syncthreads();
  const float m = (float)aug_border_level((part[0] + part[1]) + (part[2] + part[3]), (long long)H * w);
  // 3. the warp of augment_warp_kernel on the pool's bytes
  const StorePoolTap tap = {pixels + off, w};
  aug_warp_tile(s, tap, m, warp, gy, gx, GY, lf, dr + 2, H, W, w, xoff, X0, yb, mb);
}

extern "C" int hwg_store_line_stats(const unsigned char* pixels, long long pixel_bytes, const long long* offsets, const int* widths, int n_lines,
                                    int H, int* thr, int* hist, void* stream) {
  HWG_REQUIRE(pixels && offsets && widths && thr && hist, "store_line_stats: null argument");
  HWG_REQUIRE(n_lines > 0 && pixel_bytes > 0 && H > 0, "store_line_stats: bad sizes n_lines=%d pixel_bytes=%lld H=%d", n_lines, pixel_bytes, H);
  HWG_REQUIRE(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)widths & 3) == 0 && ((uintptr_t)thr & 3) == 0 && ((uintptr_t)hist & 3) == 0,
              "store_line_stats: the tables must be aligned to their element size");
  hipLaunchKernelGGL(store_line_stats_kernel, dim3((unsigned)n_lines), dim3(SLS_BLOCK), 0, (hipStream_t)stream, pixels, pixel_bytes, offsets,
                     widths, H, thr, hist);
  HWG_LAUNCH_CHECK("store_line_stats");
  return HWG_OK;
}

extern "C" int hwg_store_warp_batch(const unsigned char* pixels, long long pixel_bytes, const long long* offsets, const int* widths, int n_lines,
                                    const int* thr, const int* hist, const int* line, const int* lines_i, const float* lines_f, int lf_stride,
                                    const float* draws, int draw_stride, int B, int H, int W, int GY, int GX, float* out, float* map_out,
                                    long long out_elems, void* stream) {
  HWG_REQUIRE(pixels && offsets && widths && thr && hist && line && lines_i && lines_f && draws && out, "store_warp_batch: null argument");
  HWG_REQUIRE(B > 0 && H > 0 && W > 0, "store_warp_batch: bad sizes B=%d H=%d W=%d", B, H, W);
  HWG_REQUIRE(n_lines > 0 && pixel_bytes > 0, "store_warp_batch: bad sizes n_lines=%d pixel_bytes=%lld", n_lines, pixel_bytes);
  HWG_REQUIRE(B <= 65535, "store_warp_batch: batch of %d rows is too large (at most 65535)", B);
  HWG_REQUIRE(GY >= 0 && GX >= 0 && GY <= AUG_MAXR, "store_warp_batch: %d x %d lattice (at most %d rows: lines up to ~190 px high)", GY, GX, AUG_MAXR);
  HWG_REQUIRE(lf_stride >= 4 + (long long)GY + GX && (long long)draw_stride >= 2 + 2LL * GY * GX,
              "store_warp_batch: table strides too small for a %d x %d lattice", GY, GX);
  HWG_REQUIRE(((uintptr_t)offsets & 7) == 0 && (((uintptr_t)widths | (uintptr_t)thr | (uintptr_t)hist | (uintptr_t)line | (uintptr_t)lines_i |
                                                 (uintptr_t)lines_f | (uintptr_t)draws | (uintptr_t)out | (uintptr_t)map_out) & 3) == 0,
              "store_warp_batch: the tables and the outputs must be aligned to their element size");
  HWG_REQUIRE((long long)B * H <= 0x7fffffffffffffffll / W, "store_warp_batch: B*H*W = %d*%d*%d does not fit 64 bits", B, H, W);
  HWG_REQUIRE(out_elems >= (long long)B * H * W, "store_warp_batch: out holds %lld elements, B*H*W needs %lld", out_elems, (long long)B * H * W);
  hipLaunchKernelGGL(store_warp_kernel, dim3(hwg_cdiv(W, AUG_TILE), B), dim3(256), 0, (hipStream_t)stream, pixels, pixel_bytes, offsets, widths,
                     n_lines, thr, hist, line, lines_i, lines_f, lf_stride, draws, draw_stride, H, W, GY, GX, out, map_out);
  HWG_LAUNCH_CHECK("store_warp_batch");
  return HWG_OK;
}
