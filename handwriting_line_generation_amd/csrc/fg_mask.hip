// Foreground masks of grey text lines, for the foreground-only reconstruction loss (reference: datasets/author_hw_dataset.py:197-220 and
// author_rimeslines_dataset.py, there per line on the host through OpenCV):
//     th, b = cv2.threshold(img, 0, 255, cv2.THRESH_BINARY + cv2.THRESH_OTSU);  b = 255 - b
//     mask  = cv2.dilate(b, cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (9, 9)))
// One launch for a whole ragged pool of lines, one workgroup per line:
//   1. 256-bin histogram of the line in LDS (one histogram per wavefront, no atomics), Otsu threshold t by the definition
//      augment_stats_kernel (augment.hip) fixes - restated here so that that file stays as it is: exact integer sums,
//      var = (s0 w1 - s1 w0)^2 / (w0 w1) with the square and the quotient each rounded once in fp64, lowest level on ties, t = 0 for a
//      constant line;
//   2. the line binarised (foreground = p <= t, which is 255 - THRESH_BINARY) into BIT COLUMNS: one 64-bit word per image column, bit y = row y
//      (H <= 64), a chunk of columns with a 4-column halo at a time in LDS; columns outside the line are 0 (cv2's default morphology border
//      never counts), so no neighbour in the pool leaks in;
//   3. the dilation on the words and byte stores of 255 / 0.
//
// The element. cv2 is on no machine of this project, so the 9 x 9 ellipse is derived from OpenCV's construction rather than pinned to a
// recorded array: getStructuringElement(MORPH_ELLIPSE, (9, 9)) has r = c = 4 and fills, in the row at distance dy from the centre, the
// columns c - dx .. c + dx with dx = saturate_cast<int>(c * sqrt((r*r - dy*dy) / (r*r))) = round(4 * sqrt((16 - dy^2) / 16)):
//     dy = 0: 4    dy = +-1: round(3.873) = 4    dy = +-2: round(3.464) = 3    dy = +-3: round(2.646) = 3    dy = +-4: 0
// i.e. half-widths [0, 3, 3, 4, 4, 4, 3, 3, 0] for dy = -4 .. 4, 57 cells, anchor at the centre, symmetric in both axes. Read by columns: the
// column at distance 0 holds dy = -4 .. 4, those at distance 1, 2, 3 hold dy = -3 .. 3 and those at distance 4 hold dy = -1 .. 1. A dilation
// is an OR over the element's cells, and shifting a bit column up or down distributes over OR, hence
//     out[x] = V4(c[x]) | V3(c[x-3] | c[x-2] | c[x-1] | c[x+1] | c[x+2] | c[x+3]) | V1(c[x-4] | c[x+4]),   Vk(c) = OR over |j| <= k of c shifted by j rows.
// Bits shifted below row 0 fall off the word; bits shifted to rows >= H are masked off.
#include "hwg_common.h"

constexpr int FGM_BLOCK = 512;
constexpr int FGM_CHUNK = 1024;         // columns dilated per pass; LDS: (1024 + 8) words of 8 bytes
constexpr int FGM_HALO = 4;

template <int K>
__device__ __forceinline__ unsigned long long fgm_vdilate(unsigned long long c) {
  unsigned long long r = c;
#pragma unroll
  for (int j = 1; j <= K; ++j) r |= (c << j) | (c >> j);
  return r;
}

__global__ __launch_bounds__(FGM_BLOCK) void fg_mask_kernel(const unsigned char* __restrict__ pixels, long long pixel_bytes,
                                                            const long long* __restrict__ offsets, const int* __restrict__ widths, int H,
                                                            unsigned char* __restrict__ out, int* __restrict__ thr_out) {
  __shared__ int whist[8][256];          // one histogram per wavefront: only one lane of a wavefront writes at a time
  __shared__ int hist[256];
  __shared__ double var[256];
  __shared__ unsigned long long cols[FGM_CHUNK + 2 * FGM_HALO];
  __shared__ int thr;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long off = offsets[b];
  const int w = widths[b];
  // a bad table entry (ops.fg_masks refuses it on the host) touches nothing
  if (!hwg_line_in_pool(off, w, H, pixel_bytes)) {
    if (thr_out && tid == 0) thr_out[b] = -1;
    return;
  }
  const unsigned char* img = pixels + off;
  unsigned char* dst = out + off;
  for (int i = tid; i < 8 * 256; i += FGM_BLOCK) (&whist[0][0])[i] = 0;
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
    thr = t;
    if (thr_out) thr_out[b] = t;
  }
  __syncthreads();
  const int t = thr;
  const unsigned long long rows = H >= 64 ? ~0ull : ((1ull << H) - 1ull);
  for (int X0 = 0; X0 < w; X0 += FGM_CHUNK) {
    for (int i = tid; i < FGM_CHUNK + 2 * FGM_HALO; i += FGM_BLOCK) {
      const int x = X0 - FGM_HALO + i;
      unsigned long long c = 0ull;
      if (x >= 0 && x < w)
        for (int y = 0; y < H; ++y) c |= (unsigned long long)(img[(size_t)y * w + x] <= t) << y;
      cols[i] = c;
    }
    __syncthreads();
    for (int i = tid; i < FGM_CHUNK && X0 + i < w; i += FGM_BLOCK) {
      const unsigned long long* c = cols + FGM_HALO + i;
      const unsigned long long near = c[-3] | c[-2] | c[-1] | c[1] | c[2] | c[3];
      const unsigned long long m = (fgm_vdilate<4>(c[0]) | fgm_vdilate<3>(near) | fgm_vdilate<1>(c[-4] | c[4])) & rows;
      const int x = X0 + i;
      for (int y = 0; y < H; ++y) dst[(size_t)y * w + x] = ((m >> y) & 1ull) ? 255 : 0;
    }
    __syncthreads();
  }
}

extern "C" int hwg_fg_masks(const unsigned char* pixels, long long pixel_bytes, const long long* offsets, const int* widths, int B, int H,
                            unsigned char* out, int* thresholds, void* stream) {
  HWG_REQUIRE(pixels && offsets && widths && out, "fg_masks: null argument");
  HWG_REQUIRE(out != pixels, "fg_masks: out must not be the input pool");
  HWG_REQUIRE(B > 0 && pixel_bytes > 0, "fg_masks: bad sizes B=%d pixel_bytes=%lld", B, pixel_bytes);
  HWG_REQUIRE(H >= 1 && H <= 64, "fg_masks: line height %d, need 1..64 (a column is one 64-bit word)", H);
  hipLaunchKernelGGL(fg_mask_kernel, dim3(B), dim3(FGM_BLOCK), 0, (hipStream_t)stream, pixels, pixel_bytes, offsets, widths, H, out, thresholds);
  HWG_LAUNCH_CHECK("fg_masks");
  return HWG_OK;
}
