// Line augmentation on the collated batch: Tensmeyer brightness (Otsu threshold, foreground / background shifted) and the mesh warp of the
// reference's recogniser pre-training (utils/augmentation.py:5-31, utils/grid_distortion.py:11-66, called from datasets/hw_dataset.py:143-152,
// datasets/author_hw_dataset.py:429-432, datasets/author_rimeslines_dataset.py:428-434), which the reference runs per line in the loader
// workers through OpenCV and scipy.interpolate.griddata. Two launches for the whole ragged batch:
//   1. augment_stats_kernel: one workgroup per line - 256-bin histogram of the valid columns in LDS, Otsu threshold, brightness LUT, border level;
//   2. augment_warp_kernel : one workgroup per 64 columns of a line - the inverse map (piecewise linear over the triangulated control lattice)
//      and the bilinear resample of the LUT-mapped line.
// Image values are levels p = (1 - x) * 128 (integers 0..255; the padding value -1 is level 256, which no pixel has), outputs are 1 - level / 128.
//
// Tables (see include/hwg.h): lines_i [B][4] = {valid width w, lattice rows gy (0 = no warp), lattice columns gx, first valid column x_off},
// lines_f [B][lf_stride] = {foreground scale, background scale, row sigma, column sigma, src_y[GY], src_x[GX]},
// draws [B][draw_stride] = {fg, bg, row displacements [gy][gx], column displacements [gy][gx]} (unit draws, multiplied by the scales / sigmas).
#include "augment_warp.h"      // the constants, the LUT entry and the warp of one tile: shared with store_warp.hip

__global__ __launch_bounds__(512) void augment_stats_kernel(const float* __restrict__ x, const int* __restrict__ lines_i,
                                                            const float* __restrict__ lines_f, int lf_stride,
                                                            const float* __restrict__ draws, int draw_stride, int H, int W,
                                                            int* __restrict__ stats) {
  __shared__ int whist[8][256];          // one histogram per wavefront: only one lane of a wavefront writes at a time, no atomics
  __shared__ int hist[256];
  __shared__ double var[256];
  __shared__ int lut[256];
  __shared__ int thr;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int xoff = max(lines_i[4 * b + 3], 0);
  const int w = max(min(lines_i[4 * b], W - xoff), 0);
  for (int i = tid; i < 8 * 256; i += 512) (&whist[0][0])[i] = 0;
  __syncthreads();
  const float* img = x + (size_t)b * H * W + xoff;
  for (int y = wv; y < H; y += 8) {
    for (int x0 = 0; x0 < w; x0 += 64) {
      const int xl = x0 + lane;
      const bool valid = xl < w;
      const int p = valid ? aug_level(img[(size_t)y * W + xl]) : -1;
      // lines are mostly paper: most lanes of a wavefront hold the same level. The lanes that share the first pending lane's level are
      // counted with one ballot and added by that lane - a few rounds per wavefront row instead of a 64-way same-address conflict
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
    // Otsu: between-class variance of the split {<= tid} / {> tid}, up to the common factor 1 / N^2: (s0 w1 - s1 w0)^2 / (w0 w1), the
    // integer parts exact, the square and the quotient each rounded once in fp64
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
  }
  __syncthreads();
  if (tid < 256) {
    lut[tid] = aug_lut_entry(tid, thr, lines_f + (size_t)b * lf_stride, draws + (size_t)b * draw_stride);
    stats[(size_t)b * AUG_STATS + 2 + tid] = lut[tid];
  }
  __syncthreads();
  if (tid == 0) {
    long long sq = 0;
    for (int p = 0; p < 256; ++p) sq += (long long)hist[p] * lut[p];
    stats[(size_t)b * AUG_STATS] = thr;
    stats[(size_t)b * AUG_STATS + 1] = aug_border_level(sq, N);
  }
}

// the line's pixels as the collated batch holds them: 1 - level / 128
struct AugImageTap {
  const float* img;                      // first valid column of row 0
  int W;
  __device__ __forceinline__ int operator()(int yy, int xx) const { return aug_level(img[(size_t)yy * W + xx]); }
};

__global__ __launch_bounds__(256) void augment_warp_kernel(const float* __restrict__ x, const int* __restrict__ lines_i,
                                                           const float* __restrict__ lines_f, int lf_stride,
                                                           const float* __restrict__ draws, int draw_stride, const int* __restrict__ stats,
                                                           int H, int W, int GY, int GX, float* __restrict__ yout, float* __restrict__ map_out) {
  __shared__ AugTileLds s;
  const int b = blockIdx.y, X0 = blockIdx.x * AUG_TILE, tid = threadIdx.x;
  const int xoff = max(lines_i[4 * b + 3], 0);
  const int w = max(min(lines_i[4 * b], W - xoff), 0);
  const int gy = lines_i[4 * b + 1], gx = lines_i[4 * b + 2];
  const bool warp = gy >= 2 && gx >= 2 && gy <= GY && gx <= GX && gy <= AUG_MAXR && H > 5 && w > 5;
  float* yb = yout + (size_t)b * H * W;
  float* mb = map_out ? map_out + (size_t)b * 2 * H * W : nullptr;
  if (max(X0 - xoff, 0) > min(X0 + AUG_TILE - 1 - xoff, w - 1)) {      // padding only
    aug_padding_tile(H, W, X0, yb, mb);
    return;
  }
  const float m = (float)stats[(size_t)b * AUG_STATS + 1];
  s.lut[tid] = (float)stats[(size_t)b * AUG_STATS + 2 + tid];
  const AugImageTap tap = {x + (size_t)b * H * W + xoff, W};
  aug_warp_tile(s, tap, m, warp, gy, gx, GY, lines_f + (size_t)b * lf_stride, draws + (size_t)b * draw_stride + 2, H, W, w, xoff, X0, yb, mb);
}

extern "C" int hwg_augment_stats(const float* x, const int* lines_i, const float* lines_f, int lf_stride, const float* draws, int draw_stride,
                                 int B, int H, int W, int* stats, void* stream) {
  HWG_REQUIRE(x && lines_i && lines_f && draws && stats && B > 0 && H > 0 && W > 0, "augment_stats: bad arguments");
  HWG_REQUIRE(lf_stride >= 4 && draw_stride >= 2, "augment_stats: table strides too small");
  HWG_REQUIRE((long long)H * W <= (1LL << 22), "augment_stats: line of %d x %d pixels is too large for the exact fp64 Otsu sums", H, W);
  hipLaunchKernelGGL(augment_stats_kernel, dim3(B), dim3(512), 0, (hipStream_t)stream, x, lines_i, lines_f, lf_stride, draws, draw_stride, H, W, stats);
  HWG_LAUNCH_CHECK("augment_stats");
  return HWG_OK;
}

extern "C" int hwg_augment_warp(const float* x, const int* lines_i, const float* lines_f, int lf_stride, const float* draws, int draw_stride,
                                const int* stats, int B, int H, int W, int GY, int GX, float* y, float* map_out, void* stream) {
  HWG_REQUIRE(x && lines_i && lines_f && draws && stats && y && y != x && B > 0 && H > 0 && W > 0, "augment_warp: bad arguments");
  HWG_REQUIRE(GY >= 0 && GX >= 0 && GY <= AUG_MAXR, "augment_warp: %d lattice rows (at most %d: lines up to ~190 px high)", GY, AUG_MAXR);
  HWG_REQUIRE(lf_stride >= 4 + GY + GX && (long long)draw_stride >= 2 + 2LL * GY * GX, "augment_warp: table strides too small for a %d x %d lattice", GY, GX);
  HWG_REQUIRE(B <= 65535, "augment_warp: batch too large");
  hipLaunchKernelGGL(augment_warp_kernel, dim3(hwg_cdiv(W, AUG_TILE), B), dim3(256), 0, (hipStream_t)stream, x, lines_i, lines_f, lf_stride, draws,
                     draw_stride, stats, H, W, GY, GX, y, map_out);
  HWG_LAUNCH_CHECK("augment_warp");
  return HWG_OK;
}
