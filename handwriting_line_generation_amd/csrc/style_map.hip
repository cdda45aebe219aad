// The style-space map of umap_styles.py (reference: umap_styles.py:105-110, there umap-learn's NN-descent and its racy numba layout loop on
// the host): an exact k-nearest-neighbour graph over all pairs of style vectors, and the force-directed layout epochs over the fuzzy graph
// the host builds from it (handwriting_line_generation_amd/style_map.py). Nothing of size N x N exists, no atomics, nothing crosses a
// workgroup inside a launch; the same input and seed give the same bytes.
//
// hwg_knn_rows. The distance part is writer_id.hip's, restated: a workgroup (4 wavefronts) owns SM_BR = 16 rows and walks all columns in
// blocks of SM_BC = 256, depth in tiles of SM_DK = 32, both tiles transposed in LDS; a lane holds a 4 x 4 register tile and one fp32 chain
// fma(diff, diff, acc) per (row, column) over d = 0 .. D-1 ascending - the depth loop stops at D, so a distance is the same bits whatever
// its tile position or lane. A finished column block is handed through LDS (cand[16][256]) to the merge: wavefront w owns the rows
// 4 w .. 4 w + 3 of the workgroup and keeps each row's list of the 64 smallest keys (d2, column) in REGISTERS, entry l in lane l, ascending
// (unused entries are (+inf, INT_MAX), which no real key is above). Per row and 64 candidates: a lane tests its candidate against the
// row's K-th key (lane K - 1), never its own column (excluded by index); the survivors' ballot is walked in ascending lane order, and a
// survivor is inserted at p = the number of list keys below it: lanes above p take their lower neighbour's entry (one lane shift), lane p
// the new key. After the first blocks almost nothing survives. The walk is in column order, but the result does not depend on it: the
// list is the K smallest keys of the row under a total order. Lanes 0 .. K-1 store the row at the end (plain vector stores).
//
// hwg_umap_layout. One launch per epoch, reading one position buffer and writing the other; the kernel boundary is the grid-wide
// synchronisation and the epoch loop is in the entry point. A fixed group of SM_LG = 16 lanes owns a vertex i. SUMMATION ORDER (fp32,
// fixed for a graph): lane g of the group walks the edges row_ptr[i] + g, + 16, + 32, ... in ascending order and adds, per active edge,
// the attraction term and then the repulsion terms t = 0 .. neg-1 to its own partial sum (x and y apart); the 16 partial sums are then
// combined by a butterfly over lane distances 8, 4, 2, 1 (every lane ends with the same bits: an fp32 add commutes), and
// y_i' = y_i + alpha * sum. An edge's schedule is integer arithmetic, its random vertices are Philox words of (seed, epoch, edge, t):
// nothing depends on which lane or workgroup does the work.
#include "hwg_common.h"
#include "philox.h"
#include <limits.h>
#include <math.h>

constexpr int SM_BR = 16, SM_BC = 256, SM_DK = 32, SM_BLOCK = 256;
constexpr int SM_RS = SM_BR + 4, SM_CS = SM_BC + 4;           // row strides of the transposed tiles: 16-byte multiples
constexpr int SM_MAX_N = 1 << 20, SM_MAX_D = 65536, SM_MAX_K = 64;
constexpr int SM_LG = 16;                                     // lanes per vertex of the layout kernel
constexpr int SM_MAX_NEG = 16, SM_MAX_EPOCHS = 32767;         // 65536 * n_epochs (the largest period, the schedule's products) fits 31 bits

__device__ __forceinline__ bool sm_below(float d, int c, float d2, int c2) { return d < d2 || (d == d2 && c < c2); }

__global__ __launch_bounds__(SM_BLOCK) void sm_knn_kernel(const float* __restrict__ styles, int N, int D, int K, int* __restrict__ idx,
                                                          float* __restrict__ d2out) {
  __shared__ __attribute__((aligned(16))) float Rs[SM_DK * SM_RS];          // [d][row]
  __shared__ __attribute__((aligned(16))) float Cs[SM_DK * SM_CS];          // [d][column]
  __shared__ __attribute__((aligned(16))) float cand[SM_BR * SM_BC];        // [row][column of the block]: the finished distances
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, tx = tid & 15, ty = (tid >> 4) & 3;
  const int row0 = blockIdx.x * SM_BR;

  float kd[4];                              // this wavefront's rows 4 w + r: entry `lane` of the row's ascending key list
  int kc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { kd[r] = INFINITY; kc[r] = INT_MAX; }

  for (int col0 = 0; col0 < N; col0 += SM_BC) {
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;

    for (int d0 = 0; d0 < D; d0 += SM_DK) {
      __syncthreads();                      // the previous tile has been read by everyone (and the previous block's cand has been merged)
      for (int i = tid; i < SM_BR * SM_DK; i += SM_BLOCK) {
        const int d = i % SM_DK, r = i / SM_DK, row = row0 + r;
        Rs[d * SM_RS + r] = (row < N && d0 + d < D) ? styles[(size_t)row * D + d0 + d] : 0.f;
      }
      for (int i = tid; i < SM_BC * SM_DK; i += SM_BLOCK) {
        const int d = i % SM_DK, c = i / SM_DK, col = col0 + c;
        Cs[d * SM_CS + c] = (col < N && d0 + d < D) ? styles[(size_t)col * D + d0 + d] : 0.f;
      }
      __syncthreads();
      const int depth = D - d0 < SM_DK ? D - d0 : SM_DK;
      const float* rp = Rs + ty * 4;
      const float* cp = Cs + w * 64 + tx * 4;
#pragma unroll 4
      for (int d = 0; d < depth; ++d) {
        const f32x4 rv = *(const f32x4*)(rp + d * SM_RS);
        const f32x4 cv = *(const f32x4*)(cp + d * SM_CS);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = hwg_dist_step<1>(acc[r][c], rv[r], cv[c]);   // the distance step of writer_id.hip (squared L2)
      }
    }

    // hand the block's distances to the wavefronts that own the rows (D >= 1: the barriers of the depth loop above separate this block's
    // writes from the previous block's reads)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      f32x4 v;
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = acc[r][c];
      *(f32x4*)(cand + (ty * 4 + r) * SM_BC + w * 64 + tx * 4) = v;
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = w * 4 + r, row = row0 + lrow;
      if (row >= N) continue;               // wavefront-uniform
      for (int chunk = 0; chunk < SM_BC / 64; ++chunk) {
        const int cbase = col0 + chunk * 64;
        if (cbase >= N) break;
        const int col = cbase + lane;
        const float dist = cand[lrow * SM_BC + chunk * 64 + lane];
        const float td = __shfl(kd[r], K - 1, 64);
        const int tc = __shfl(kc[r], K - 1, 64);
        const bool pass = col < N && col != row && sm_below(dist, col, td, tc);
        unsigned long long mask = __ballot(pass);
        while (mask) {
          const int src = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const float nd = __shfl(dist, src, 64);
          const int nc = cbase + src;
          const int p = __popcll(__ballot(sm_below(kd[r], kc[r], nd, nc)));   // the list is ascending: the keys below are a prefix
          if (p >= K) continue;             // the K-th key has moved below this one since the test
          const float ud = __shfl_up(kd[r], 1, 64);
          const int uc = __shfl_up(kc[r], 1, 64);
          if (lane == p) { kd[r] = nd; kc[r] = nc; }
          else if (lane > p) { kd[r] = ud; kc[r] = uc; }
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + w * 4 + r;
    if (row < N && lane < K) {              // K <= N - 1: every one of the K entries is a real key
      idx[(size_t)row * K + lane] = kc[r];
      d2out[(size_t)row * K + lane] = kd[r];
    }
  }
}

extern "C" int hwg_knn_rows(const float* styles, int N, int D, int K, int* idx, float* d2, void* stream) {
  HWG_REQUIRE(styles && idx && d2, "knn_rows: null argument");
  HWG_REQUIRE(N >= 2 && D >= 1 && K >= 1, "knn_rows: bad sizes N=%d D=%d K=%d", N, D, K);
  HWG_REQUIRE(N <= SM_MAX_N && D <= SM_MAX_D && K <= SM_MAX_K && K <= N - 1,
              "knn_rows: beyond the limit N=%d (<= %d) D=%d (<= %d) K=%d (<= %d and <= N - 1)", N, SM_MAX_N, D, SM_MAX_D, K, SM_MAX_K);
  HWG_REQUIRE(((uintptr_t)styles & 15) == 0 && ((uintptr_t)idx & 3) == 0 && ((uintptr_t)d2 & 3) == 0,
              "knn_rows: styles must be 16-byte aligned, idx and d2 4-byte aligned");
  hipLaunchKernelGGL(sm_knn_kernel, dim3(hwg_cdiv(N, SM_BR)), dim3(SM_BLOCK), 0, (hipStream_t)stream, styles, N, D, K, idx, d2);
  HWG_LAUNCH_CHECK("knn_rows");
  return HWG_OK;
}

// ---- layout ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sm_clip(float v) { return fminf(fmaxf(v, -4.f), 4.f); }

__global__ __launch_bounds__(SM_BLOCK) void sm_layout_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col,
                                                             const int* __restrict__ period_q, int N, int E, const float* __restrict__ src,
                                                             float* __restrict__ dst, int n, float alpha, float a, float b, int neg,
                                                             unsigned long long seed) {
  const int g = threadIdx.x & (SM_LG - 1);
  const int i = blockIdx.x * (SM_BLOCK / SM_LG) + (threadIdx.x / SM_LG);
  const bool live = i < N;                  // (dead groups keep walking to the lane exchanges below with empty rows)
  const int e0 = live ? row_ptr[i] : 0, e1 = live ? row_ptr[i + 1] : 0;
  const float2 yi = live ? ((const float2*)src)[i] : make_float2(0.f, 0.f);
  const unsigned blocks = (unsigned)(neg + 3) / 4u;
  const unsigned hi_n = (unsigned)n * 65536u, lo_n = (unsigned)(n - 1) * 65536u;
  float sx = 0.f, sy = 0.f;
  for (int e = e0 + g; e < e1; e += SM_LG) {
    const unsigned q = (unsigned)period_q[e];
    if (hi_n / q <= lo_n / q) continue;     // not this epoch
    const float2 yj = ((const float2*)src)[col[e]];
    {
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float s = fmaf(dy, dy, dx * dx);
      if (s > 0.f) {
        const float c = (-2.f * a * b * powf(s, b - 1.f)) / (a * powf(s, b) + 1.f);
        sx += 2.f * sm_clip(c * dx);
        sy += 2.f * sm_clip(c * dy);
      }
    }
    const unsigned long long ctr0 = ((unsigned long long)n * (unsigned long long)E + (unsigned long long)e) * blocks;
    uint32_t word[4];
    for (int t = 0; t < neg; ++t) {
      if ((t & 3) == 0) hwg_philox4(seed, ctr0 + (unsigned)(t >> 2), word);
      const uint32_t wv = (t & 3) == 0 ? word[0] : (t & 3) == 1 ? word[1] : (t & 3) == 2 ? word[2] : word[3];
      const int r = (int)(((unsigned long long)wv * (unsigned long long)N) >> 32);
      if (r == i) continue;
      const float2 yr = ((const float2*)src)[r];
      const float dx = yi.x - yr.x, dy = yi.y - yr.y;
      const float s = fmaf(dy, dy, dx * dx);
      if (s > 0.f) {
        const float c = (2.f * b) / ((0.001f + s) * (a * powf(s, b) + 1.f));
        sx += sm_clip(c * dx);
        sy += sm_clip(c * dy);
      } else {
        sx += 4.f;
        sy += 4.f;
      }
    }
  }
#pragma unroll
  for (int o = SM_LG / 2; o > 0; o >>= 1) {
    sx += __shfl_xor(sx, o, 64);
    sy += __shfl_xor(sy, o, 64);
  }
  if (live && g == 0) ((float2*)dst)[i] = make_float2(fmaf(alpha, sx, yi.x), fmaf(alpha, sy, yi.y));
}

__global__ __launch_bounds__(SM_BLOCK) void sm_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int count) {
  for (int i = blockIdx.x * SM_BLOCK + threadIdx.x; i < count; i += gridDim.x * SM_BLOCK) dst[i] = src[i];
}

extern "C" int hwg_umap_layout(const int* row_ptr, const int* col, const int* period_q, int N, int E, float* y, float* y_scratch,
                               int epoch_begin, int epoch_end, int n_epochs, float a, float b, int neg, unsigned long long seed, void* stream) {
  HWG_REQUIRE(row_ptr && col && period_q && y && y_scratch, "umap_layout: null argument");
  HWG_REQUIRE(y != y_scratch, "umap_layout: y and y_scratch must be two buffers");
  HWG_REQUIRE(N >= 1 && E >= 1 && n_epochs >= 1 && 0 <= epoch_begin && epoch_begin <= epoch_end && epoch_end <= n_epochs,
              "umap_layout: bad sizes N=%d E=%d epochs %d..%d of %d", N, E, epoch_begin, epoch_end, n_epochs);
  HWG_REQUIRE(N <= SM_MAX_N && neg >= 1 && neg <= SM_MAX_NEG && n_epochs <= SM_MAX_EPOCHS,
              "umap_layout: beyond the limit N=%d (<= %d) neg=%d (1..%d) n_epochs=%d (<= %d)", N, SM_MAX_N, neg, SM_MAX_NEG, n_epochs,
              SM_MAX_EPOCHS);
  HWG_REQUIRE(a > 0.f && b > 0.f && a < INFINITY && b < INFINITY, "umap_layout: a and b must be positive and finite, got %g %g", (double)a,
              (double)b);
  HWG_REQUIRE(((uintptr_t)row_ptr & 3) == 0 && ((uintptr_t)col & 3) == 0 && ((uintptr_t)period_q & 3) == 0 && ((uintptr_t)y & 7) == 0 &&
                  ((uintptr_t)y_scratch & 7) == 0,
              "umap_layout: row_ptr, col and period_q must be 4-byte aligned, y and y_scratch 8-byte aligned");
  const int count = epoch_end - epoch_begin;
  if (count == 0) return HWG_OK;
  // the launches alternate between the two buffers and the last one writes y: an odd number of epochs starts from a copy in y_scratch
  float* from = y;
  float* to = y_scratch;
  if (count & 1) {
    hipLaunchKernelGGL(sm_copy_kernel, dim3(hwg_stream_grid(2LL * N, SM_BLOCK)), dim3(SM_BLOCK), 0, (hipStream_t)stream, (const float*)y,
                       y_scratch, 2 * N);
    HWG_LAUNCH_CHECK("umap_layout copy");
    from = y_scratch;
    to = y;
  }
  const dim3 grid(hwg_cdiv(N, SM_BLOCK / SM_LG)), block(SM_BLOCK);
  for (int n = epoch_begin + 1; n <= epoch_end; ++n) {
    const float alpha = (float)(1.0 - (double)(n - 1) / (double)n_epochs);
    hipLaunchKernelGGL(sm_layout_kernel, grid, block, 0, (hipStream_t)stream, row_ptr, col, period_q, N, E, (const float*)from, to, n, alpha, a,
                       b, neg, seed);
    HWG_LAUNCH_CHECK("umap_layout epoch");
    float* t = from; from = to; to = t;
  }
  return HWG_OK;
}
