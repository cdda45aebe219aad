// Writer retrieval over style vectors: for every line i, the place of the nearest OTHER entry of the same writer in the stable order of
// row i of the all-pairs distance matrix (reference: eval_writer_id.py:15-29 topN over :70-81 l1 / l2 / gt - there two nested Python
// loops, two N x N fp64 matrices and a Python sort of N tuples per row). Nothing of size N x N exists here.
//
// The stable order of a row is the lexicographic order of the key (distance, column); a column's place is the number of keys below
// its own, and place 0 belongs to the row's smallest key alone. So per row:
//   sweep 1: the smallest key of the row (g) and the smallest and second smallest key among the columns of the row's writer (s1, s2).
//            The target is s1 unless s1 is g, then s2; without one the row has no match. Left in the outputs: nearest_same = the
//            target's distance (+inf without), first_rank = the target's column (-1 without).
//   sweep 2: first_rank = the number of columns whose key is below the target's (N without a target).
// Sweep 2 computes every distance again, so a distance has to be the same bits wherever it is computed: both sweeps are one kernel
// template around wid_accumulate - one fp32 chain per (row, column) over d = 0 .. D-1 in ascending order, `acc + |diff|` or
// `fma(diff, diff, acc)`, independent of tile position and lane (the depth loop stops at D; the zero padding of a tile is never added
// and would be exact if it were).
//
// A workgroup (4 wavefronts) owns WID_BR = 16 rows and walks all columns in blocks of WID_BC = 256, depth in tiles of WID_DK = 32.
// Both tiles are staged in LDS transposed ([d][row], [d][column]) so that a lane reads its 4 rows and its 4 columns with one 16-byte
// read each (rows: 4 addresses per wavefront, broadcast; columns: 16 lanes x 16 B contiguous); wavefront w takes columns
// 64 w .. 64 w + 63 of the block, a lane a 4 x 4 register tile. 16 rows per workgroup because the grid is N / 16 workgroups and a
// split's line count is a few thousand: larger row blocks leave most CUs without work. The 64 lanes that share a row (16 per wavefront
// x 4 wavefronts) are combined through LDS (sweep 1: key merges) or lane exchanges + LDS (sweep 2: sums). No atomics, nothing crosses
// workgroups; the kernel boundary between the sweeps is the only grid-wide synchronisation. VALU bound: 2 N^2 D lane operations
// per sweep (L2 stays off the matrix cores: a Gram-matrix form rounds differently and would change the order of near ties).
#include "hwg_common.h"
#include <limits.h>
#include <math.h>

constexpr int WID_BR = 16, WID_BC = 256, WID_DK = 32, WID_BLOCK = 256;
constexpr int WID_RS = WID_BR + 4, WID_CS = WID_BC + 4;       // row strides of the transposed tiles: 16-byte multiples
constexpr int WID_SHARERS = WID_BLOCK / 4;                    // lanes of the workgroup that hold part of one row
constexpr int WID_MAX_N = 1 << 20, WID_MAX_D = 65536;
constexpr int WID_TILE_FLOATS = WID_DK * (WID_RS + WID_CS);
constexpr int WID_MERGE_FLOATS = 6 * WID_BR * WID_SHARERS;
constexpr int WID_LDS_FLOATS = WID_TILE_FLOATS > WID_MERGE_FLOATS ? WID_TILE_FLOATS : WID_MERGE_FLOATS;

// the one place a distance term is added (both sweeps, both tiles of a pair, every lane): hwg_common.h's step, shared with the other
// style-distance kernels
template <int METRIC>
__device__ __forceinline__ float wid_accumulate(float acc, float a, float b) { return hwg_dist_step<METRIC>(acc, a, b); }

__device__ __forceinline__ bool wid_below(float d, int c, float d2, int c2) { return d < d2 || (d == d2 && c < c2); }

// SWEEP 0: targets into (nearest_same, first_rank); SWEEP 1: counts into first_rank
template <int METRIC, int SWEEP>
__global__ __launch_bounds__(WID_BLOCK) void wid_sweep_kernel(const float* __restrict__ styles, const int* __restrict__ author, int N, int D,
                                                              int* __restrict__ first_rank, float* __restrict__ nearest_same) {
  __shared__ __attribute__((aligned(16))) float lds[WID_LDS_FLOATS];
  float* Rs = lds;                          // [WID_DK][WID_RS]
  float* Cs = lds + WID_DK * WID_RS;        // [WID_DK][WID_CS]
  const int tid = threadIdx.x, w = tid >> 6, tx = tid & 15, ty = (tid >> 4) & 3;
  const int row0 = blockIdx.x * WID_BR;

  int ra[4];                                // the rows' writers (SWEEP 0) / target columns (SWEEP 1)
  float td[4];                              // target distances (SWEEP 1)
  float gd[4], s1d[4], s2d[4];
  int gc[4], s1c[4], s2c[4], below[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + ty * 4 + r;
    gd[r] = s1d[r] = s2d[r] = INFINITY;
    gc[r] = s1c[r] = s2c[r] = INT_MAX;
    below[r] = 0;
    td[r] = 0.f;
    ra[r] = -1;
    if (row < N) {
      if (SWEEP == 0) ra[r] = author[row];
      else { ra[r] = first_rank[row]; td[r] = nearest_same[row]; }
    }
  }

  for (int col0 = 0; col0 < N; col0 += WID_BC) {
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;

    for (int d0 = 0; d0 < D; d0 += WID_DK) {
      __syncthreads();                      // the previous tile has been read by everyone
      for (int i = tid; i < WID_BR * WID_DK; i += WID_BLOCK) {
        const int d = i % WID_DK, r = i / WID_DK, row = row0 + r;
        Rs[d * WID_RS + r] = (row < N && d0 + d < D) ? styles[(size_t)row * D + d0 + d] : 0.f;
      }
      for (int i = tid; i < WID_BC * WID_DK; i += WID_BLOCK) {
        const int d = i % WID_DK, c = i / WID_DK, col = col0 + c;
        Cs[d * WID_CS + c] = (col < N && d0 + d < D) ? styles[(size_t)col * D + d0 + d] : 0.f;
      }
      __syncthreads();
      const int depth = D - d0 < WID_DK ? D - d0 : WID_DK;
      const float* rp = Rs + ty * 4;
      const float* cp = Cs + w * 64 + tx * 4;
#pragma unroll 4
      for (int d = 0; d < depth; ++d) {
        const f32x4 rv = *(const f32x4*)(rp + d * WID_RS);
        const f32x4 cv = *(const f32x4*)(cp + d * WID_CS);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = wid_accumulate<METRIC>(acc[r][c], rv[r], cv[c]);
      }
    }

    // fold the finished distances into the per-row running keys / counts
    const int cbase = col0 + w * 64 + tx * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = cbase + c;
      if (col >= N) continue;
      const int ca = SWEEP == 0 ? author[col] : 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dist = acc[r][c];
        if (SWEEP == 0) {
          if (wid_below(dist, col, gd[r], gc[r])) { gd[r] = dist; gc[r] = col; }
          if (ca == ra[r]) {
            if (wid_below(dist, col, s1d[r], s1c[r])) { s2d[r] = s1d[r]; s2c[r] = s1c[r]; s1d[r] = dist; s1c[r] = col; }
            else if (wid_below(dist, col, s2d[r], s2c[r])) { s2d[r] = dist; s2c[r] = col; }
          }
        } else {
          below[r] += wid_below(dist, col, td[r], ra[r]) ? 1 : 0;
        }
      }
    }
  }

  __syncthreads();                          // the tiles are dead: their LDS carries the per-row combination
  if (SWEEP == 0) {
    float* md = lds;                                          // [3][WID_BR][WID_SHARERS] distances
    int* mc = (int*)(lds + 3 * WID_BR * WID_SHARERS);         // [3][WID_BR][WID_SHARERS] columns
    const int k = w * 16 + tx;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = (ty * 4 + r) * WID_SHARERS + k;
      md[s] = gd[r]; mc[s] = gc[r];
      md[WID_BR * WID_SHARERS + s] = s1d[r]; mc[WID_BR * WID_SHARERS + s] = s1c[r];
      md[2 * WID_BR * WID_SHARERS + s] = s2d[r]; mc[2 * WID_BR * WID_SHARERS + s] = s2c[r];
    }
    __syncthreads();
    if (tid < WID_BR && row0 + tid < N) {
      float g_d = INFINITY, a_d = INFINITY, b_d = INFINITY;   // g: row minimum, a / b: smallest / second smallest of the row's writer
      int g_c = INT_MAX, a_c = INT_MAX, b_c = INT_MAX;
      for (int k2 = 0; k2 < WID_SHARERS; ++k2) {
        const int s = tid * WID_SHARERS + k2;
        if (wid_below(md[s], mc[s], g_d, g_c)) { g_d = md[s]; g_c = mc[s]; }
#pragma unroll
        for (int part = 1; part <= 2; ++part) {               // a lane's two candidates, smaller first
          const float d = md[part * WID_BR * WID_SHARERS + s];
          const int c = mc[part * WID_BR * WID_SHARERS + s];
          if (c == INT_MAX) continue;
          if (wid_below(d, c, a_d, a_c)) { b_d = a_d; b_c = a_c; a_d = d; a_c = c; }
          else if (wid_below(d, c, b_d, b_c)) { b_d = d; b_c = c; }
        }
      }
      float t_d = a_d;
      int t_c = a_c;
      if (a_c != INT_MAX && a_c == g_c) { t_d = b_d; t_c = b_c; }
      const bool none = t_c == INT_MAX;
      nearest_same[row0 + tid] = none ? INFINITY : t_d;
      first_rank[row0 + tid] = none ? -1 : t_c;
    }
  } else {
    int* sums = (int*)lds;                                    // [4 wavefronts][WID_BR]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int v = below[r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // the 16 lanes of a wavefront that share the row
      if (tx == 0) sums[w * WID_BR + ty * 4 + r] = v;
    }
    __syncthreads();
    if (tid < WID_BR && row0 + tid < N) {
      const int row = row0 + tid;
      const int total = sums[tid] + sums[WID_BR + tid] + sums[2 * WID_BR + tid] + sums[3 * WID_BR + tid];
      first_rank[row] = first_rank[row] < 0 ? N : total;
    }
  }
}

extern "C" int hwg_writer_first_rank(const float* styles, const int* author_id, int N, int D, int metric, int* first_rank, float* nearest_same,
                                     void* stream) {
  HWG_REQUIRE(styles && author_id && first_rank && nearest_same, "writer_first_rank: null argument");
  HWG_REQUIRE(N >= 1 && D >= 1 && (metric == 0 || metric == 1), "writer_first_rank: bad sizes N=%d D=%d metric=%d (0 L1, 1 squared L2)", N, D,
              metric);
  HWG_REQUIRE(N <= WID_MAX_N && D <= WID_MAX_D, "writer_first_rank: beyond the limit N=%d (<= %d) D=%d (<= %d)", N, WID_MAX_N, D, WID_MAX_D);
  HWG_REQUIRE(((uintptr_t)styles & 15) == 0 && ((uintptr_t)author_id & 3) == 0 && ((uintptr_t)first_rank & 3) == 0 &&
                  ((uintptr_t)nearest_same & 3) == 0,
              "writer_first_rank: styles must be 16-byte aligned, author_id, first_rank and nearest_same 4-byte aligned");
  const dim3 grid(hwg_cdiv(N, WID_BR)), block(WID_BLOCK);
  if (metric == 0) {
    hipLaunchKernelGGL((wid_sweep_kernel<0, 0>), grid, block, 0, (hipStream_t)stream, styles, author_id, N, D, first_rank, nearest_same);
    HWG_LAUNCH_CHECK("writer_first_rank targets");
    hipLaunchKernelGGL((wid_sweep_kernel<0, 1>), grid, block, 0, (hipStream_t)stream, styles, author_id, N, D, first_rank, nearest_same);
  } else {
    hipLaunchKernelGGL((wid_sweep_kernel<1, 0>), grid, block, 0, (hipStream_t)stream, styles, author_id, N, D, first_rank, nearest_same);
    HWG_LAUNCH_CHECK("writer_first_rank targets");
    hipLaunchKernelGGL((wid_sweep_kernel<1, 1>), grid, block, 0, (hipStream_t)stream, styles, author_id, N, D, first_rank, nearest_same);
  }
  HWG_LAUNCH_CHECK("writer_first_rank counts");
  return HWG_OK;
}
