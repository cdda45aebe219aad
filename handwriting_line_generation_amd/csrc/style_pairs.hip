// Same-writer / different-writer distances in style space: over all unordered pairs i < j of style vectors, count, sum of d and sum of d^2
// per cell - two cells (same writer, different writers) or one cell per writer pair -, the smallest and largest d^2, and optionally a
// histogram of the same-writer and of the different-writer distances (reference: play_styles.py:19-39, there a double Python loop over
// N (N - 1) / 2 pairs that appends to three lists; its writer x writer matrices, :43-53, sit behind an exit() and are keyed by line).
// Nothing of size N x N exists, no floating-point atomics, nothing crosses a workgroup inside a launch: the kernel boundaries are the
// grid-wide synchronisation (the XCDs' L2s are not coherent with each other), and two runs give the same bits.
//
// A pair's d^2 is the fp32 chain of writer_id.hip (hwg_dist_step<1> over d = 0 .. D-1 ascending; the depth loop stops at D), d is
// sqrt((double) d^2), and a cell sums d and (double) d^2 in fp64. The rows are sorted by writer (the caller's stable sort), so a writer is
// a contiguous range of rows and of columns.
//
// SWEEP. The distance part is writer_id.hip's: a workgroup (4 wavefronts) owns SP_BR = 16 consecutive rows and walks the column blocks of
// SP_BC = 256 from the one that holds its first row to the last, depth in tiles of SP_DK = 32, both tiles transposed in LDS, a 4 x 4
// register tile per lane; pairs with column <= row are computed and dropped. Workgroup b owns rows 16 b ..: the workgroups with the most
// columns have the lowest indices and start first, the grid's tail is made of the shortest ones.
//   mode 0 - every lane adds its pairs to its own two cells in the order (column block, r, c); at the end the 256 lanes are combined by a
//            butterfly over lane distances 32 .. 1 (an add commutes: every lane ends with the same bits) and the four wavefronts in order
//            0, 1, 2, 3 -> partial[row block][2].
//   mode 1 - the 16 rows fall into runs of one writer each. Per run and column block: a column's sum over the run's rows is formed in the
//            lane (r ascending), then over the four lanes that share the column (butterfly over lane distances 16, 32) -> cs[column]. A
//            writer's columns inside the block are one segment; its sum is formed in two fixed levels: within every aligned group of
//            SP_GROUP = 8 columns the first column of each segment piece adds the piece's columns in ascending order, then the segment's
//            first column adds its own piece and the following groups' first pieces in ascending order. A segment that runs on into the
//            next column block is carried (carry + the next block's sum); one that ends is stored: partial[row block + writer][column
//            writer] - row block + writer is a different slot for every (row block, run), because the writers only rise.
// REDUCE (second launch). mode 0: 256 lanes add contiguous ranges of row blocks in ascending order, lane 0 adds the 256 sums in order.
// mode 1: one lane per cell a <= b adds the slots of writer a's row blocks in ascending order and stores (a, b) and (b, a); a writer's row
// range comes from a binary search over the writer array (first launch of mode 1). A cell without pairs is (0, 0, 0).
// Histogram: bin k holds the pairs with edge2[k] <= d^2 < edge2[k + 1], compared in fp32 on the bits of d^2; the bin is guessed from
// sqrtf(d^2) and equal-width edges and then moved by these comparisons until they hold, so any ascending edges give the right answer.
// Counters are 32-bit integers in LDS per workgroup, added to the int64 output with integer atomics (order cannot change an integer sum).
// What the writer array holds cannot make the kernels leave their buffers: ids outside 0 .. A-1 are dropped, every index is derived from
// N, A and the launch geometry. An array that is not sorted gives meaningless sums - ops.style_pair_stats refuses it.
#include "hwg_common.h"
#include <math.h>

constexpr int SP_BR = 16, SP_BC = 256, SP_DK = 32, SP_BLOCK = 256, SP_GROUP = 8;
constexpr int SP_RS = SP_BR + 4, SP_CS = SP_BC + 4;           // row strides of the transposed tiles: 16-byte multiples
constexpr int SP_MAX_N = 1 << 20, SP_MAX_D = 65536, SP_MAX_A = 4096, SP_MAX_BINS = 256;

// the workspace, carved up (all offsets multiples of 16 bytes)
struct SpWorkspace {
  size_t range, n0, s0, q0, start, n1, s1, q1, bytes;
  int row_blocks, slots;
};

static size_t sp_align(size_t v) { return (v + 15) & ~(size_t)15; }

static SpWorkspace sp_workspace(int N, int A, int mode) {
  SpWorkspace w;
  memset(&w, 0, sizeof(w));
  w.row_blocks = hwg_cdiv(N, SP_BR);
  w.slots = w.row_blocks + A;
  size_t at = 0;
  w.range = at; at = sp_align(at + (size_t)w.row_blocks * 2 * sizeof(float));
  if (mode == 0) {
    w.n0 = at; at = sp_align(at + (size_t)w.row_blocks * 2 * sizeof(long long));
    w.s0 = at; at = sp_align(at + (size_t)w.row_blocks * 2 * sizeof(double));
    w.q0 = at; at = sp_align(at + (size_t)w.row_blocks * 2 * sizeof(double));
  } else {
    const size_t cells = (size_t)w.slots * (size_t)A;
    w.start = at; at = sp_align(at + (size_t)(A + 1) * sizeof(int));
    w.s1 = at; at = sp_align(at + cells * sizeof(double));
    w.q1 = at; at = sp_align(at + cells * sizeof(double));
    w.n1 = at; at = sp_align(at + cells * sizeof(int));
  }
  w.bytes = at;
  return w;
}

struct SpPartials {
  float* range;             // [row blocks][2]: smallest, largest d^2
  long long* n0;            // mode 0 [row blocks][2]
  double* s0;
  double* q0;
  int* n1;                  // mode 1 [slots][A]
  double* s1;
  double* q1;
};

// bin of d2 under edges e[0 .. bins] (LDS), -1 outside [e[0], e[bins]): a guess from equal-width bins in d, corrected by the comparisons
__device__ __forceinline__ int sp_bin(const float* e, int bins, float d2, float e1, float inv_w) {
  float g = bins > 2 ? 1.f + (sqrtf(d2) - e1) * inv_w : 0.f;
  g = fminf(fmaxf(g, 0.f), (float)(bins - 1));                // (a NaN becomes 0)
  int k = (int)g;
  while (k > 0 && d2 < e[k]) --k;
  while (k < bins - 1 && d2 >= e[k + 1]) ++k;
  return (d2 >= e[k] && d2 < e[k + 1]) ? k : -1;
}

template <int MODE, int HIST>
__global__ __launch_bounds__(SP_BLOCK) void sp_sweep_kernel(const float* __restrict__ styles, const int* __restrict__ writer, int N, int D, int A,
                                                            const float* __restrict__ edge2, int bins, SpPartials p,
                                                            unsigned long long* __restrict__ hist) {
  __shared__ __attribute__((aligned(16))) float Rs[SP_DK * SP_RS];          // [d][row]
  __shared__ __attribute__((aligned(16))) float Cs[SP_DK * SP_CS];          // [d][column]
  __shared__ int rw[SP_BR];                                                 // the rows' writers (-1 beyond N)
  __shared__ int cw[SP_BC + 2];                                             // writers of columns col0 - 1 .. col0 + SP_BC (-2 outside 0 .. N-1)
  __shared__ double cs_s[MODE ? SP_BC : 1], cs_q[MODE ? SP_BC : 1];         // mode 1: per-column sums of the current run
  __shared__ int cs_n[MODE ? SP_BC : 1];
  __shared__ double carry_s[2][MODE ? SP_BR : 1], carry_q[2][MODE ? SP_BR : 1];   // mode 1: [column block parity][run]
  __shared__ int carry_n[2][MODE ? SP_BR : 1];
  __shared__ int run_start[SP_BR + 1];
  __shared__ int run_count;
  __shared__ unsigned hist_l[HIST ? 2 * SP_MAX_BINS : 1];
  __shared__ float edge_l[HIST ? SP_MAX_BINS + 1 : 1];
  __shared__ double red_d[4][4];
  __shared__ long long red_n[4][2];
  __shared__ float red_f[4][2];

  const int tid = threadIdx.x, w = tid >> 6, tx = tid & 15, ty = (tid >> 4) & 3;
  const int rb = blockIdx.x, row0 = rb * SP_BR;

  if (tid < SP_BR) rw[tid] = row0 + tid < N ? writer[row0 + tid] : -1;
  if (MODE) {
    for (int i = tid; i < 2 * SP_BR; i += SP_BLOCK) {
      carry_s[i / SP_BR][i % SP_BR] = 0.0;
      carry_q[i / SP_BR][i % SP_BR] = 0.0;
      carry_n[i / SP_BR][i % SP_BR] = 0;
    }
  }
  if (HIST) {
    for (int i = tid; i < 2 * SP_MAX_BINS; i += SP_BLOCK) hist_l[i] = 0u;
    for (int i = tid; i <= bins; i += SP_BLOCK) edge_l[i] = edge2[i];
  }
  __syncthreads();
  if (MODE && tid == 0) {
    const int valid = N - row0 < SP_BR ? N - row0 : SP_BR;
    int k = 0;
    run_start[0] = 0;
    for (int r = 1; r < valid; ++r)
      if (rw[r] != rw[r - 1]) run_start[++k] = r;
    run_start[k + 1] = valid;
    run_count = k + 1;
  }
  float e1 = 0.f, inv_w = 0.f;
  if (HIST && bins > 2) {
    e1 = sqrtf(edge_l[1]);
    const float span = sqrtf(edge_l[bins - 1]) - e1;
    inv_w = span > 0.f ? (float)(bins - 2) / span : 0.f;
  }
  int rwr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rwr[r] = rw[ty * 4 + r];

  float lo = INFINITY, hi = -INFINITY;
  long long n_same = 0, n_diff = 0;                           // mode 0: this lane's two cells
  double s_same = 0.0, q_same = 0.0, s_diff = 0.0, q_diff = 0.0;
  int parity = 0;

  for (int col0 = (row0 / SP_BC) * SP_BC; col0 < N; col0 += SP_BC, parity ^= 1) {
    __syncthreads();                        // the previous block's epilogue has read cw
    for (int i = tid; i < SP_BC + 2; i += SP_BLOCK) {
      const int col = col0 - 1 + i;
      cw[i] = (col >= 0 && col < N) ? writer[col] : -2;
    }
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;

    for (int d0 = 0; d0 < D; d0 += SP_DK) {
      __syncthreads();                      // the previous tile has been read by everyone
      for (int i = tid; i < SP_BR * SP_DK; i += SP_BLOCK) {
        const int d = i % SP_DK, r = i / SP_DK, row = row0 + r;
        Rs[d * SP_RS + r] = (row < N && d0 + d < D) ? styles[(size_t)row * D + d0 + d] : 0.f;
      }
      for (int i = tid; i < SP_BC * SP_DK; i += SP_BLOCK) {
        const int d = i % SP_DK, c = i / SP_DK, col = col0 + c;
        Cs[d * SP_CS + c] = (col < N && d0 + d < D) ? styles[(size_t)col * D + d0 + d] : 0.f;
      }
      __syncthreads();
      const int depth = D - d0 < SP_DK ? D - d0 : SP_DK;
      const float* rp = Rs + ty * 4;
      const float* cp = Cs + w * 64 + tx * 4;
#pragma unroll 4
      for (int d = 0; d < depth; ++d) {
        const f32x4 rv = *(const f32x4*)(rp + d * SP_RS);
        const f32x4 cv = *(const f32x4*)(cp + d * SP_CS);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = hwg_dist_step<1>(acc[r][c], rv[r], cv[c]);
      }
    }

    // the finished distances of this lane: rows row0 + 4 ty + r, columns cbase + c; a pair is a column right of its row
    const int lc = w * 64 + tx * 4, cbase = col0 + lc;
    bool active[4][4];
    double dd[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int row = row0 + ty * 4 + r, col = cbase + c;
        active[r][c] = col < N && col > row;          // (col < N and row < col: row < N)
        dd[r][c] = 0.0;
        if (active[r][c]) {
          const float d2 = acc[r][c];
          const bool same = rwr[r] == cw[lc + c + 1];
          lo = fminf(lo, d2);
          hi = fmaxf(hi, d2);
          dd[r][c] = sqrt((double)d2);
          if (MODE == 0) {
            if (same) { n_same += 1; s_same += dd[r][c]; q_same += (double)d2; }
            else { n_diff += 1; s_diff += dd[r][c]; q_diff += (double)d2; }
          }
          if (HIST) {
            const int k = sp_bin(edge_l, bins, d2, e1, inv_w);
            if (k >= 0) atomicAdd(&hist_l[(same ? 0 : bins) + k], 1u);
          }
        }
      }

    if (MODE) {
      const int runs = run_count;
      for (int run = 0; run < runs; ++run) {
        const int r_lo = run_start[run], r_hi = run_start[run + 1], a = rw[r_lo];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double s = 0.0, q = 0.0;
          int n = 0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int lr = ty * 4 + r;
            if (lr >= r_lo && lr < r_hi && active[r][c]) { s += dd[r][c]; q += (double)acc[r][c]; n += 1; }
          }
#pragma unroll
          for (int o = 16; o <= 32; o <<= 1) {                // the four lanes of the wavefront that hold this column
            s += __shfl_xor(s, o, 64);
            q += __shfl_xor(q, o, 64);
            n += __shfl_xor(n, o, 64);
          }
          if (ty == 0) { cs_s[lc + c] = s; cs_q[lc + c] = q; cs_n[lc + c] = n; }
        }
        __syncthreads();
        // level 1: the first column of every segment piece inside its group of SP_GROUP columns adds the piece, ascending
        const int b = cw[tid + 1];
        const bool piece_head = (tid % SP_GROUP) == 0 || cw[tid] != b;
        if (piece_head) {
          double s = cs_s[tid], q = cs_q[tid];
          int n = cs_n[tid];
          const int end = (tid / SP_GROUP + 1) * SP_GROUP;
          for (int k = tid + 1; k < end && cw[k + 1] == b; ++k) { s += cs_s[k]; q += cs_q[k]; n += cs_n[k]; }
          cs_s[tid] = s; cs_q[tid] = q; cs_n[tid] = n;        // nobody else reads or writes this entry in level 1 (see the top of the file)
        }
        __syncthreads();
        // level 2: the first column of a segment adds its own piece and the first pieces of the following groups, ascending
        const bool head = tid == 0 || cw[tid] != b;
        if (head && b >= 0) {
          double s = cs_s[tid], q = cs_q[tid];
          int n = cs_n[tid];
          for (int g = (tid / SP_GROUP + 1) * SP_GROUP; g < SP_BC && cw[g + 1] == b; g += SP_GROUP) { s += cs_s[g]; q += cs_q[g]; n += cs_n[g]; }
          if (tid == 0 && cw[0] == b) {                       // the segment came in from the previous column block
            s = carry_s[parity][run] + s; q = carry_q[parity][run] + q; n = carry_n[parity][run] + n;
          }
          if (cw[SP_BC] == b && cw[SP_BC + 1] == b) {         // ... and runs on into the next one
            carry_s[parity ^ 1][run] = s; carry_q[parity ^ 1][run] = q; carry_n[parity ^ 1][run] = n;
          } else if (b >= a && (unsigned)a < (unsigned)A && (unsigned)b < (unsigned)A) {
            const size_t at = (size_t)(rb + a) * (size_t)A + (size_t)b;
            p.s1[at] = s; p.q1[at] = q; p.n1[at] = n;
          }
        }
        __syncthreads();                    // cs is free for the next run
      }
    }
  }

  // the workgroup's smallest and largest d^2 (exact whatever the order)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if (MODE == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      n_same += __shfl_xor(n_same, o, 64); n_diff += __shfl_xor(n_diff, o, 64);
      s_same += __shfl_xor(s_same, o, 64); q_same += __shfl_xor(q_same, o, 64);
      s_diff += __shfl_xor(s_diff, o, 64); q_diff += __shfl_xor(q_diff, o, 64);
    }
  }
  if ((tid & 63) == 0) {
    red_f[w][0] = lo; red_f[w][1] = hi;
    if (MODE == 0) {
      red_n[w][0] = n_same; red_n[w][1] = n_diff;
      red_d[w][0] = s_same; red_d[w][1] = s_diff; red_d[w][2] = q_same; red_d[w][3] = q_diff;
    }
  }
  __syncthreads();
  if (tid == 0) {
    p.range[2 * rb] = fminf(fminf(red_f[0][0], red_f[1][0]), fminf(red_f[2][0], red_f[3][0]));
    p.range[2 * rb + 1] = fmaxf(fmaxf(red_f[0][1], red_f[1][1]), fmaxf(red_f[2][1], red_f[3][1]));
  }
  if (MODE == 0 && tid < 2) {
    p.n0[2 * rb + tid] = ((red_n[0][tid] + red_n[1][tid]) + red_n[2][tid]) + red_n[3][tid];
    p.s0[2 * rb + tid] = ((red_d[0][tid] + red_d[1][tid]) + red_d[2][tid]) + red_d[3][tid];
    p.q0[2 * rb + tid] = ((red_d[0][2 + tid] + red_d[1][2 + tid]) + red_d[2][2 + tid]) + red_d[3][2 + tid];
  }
  if (HIST) {
    for (int i = tid; i < 2 * bins; i += SP_BLOCK)
      if (hist_l[i]) atomicAdd(&hist[i], (unsigned long long)hist_l[i]);
  }
}

// mode 1, first launch: start[a] = the first row whose writer is >= a (a = 0 .. A: start[A] = N for ids below A)
__global__ __launch_bounds__(SP_BLOCK) void sp_bounds_kernel(const int* __restrict__ writer, int N, int A, int* __restrict__ start) {
  const int a = blockIdx.x * SP_BLOCK + threadIdx.x;
  if (a > A) return;
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (writer[mid] < a) lo = mid + 1;
    else hi = mid;
  }
  start[a] = lo;
}

// one workgroup: the per-row-block ranges, and in mode 0 the per-row-block cells, in a fixed order
__global__ __launch_bounds__(SP_BLOCK) void sp_reduce_kernel(int row_blocks, int cells, SpPartials p, long long* __restrict__ count,
                                                             double* __restrict__ sum, double* __restrict__ sumsq,
                                                             float* __restrict__ d2_range) {
  __shared__ float f_lo[SP_BLOCK], f_hi[SP_BLOCK];
  __shared__ long long l_n[2][SP_BLOCK];
  __shared__ double l_s[2][SP_BLOCK], l_q[2][SP_BLOCK];
  const int tid = threadIdx.x, per = (row_blocks + SP_BLOCK - 1) / SP_BLOCK;
  const int b0 = tid * per, b1 = b0 + per < row_blocks ? b0 + per : row_blocks;
  float lo = INFINITY, hi = -INFINITY;
  long long n[2] = {0, 0};
  double s[2] = {0.0, 0.0}, q[2] = {0.0, 0.0};
  for (int b = b0; b < b1; ++b) {
    lo = fminf(lo, p.range[2 * b]);
    hi = fmaxf(hi, p.range[2 * b + 1]);
    if (cells)
      for (int k = 0; k < 2; ++k) { n[k] += p.n0[2 * b + k]; s[k] += p.s0[2 * b + k]; q[k] += p.q0[2 * b + k]; }
  }
  f_lo[tid] = lo; f_hi[tid] = hi;
  for (int k = 0; k < 2; ++k) { l_n[k][tid] = n[k]; l_s[k][tid] = s[k]; l_q[k][tid] = q[k]; }
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < SP_BLOCK; ++t) { lo = fminf(lo, f_lo[t]); hi = fmaxf(hi, f_hi[t]); }
    d2_range[0] = lo;
    d2_range[1] = hi;
  }
  if (cells && tid < 2) {
    long long tn = 0;
    double ts = 0.0, tq = 0.0;
    for (int t = 0; t < SP_BLOCK; ++t) { tn += l_n[tid][t]; ts += l_s[tid][t]; tq += l_q[tid][t]; }
    count[tid] = tn; sum[tid] = ts; sumsq[tid] = tq;
  }
}

// mode 1: cell (a, b), a <= b = the slots of writer a's row blocks in ascending order; stored at (a, b) and (b, a)
__global__ __launch_bounds__(SP_BLOCK) void sp_cells_kernel(int A, const int* __restrict__ start, SpPartials p, long long* __restrict__ count,
                                                            double* __restrict__ sum, double* __restrict__ sumsq) {
  const long long idx = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
  if (idx >= (long long)A * A) return;
  const int a = (int)(idx / A), b = (int)(idx % A);
  if (a > b) return;
  long long n = 0;
  double s = 0.0, q = 0.0;
  const int a0 = start[a], a1 = start[a + 1];
  if (a1 > a0 && start[b + 1] > start[b]) {
    for (int rb = a0 / SP_BR; rb <= (a1 - 1) / SP_BR; ++rb) {
      const size_t at = (size_t)(rb + a) * (size_t)A + (size_t)b;
      n += p.n1[at]; s += p.s1[at]; q += p.q1[at];
    }
  }
  const size_t ab = (size_t)a * A + b, ba = (size_t)b * A + a;
  count[ab] = n; sum[ab] = s; sumsq[ab] = q;
  count[ba] = n; sum[ba] = s; sumsq[ba] = q;
}

extern "C" size_t hwg_style_pair_stats_workspace(int N, int A, int mode) {
  if (N < 1 || N > SP_MAX_N || (mode != 0 && mode != 1) || A < 1 || A > N || (mode == 1 && A > SP_MAX_A)) return 0;
  return sp_workspace(N, A, mode).bytes;
}

extern "C" int hwg_style_pair_stats(const float* styles, const int* writer, int N, int D, int A, int mode, const float* edge2, int bins,
                                    long long* count, double* sum, double* sumsq, float* d2_range, long long* hist, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  HWG_REQUIRE(styles && writer && count && sum && sumsq && d2_range && workspace, "style_pair_stats: null argument");
  HWG_REQUIRE((edge2 == nullptr) == (hist == nullptr) && (edge2 != nullptr || bins == 0),
              "style_pair_stats: edge2 and hist come together (with bins >= 1) or not at all (with bins == 0)");
  HWG_REQUIRE(N >= 1 && D >= 1 && A >= 1 && A <= N && (mode == 0 || mode == 1) && (edge2 == nullptr || bins >= 1),
              "style_pair_stats: bad sizes N=%d D=%d A=%d (1..N) mode=%d (0 same / different, 1 writer x writer) bins=%d", N, D, A, mode, bins);
  HWG_REQUIRE(N <= SP_MAX_N && D <= SP_MAX_D && bins <= SP_MAX_BINS && (mode == 0 || A <= SP_MAX_A),
              "style_pair_stats: beyond the limit N=%d (<= %d) D=%d (<= %d) bins=%d (<= %d) A=%d (<= %d in mode 1)", N, SP_MAX_N, D, SP_MAX_D,
              bins, SP_MAX_BINS, A, SP_MAX_A);
  HWG_REQUIRE(((uintptr_t)styles & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)writer & 3) == 0 &&
                  ((uintptr_t)edge2 & 3) == 0 && ((uintptr_t)d2_range & 3) == 0 && ((uintptr_t)count & 7) == 0 && ((uintptr_t)sum & 7) == 0 &&
                  ((uintptr_t)sumsq & 7) == 0 && ((uintptr_t)hist & 7) == 0,
              "style_pair_stats: styles and workspace must be 16-byte aligned, count, sum, sumsq and hist 8-byte, writer, edge2 and "
              "d2_range 4-byte aligned");
  const SpWorkspace w = sp_workspace(N, A, mode);
  HWG_REQUIRE(workspace_bytes >= w.bytes, "style_pair_stats: workspace of %zu bytes, N=%d A=%d mode=%d needs %zu", workspace_bytes, N, A, mode,
              w.bytes);
  char* base = (char*)workspace;
  SpPartials p;
  p.range = (float*)(base + w.range);
  p.n0 = (long long*)(base + w.n0); p.s0 = (double*)(base + w.s0); p.q0 = (double*)(base + w.q0);
  p.n1 = (int*)(base + w.n1); p.s1 = (double*)(base + w.s1); p.q1 = (double*)(base + w.q1);
  int* start = (int*)(base + w.start);
  hipStream_t st = (hipStream_t)stream;
  if (hist) {
    if (hipMemsetAsync(hist, 0, (size_t)2 * bins * sizeof(long long), st) != hipSuccess) {
      hwg_set_error("style_pair_stats: clearing the histogram failed");
      return HWG_ERR_LAUNCH;
    }
  }
  const dim3 grid(w.row_blocks), block(SP_BLOCK);
  unsigned long long* h = (unsigned long long*)hist;
  if (mode == 0) {
    if (hist) hipLaunchKernelGGL((sp_sweep_kernel<0, 1>), grid, block, 0, st, styles, writer, N, D, A, edge2, bins, p, h);
    else hipLaunchKernelGGL((sp_sweep_kernel<0, 0>), grid, block, 0, st, styles, writer, N, D, A, edge2, bins, p, h);
    HWG_LAUNCH_CHECK("style_pair_stats sweep");
    hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), block, 0, st, w.row_blocks, 1, p, count, sum, sumsq, d2_range);
    HWG_LAUNCH_CHECK("style_pair_stats reduce");
  } else {
    hipLaunchKernelGGL(sp_bounds_kernel, dim3(hwg_cdiv(A + 1, SP_BLOCK)), block, 0, st, writer, N, A, start);
    HWG_LAUNCH_CHECK("style_pair_stats bounds");
    if (hist) hipLaunchKernelGGL((sp_sweep_kernel<1, 1>), grid, block, 0, st, styles, writer, N, D, A, edge2, bins, p, h);
    else hipLaunchKernelGGL((sp_sweep_kernel<1, 0>), grid, block, 0, st, styles, writer, N, D, A, edge2, bins, p, h);
    HWG_LAUNCH_CHECK("style_pair_stats sweep");
    hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), block, 0, st, w.row_blocks, 0, p, count, sum, sumsq, d2_range);
    HWG_LAUNCH_CHECK("style_pair_stats range");
    hipLaunchKernelGGL(sp_cells_kernel, dim3(hwg_cdiv((long long)A * A, SP_BLOCK)), block, 0, st, A, (const int*)start, p, count, sum, sumsq);
    HWG_LAUNCH_CHECK("style_pair_stats cells");
  }
  return HWG_OK;
}
