// Recognition error rates on the device: what HWWithStyleTrainer.getCER does per line on the host - np.argmax over the classes, the greedy
// CTC decode of utils/string_utils.naive_decode, " ".join(h.split()), and the character and word Levenshtein distances of
// string_utils.cer / wer (reference: trainer/hw_with_style_trainer.py:894-914, utils/error_rates.py:2-26) - as two launches that leave
// integers only: the host divides.
//
//  1. er_argmax_kernel: 16 lanes per row of pred [T*B][C], 16-byte loads when C % 4 == 0; np.argmax's order (first maximum, a NaN beats
//     every number, the first NaN wins). The class ids are written transposed, raw[b][t], into the `decoded` part of the output.
//  2. er_line_kernel: one wavefront per line. The line's ids go to LDS, are decoded (blank = 0 dropped, repeats of the raw predecessor
//     dropped) and written back as decoded[b][:], then mapped to code points and white-space normalised in place. Both distances run on
//     one scheme: the reference string lies along the columns, lane l owns the CH consecutive columns l*CH+1 .. l*CH+CH in registers, and a
//     row of the table is
//         tmp[j] = min(prev[j] + 1, prev[j-1] + (ref[j] != hyp[i])),   D[i][j] = j + min over k <= j of (tmp[k] - k),   tmp[0] = i
//     i.e. a min-scan across the wavefront (register-to-register lane moves) in place of the textbook loop's left-to-right dependence. Words are compared as integers: a
//     reference word's id is the index of the first reference word with the same code points, a hypothesis word's id that of the first
//     equal reference word or ER_NO_WORD; a hash only filters in front of the full compare.
// No atomics, nothing crosses workgroups, plain vector stores only.
#include "hwg_common.h"
#include <limits.h>
#include <math.h>

constexpr int ER_MAX_T = 8192, ER_MAX_C = 1024, ER_MAX_REF = 2047;
constexpr int ER_MAX_REF_WORDS = (ER_MAX_REF + 1) / 2;      // words of at least one character, one space between them
constexpr int ER_ROW_LANES = 16;                            // lanes that share one row of pred
constexpr int ER_ARGMAX_BLOCK = 256;
constexpr int ER_ROWS_PER_BLOCK = ER_ARGMAX_BLOCK / ER_ROW_LANES;
constexpr int ER_SPACE = 32;
constexpr int ER_NO_WORD = -1;                              // a hypothesis word no reference word equals
constexpr int ER_PAD = -2;                                  // reference columns past the end: equal to nothing
constexpr int ER_STATS = 8;

// np.argmax's order as a strict "candidate (v, i) beats the holder (bv, bi)"
__device__ __forceinline__ bool er_beats(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (bn) return vn && i < bi;
  if (vn) return true;
  return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(ER_ARGMAX_BLOCK) void er_argmax_kernel(const float* __restrict__ pred, int T, int B, int C, int vec,
                                                                    int* __restrict__ raw) {
  const int sub = threadIdx.x & (ER_ROW_LANES - 1);
  const long long rows = (long long)T * B, stride = (long long)gridDim.x * ER_ROWS_PER_BLOCK;
  for (long long row = (long long)blockIdx.x * ER_ROWS_PER_BLOCK + threadIdx.x / ER_ROW_LANES; row < rows; row += stride) {
    const float* x = pred + row * C;
    float bv = -INFINITY;          // (-inf, INT_MAX) loses to every element, a -inf one included
    int bi = INT_MAX;
    if (vec) {
      for (int c = 4 * sub; c < C; c += 4 * ER_ROW_LANES) {
        const f32x4 v = *(const f32x4*)(x + c);
        if (er_beats(v.x, c, bv, bi)) { bv = v.x; bi = c; }
        if (er_beats(v.y, c + 1, bv, bi)) { bv = v.y; bi = c + 1; }
        if (er_beats(v.z, c + 2, bv, bi)) { bv = v.z; bi = c + 2; }
        if (er_beats(v.w, c + 3, bv, bi)) { bv = v.w; bi = c + 3; }
      }
    } else {
      for (int c = sub; c < C; c += ER_ROW_LANES) {
        const float v = x[c];
        if (er_beats(v, c, bv, bi)) { bv = v; bi = c; }
      }
    }
#pragma unroll
    for (int o = ER_ROW_LANES / 2; o > 0; o >>= 1) {      // the order is total, so every lane of the row ends with the same winner
      const float ov = __shfl_xor(bv, o, ER_ROW_LANES);
      const int oi = __shfl_xor(bi, o, ER_ROW_LANES);
      if (er_beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (sub == 0) raw[(row % B) * T + row / B] = bi;      // row = t * B + b
  }
}

__device__ __forceinline__ int er_rank(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// Cross-lane steps of a table row as data-parallel-primitive moves (register to register; a __shfl_up goes through the LDS crossbar, and a
// row is a chain of eight of them). All 64 lanes are active wherever these are called. A lane without a source keeps the first operand.
constexpr int ER_DPP_ROW_SHR = 0x110, ER_DPP_WAVE_SHR1 = 0x138, ER_DPP_ROW_BCAST15 = 0x142, ER_DPP_ROW_BCAST31 = 0x143;

// inclusive min-scan over the wavefront: shifts by 1, 2, 4, 8 inside each row of 16 lanes, then each row's last lane into the rows after it
__device__ __forceinline__ int er_wave_min_scan(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, ER_DPP_ROW_SHR | 1, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, ER_DPP_ROW_SHR | 2, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, ER_DPP_ROW_SHR | 4, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, ER_DPP_ROW_SHR | 8, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, ER_DPP_ROW_BCAST15, 0xa, 0xf, false));      // lane 15 -> row 1, lane 47 -> row 3
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, ER_DPP_ROW_BCAST31, 0xc, 0xf, false));      // lane 31 -> rows 2 and 3
  return v;
}

// lane l takes lane l - 1's value, lane 0 takes `first`
__device__ __forceinline__ int er_lane_shr1(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, ER_DPP_WAVE_SHR1, 0xf, 0xf, false); }

// Levenshtein distance between ref[0..n) (flat pointer: global or LDS) and hyp[0..m) (LDS), n <= 64 * CH; the same value in every lane
template <int CH>
__device__ __forceinline__ int er_lev_chunk(const int* ref, int n, const int* hyp, int m, int lane) {
  int rc[CH], prev[CH], tmp[CH];
  const int col0 = lane * CH + 1;                       // this lane's first column
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int j = col0 - 1 + c;
    rc[c] = j < n ? ref[j] : ER_PAD;
    prev[c] = col0 + c;                                 // D[0][j] = j
  }
  for (int i = 1; i <= m; ++i) {
    const int h = hyp[i - 1];
    int diag = er_lane_shr1(prev[CH - 1], i - 1);       // D[i-1][col0 - 1]; lane 0: D[i-1][0]
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int t = min(prev[c] + 1, diag + (rc[c] != h ? 1 : 0));
      diag = prev[c];
      tmp[c] = t - (col0 + c);
    }
#pragma unroll
    for (int c = 1; c < CH; ++c) tmp[c] = min(tmp[c], tmp[c - 1]);
    const int excl = min(er_lane_shr1(er_wave_min_scan(tmp[CH - 1]), INT_MAX), i);      // column 0: tmp[0] - 0 = i
#pragma unroll
    for (int c = 0; c < CH; ++c) prev[c] = min(tmp[c], excl) + (col0 + c);
  }
  int res = 0;
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (c == (n - 1) % CH) res = prev[c];
  return __shfl(res, (n - 1) / CH);
}

__device__ __forceinline__ int er_lev(const int* ref, int n, const int* hyp, int m, int lane) {
  if (n <= 0) return m;
  if (n <= 64) return er_lev_chunk<1>(ref, n, hyp, m, lane);
  if (n <= 128) return er_lev_chunk<2>(ref, n, hyp, m, lane);
  if (n <= 256) return er_lev_chunk<4>(ref, n, hyp, m, lane);
  if (n <= 512) return er_lev_chunk<8>(ref, n, hyp, m, lane);
  if (n <= 1024) return er_lev_chunk<16>(ref, n, hyp, m, lane);
  return er_lev_chunk<32>(ref, n, hyp, m, lane);        // n <= ER_MAX_REF
}

__device__ __forceinline__ unsigned er_hash_step(unsigned h, int code) { return (h ^ (unsigned)code) * 16777619u; }

// word starts of s[0..n) (a word starts where a non-space follows a space or the beginning) -> starts[0..cap), returns their number (<= cap)
__device__ __forceinline__ int er_word_starts(const int* s, int n, int* starts, int cap, int lane) {
  int nw = 0;
  for (int base = 0; base < n; base += HWG_WAVE) {
    const int p = base + lane;
    const bool start = p < n && s[p] != ER_SPACE && (p == 0 || s[p - 1] == ER_SPACE);
    const unsigned long long mask = __ballot(start);
    const int k = nw + er_rank(mask, lane);
    if (start && k < cap) starts[k] = p;
    nw += __popcll(mask);
  }
  return min(nw, cap);
}

__global__ __launch_bounds__(HWG_WAVE) void er_line_kernel(int T, int B, int C, const int* __restrict__ class_code,
                                                           const int* __restrict__ ref_codes, const int* __restrict__ ref_offsets,
                                                           int* __restrict__ out) {
  __shared__ int rword[ER_MAX_REF_WORDS];               // reference word k: start | length << 11 (both below 2048)
  __shared__ unsigned rhash[ER_MAX_REF_WORDS];
  __shared__ int rid[ER_MAX_REF_WORDS];
  extern __shared__ int er_dyn[];
  int* seq = er_dyn;                                    // [T] raw ids -> decoded ids -> normalised code points
  int* hword = er_dyn + T;                              // [(T + 1) / 2] hypothesis word starts -> ids
  const int b = blockIdx.x, lane = threadIdx.x;
  int* stats = out + (long long)ER_STATS * b;
  int* dec = out + (long long)ER_STATS * B + (long long)b * T;

  for (int t = lane; t < T; t += HWG_WAVE) seq[t] = dec[t];
  __syncthreads();

  // greedy CTC decode, compacted in place: a write never lands behind the position it was read from
  int nd = 0, last = 0;                                 // (a predecessor of 0 at t = 0 changes nothing: a 0 is dropped anyway)
  for (int base = 0; base < T; base += HWG_WAVE) {
    const int t = base + lane;
    const int v = t < T ? seq[t] : 0;
    int p = __shfl_up(v, 1);
    if (lane == 0) p = last;
    last = __shfl(v, HWG_WAVE - 1);
    const bool keep = t < T && v != 0 && v != p;
    const unsigned long long mask = __ballot(keep);
    __syncthreads();
    if (keep) seq[nd + er_rank(mask, lane)] = v;
    nd += __popcll(mask);
  }
  __syncthreads();
  for (int t = lane; t < T; t += HWG_WAVE) dec[t] = t < nd ? seq[t] : 0;

  // classes -> code points; " ".join(h.split()): a space after a space (or in front) is dropped, then one at the end
  int m = 0, prevcode = ER_SPACE;
  for (int base = 0; base < nd; base += HWG_WAVE) {
    const int p = base + lane;
    const int code = p < nd ? class_code[min(max(seq[p], 0), C - 1)] : ER_SPACE;
    int pc = __shfl_up(code, 1);
    if (lane == 0) pc = prevcode;
    prevcode = __shfl(code, HWG_WAVE - 1);
    const bool keep = p < nd && !(code == ER_SPACE && pc == ER_SPACE);
    const unsigned long long mask = __ballot(keep);
    __syncthreads();
    if (keep) seq[m + er_rank(mask, lane)] = code;
    m += __popcll(mask);
  }
  __syncthreads();
  if (m > 0 && seq[m - 1] == ER_SPACE) --m;

  const int off = ref_offsets[b];
  const int n = min(max(ref_offsets[b + 1] - off, 0), ER_MAX_REF);      // the caller validated the table; a bad entry still fits the LDS tables
  const int* ref = ref_codes + off;
  const int char_dist = er_lev(ref, n, seq, m, lane);

  // reference words: start, length, hash; then the id = first reference word with the same code points
  const int nrw = er_word_starts(ref, n, rword, ER_MAX_REF_WORDS, lane);
  __syncthreads();
  for (int k = lane; k < nrw; k += HWG_WAVE) {
    const int s = rword[k];
    int len = 0;
    unsigned h = 2166136261u;
    while (s + len < n && ref[s + len] != ER_SPACE) h = er_hash_step(h, ref[s + len++]);
    rword[k] = s | (len << 11);
    rhash[k] = h;
  }
  __syncthreads();
  for (int k = lane; k < nrw; k += HWG_WAVE) {
    const int s = rword[k] & 2047, len = rword[k] >> 11;
    int id = k;
    for (int q = 0; q < k; ++q) {
      if (rhash[q] != rhash[k] || (rword[q] >> 11) != len) continue;
      const int sq = rword[q] & 2047;
      int e = 0;
      while (e < len && ref[sq + e] == ref[s + e]) ++e;
      if (e == len) { id = q; break; }
    }
    rid[k] = id;
  }
  // hypothesis words: the id of the first equal reference word
  const int nhw = er_word_starts(seq, m, hword, (T + 1) / 2, lane);
  __syncthreads();
  for (int k = lane; k < nhw; k += HWG_WAVE) {
    const int s = hword[k];
    int len = 0;
    unsigned h = 2166136261u;
    while (s + len < m && seq[s + len] != ER_SPACE) h = er_hash_step(h, seq[s + len++]);
    int id = ER_NO_WORD;
    for (int q = 0; q < nrw; ++q) {
      if (rhash[q] != h || (rword[q] >> 11) != len) continue;
      const int sq = rword[q] & 2047;
      int e = 0;
      while (e < len && ref[sq + e] == seq[s + e]) ++e;
      if (e == len) { id = q; break; }                  // the first equal one is its own id
    }
    hword[k] = id;
  }
  __syncthreads();
  const int word_dist = er_lev(rid, nrw, hword, nhw, lane);

  if (lane < ER_STATS)
    stats[lane] = lane == 0 ? nd : lane == 1 ? char_dist : lane == 2 ? m : lane == 3 ? word_dist : lane == 4 ? nhw : 0;
}

extern "C" int hwg_ctc_error_rates(const float* pred, int T, int B, int C, const int* class_code, const int* ref_codes, const int* ref_offsets,
                                   int max_ref_len, int* out, void* stream) {
  HWG_REQUIRE(pred && class_code && ref_codes && ref_offsets && out, "ctc_error_rates: null argument");
  HWG_REQUIRE(T >= 1 && B >= 1 && C >= 2 && max_ref_len >= 0, "ctc_error_rates: bad sizes T=%d B=%d C=%d max_ref_len=%d", T, B, C, max_ref_len);
  HWG_REQUIRE(T <= ER_MAX_T && C <= ER_MAX_C && max_ref_len <= ER_MAX_REF,
              "ctc_error_rates: beyond the limit T=%d (<= %d) C=%d (<= %d) longest reference %d (<= %d)", T, ER_MAX_T, C, ER_MAX_C, max_ref_len,
              ER_MAX_REF);
  HWG_REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)out & 3) == 0, "ctc_error_rates: pred and out must be 4-byte aligned");
  const int vec = C % 4 == 0 && ((uintptr_t)pred & 15) == 0;
  const long long rows = (long long)T * B;
  const long long blocks = (rows + ER_ROWS_PER_BLOCK - 1) / ER_ROWS_PER_BLOCK;
  const int grid = (int)(blocks < 65536 ? blocks : 65536);
  hipLaunchKernelGGL(er_argmax_kernel, dim3(grid), dim3(ER_ARGMAX_BLOCK), 0, (hipStream_t)stream, pred, T, B, C, vec,
                     out + (long long)ER_STATS * B);
  HWG_LAUNCH_CHECK("ctc_error_rates argmax");
  const size_t lds = sizeof(int) * ((size_t)T + (size_t)(T + 1) / 2);
  hipLaunchKernelGGL(er_line_kernel, dim3(B), dim3(HWG_WAVE), lds, (hipStream_t)stream, T, B, C, class_code, ref_codes, ref_offsets, out);
  HWG_LAUNCH_CHECK("ctc_error_rates lines");
  return HWG_OK;
}
