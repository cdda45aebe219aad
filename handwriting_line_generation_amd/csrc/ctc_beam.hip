// CTC prefix beam search on the device: the decoder that sums the alignments of a text, in front of the unchanged er_line_kernel of
// error_rate.hip, so that CER / WER of the beam text come out of the same counting code as the greedy ones.
//
// pred [T][B][C] fp32 is read as log-probabilities as they stand (class 0 the blank, a NaN as -inf). One workgroup of 256 lanes per line,
// the frame loop inside the kernel; nothing crosses a workgroup. Per line:
//   beam (LDS)   at most K slots, kept sorted best first: node, pb, pnb, tot = pb (+) pnb, last class, length, parent node and the slot the
//                parent holds in this beam (-1: not in it). (+) is log-add-exp, max + log1pf(expf(min - max)), symmetric in its operands.
//   nodes (ws)   the prefixes as a trie, node = (parent, class); node 0 is the empty prefix. Nodes are CANONICAL: a (parent, class) -> node
//                open-addressing table in the workspace, never deleted from and touched by this workgroup alone, is asked before a node
//                is made, so one string has one node for the whole line and "same prefix" is "same node" - decided on the full
//                (parent, class) key, the hash only picks the first slot to probe. A prefix that left the beam and comes back gets its old
//                node, whose children (still in the beam, maybe) keep pointing at it. At most K new nodes per frame: K * T + 1 in all.
// A frame: the row lp[t] goes to LDS; slot m's "stay" entry takes pb = lp[0] + tot(m) and pnb = lp[last] + pnb(m), (+) the extension of
// its parent by its last class when the parent sits in the beam (the only other contribution a beam prefix can get: a string has one
// parent). Candidate (j, c) - c = 0: slot j's stay entry, c >= 1: slot j extended by c, -inf where that extension was merged into a stay
// entry - has the index j * C + c. Every candidate's total is computed once per frame into LDS ([K][C] ordered words, up to 128 KiB of
// dynamic LDS: with every round recomputing its owner's candidates a frame took 76 us at K = 16, C = 80, with this 27 us); a key is
// that word above INT_MAX - index, 0 for no candidate. The new beam is drawn by K rounds of a workgroup-wide maximum over the keys (tot, smaller index first):
// TIE RULE: of exactly equal totals the candidate of the earlier beam slot wins, within a slot the stay entry, then the smaller class.
// An entry whose total is -inf (or NaN, which only +inf inputs can make) never enters. Every sum has a fixed order, a line reads and
// writes its own rows only: the same bits whatever B and the neighbours are.
// At the end the totals go to scores [B][K] (descending, -inf padded) and the best prefix to decoded[b] as its shortest CTC path - the
// classes with one blank between equal neighbours, zero padded to T -, which er_line_kernel's greedy collapse turns back into exactly
// the prefix. A prefix with a finite total has an alignment of T frames, so the path fits; the writes are bounded by T all the same.
// Barriers: every __syncthreads() is reached by all 256 lanes; trip counts depend on T, C, K and on LDS values all lanes read alike.
// Probe loops are bounded by the table's size, the chain walk by the prefix's length. No floating-point atomics; the one atomic is the
// 64-bit integer compare-and-swap that claims a table slot.
#include "hwg_common.h"
#include <limits.h>
#include <math.h>

constexpr int CB_MAX_BEAM = 32, CB_MAX_T = 2048, CB_MAX_C = 1024, CB_MAX_REF = 2047;      // CB_MAX_REF: the reference limit of er_line_kernel
constexpr int CB_BLOCK = 256, CB_WAVES = CB_BLOCK / HWG_WAVE;
constexpr int CB_STATS = 8;                                                             // error_rate.hip's ER_STATS
constexpr int CB_MASK_WORDS = CB_MAX_C / 32;
constexpr int CB_SCAN = 8;
constexpr unsigned long long CB_EMPTY = ~0ull;

// defined in error_rate.hip: greedy collapse, normalisation, both Levenshtein distances, the stats (one wavefront per line)
__global__ __launch_bounds__(HWG_WAVE) void er_line_kernel(int T, int B, int C, const int* __restrict__ class_code,
                                                           const int* __restrict__ ref_codes, const int* __restrict__ ref_offsets,
                                                           int* __restrict__ out);

static inline long long cb_nodes(int T, int beam) { return (long long)T * beam + 1; }
static inline long long cb_table_slots(int T, int beam) {
  long long cap = 4;
  while (cap < 2 * cb_nodes(T, beam)) cap <<= 1;       // load factor below 1/2, a power of two
  return cap;
}
static inline long long cb_line_words(int T, int beam) { return cb_table_slots(T, beam) + cb_nodes(T, beam); }      // 8-byte words

__device__ __forceinline__ float cb_lse(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (!(lo > -INFINITY)) return (a != a || b != b) ? NAN : hi;      // -inf is the neutral element
  return hi + log1pf(expf(lo - hi));
}

// a total as the upper half of a key: larger total, larger word; totals that never enter (-inf, NaN) have no key
__device__ __forceinline__ unsigned cb_order(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cb_unorder(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// maximum over the wavefront, the same value in every lane: data-parallel-primitive moves as in error_rate.hip (register to register; the
// shuffle spelling goes through the LDS crossbar, and a frame does 2 K of these). All 64 lanes are active wherever it is called.
__device__ __forceinline__ unsigned cb_wave_max(unsigned x) {
  int v = (int)(x ^ 0x80000000u);                                // unsigned order as signed order; INT_MIN is the identity
  v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x111, 0xf, 0xf, false));      // row_shr 1, 2, 4, 8
  v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x112, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x114, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x118, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x142, 0xa, 0xf, false));      // row_bcast15: lane 15 -> row 1, lane 47 -> row 3
  v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x143, 0xc, 0xf, false));      // row_bcast31: lane 31 -> rows 2 and 3
  return (unsigned)__builtin_amdgcn_readlane(v, HWG_WAVE - 1) ^ 0x80000000u;        // lane 63 holds the inclusive scan's end
}

__device__ __forceinline__ unsigned cb_hash(unsigned key, unsigned mask) {
  unsigned h = key * 2654435761u;
  return (h ^ (h >> 15)) & mask;
}

__global__ __launch_bounds__(CB_BLOCK) void cb_beam_kernel(const float* __restrict__ pred, int T, int B, int C, int K, int vec, long long nn,
                                                           unsigned cap, unsigned long long* __restrict__ ws, float* __restrict__ scores,
                                                           int* __restrict__ out) {
  __shared__ float row[CB_MAX_C];
  __shared__ unsigned merged[CB_MAX_BEAM * CB_MASK_WORDS];      // bit c of slot j: the extension (j, c) was added to a stay entry
  __shared__ int path[CB_MAX_T];
  __shared__ int b_node[CB_MAX_BEAM], b_last[CB_MAX_BEAM], b_len[CB_MAX_BEAM], b_par[CB_MAX_BEAM], b_pslot[CB_MAX_BEAM];
  __shared__ float b_pb[CB_MAX_BEAM], b_pnb[CB_MAX_BEAM], b_tot[CB_MAX_BEAM];
  __shared__ float s_pb[CB_MAX_BEAM], s_pnb[CB_MAX_BEAM], s_tot[CB_MAX_BEAM];      // the stay entries of this frame
  __shared__ unsigned long long sel[CB_MAX_BEAM], wbest[2][CB_WAVES];
  __shared__ int s_n, s_nodes;
  extern __shared__ unsigned cand[];                             // [K][C] this frame's candidate totals as ordered words

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (HWG_WAVE - 1), wave = tid / HWG_WAVE;
  unsigned long long* table = ws + (long long)b * ((long long)cap + nn);
  unsigned long long* nodes = table + cap;                       // node i: parent | class << 32
  const int mwords = (C + 31) / 32;

  for (unsigned i = tid; i < cap; i += CB_BLOCK) table[i] = CB_EMPTY;
  if (tid == 0) {
    nodes[0] = 0ull;
    b_node[0] = 0; b_last[0] = 0; b_len[0] = 0; b_par[0] = -1; b_pslot[0] = -1;
    b_pb[0] = 0.f; b_pnb[0] = -INFINITY; b_tot[0] = 0.f;
    s_n = 1; s_nodes = 1;
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const int n = s_n;                                           // the same in every lane: written before the last barrier
    const float* x = pred + ((long long)t * B + b) * C;
    if (vec) {
      for (int c = 4 * tid; c < C; c += 4 * CB_BLOCK) {
        const f32x4 v = *(const f32x4*)(x + c);
        row[c] = v.x == v.x ? v.x : -INFINITY;
        row[c + 1] = v.y == v.y ? v.y : -INFINITY;
        row[c + 2] = v.z == v.z ? v.z : -INFINITY;
        row[c + 3] = v.w == v.w ? v.w : -INFINITY;
      }
    } else {
      for (int c = tid; c < C; c += CB_BLOCK) {
        const float v = x[c];
        row[c] = v == v ? v : -INFINITY;
      }
    }
    for (int i = tid; i < n * mwords; i += CB_BLOCK) merged[(i / mwords) * CB_MASK_WORDS + i % mwords] = 0u;
    __syncthreads();

    if (tid < n) {                                               // stay entries
      const int m = tid, c = b_last[m], j = b_pslot[m];
      float pnb = c ? row[c] + b_pnb[m] : -INFINITY;
      if (j >= 0) {                                              // the parent is in the beam: its extension by c is this prefix
        pnb = cb_lse(pnb, row[c] + (c == b_last[j] ? b_pb[j] : b_tot[j]));
        atomicOr(&merged[j * CB_MASK_WORDS + (c >> 5)], 1u << (c & 31));
      }
      const float pb = row[0] + b_tot[m];
      s_pb[m] = pb; s_pnb[m] = pnb; s_tot[m] = cb_lse(pb, pnb);
    }
    __syncthreads();

    // every candidate's total, once, as its ordered word (0: none): lane `tid` owns the classes tid, tid + 256, ... of every slot and is
    // the only one to read them again
    for (int c = tid; c < C; c += CB_BLOCK) {
      const float lpc = row[c];
#pragma unroll 4
      for (int j = 0; j < n; ++j) {
        const float stay = s_tot[j], ext = lpc + (c == b_last[j] ? b_pb[j] : b_tot[j]);
        const bool gone = (merged[j * CB_MASK_WORDS + (c >> 5)] >> (c & 31)) & 1u;
        const float v = c == 0 ? stay : gone ? -INFINITY : ext;
        cand[j * C + c] = v > -INFINITY ? cb_order(v) : 0u;
      }
    }
    // K rounds: every lane offers the best of its candidates below `limit`, the workgroup's maximum is drawn, its owner moves on
    unsigned long long limit = CB_EMPTY, mine = 0ull;
    bool rescan = true;
    int nsel = 0;
    for (int r = 0; r < K; ++r) {
      if (rescan) {
        mine = 0ull;
        for (int c = tid; c < C; c += CB_BLOCK)
          for (int j0 = 0; j0 < n; j0 += CB_SCAN) {              // CB_SCAN independent LDS reads in flight: the round is a latency chain
            unsigned o[CB_SCAN];
#pragma unroll
            for (int u = 0; u < CB_SCAN; ++u) o[u] = j0 + u < n ? cand[(j0 + u) * C + c] : 0u;
#pragma unroll
            for (int u = 0; u < CB_SCAN; ++u) {
              const unsigned long long k = o[u] ? ((unsigned long long)o[u] << 32) | (unsigned)(INT_MAX - ((j0 + u) * C + c)) : 0ull;
              if (k < limit && k > mine) mine = k;
            }
          }
        rescan = false;
      }
      // the wavefront's largest total, then the smallest index among the lanes that hold it
      const unsigned top = cb_wave_max((unsigned)(mine >> 32));
      const unsigned low = cb_wave_max((unsigned)(mine >> 32) == top ? (unsigned)(mine & 0xffffffffull) : 0u);
      unsigned long long best = ((unsigned long long)top << 32) | low;
      if (lane == 0) wbest[r & 1][wave] = best;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < CB_WAVES; ++w) best = wbest[r & 1][w] > best ? wbest[r & 1][w] : best;
      if (best == 0ull) break;                                   // nothing finite is left: the same answer in every lane
      if (tid == 0) sel[r] = best;
      if (mine == best) { limit = best; rescan = true; }         // keys are distinct: exactly one owner
      nsel = r + 1;
    }
    __syncthreads();

    // the new beam, slot r = the r-th draw (best first); lanes 0 .. nsel-1 of wavefront 0
    int node = -1, last = 0, len = 0, par = -1;
    float pb = -INFINITY, pnb = -INFINITY, tot = -INFINITY;
    unsigned key = 0;
    bool make = false;
    if (tid < nsel) {
      const unsigned long long k = sel[tid];
      const int index = INT_MAX - (int)(unsigned)(k & 0xffffffffull);
      const int j = min(max(index / C, 0), n - 1), c = index % C;
      tot = cb_unorder((unsigned)(k >> 32));
      if (c == 0) {
        node = b_node[j]; last = b_last[j]; len = b_len[j]; par = b_par[j];
        pb = s_pb[j]; pnb = s_pnb[j];
      } else {
        last = c; len = b_len[j] + 1; par = b_node[j];
        pnb = tot;
        key = ((unsigned)par << 10) | (unsigned)c;               // par <= 65536, c < 1024
        unsigned slot = cb_hash(key, cap - 1);
        make = true;
        for (unsigned probe = 0; probe < cap; ++probe) {
          const unsigned long long e = table[slot];
          if (e == CB_EMPTY) break;
          if ((unsigned)(e >> 32) == key) { node = (int)(unsigned)(e & 0xffffffffull); make = false; break; }
          slot = (slot + 1) & (cap - 1);
        }
      }
    }
    unsigned long long makers = 0ull;                            // wavefront 0: the lanes whose prefix has no node yet
    if (wave == 0) {
      makers = __ballot(make);
      if (make) {
        node = s_nodes + __popcll(makers & ((1ull << lane) - 1ull));
        if (node < nn) {
          nodes[node] = (unsigned long long)(unsigned)par | ((unsigned long long)(unsigned)last << 32);
          const unsigned long long e = ((unsigned long long)key << 32) | (unsigned)node;
          unsigned slot = cb_hash(key, cap - 1);
          for (unsigned probe = 0; probe < cap; ++probe) {
            if (atomicCAS(&table[slot], CB_EMPTY, e) == CB_EMPTY) break;
            slot = (slot + 1) & (cap - 1);
          }
        } else {
          node = 0;                                              // cannot happen (K new nodes per frame at most); stays inside the buffers
        }
      }
    }
    __syncthreads();                                             // the old beam has been read by every lane
    if (tid < nsel) {
      b_node[tid] = node; b_last[tid] = last; b_len[tid] = len; b_par[tid] = par;
      b_pb[tid] = pb; b_pnb[tid] = pnb; b_tot[tid] = tot;
    }
    if (tid == 0) {
      s_n = nsel;
      s_nodes = (int)min((long long)s_nodes + __popcll(makers), nn);
    }
    __syncthreads();
    if (tid < nsel) {
      int ps = -1;
      for (int q = 0; q < nsel; ++q)
        if (b_node[q] == par) ps = q;
      b_pslot[tid] = ps;
    }
    __syncthreads();
  }

  // scores, and the best prefix as its shortest CTC path
  const int n = s_n;
  for (int k = tid; k < K; k += CB_BLOCK) scores[(long long)b * K + k] = k < n ? b_tot[k] : -INFINITY;
  for (int i = tid; i < T; i += CB_BLOCK) path[i] = 0;
  __syncthreads();
  if (tid == 0 && n > 0) {
    const int len = min(b_len[0], T);
    int equal = 0, nd = b_node[0], prev = -1;
    for (int i = len - 1; i >= 0 && nd > 0 && nd < nn; --i) {    // classes, last first, into the upper end
      const unsigned long long e = nodes[nd];
      const int c = (int)(unsigned)(e >> 32);
      path[T - len + i] = c;
      equal += c == prev;
      prev = c;
      nd = (int)(unsigned)(e & 0xffffffffull);
    }
    if (len + equal <= T) {                                      // always, for a prefix with a finite total
      int pos = 0;
      prev = -1;
      for (int i = 0; i < len; ++i) {                            // pos <= T - len + i: a write never passes the position still to be read
        const int c = path[T - len + i];
        if (c == prev) path[pos++] = 0;
        path[pos++] = c;
        prev = c;
      }
      for (; pos < T; ++pos) path[pos] = 0;
    } else {
      for (int i = 0; i < T; ++i) path[i] = 0;
    }
  }
  __syncthreads();
  int* dec = out + (long long)CB_STATS * B + (long long)b * T;
  for (int i = tid; i < T; i += CB_BLOCK) dec[i] = path[i];
}

extern "C" size_t hwg_ctc_beam_workspace(int T, int B, int C, int beam) {
  if (T < 1 || B < 1 || C < 2 || beam < 1 || T > CB_MAX_T || C > CB_MAX_C || beam > CB_MAX_BEAM) return 0;
  return (size_t)B * (size_t)cb_line_words(T, beam) * sizeof(unsigned long long);
}

extern "C" int hwg_ctc_beam_error_rates(const float* pred, int T, int B, int C, int beam, const int* class_code, const int* ref_codes,
                                        const int* ref_offsets, int max_ref_len, int* out, float* scores, void* ws, size_t ws_bytes,
                                        void* stream) {
  HWG_REQUIRE(pred && class_code && ref_codes && ref_offsets && out && scores, "ctc_beam_error_rates: null argument");
  HWG_REQUIRE(T >= 1 && B >= 1 && C >= 2 && max_ref_len >= 0, "ctc_beam_error_rates: bad sizes T=%d B=%d C=%d max_ref_len=%d", T, B, C,
              max_ref_len);
  HWG_REQUIRE(beam >= 1 && beam <= CB_MAX_BEAM && T <= CB_MAX_T && C <= CB_MAX_C && max_ref_len <= CB_MAX_REF,
              "ctc_beam_error_rates: beyond the limit beam=%d (1 .. %d) T=%d (<= %d) C=%d (<= %d) longest reference %d (<= %d)", beam,
              CB_MAX_BEAM, T, CB_MAX_T, C, CB_MAX_C, max_ref_len, CB_MAX_REF);
  HWG_REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)ws & 7) == 0,
              "ctc_beam_error_rates: pred, out and scores must be 4-byte aligned, the workspace 8-byte aligned");
  if (!ws || ws_bytes < hwg_ctc_beam_workspace(T, B, C, beam)) {
    hwg_set_error("ctc_beam_error_rates: workspace too small");
    return HWG_ERR_WORKSPACE;
  }
  const int vec = C % 4 == 0 && ((uintptr_t)pred & 15) == 0;
  const size_t cand_bytes = sizeof(unsigned) * (size_t)beam * (size_t)C;         // at most 128 KiB next to 18 KiB of static LDS
  if (cand_bytes > 32768) {      // beyond 64 KiB with the static part a kernel's LDS has to be asked for (per device: asked on every such call)
    if (hipFuncSetAttribute((const void*)cb_beam_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(unsigned) * CB_MAX_BEAM * CB_MAX_C)) != hipSuccess) {
      (void)hipGetLastError();
      hwg_set_error("ctc_beam_error_rates: the device refuses %d bytes of LDS per workgroup", (int)(sizeof(unsigned) * CB_MAX_BEAM * CB_MAX_C));
      return HWG_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(cb_beam_kernel, dim3(B), dim3(CB_BLOCK), cand_bytes, (hipStream_t)stream, pred, T, B, C, beam, vec, cb_nodes(T, beam),
                     (unsigned)cb_table_slots(T, beam), (unsigned long long*)ws, scores, out);
  HWG_LAUNCH_CHECK("ctc_beam_error_rates beam");
  const size_t lds = sizeof(int) * ((size_t)T + (size_t)(T + 1) / 2);
  hipLaunchKernelGGL(er_line_kernel, dim3(B), dim3(HWG_WAVE), lds, (hipStream_t)stream, T, B, C, class_code, ref_codes, ref_offsets, out);
  HWG_LAUNCH_CHECK("ctc_beam_error_rates lines");
  return HWG_OK;
}
