// One bidirectional LSTM layer (the CRNN recogniser's recurrence; reference: torch.nn.LSTM inside model/cnn_lstm.py:14), forward and backward.
//
// Schedule: ONE LAUNCH PER TIME STEP, both directions in it (gridDim.y = 2; the reverse direction walks t downwards). Step t needs every
// workgroup's h_{t-1}; the kernel boundary is the only thing that orders them - no flags, counters, atomics, spin-waits or grid barriers,
// plain vector stores only. The step loop lives in the entry points below, so T launches cost one call from Python.
//
// Tiling: a workgroup (4 wavefronts) owns LSTM_UNITS = 4 hidden units - all four gate rows of them - for every line of the batch chunk, and
// blockIdx.x -> units is the same function in every launch (a slice of W_hh stays in the same XCD's L2 from step to step). h_{t-1} (forward) or
// one gate block of dgates[t+-1] (backward) is staged in LDS as [lines][H]; a batch wider than the LDS image is walked in chunks of
// lstm_chunk(H) lines (the recurrence is independent per line, so chunking changes no bits).
//
// Gate order and arithmetic are torch's: (i, f, g, o) = split(xproj[t] + b_hh + h_{t-1} W_hh^T), c_t = sig(f) c_{t-1} + sig(i) tanh(g),
// h_t = sig(o) tanh(c_t), h_{-1} = c_{-1} = 0, with the accurate expf / tanhf.
//
// SUMMATION ORDER (fixed: depends on H alone, never on B, T, the direction or the grid). The dot product of one (line, unit, gate) over
// k = 0 .. H-1 is split over 16 lanes; lane s sums its elements k = 64 j + 4 s + i in the order j = 0 .. ceil(H/64)-1 (outer), i = 0 .. 3
// (inner) as one fmaf chain starting from +0 (a lane whose k would be >= H keeps +0); the 16 partial sums are then added pairwise
// by a butterfly over the lane distances 1, 2, 4, 8 (v = v + v[s ^ 1]; v = v + v[s ^ 2]; ...). The pre-activation is
// (xproj + b_hh) + that sum; at the first step of a direction (h = 0) the sum is +0. The backward product dh_rec = dgates[t+-1] W_hh is summed
// the same way with k running over one gate block at a time, the four blocks (i, f, g, o) outermost.
#include "hwg_common.h"

namespace {

constexpr int LSTM_UNITS = 4;            // hidden units per workgroup = wavefronts per workgroup
constexpr int LSTM_MAX_CHUNK = 32;       // lines per LDS image (two kept sums per lane in the forward kernel, eight accumulators in the backward kernel)
constexpr int LSTM_LDS_FLOATS = 16384;   // 64 KB

static inline int lstm_chunk(int H) {
  int c = LSTM_LDS_FLOATS / H;
  return c > LSTM_MAX_CHUNK ? LSTM_MAX_CHUNK : c;
}

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <int CTRL>
__device__ __forceinline__ float lstm_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// Butterfly over the 16 lanes that share lane >> 4 (one DPP row), in registers: quad_perm [1,0,3,2], quad_perm [2,3,0,1], then row_half_mirror
// and row_mirror. After the first two steps the four lanes of a quad hold the same value, after the third the eight lanes of a half row do, so
// the mirrored lane (7 - s, 15 - s) holds exactly what lane s ^ 4 (s ^ 8) holds: the sums are those of the xor butterfly 1, 2, 4, 8.
__device__ __forceinline__ float lstm_group_sum(float v) {
  v += lstm_dpp<0xB1>(v);
  v += lstm_dpp<0x4E>(v);
  v += lstm_dpp<0x141>(v);
  v += lstm_dpp<0x140>(v);
  return v;
}

// wavefront = unit, lane >> 4 = gate, lane & 15 = slice of k
template <int NJ>
__global__ __launch_bounds__(256) void lstm_fwd_step_kernel(const float* __restrict__ xp_f, const float* __restrict__ xp_r,
                                                            const float* __restrict__ w_f, const float* __restrict__ w_r,
                                                            const float* __restrict__ b_f, const float* __restrict__ b_r, float* __restrict__ y,
                                                            float* __restrict__ gates, float* __restrict__ cbuf, float* __restrict__ hseq, int T, int B, int H,
                                                            int b0, int nb, int step, int training) {
  extern __shared__ float4 lds4[];       // [nb][H / 4]: h_{t-1} of the chunk's lines
  const int d = blockIdx.y;
  const int t = d ? T - 1 - step : step;
  const int tp = d ? t + 1 : t - 1;      // the neighbouring time row holding h_{t-1} (valid when step > 0)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, s = lane & 15;
  const int u = blockIdx.x * LSTM_UNITS + wave;
  const int H4 = H >> 2;
  const float* xp = d ? xp_r : xp_f;
  const float* w = d ? w_r : w_f;
  const float* bias = d ? b_r : b_f;

  const size_t BH = (size_t)B * H;
  float* cw = training ? cbuf + ((size_t)d * T + t) * BH : cbuf + ((size_t)(step & 1) * 2 + d) * BH;
  const float* cr = cw;                  // c_{t-1}: there is none at a direction's first step (tp is out of range then), and it is not read
  if (step > 0) cr = training ? cbuf + ((size_t)d * T + tp) * BH : cbuf + ((size_t)((step + 1) & 1) * 2 + d) * BH;
  // what the gate arithmetic at the end reads is asked for first, so that it travels while h is staged and the products run
  float xb[2] = {0.f, 0.f}, cpv[2] = {0.f, 0.f};
  {
    const float bq = bias[q * H + u];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (16 * kk < nb) {
        const int b = s + 16 * kk;
        const int bb = b0 + (b < nb ? b : nb - 1);
        xb[kk] = xp[((size_t)t * B + bb) * 4 * H + (size_t)q * H + u] + bq;
        if (step > 0) cpv[kk] = cr[(size_t)bb * H + u];
      }
    }
  }
  float k0 = 0.f, k1 = 0.f;              // the dot products of lines s and s + 16 (this lane's gate, this wavefront's unit)
  if (step > 0) {
    for (int idx = tid; idx < nb * H4; idx += 256) {
      const int b = idx / H4, k4 = idx - b * H4;
      lds4[idx] = *reinterpret_cast<const float4*>(y + ((size_t)tp * B + b0 + b) * 2 * H + (size_t)d * H + 4 * k4);
    }
    float4 wr[NJ];
    const float* wrow = w + ((size_t)q * H + u) * H;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int k = 64 * j + 4 * s;
      wr[j] = k < H ? *reinterpret_cast<const float4*>(wrow + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    // four lines per pass: four independent fmaf chains (one wavefront per SIMD here, so the overlap has to come from inside the wavefront);
    // every line's own chain is the documented one. A pass's lines past the chunk re-read its last line and are dropped.
    for (int b = 0; b < nb; b += 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      int row[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) row[i] = (b + i < nb ? b + i : nb - 1) * H4;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k4 = 16 * j + s;
        if (k4 < H4) {
          float4 hv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) hv[i] = lds4[row[i] + k4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[i] = fmaf(wr[j].x, hv[i].x, acc[i]);
            acc[i] = fmaf(wr[j].y, hv[i].y, acc[i]);
            acc[i] = fmaf(wr[j].z, hv[i].z, acc[i]);
            acc[i] = fmaf(wr[j].w, hv[i].w, acc[i]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = lstm_group_sum(acc[i]);
        if (b + i < nb && s == ((b + i) & 15)) {
          if (b + i < 16) k0 = v; else k1 = v;
        }
      }
    }
  }
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int b = s + 16 * kk;
    if (16 * kk >= nb) break;            // uniform over the workgroup
    const bool live = b < nb;
    const int bb = b0 + (live ? b : nb - 1);
    const float pre = xb[kk] + (kk ? k1 : k0);
    const float a = q == 2 ? tanhf(pre) : lstm_sigmoid(pre);
    const float gi = __shfl(a, s, 64), gf = __shfl(a, 16 + s, 64), gg = __shfl(a, 32 + s, 64), go = __shfl(a, 48 + s, 64);
    if (!live) continue;
    if (training) gates[(((size_t)d * T + t) * B + bb) * 4 * H + (size_t)q * H + u] = a;
    if (q == 0) {
      const float cp = cpv[kk];
      const float c = gf * cp + gi * gg;
      const float h = go * tanhf(c);
      cw[(size_t)bb * H + u] = c;
      y[((size_t)t * B + bb) * 2 * H + (size_t)d * H + u] = h;
      if (training) {
        // h_prev rows of the weight gradient's GEMM: hseq[0][t + 1] = h_t with hseq[0][0] = 0; hseq[1][t] = h_t with hseq[1][T] = 0
        float* hs = hseq + (size_t)d * (T + 1) * BH;
        hs[((size_t)(d ? t : t + 1)) * BH + (size_t)bb * H + u] = h;
        if (step == 0) hs[((size_t)(d ? T : 0)) * BH + (size_t)bb * H + u] = 0.f;
      }
    }
  }
}

// wavefront w = lines w, w + 4, ... of the chunk; lane >> 4 = unit, lane & 15 = slice of k
template <int NJ>
__global__ __launch_bounds__(256) void lstm_bwd_step_kernel(const float* __restrict__ dy, const float* __restrict__ gates, const float* __restrict__ cseq,
                                                            const float* __restrict__ wt, float* __restrict__ dgates, float* __restrict__ dcbuf, int T, int B,
                                                            int H, int b0, int nb, int step) {
  extern __shared__ float4 lds4[];       // [nb][H / 4]: one gate block of dgates[t+-1] of the chunk's lines
  const int d = blockIdx.y;
  const int t = d ? step : T - 1 - step;
  const int tn = d ? t - 1 : t + 1;      // the time row the previous launch finished (valid when step > 0)
  const int tp = d ? t + 1 : t - 1;      // the row of c_{t-1} (valid unless this is the direction's first forward step)
  const bool has_prev = d ? (t < T - 1) : (t > 0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, s = lane & 15;
  const int u = blockIdx.x * LSTM_UNITS + q;
  const int H4 = H >> 2;
  const size_t BH = (size_t)B * H;

  // the lane that does the gate backward of (line wave + 4 s, unit u) asks for what it reads there first: it travels while dgates[t+-1] is
  // staged and the products run
  const int bl = wave + 4 * s;
  const bool own = s < LSTM_MAX_CHUNK / 4 && bl < nb;
  const int bb = b0 + (own ? bl : 0);
  float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, c = 0.f, cp = 0.f, dyv = 0.f, dcn = 0.f;
  if (own) {
    const float* g = gates + (((size_t)d * T + t) * B + bb) * 4 * H + u;
    gi = g[0]; gf = g[H]; gg = g[2 * (size_t)H]; go = g[3 * (size_t)H];
    c = cseq[((size_t)d * T + t) * BH + (size_t)bb * H + u];
    if (has_prev) cp = cseq[((size_t)d * T + tp) * BH + (size_t)bb * H + u];
    dyv = dy[((size_t)t * B + bb) * 2 * H + (size_t)d * H + u];
    if (step > 0) dcn = dcbuf[((size_t)((step + 1) & 1) * 2 + d) * BH + (size_t)bb * H + u];
  }

  float acc[LSTM_MAX_CHUNK / 4];
#pragma unroll
  for (int i = 0; i < LSTM_MAX_CHUNK / 4; ++i) acc[i] = 0.f;
  if (step > 0) {
    const float* dgn = dgates + (((size_t)d * T + tn) * B + b0) * 4 * H;
    const float* wrow = wt + ((size_t)d * H + u) * 4 * H;
    for (int gblk = 0; gblk < 4; ++gblk) {
      __syncthreads();
      for (int idx = tid; idx < nb * H4; idx += 256) {
        const int b = idx / H4, k4 = idx - b * H4;
        lds4[idx] = *reinterpret_cast<const float4*>(dgn + (size_t)b * 4 * H + (size_t)gblk * H + 4 * k4);
      }
      float4 wr[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + 4 * s;
        wr[j] = k < H ? *reinterpret_cast<const float4*>(wrow + (size_t)gblk * H + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      __syncthreads();
      // this wavefront's lines in two passes of four (lines wave + 4 bi): four independent fmaf chains per pass, lines past the chunk re-read
      // the chunk's last line and are dropped below
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (wave + 16 * half < nb) {     // uniform over the wavefront
          float4 gv[4];
          int row[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = wave + 4 * (4 * half + i);
            row[i] = (b < nb ? b : nb - 1) * H4;
          }
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int k4 = 16 * j + s;
            if (k4 < H4) {
#pragma unroll
              for (int i = 0; i < 4; ++i) gv[i] = lds4[row[i] + k4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                float a = acc[4 * half + i];
                a = fmaf(wr[j].x, gv[i].x, a);
                a = fmaf(wr[j].y, gv[i].y, a);
                a = fmaf(wr[j].z, gv[i].z, a);
                a = fmaf(wr[j].w, gv[i].w, a);
                acc[4 * half + i] = a;
              }
            }
          }
        }
      }
    }
  }
  float dh_rec = 0.f;
#pragma unroll
  for (int bi = 0; bi < LSTM_MAX_CHUNK / 4; ++bi) {
    if (wave + 4 * bi < nb) {            // uniform over the wavefront
      const float v = lstm_group_sum(acc[bi]);
      if (s == bi) dh_rec = v;
    }
  }
  if (own) {
    float* dcw = dcbuf + ((size_t)(step & 1) * 2 + d) * BH;
    const float dh = dyv + dh_rec;
    const float tc = tanhf(c);
    const float dc = dcn + dh * go * (1.f - tc * tc);
    float* dg = dgates + (((size_t)d * T + t) * B + bb) * 4 * H + u;
    dg[0] = dc * gg * gi * (1.f - gi);
    dg[H] = dc * cp * gf * (1.f - gf);
    dg[2 * (size_t)H] = dc * gi * (1.f - gg * gg);
    dg[3 * (size_t)H] = dh * tc * go * (1.f - go);
    dcw[(size_t)bb * H + u] = dc * gf;
  }
}

// wt[d][k][r] = w_d[r][k]: the [2][H][4H] image the backward kernel reads (32 x 32 tiles through LDS, both sides coalesced)
__global__ __launch_bounds__(256) void lstm_pack_whh_kernel(const float* __restrict__ w_f, const float* __restrict__ w_r, float* __restrict__ wt, int H) {
  __shared__ float tile[32][33];
  const int d = blockIdx.z;
  const float* w = d ? w_r : w_f;
  const int r0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, k = k0 + tx;
    tile[i][tx] = (r < 4 * H && k < H) ? w[(size_t)r * H + k] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int k = k0 + i, r = r0 + tx;
    if (k < H && r < 4 * H) wt[((size_t)d * H + k) * 4 * H + r] = tile[tx][i];
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int NJ>
int lstm_fwd_run(const float* xp_f, const float* xp_r, const float* w_f, const float* w_r, const float* b_f, const float* b_r, float* y, float* gates,
                 float* c, float* hseq, int T, int B, int H, int training, hipStream_t st) {
  const int chunk = lstm_chunk(H);
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = B - b0 < chunk ? B - b0 : chunk;
    for (int step = 0; step < T; ++step) {
      hipLaunchKernelGGL(lstm_fwd_step_kernel<NJ>, dim3(H / LSTM_UNITS, 2), dim3(256), (size_t)nb * H * sizeof(float), st, xp_f, xp_r, w_f, w_r, b_f, b_r,
                         y, gates, c, hseq, T, B, H, b0, nb, step, training);
    }
  }
  HWG_LAUNCH_CHECK("lstm_fwd");
  return HWG_OK;
}

template <int NJ>
int lstm_bwd_run(const float* dy, const float* gates, const float* c, const float* wt, float* dgates, float* dc_ws, int T, int B, int H, hipStream_t st) {
  const int chunk = lstm_chunk(H);
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = B - b0 < chunk ? B - b0 : chunk;
    for (int step = 0; step < T; ++step) {
      hipLaunchKernelGGL(lstm_bwd_step_kernel<NJ>, dim3(H / LSTM_UNITS, 2), dim3(256), (size_t)nb * H * sizeof(float), st, dy, gates, c, wt, dgates, dc_ws,
                         T, B, H, b0, nb, step);
    }
  }
  HWG_LAUNCH_CHECK("lstm_bwd");
  return HWG_OK;
}

int lstm_check(const char* who, int T, int B, int H) {
  HWG_REQUIRE(T >= 1 && B >= 1 && H >= 1, "%s: T, B, H must be positive (T %d, B %d, H %d)", who, T, B, H);
  HWG_REQUIRE(H % LSTM_UNITS == 0, "%s: H = %d is not a multiple of the unit slice (%d)", who, H, LSTM_UNITS);
  HWG_REQUIRE(H <= 1024, "%s: H = %d exceeds 1024 (one line's h must fit the LDS image 16 times over)", who, H);
  HWG_REQUIRE((long long)T * B * 4 * H < (1ll << 31), "%s: T * B * 4H = %lld does not fit 31 bits", who, (long long)T * B * 4 * H);
  return HWG_OK;
}

}  // namespace

extern "C" int hwg_lstm_batch_tile(int H) { return (H >= 1 && H <= 1024) ? lstm_chunk(H) : 0; }

extern "C" int hwg_lstm_unit_slice(void) { return LSTM_UNITS; }

extern "C" int hwg_lstm_fwd(const float* xproj_f, const float* xproj_r, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
                            float* y, float* gates, float* c, float* hseq, int T, int B, int H, int training, void* stream) {
  if (int rc = lstm_check("lstm_fwd", T, B, H)) return rc;
  HWG_REQUIRE(xproj_f && xproj_r && whh_f && whh_r && bhh_f && bhh_r && y && c, "lstm_fwd: NULL argument");
  HWG_REQUIRE(!training || (gates && hseq), "lstm_fwd: training needs the gates and hseq buffers");
  HWG_REQUIRE(aligned16(whh_f) && aligned16(whh_r) && aligned16(y), "lstm_fwd: W_hh and y must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nj = (H + 63) / 64;
  if (nj <= 1) return lstm_fwd_run<1>(xproj_f, xproj_r, whh_f, whh_r, bhh_f, bhh_r, y, gates, c, hseq, T, B, H, training, st);
  if (nj <= 2) return lstm_fwd_run<2>(xproj_f, xproj_r, whh_f, whh_r, bhh_f, bhh_r, y, gates, c, hseq, T, B, H, training, st);
  if (nj <= 4) return lstm_fwd_run<4>(xproj_f, xproj_r, whh_f, whh_r, bhh_f, bhh_r, y, gates, c, hseq, T, B, H, training, st);
  if (nj <= 8) return lstm_fwd_run<8>(xproj_f, xproj_r, whh_f, whh_r, bhh_f, bhh_r, y, gates, c, hseq, T, B, H, training, st);
  return lstm_fwd_run<16>(xproj_f, xproj_r, whh_f, whh_r, bhh_f, bhh_r, y, gates, c, hseq, T, B, H, training, st);
}

extern "C" int hwg_lstm_bwd(const float* dy, const float* gates, const float* c, const float* whh_t, float* dgates, float* dc_ws, int T, int B, int H,
                            void* stream) {
  if (int rc = lstm_check("lstm_bwd", T, B, H)) return rc;
  HWG_REQUIRE(dy && gates && c && whh_t && dgates && dc_ws, "lstm_bwd: NULL argument");
  HWG_REQUIRE(aligned16(whh_t) && aligned16(dgates), "lstm_bwd: the packed W_hh and dgates must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nj = (H + 63) / 64;
  if (nj <= 1) return lstm_bwd_run<1>(dy, gates, c, whh_t, dgates, dc_ws, T, B, H, st);
  if (nj <= 2) return lstm_bwd_run<2>(dy, gates, c, whh_t, dgates, dc_ws, T, B, H, st);
  if (nj <= 4) return lstm_bwd_run<4>(dy, gates, c, whh_t, dgates, dc_ws, T, B, H, st);
  if (nj <= 8) return lstm_bwd_run<8>(dy, gates, c, whh_t, dgates, dc_ws, T, B, H, st);
  return lstm_bwd_run<16>(dy, gates, c, whh_t, dgates, dc_ws, T, B, H, st);
}

extern "C" int hwg_lstm_pack_whh(const float* whh_f, const float* whh_r, int H, float* whh_t, void* stream) {
  HWG_REQUIRE(whh_f && whh_r && whh_t && H >= 1 && H <= 1024, "lstm_pack_whh: bad arguments");
  hipLaunchKernelGGL(lstm_pack_whh_kernel, dim3((4 * H + 31) / 32, (H + 31) / 32, 2), dim3(256), 0, (hipStream_t)stream, whh_f, whh_r, whh_t, H);
  HWG_LAUNCH_CHECK("lstm_pack_whh");
  return HWG_OK;
}
