// The stretch film's labels: one aligned line of class indices, re-sampled along time to F lengths, as one-hot rows in both layouts.
// The reference (generate.py:830-852 interpolate_horz) builds each frame with a dense one-hot, two permutes and
// F.interpolate(mode='linear') - 79 times per film. Here the indices go in and one launch writes every frame: the interpolated one-hot
// row of (frame, time step, line) is w0 at class label[i0] and w1 at class label[i1] (w0 + w1 where the two agree), zero elsewhere, so no
// dense one-hot is ever read.
//
// Work: blockIdx.y is the frame; a lane owns 4 consecutive floats of the frame's flat [B][T_out][ncls] block and the same 4 of its
// [T_out][B][ncls] block - one 16-byte store to each (ncls need not be a multiple of 4: a quad may span two rows; the last quad of a
// frame whose size is no multiple of 4 is stored float by float). Every element of both blocks is written, zeros included. Write-bound:
// 2 * sum_f T_out_f * B * ncls * 4 bytes; the T * B label indices stay in cache.
#include "hwg_common.h"

constexpr int STRETCH_BLOCK = 256;

struct StretchTap { int l0, l1; float w0, w1; };

// (the helpers below also compile for the host: a stand-alone CPU program that includes this file can walk every quad of a frame through
// the same index arithmetic under a sanitizer; there fmaf is the fused operation)
#if defined(__HIP_DEVICE_COMPILE__)
#define STRETCH_FMA(a, b, c) __fmaf_rn(a, b, c)
#else
#define STRETCH_FMA(a, b, c) fmaf(a, b, c)
#endif

// source taps of output step t: torch's CPU rule for mode='linear', align_corners=False with a given scale factor. The fused multiply-add
// is ONE rounding (__fmaf_rn, never contracted differently): rounding r * (t + 0.5) first moves i0 at integer crossings.
__host__ __device__ __forceinline__ StretchTap stretch_tap(const int* __restrict__ label, int T, int B, int b, int t, float r, int identity) {
  StretchTap s;
  if (identity) {
    s.l0 = s.l1 = label[t * B + b];
    s.w0 = 1.0f;
    s.w1 = 0.0f;
    return s;
  }
  float src = STRETCH_FMA(r, (float)t + 0.5f, -0.5f);
  src = fmaxf(src, 0.0f);
  const int i0 = (int)src < T - 1 ? (int)src : T - 1;
  const int i1 = i0 + 1 < T - 1 ? i0 + 1 : T - 1;
  s.w1 = src - (float)i0;
  s.w0 = 1.0f - s.w1;
  s.l0 = label[i0 * B + b];
  s.l1 = label[i1 * B + b];
  return s;
}

__host__ __device__ __forceinline__ float stretch_value(const StretchTap& s, int c) { return (s.l0 == c ? s.w0 : 0.0f) + (s.l1 == c ? s.w1 : 0.0f); }

// LAYOUT 0: rows ordered [b][t] (NHWC rows), 1: rows ordered [t][b] (time major)
template <int LAYOUT>
__host__ __device__ __forceinline__ void stretch_quad(const int* __restrict__ label, int T, int B, int ncls, int T_out, float r, int identity,
                                                      unsigned first, unsigned n, float* __restrict__ out) {
  unsigned row = first / (unsigned)ncls;
  int c = (int)(first - row * (unsigned)ncls);
  float v[4];
  StretchTap s;
  bool fresh = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (first + k < n) {          // (rows behind the frame's last are never decoded: no label index outside [0, T * B))
      if (fresh) {
        const int b = LAYOUT == 0 ? (int)(row / (unsigned)T_out) : (int)(row % (unsigned)B);
        const int t = LAYOUT == 0 ? (int)(row % (unsigned)T_out) : (int)(row / (unsigned)B);
        s = stretch_tap(label, T, B, b, t, r, identity);
        fresh = false;
      }
      v[k] = stretch_value(s, c);
      if (++c == ncls) {
        c = 0;
        ++row;
        fresh = true;
      }
    } else {
      v[k] = 0.0f;
    }
  }
  if (first + 4 <= n) {
    const f32x4 q = {v[0], v[1], v[2], v[3]};
    *(f32x4*)(out + first) = q;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (first + k < n) out[first + k] = v[k];
  }
}

// A table entry that does not fit (T_out outside [1, max_T_out], a block that is misaligned or ends behind its buffer) writes nothing:
// the caller validated the table, a bad entry still cannot store outside the two buffers.
__global__ __launch_bounds__(STRETCH_BLOCK) void stretch_onehot_kernel(const int* __restrict__ label, int T, int B, int ncls,
                                                                       const hwg_stretch_frame* __restrict__ frames, int max_T_out,
                                                                       float* __restrict__ out_blc, long long blc_elems,
                                                                       float* __restrict__ out_lbc, long long lbc_elems) {
  const hwg_stretch_frame fr = frames[blockIdx.y];
  if (fr.T_out < 1 || fr.T_out > max_T_out) return;
  const unsigned n = (unsigned)B * (unsigned)fr.T_out * (unsigned)ncls;      // < 2^31: checked at the entry point for max_T_out
  if (!hwg_block_in_buffer(fr.off_blc, (long long)n, blc_elems) || !hwg_block_in_buffer(fr.off_lbc, (long long)n, lbc_elems)) return;
  const int identity = fr.identity && fr.T_out == T;      // (an identity frame of another length would read labels behind step T - 1)
  const unsigned quads = (n + 3u) / 4u;
  for (unsigned q = blockIdx.x * STRETCH_BLOCK + threadIdx.x; q < quads; q += gridDim.x * STRETCH_BLOCK) {
    stretch_quad<0>(label, T, B, ncls, fr.T_out, fr.r, identity, 4u * q, n, out_blc + fr.off_blc);
    stretch_quad<1>(label, T, B, ncls, fr.T_out, fr.r, identity, 4u * q, n, out_lbc + fr.off_lbc);
  }
}

extern "C" int hwg_stretch_onehot(const int* label, int T, int B, int ncls, const hwg_stretch_frame* frames, int F, int max_T_out,
                                  float* out_blc, long long blc_elems, float* out_lbc, long long lbc_elems, void* stream) {
  HWG_REQUIRE(label && frames && out_blc && out_lbc, "stretch_onehot: null argument");
  HWG_REQUIRE(T > 0 && B > 0 && ncls > 0 && max_T_out > 0, "stretch_onehot: bad sizes T=%d B=%d ncls=%d max_T_out=%d", T, B, ncls, max_T_out);
  HWG_REQUIRE(F > 0 && F <= 65535, "stretch_onehot: %d frames (1 .. 65535)", F);
  HWG_REQUIRE((long long)T * B < (1ll << 31) && T < (1 << 23), "stretch_onehot: label too large T=%d B=%d", T, B);
  HWG_REQUIRE((long long)B * max_T_out * ncls < (1ll << 31) - 4, "stretch_onehot: a frame of %d x %d x %d is too large for 32-bit element indices",
              B, max_T_out, ncls);
  HWG_REQUIRE(blc_elems > 0 && lbc_elems > 0, "stretch_onehot: empty output buffer");
  HWG_REQUIRE(((uintptr_t)out_blc & 15) == 0 && ((uintptr_t)out_lbc & 15) == 0, "stretch_onehot: the output buffers must be 16-byte aligned");
  HWG_REQUIRE(((uintptr_t)frames & 7) == 0 && ((uintptr_t)label & 3) == 0, "stretch_onehot: frames must be 8-byte and label 4-byte aligned");
  const long long quads = ((long long)B * max_T_out * ncls + 3) / 4;
  int gx = hwg_cdiv(quads, STRETCH_BLOCK);
  const int cap = F < 2048 ? 2048 / F : 1;   // ~2048 workgroups over all frames, the rest by grid stride
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(stretch_onehot_kernel, dim3(gx, F), dim3(STRETCH_BLOCK), 0, (hipStream_t)stream, label, T, B, ncls, frames, max_T_out,
                     out_blc, blc_elems, out_lbc, lbc_elems);
  HWG_LAUNCH_CHECK("stretch_onehot");
  return HWG_OK;
}
