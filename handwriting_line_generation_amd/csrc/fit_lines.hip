// Line images fitted to the recognisers' height on the device: what every loader does on the host with PIL for a line read from disk
// (datasets/hw_dataset.py:128-131 and :157, the reference's generate.py:655-663; here data/author_hw_dataset.py `_resize`) - resize to H rows
// and the width that keeps the aspect, bicubic, then 1 - p / 128, then collate padded with -1 - for a ragged pool of grey 8-bit pictures of
// differing heights and widths, in one launch, with PIL's bytes.
//
// Pillow's 8-bit resize (Resample.c) is integer arithmetic: a pass over one axis computes, per output index, acc = 2^21 + sum pixel * k over
// a window of the input with 22-bit fixed-point coefficients k, and writes clamp(acc >> 22, 0, 255). The horizontal pass runs first into an
// 8-bit intermediate, the vertical pass second; a pass whose input and output sizes agree is skipped. (Image.resize of recent Pillow turns
// the order round for a picture more than 100 times as tall as wide that shrinks vertically: the table entry carries the order, and the
// vertical-first path below serves pictures of at most FIT_TILE columns, which covers every such picture within the height limit.)
// The windows and coefficients are computed on the host in fp64 (data/fit_tables.py) and arrive as int32 tables; this file does the
// integer sums, the intermediate rounding, the map to fp32 (exact: p / 128 is a power-of-two scaling) and the stores.
//
// One workgroup owns FIT_TILE output columns of one line: the horizontal pass of ALL the line's input rows for those columns goes into LDS
// as bytes [in_h][FIT_TILE], the vertical pass reads LDS (one 32-bit read = 4 columns of a row) and writes 16-byte stores. No intermediate
// picture goes to global memory, no atomics, no hand-off between workgroups: a line's bytes depend on its own table entry alone.
//
// The per-line table `lines` [B][10] int64 (device): {byte offset of the picture in `pixels`, in_h, in_w, out_w, htab, hks, vtab, vks,
// order (0: horizontal pass first, 1: vertical pass first), 0}.
// An axis table of `out` outputs and `ks` taps starts at element htab / vtab of `coef` (int32) and holds first[out], count[out], k[out][ks];
// ks == 0 says the pass is skipped and is legal only where the sizes agree. The caller validated the table; an entry that is bad all the
// same turns its WHOLE line into padding without a read through it (every workgroup of the line checks every window of both axes, so the
// workgroups agree): a picture outside the pool (hwg_line_in_pool), sizes outside their limits, out_w > W, an axis table outside `coef` or
// misaligned (hwg_block_in_buffer), a window that leaves the picture or holds more than ks taps, an order that is neither 0 nor 1, or 1
// for a picture wider than FIT_TILE.
#include "hwg_common.h"

constexpr int FIT_TILE = 64;               // output columns per workgroup = bytes per LDS row
constexpr int FIT_BLOCK = 256;
constexpr int FIT_ENTRY = 10;              // int64 words of a line's table entry
constexpr int FIT_MAX_IN_H = 1024;         // rows of the 8-bit intermediate in LDS: 1024 x 64 bytes = 64 KiB of the CU's 160 KiB
constexpr int FIT_MAX_H = 1024;
constexpr int FIT_MAX_W = 1 << 20;         // of the batch and of a picture
constexpr int FIT_MAX_KS = 1 << 16;        // taps of one window (2 * ceil(2 * in / out) + 1)

__device__ __forceinline__ unsigned fit_clip8(unsigned acc) {
  const int v = (int)acc >> 22;            // the sum wraps like the host's 32-bit integers; arithmetic shift
  return (unsigned)min(max(v, 0), 255);
}

// every window of an axis table lies inside [0, in) and holds at most ks taps (strided over the workgroup; the caller ORs the verdicts)
__device__ __forceinline__ bool fit_windows_bad(const int* __restrict__ tab, int out, int ks, int in) {
  bool bad = false;
  for (int i = threadIdx.x; i < out; i += FIT_BLOCK) {
    const int first = tab[i], n = tab[out + i];
    bad |= !(first >= 0 && n >= 0 && n <= ks && first <= in && n <= in - first);
  }
  return bad;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_lines_kernel(const unsigned char* __restrict__ pixels, long long pixel_bytes,
                                                              const long long* __restrict__ lines, const int* __restrict__ coef,
                                                              long long coef_elems, int max_in_h, int H, int W, float* __restrict__ out) {
  extern __shared__ unsigned char mid[];                    // [in_h][FIT_TILE]: the first pass's bytes of this tile ([H][FIT_TILE] vertical first)
  const int b = blockIdx.y, tid = threadIdx.x;
  const int col0 = blockIdx.x * FIT_TILE;
  const long long* e = lines + (size_t)b * FIT_ENTRY;
  const long long off = e[0], in_h_ = e[1], in_w_ = e[2], out_w_ = e[3], htab = e[4], hks_ = e[5], vtab = e[6], vks_ = e[7], order = e[8];

  // the entry itself (uniform over the workgroup), in 64 bits before anything is narrowed
  bool ok = in_h_ >= 1 && in_h_ <= max_in_h && in_w_ >= 1 && in_w_ <= FIT_MAX_W && out_w_ >= 1 && out_w_ <= W && hks_ >= 0 && hks_ <= FIT_MAX_KS &&
            vks_ >= 0 && vks_ <= FIT_MAX_KS && (order == 0 || (order == 1 && in_w_ <= FIT_TILE));
  const int in_h = (int)in_h_, in_w = (int)in_w_, out_w = (int)out_w_, hks = (int)hks_, vks = (int)vks_;
  ok = ok && hwg_line_in_pool(off, in_w, in_h, pixel_bytes);
  ok = ok && (hks > 0 ? hwg_block_in_buffer(htab, (long long)out_w * (2 + hks), coef_elems) : in_w == out_w);
  ok = ok && (vks > 0 ? hwg_block_in_buffer(vtab, (long long)H * (2 + vks), coef_elems) : in_h == H);
  const int* ht = coef + (ok ? htab : 0);
  const int* vt = coef + (ok ? vtab : 0);
  bool bad = !ok;
  if (ok && hks > 0) bad |= fit_windows_bad(ht, out_w, hks, in_w);
  if (ok && vks > 0) bad |= fit_windows_bad(vt, H, vks, in_h);
  bad = __syncthreads_or(bad);

  const f32x4 pad = {-1.0f, -1.0f, -1.0f, -1.0f};           // PADDING_CONSTANT
  const int groups = min(FIT_TILE, W - col0) / 4;           // 4-column groups of this tile inside the batch (W % 4 == 0)
  if (bad || col0 >= out_w) {
    for (int i = tid; i < H * groups; i += FIT_BLOCK) {
      const int y = i / groups, g = i - y * groups;
      *(f32x4*)(out + ((size_t)b * H + y) * W + col0 + 4 * g) = pad;
    }
    return;
  }

  const unsigned char* src = pixels + off;
  if (order == 1) {
    // vertical pass first, of all in_w <= FIT_TILE columns of the picture, out of global memory into mid [H][FIT_TILE]
    for (int i = tid; i < H * in_w; i += FIT_BLOCK) {
      const int y = i / in_w, c = i - y * in_w;
      unsigned p;
      if (vks == 0) {
        p = src[(size_t)y * in_w + c];
      } else {
        const int first = vt[y], n = vt[H + y];
        const int* k = vt + 2 * (size_t)H + (size_t)y * vks;
        unsigned acc = 1u << 21;
        for (int x = 0; x < n; ++x) acc += (unsigned)src[(size_t)(first + x) * in_w + c] * (unsigned)k[x];
        p = fit_clip8(acc);
      }
      mid[y * FIT_TILE + c] = (unsigned char)p;
    }
    __syncthreads();
    // horizontal pass out of LDS: one lane = 4 columns of one output row
    for (int i = tid; i < H * groups; i += FIT_BLOCK) {
      const int y = i / groups, g = i - y * groups, x0 = col0 + 4 * g;
      float v[4];
      for (int j = 0; j < 4; ++j) {
        const int xx = x0 + j;
        v[j] = -1.0f;
        if (xx < out_w) {
          unsigned p;
          if (hks == 0) {
            p = mid[y * FIT_TILE + xx];                      // out_w == in_w <= FIT_TILE
          } else {
            const int first = ht[xx], n = ht[out_w + xx];
            const int* k = ht + 2 * (size_t)out_w + (size_t)xx * hks;
            unsigned acc = 1u << 21;
            for (int x = 0; x < n; ++x) acc += (unsigned)mid[y * FIT_TILE + first + x] * (unsigned)k[x];
            p = fit_clip8(acc);
          }
          v[j] = 1.0f - (float)p / 128.0f;
        }
      }
      const f32x4 q = {v[0], v[1], v[2], v[3]};
      *(f32x4*)(out + ((size_t)b * H + y) * W + x0) = q;
    }
    return;
  }

  // horizontal pass (or the bytes as they are): lane -> one column of the tile, rows strided over the wavefronts
  {
    const int c = tid & (FIT_TILE - 1), xx = col0 + c;
    if (xx >= out_w) {
      for (int r = tid / FIT_TILE; r < in_h; r += FIT_BLOCK / FIT_TILE) mid[r * FIT_TILE + c] = 0;
    } else if (hks == 0) {
      for (int r = tid / FIT_TILE; r < in_h; r += FIT_BLOCK / FIT_TILE) mid[r * FIT_TILE + c] = src[(size_t)r * in_w + xx];
    } else {
      const int first = ht[xx], n = ht[out_w + xx];
      const int* k = ht + 2 * (size_t)out_w + (size_t)xx * hks;
      for (int r = tid / FIT_TILE; r < in_h; r += FIT_BLOCK / FIT_TILE) {
        const unsigned char* row = src + (size_t)r * in_w + first;
        unsigned acc = 1u << 21;
        for (int x = 0; x < n; ++x) acc += (unsigned)row[x] * (unsigned)k[x];
        mid[r * FIT_TILE + c] = (unsigned char)fit_clip8(acc);
      }
    }
  }
  __syncthreads();

  // vertical pass out of LDS: one lane = 4 columns of one output row
  for (int i = tid; i < H * groups; i += FIT_BLOCK) {
    const int y = i / groups, g = i - y * groups;
    unsigned p0, p1, p2, p3;
    if (vks == 0) {
      const unsigned px = *(const unsigned*)(mid + y * FIT_TILE + 4 * g);
      p0 = px & 255u, p1 = (px >> 8) & 255u, p2 = (px >> 16) & 255u, p3 = px >> 24;
    } else {
      const int first = vt[y], n = vt[H + y];
      const int* k = vt + 2 * (size_t)H + (size_t)y * vks;
      unsigned a0 = 1u << 21, a1 = a0, a2 = a0, a3 = a0;
      for (int x = 0; x < n; ++x) {
        const unsigned px = *(const unsigned*)(mid + (first + x) * FIT_TILE + 4 * g);
        const unsigned kk = (unsigned)k[x];
        a0 += (px & 255u) * kk, a1 += ((px >> 8) & 255u) * kk, a2 += ((px >> 16) & 255u) * kk, a3 += (px >> 24) * kk;
      }
      p0 = fit_clip8(a0), p1 = fit_clip8(a1), p2 = fit_clip8(a2), p3 = fit_clip8(a3);
    }
    const int x0 = col0 + 4 * g;
    f32x4 v;
    v.x = x0 + 0 < out_w ? 1.0f - (float)p0 / 128.0f : -1.0f;
    v.y = x0 + 1 < out_w ? 1.0f - (float)p1 / 128.0f : -1.0f;
    v.z = x0 + 2 < out_w ? 1.0f - (float)p2 / 128.0f : -1.0f;
    v.w = x0 + 3 < out_w ? 1.0f - (float)p3 / 128.0f : -1.0f;
    *(f32x4*)(out + ((size_t)b * H + y) * W + x0) = v;
  }
}

extern "C" int hwg_fit_lines(const unsigned char* pixels, long long pixel_bytes, const long long* lines, const int* coef, long long coef_elems,
                             int max_in_h, int B, int H, int W, float* out, void* stream) {
  HWG_REQUIRE(pixels && lines && coef && out, "fit_lines: null argument");
  HWG_REQUIRE(B > 0 && H > 0 && W > 0 && pixel_bytes > 0 && coef_elems > 0 && max_in_h > 0,
              "fit_lines: bad sizes B=%d H=%d W=%d pixel_bytes=%lld coef_elems=%lld max_in_h=%d", B, H, W, pixel_bytes, coef_elems, max_in_h);
  HWG_REQUIRE(B <= 65535 && H <= FIT_MAX_H && W <= FIT_MAX_W && max_in_h <= FIT_MAX_IN_H,
              "fit_lines: beyond the limit B=%d (<= 65535) H=%d (<= %d) W=%d (<= %d) tallest picture %d (<= %d)", B, H, FIT_MAX_H, W, FIT_MAX_W,
              max_in_h, FIT_MAX_IN_H);
  HWG_REQUIRE(W % 4 == 0, "fit_lines: batch width %d is not a multiple of 4", W);
  HWG_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)lines & 7) == 0 && ((uintptr_t)coef & 15) == 0,
              "fit_lines: out and coef must be 16-byte aligned, lines 8-byte aligned");
  const size_t lds = (size_t)(max_in_h > H ? max_in_h : H) * FIT_TILE;       // (a line taller than max_in_h is refused by the kernel)
  if (lds > 32768) {             // towards 64 KiB a kernel's LDS has to be asked for (per device: asked on every such call)
    if (hipFuncSetAttribute((const void*)fit_lines_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FIT_MAX_IN_H * FIT_TILE) != hipSuccess) {
      (void)hipGetLastError();
      hwg_set_error("fit_lines: the device refuses %d bytes of LDS per workgroup", FIT_MAX_IN_H * FIT_TILE);
      return HWG_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(fit_lines_kernel, dim3(hwg_cdiv(W, FIT_TILE), B), dim3(FIT_BLOCK), lds, (hipStream_t)stream, pixels, pixel_bytes, lines,
                     coef, coef_elems, max_in_h, H, W, out);
  HWG_LAUNCH_CHECK("fit_lines");
  return HWG_OK;
}
