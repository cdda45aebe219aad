// Generated lines as 8-bit grey pictures: the reference turns the generator's fp32 image into what it writes to disk with
// ((1 - im) * 127.5).astype(np.uint8) on the host (generate.py:303, 344, 426, 496, 525, 622, 692, 718, 786), after downloading the whole
// padded fp32 batch. Here one launch converts the batch on the device and packs it ragged: line b becomes a finished H x widths[b] picture
// at out + offsets[b] (row stride widths[b], no gaps), so that a quarter of the fp32 bytes - and none of the blank tail batching gives a
// line - crosses to the host.
//
// One lane converts 4 columns: one 16-byte load, one 32-bit store. W, widths[b] and offsets[b] are multiples of 4 (the generator emits 4
// columns per content step), which keeps both accesses aligned; columns >= widths[b] are never read.
#include "hwg_common.h"

constexpr int LINES_BLOCK = 256;         // lanes per workgroup = 1024 columns of one image row

// v = (1 - x) * 127.5 in fp32 (a subtraction, then a multiplication: nothing to contract), clamped to [0, 255], NaN -> 0, truncated
// toward zero. Inside [-1, 1] this is numpy's arithmetic bit for bit; outside it numpy's astype wraps and this clamps.
__device__ __forceinline__ unsigned lines_level(float x) {
  const float v = (1.0f - x) * 127.5f;
  return (unsigned)(int)fminf(fmaxf(v, 0.0f), 255.0f);      // fmaxf(NaN, 0) = 0
}

__global__ __launch_bounds__(LINES_BLOCK) void lines_to_u8_kernel(const float* __restrict__ img, int H, int W, const int* __restrict__ widths,
                                                                  const long long* __restrict__ offsets, unsigned char* __restrict__ out) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int col = 4 * (blockIdx.x * LINES_BLOCK + threadIdx.x);
  const int w = min(widths[b], W) & ~3;            // the caller validated the table; a bad entry still cannot read past the row
  if (col >= w) return;
  const f32x4 v = *(const f32x4*)(img + ((size_t)b * H + y) * W + col);
  const unsigned px = lines_level(v.x) | (lines_level(v.y) << 8) | (lines_level(v.z) << 16) | (lines_level(v.w) << 24);
  *(unsigned*)(out + offsets[b] + (size_t)y * w + col) = px;
}

extern "C" int hwg_lines_to_u8(const float* img, int B, int H, int W, const int* widths, const long long* offsets, unsigned char* out,
                               void* stream) {
  HWG_REQUIRE(img && widths && offsets && out, "lines_to_u8: null argument");
  HWG_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && H <= 65535, "lines_to_u8: bad sizes B=%d H=%d W=%d", B, H, W);
  HWG_REQUIRE(W % 4 == 0, "lines_to_u8: image width %d is not a multiple of 4", W);
  HWG_REQUIRE(((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 3) == 0, "lines_to_u8: img must be 16-byte aligned and out 4-byte aligned");
  hipLaunchKernelGGL(lines_to_u8_kernel, dim3(hwg_cdiv(W / 4, LINES_BLOCK), H, B), dim3(LINES_BLOCK), 0, (hipStream_t)stream, img, H, W, widths,
                     offsets, out);
  HWG_LAUNCH_CHECK("lines_to_u8");
  return HWG_OK;
}

// ---- the way back: ragged 8-bit lines (the layout above) into a collated fp32 batch, mixed with the rows of a real batch ----------------
// What HWDataset.__getitem__ and collate do on the host for a line read from disk - 1 - p / 128, padded with -1 to the widest line of the
// batch - for lines that were generated on this device and never left it. One launch writes EVERY element of out [B,1,H,W]: row b is line
// select[b] = k >= 0 of the pool (pixels, offsets, widths), or row r of `real` [Br,1,H,Wr] for select[b] = -1 - r.
//
// A pool row: one lane owns 4 output columns - one 32-bit load, one 16-byte store; columns >= widths[k] are never read. A real row has an
// arbitrary Wr (row stride and alignment are no multiples of 4): four scalar loads, one 16-byte store. Every level is exact in fp32
// (p / 128 is a power-of-two scaling, 1 - q with q a multiple of 2^-7 below 2), so this IS the host's arithmetic.
//
// The caller validated the tables; an entry that is bad all the same (k >= n_lines, r >= Br, a width that is no multiple of 4 or above W,
// an offset that is negative or no multiple of 4, a line that ends behind pixel_bytes - hwg_line_in_pool of table_guard.h, for any 64-bit
// offset) makes its row padding: nothing is read through it. All stores are inside out [B,1,H,W] whatever the tables hold.
__global__ __launch_bounds__(LINES_BLOCK) void lines_from_u8_kernel(const unsigned char* __restrict__ pixels, long long pixel_bytes,
                                                                    const long long* __restrict__ offsets, const int* __restrict__ widths,
                                                                    int n_lines, const int* __restrict__ select, const float* __restrict__ real,
                                                                    int Br, int Wr, int H, int W, float* __restrict__ out) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int col = 4 * (blockIdx.x * LINES_BLOCK + threadIdx.x);
  if (col >= W) return;
  const int s = select[b];
  f32x4 v = {-1.0f, -1.0f, -1.0f, -1.0f};          // PADDING_CONSTANT
  if (s >= 0) {
    if (s < n_lines) {
      const int w = widths[s];
      const long long off = offsets[s];
      const bool ok = w <= W && (w & 3) == 0 && (off & 3) == 0 && hwg_line_in_pool(off, w, H, pixel_bytes);
      if (ok && col < w) {
        const unsigned px = *(const unsigned*)(pixels + off + (size_t)y * w + col);
        v.x = 1.0f - (float)(px & 255u) / 128.0f;
        v.y = 1.0f - (float)((px >> 8) & 255u) / 128.0f;
        v.z = 1.0f - (float)((px >> 16) & 255u) / 128.0f;
        v.w = 1.0f - (float)(px >> 24) / 128.0f;
      }
    }
  } else {
    const int r = -1 - s;
    if (r < Br) {
      const float* row = real + ((size_t)r * H + y) * Wr;
      if (col + 0 < Wr) v.x = row[col + 0];
      if (col + 1 < Wr) v.y = row[col + 1];
      if (col + 2 < Wr) v.z = row[col + 2];
      if (col + 3 < Wr) v.w = row[col + 3];
    }
  }
  *(f32x4*)(out + ((size_t)b * H + y) * W + col) = v;
}

extern "C" int hwg_lines_from_u8(const unsigned char* pixels, long long pixel_bytes, const long long* offsets, const int* widths, int n_lines,
                                 const int* select, int min_select, const float* real, int Br, int Wr, int B, int H, int W, float* out,
                                 void* stream) {
  HWG_REQUIRE(pixels && offsets && widths && select && out, "lines_from_u8: null argument");
  HWG_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && H <= 65535, "lines_from_u8: bad sizes B=%d H=%d W=%d", B, H, W);
  HWG_REQUIRE(n_lines >= 0 && pixel_bytes >= 0, "lines_from_u8: bad sizes n_lines=%d pixel_bytes=%lld", n_lines, pixel_bytes);
  HWG_REQUIRE(W % 4 == 0, "lines_from_u8: batch width %d is not a multiple of 4", W);
  HWG_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)pixels & 3) == 0, "lines_from_u8: out must be 16-byte aligned and pixels 4-byte aligned");
  if (real) {
    HWG_REQUIRE(Br > 0 && Wr > 0 && Wr <= W, "lines_from_u8: bad sizes of the real batch Br=%d Wr=%d (batch width %d)", Br, Wr, W);
    HWG_REQUIRE(((uintptr_t)real & 3) == 0, "lines_from_u8: real must be 4-byte aligned");
    HWG_REQUIRE(min_select >= -Br, "lines_from_u8: select entry %d names a row behind the %d of the real batch", min_select, Br);
  } else {
    HWG_REQUIRE(min_select >= 0, "lines_from_u8: negative select entry %d without a real batch", min_select);
    Br = Wr = 0;
  }
  hipLaunchKernelGGL(lines_from_u8_kernel, dim3(hwg_cdiv(W / 4, LINES_BLOCK), H, B), dim3(LINES_BLOCK), 0, (hipStream_t)stream, pixels,
                     pixel_bytes, offsets, widths, n_lines, select, real, Br, Wr, H, W, out);
  HWG_LAUNCH_CHECK("lines_from_u8");
  return HWG_OK;
}
