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
