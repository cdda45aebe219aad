// Sample sheets of GAN training (trainer.print_dir): the reference prints a batch of lines with
//   torchvision.utils.save_image(1 - images, nrow=max(1, 2048 // W), normalize=True)      (trainer/hw_with_style_trainer.py:992-1010)
// on the host, after downloading the fp32 batch. Here the finished 8-bit sheet is made on the device in two launches, so that a quarter
// of the bytes crosses to the host and nothing on the step's thread waits for them.
//
// For images x [B][1][H][W] fp32 that call computes, every step a correctly rounded fp32 operation:
//   v = 1 - x;  lo = min(v), hi = max(v) over the WHOLE tensor (padding columns included)
//   n = (clamp(v, lo, hi) - lo) / d,  d = (float)max((double)hi - (double)lo, 1e-5)        (a true division)
//   B == 1: the sheet is the H x W image.  Otherwise xmaps = min(nrow, B), ymaps = ceil(B / xmaps), the sheet is
//   (H + 2) ymaps + 2 rows by (W + 2) xmaps + 2 columns of 0, image k at row (k / xmaps)(H + 2) + 2, column (k % xmaps)(W + 2) + 2
//   byte = trunc(clamp(n * 255 + 0.5, 0, 255)), the product and the sum each rounded to fp32
//
// hwg_sheet_minmax: workgroup g leaves (min, max) of its share of v in partials[2g], partials[2g + 1]. No atomics, nothing crosses a
//   workgroup inside the launch. Only finite v count; a share without any leaves (+inf, -inf).
// hwg_sheet_compose: every workgroup folds the (at most SHEET_MAX_PARTS) partials itself - lane t takes pair t, then a fixed shuffle tree
//   and a fixed walk over the wavefronts' results - and then writes bytes. The mapping is OUTPUT-centred: a lane owns 4 consecutive bytes
//   of the flat sheet, finds for each whether it is border or pixel (k, y, x), loads the pixels one by one and makes ONE aligned 32-bit
//   store. A cell-centred mapping cannot store words: W is any integer (the collated real batch), and even for W % 4 == 0 a cell starts
//   at column x (W + 2) + 2 of a row of (W + 2) xmaps + 2 bytes. EVERY byte of the sheet is written (borders, empty cells), nothing has
//   to be cleared first; the last word may cover up to 3 bytes behind the sheet (written 0): out holds the sheet rounded up to 4 bytes.
//
// NO CONTRACTION: at -O3 the compiler turns n * 255.0f + 0.5f into one fma, which rounds once where torch rounds twice. sheet_level()
// therefore runs under `#pragma clang fp contract(off)`, so that the kernel does operation for operation what the restatement does;
// hipcc's __fmul_rn / __fadd_rn are plain `*` and `+` and WERE fused here (v_fma_f32 ..., 0.5 in the assembly), so they are no
// protection. (For this one expression the single rounding happens to be harmless: over all fp32 n in [0, 1], scanned exhaustively on the
// host, trunc(fma(n, 255, 0.5)) equals the twice-rounded byte. The pragma keeps that from being something the bytes depend on.)
// lines_level() in lines_out.hip has nothing to contract; this file has.
//
// Values that are not finite (the reference's result is undefined for them; a diverged run must still leave a sheet): lo and hi are
// those of the finite v; a NaN pixel is 0; v = +inf is 255 and v = -inf is 0 (what the clamp gives); a batch without any finite value
// gives an all-0 sheet.
#include <math.h>
#include "hwg_common.h"

constexpr int SHEET_BLOCK = 256;
constexpr int SHEET_MAX_PARTS = 256;       // = SHEET_BLOCK: the compose kernel's lane t folds pair t
constexpr long long SHEET_PART_ELEMS = 4096;

static int sheet_parts(long long n) {
  const long long g = (n + SHEET_PART_ELEMS - 1) / SHEET_PART_ELEMS;
  return (int)(g < 1 ? 1 : g > SHEET_MAX_PARTS ? SHEET_MAX_PARTS : g);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// (lo, hi) of the calling workgroup's lanes' (lo, hi); valid in all lanes. smem: 2 * SHEET_BLOCK / 64 floats.
__device__ __forceinline__ void sheet_block_minmax(float& lo, float& hi, float* smem) {
  lo = wave_min(lo);
  hi = wave_max(hi);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    smem[2 * wid] = lo;
    smem[2 * wid + 1] = hi;
  }
  __syncthreads();
  lo = smem[0];
  hi = smem[1];
#pragma unroll
  for (int i = 1; i < SHEET_BLOCK / 64; ++i) {
    lo = fminf(lo, smem[2 * i]);
    hi = fmaxf(hi, smem[2 * i + 1]);
  }
}

__global__ __launch_bounds__(SHEET_BLOCK) void sheet_minmax_kernel(const float* __restrict__ x, long long n, float* __restrict__ partials) {
  __shared__ float smem[2 * SHEET_BLOCK / 64];
  float lo = INFINITY, hi = -INFINITY;
  const long long stride = (long long)gridDim.x * SHEET_BLOCK;
  for (long long i = (long long)blockIdx.x * SHEET_BLOCK + threadIdx.x; i < n; i += stride) {
    const float v = 1.0f - x[i];
    if (fabsf(v) < INFINITY) {             // false for NaN and both infinities
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  sheet_block_minmax(lo, hi, smem);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = lo;
    partials[2 * blockIdx.x + 1] = hi;
  }
}

// geometry of a sheet, made on the host once per call
struct SheetGeom {
  int B, H, W;
  int xmaps;       // cells per sheet row; 0 = B == 1: the image itself, no border
  int Ws;          // bytes per sheet row
  int total;       // bytes of the sheet
  int words;       // 32-bit words that cover it
};

__device__ __forceinline__ unsigned sheet_level(float v, float lo, float hi, float d) {
#pragma clang fp contract(off)              // two roundings in n * 255 + 0.5, never an fma (see the top of the file)
  if (v != v) return 0u;
  const float n = (fminf(fmaxf(v, lo), hi) - lo) / d;
  const float m = n * 255.0f;
  const float t = m + 0.5f;
  return (unsigned)(int)fminf(fmaxf(t, 0.0f), 255.0f);
}

__global__ __launch_bounds__(SHEET_BLOCK) void sheet_compose_kernel(const float* __restrict__ x, SheetGeom g, const float* __restrict__ partials,
                                                                    int n_parts, unsigned* __restrict__ out) {
  __shared__ float smem[2 * SHEET_BLOCK / 64];
  float lo = INFINITY, hi = -INFINITY;
  if ((int)threadIdx.x < n_parts) {
    lo = partials[2 * threadIdx.x];
    hi = partials[2 * threadIdx.x + 1];
  }
  sheet_block_minmax(lo, hi, smem);
  const int word = blockIdx.x * SHEET_BLOCK + threadIdx.x;
  if (word >= g.words) return;
  const bool any = lo <= hi;                // false: no finite value in the batch -> an all-0 sheet
  const float d = (float)fmax((double)hi - (double)lo, 1e-5);
  const int cw = g.W + 2, ch = g.H + 2;
  unsigned px = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = 4 * word + j;
    if (p >= g.total || !any) continue;
    const int r = p / g.Ws, c = p - r * g.Ws;
    long long src;
    if (g.xmaps == 0) {
      src = (long long)r * g.W + c;
    } else {
      if (r < 2 || c < 2) continue;
      const int cy = (r - 2) / ch, y = (r - 2) - cy * ch;
      const int cx = (c - 2) / cw, xx = (c - 2) - cx * cw;
      const int k = cy * g.xmaps + cx;
      if (y >= g.H || xx >= g.W || k >= g.B) continue;
      src = ((long long)k * g.H + y) * g.W + xx;
    }
    px |= sheet_level(1.0f - x[src], lo, hi, d) << (8 * j);
  }
  out[word] = px;
}

extern "C" int hwg_sheet_parts(long long n) { return n > 0 ? sheet_parts(n) : 0; }

extern "C" int hwg_sheet_minmax(const float* x, long long n, float* partials, int n_parts, void* stream) {
  HWG_REQUIRE(x && partials, "sheet_minmax: null argument");
  HWG_REQUIRE(n > 0, "sheet_minmax: bad size n=%lld", n);
  HWG_REQUIRE(n_parts == sheet_parts(n), "sheet_minmax: %d partials for %lld elements, hwg_sheet_parts says %d", n_parts, n, sheet_parts(n));
  HWG_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)partials & 3) == 0, "sheet_minmax: x and partials must be 4-byte aligned");
  hipLaunchKernelGGL(sheet_minmax_kernel, dim3(n_parts), dim3(SHEET_BLOCK), 0, (hipStream_t)stream, x, n, partials);
  HWG_LAUNCH_CHECK("sheet_minmax");
  return HWG_OK;
}

extern "C" int hwg_sheet_compose(const float* x, int B, int H, int W, int nrow, const float* partials, int n_parts, unsigned char* out,
                                 long long out_bytes, void* stream) {
  HWG_REQUIRE(x && partials && out, "sheet_compose: null argument");
  HWG_REQUIRE(B > 0 && H > 0 && W > 0, "sheet_compose: bad sizes B=%d H=%d W=%d", B, H, W);
  HWG_REQUIRE(nrow >= 1, "sheet_compose: nrow %d, need at least 1", nrow);
  HWG_REQUIRE(n_parts >= 1 && n_parts <= SHEET_MAX_PARTS, "sheet_compose: %d partials, between 1 and %d are folded", n_parts, SHEET_MAX_PARTS);
  const long long xmaps = nrow < B ? nrow : B, ymaps = (B + xmaps - 1) / xmaps;
  const long long Hs = B == 1 ? H : ((long long)H + 2) * ymaps + 2, Ws = B == 1 ? W : ((long long)W + 2) * xmaps + 2;
  HWG_REQUIRE(Hs <= 0x7fffffffll && Ws <= 0x7fffffffll && Hs * Ws <= 0x7fffffffll - 3, "sheet_compose: a sheet of %lld x %lld bytes does not fit int", Hs, Ws);
  const long long total = Hs * Ws, words = (total + 3) / 4;
  HWG_REQUIRE(out_bytes >= 4 * words, "sheet_compose: out holds %lld bytes, the sheet rounded up to 4 bytes needs %lld", out_bytes, 4 * words);
  HWG_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)partials & 3) == 0 && ((uintptr_t)out & 3) == 0, "sheet_compose: x, partials and out must be 4-byte aligned");
  SheetGeom g;
  g.B = B; g.H = H; g.W = W;
  g.xmaps = B == 1 ? 0 : (int)xmaps;
  g.Ws = (int)Ws; g.total = (int)total; g.words = (int)words;
  hipLaunchKernelGGL(sheet_compose_kernel, dim3(hwg_cdiv(words, SHEET_BLOCK)), dim3(SHEET_BLOCK), 0, (hipStream_t)stream, x, g, partials, n_parts,
                     (unsigned*)out);
  HWG_LAUNCH_CHECK("sheet_compose");
  return HWG_OK;
}

// ---- per-line means of a discriminator scale's prediction (the numbers of gen_text_*.txt) ----------------------------------------------
// out[r] = mean(src[r][0 .. n)) for r < rows, src rows `stride` floats apart: the reference's gp.mean(dim=1) on the host, here one
// workgroup per line, an fp32 sum (lane-strided, then the fixed shuffle tree) divided by n.
__global__ __launch_bounds__(SHEET_BLOCK) void sheet_row_means_kernel(const float* __restrict__ src, long long stride, int n, float* __restrict__ out) {
  __shared__ float smem[16];
  const float* row = src + (long long)blockIdx.x * stride;
  float s = 0.0f;
  for (int i = threadIdx.x; i < n; i += SHEET_BLOCK) s += row[i];
  s = block_sum_f(s, smem);
  if (threadIdx.x == 0) out[blockIdx.x] = s / (float)n;
}

extern "C" int hwg_sheet_row_means(const float* src, long long stride, int rows, int n, float* out, void* stream) {
  HWG_REQUIRE(src && out, "sheet_row_means: null argument");
  HWG_REQUIRE(rows > 0 && n > 0 && stride >= n, "sheet_row_means: bad sizes rows=%d n=%d stride=%lld", rows, n, stride);
  HWG_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)out & 3) == 0, "sheet_row_means: src and out must be 4-byte aligned");
  hipLaunchKernelGGL(sheet_row_means_kernel, dim3(rows), dim3(SHEET_BLOCK), 0, (hipStream_t)stream, src, stride, n, out);
  HWG_LAUNCH_CHECK("sheet_row_means");
  return HWG_OK;
}
