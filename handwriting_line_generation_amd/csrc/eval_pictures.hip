// Evaluation pictures (new_eval.py): per held-out line the real line above its reconstruction, framed, optionally with a caption strip.
// The reference builds this picture on the host (evaluators/hwdataset_eval.py:141-262): it downloads the fp32 batch and the fp32
// reconstruction, builds a float64 array per line with numpy, paints the frames through indexed assignments and hands the array to OpenCV.
// Here the finished 8-bit RGB pictures of the whole batch are made in ONE launch; 3 bytes per picture pixel cross to the host instead of
// 4 bytes per pixel of either input.
//
// image [B][1][H][Wi] fp32, recon [B][1][H][Wr] fp32 -> out [B][Hp][Wp][3] uint8 (interleaved RGB), Wp = max(Wi, Wr), Hp = 2H + 2 + S,
// S = EVAL_STRIP (50) with a caption strip, else 0.
//
// LEVEL of an input value x (eval_level): v = 1 - (1 + x) / 2, every operation a correctly rounded fp32 one (the reference's float32 numpy
// expression), then trunc(v * 255) with the EXACT product: the reference's picture is float64 by the time it multiplies, and fp32 x 255
// is exact in fp64 (24 + 8 significant bits). Does the rounded fp32 product give the same byte? YES: an exhaustive host scan over all
// 1065353217 fp32 values v in [0, 1] (every bit pattern from 0 to 0x3f800000, the fp32 product rounded to nearest against the fp64 one,
// both truncated) finds no v at which the two bytes differ - the rounded product never reaches an integer that the exact one stays
// below. So the kernel multiplies in fp32, without any fp64 or fma residual. Values outside [0, 255] are clamped and NaN is 0 (the
// reference's cast wraps there; hwg_lines_to_u8 makes the same choice). This is not hwg_lines_to_u8's (1 - x) * 127.5: on the 2304
// edge values x = fp32(1 - 2k/255) +- 0..4 ulp the two bytes differ 215 times.
//
// LAYOUT of one picture. dif = |Wi - Wr|; the narrower input is centred: dif / 2 columns of level 0 on its left, the rest on its right.
// pr = dif / 2 if the real line is the narrower one, else 0; pg the same for the reconstruction.
//   rows 0 .. H-1        the real line                         rows H, H+1   level 0
//   rows H+2 .. 2H+1     the reconstruction                    rows 2H+2 ..  the caption strip (level 0 and glyphs)
//   real frame, GREEN (0,255,0):  rows 0 and H, columns [pr, Wp - pr);      rows 0 .. H-1, columns pr and Wp-1-pr
//   recon frame, BLUE (0,0,255):  rows H+1 and 2H+1, columns [pg, Wp - pg);  rows H+2 .. 2H+1, columns pg and Wp-1-pg
// (the reference paints channel 1 and channel 0 of an array that OpenCV reads as BGR: green and blue in the written file; the bytes here
// are RGB in the order PIL takes them). The two frames never meet.
//   caption: glyph cell j of line b is atlas[codes[b][j]] ([gh][gw] grey bytes) at columns 2 + j gw .. , rows centred in the strip
//   ((S - gh) / 2 from its top); a negative code leaves the cell empty, cells are clipped at Wp, a code >= G draws nothing.
//
// MAPPING: output-centred, as sheet_compose_kernel. A lane owns 4 consecutive bytes of the flat output = parts of at most two pixels: it
// builds the 24 bits of pixel q = 4 word / 3 and of pixel q + 1, shifts the 48 bits by the word's phase and makes ONE aligned 32-bit
// store. Every byte of out is written; the tail word's bytes behind the last picture are 0: out holds the size rounded up to 4.
// No atomics, no LDS, nothing crosses a workgroup.
#include <math.h>
#include "hwg_common.h"

constexpr int EVAL_BLOCK = 256;
constexpr int EVAL_STRIP = 50;

struct EvalGeom {
  int B, H, Wi, Wr, Wp, Hp;
  int pr, pg;        // left padding of the real line / of the reconstruction
  int S;             // strip rows (0: none)
  int L, G, gh, gw;  // caption cells per line, glyphs in the atlas, glyph cell size
  int gtop;          // first picture row of the glyph cells
  int npix;          // B * Hp * Wp
  int words;         // 32-bit words that cover 3 * npix bytes
};

__device__ __forceinline__ unsigned eval_level(float x) {
#pragma clang fp contract(off)
  const float s = 1.0f + x;
  const float h = s / 2.0f;
  const float v = 1.0f - h;
  if (v != v) return 0u;
  const float p = v * 255.0f;                               // same byte as the exact product for every v in [0, 1] (see the top)
  return (unsigned)(int)fminf(fmaxf(p, 0.0f), 255.0f);
}

// the 24 bits (R | G << 8 | B << 16) of picture pixel q
__device__ __forceinline__ unsigned eval_pixel(int q, const EvalGeom& g, const float* __restrict__ image, const float* __restrict__ recon,
                                               const unsigned char* __restrict__ atlas, const int* __restrict__ codes) {
  const int per = g.Hp * g.Wp;
  const int b = q / per, rem = q - b * per;
  const int r = rem / g.Wp, c = rem - r * g.Wp;
  const int H = g.H;
  unsigned level = 0u;
  if (r < H) {
    if (c == g.pr || c == g.Wp - 1 - g.pr || (r == 0 && c >= g.pr && c < g.Wp - g.pr)) return 0x00ff00u;           // green
    const int x = c - g.pr;
    if (x >= 0 && x < g.Wi) level = eval_level(image[((long long)b * H + r) * g.Wi + x]);
  } else if (r == H) {
    if (c >= g.pr && c < g.Wp - g.pr) return 0x00ff00u;
  } else if (r == H + 1) {
    if (c >= g.pg && c < g.Wp - g.pg) return 0xff0000u;                                                             // blue
  } else if (r < 2 * H + 2) {
    const int y = r - H - 2;
    if (c == g.pg || c == g.Wp - 1 - g.pg || (y == H - 1 && c >= g.pg && c < g.Wp - g.pg)) return 0xff0000u;
    const int x = c - g.pg;
    if (x >= 0 && x < g.Wr) level = eval_level(recon[((long long)b * H + y) * g.Wr + x]);
  } else {
    const int gy = r - g.gtop, cc = c - 2;
    if (gy >= 0 && gy < g.gh && cc >= 0) {
      const int j = cc / g.gw;
      if (j < g.L) {
        const int code = codes[b * g.L + j];
        if (code >= 0 && code < g.G) level = atlas[((long long)code * g.gh + gy) * g.gw + (cc - j * g.gw)];
      }
    }
  }
  return level * 0x010101u;
}

__global__ __launch_bounds__(EVAL_BLOCK) void eval_pairs_kernel(const float* __restrict__ image, const float* __restrict__ recon, EvalGeom g,
                                                                const unsigned char* __restrict__ atlas, const int* __restrict__ codes,
                                                                unsigned* __restrict__ out) {
  const int word = blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (word >= g.words) return;
  const long long first = 4ll * word;                        // < 3 * npix for every word < words
  const int q = (int)(first / 3), phase = (int)(first - 3ll * q);
  unsigned long long bits = eval_pixel(q, g, image, recon, atlas, codes);
  if (q + 1 < g.npix) bits |= (unsigned long long)eval_pixel(q + 1, g, image, recon, atlas, codes) << 24;
  out[word] = (unsigned)(bits >> (8 * phase));                // phase 0: q's 3 bytes + 1 of q + 1; phase 1: 2 + 2; phase 2: 1 + 3
}

extern "C" int hwg_eval_strip_rows(void) { return EVAL_STRIP; }

extern "C" int hwg_eval_pairs(const float* image, const float* recon, int B, int H, int Wi, int Wr, const unsigned char* atlas, int G, int gh,
                              int gw, const int* codes, int L, unsigned char* out, long long out_bytes, void* stream) {
  HWG_REQUIRE(image && recon && out, "eval_pairs: null argument");
  HWG_REQUIRE(B > 0 && H > 0 && Wi > 0 && Wr > 0, "eval_pairs: bad sizes B=%d H=%d Wi=%d Wr=%d", B, H, Wi, Wr);
  const bool strip = codes != nullptr;
  if (strip) {
    HWG_REQUIRE(atlas, "eval_pairs: caption codes without a glyph atlas");
    HWG_REQUIRE(G > 0 && gw > 0 && gh > 0 && gh <= EVAL_STRIP && L > 0, "eval_pairs: bad caption sizes G=%d gh=%d gw=%d L=%d (gh at most %d)", G,
                gh, gw, L, EVAL_STRIP);
    HWG_REQUIRE((long long)B * L <= 0x7fffffffll && (long long)G * gh * gw <= 0x7fffffffll, "eval_pairs: caption tables do not fit int");
    HWG_REQUIRE(((uintptr_t)codes & 3) == 0, "eval_pairs: codes must be 4-byte aligned");
  }
  const long long Wp = Wi > Wr ? Wi : Wr, Hp = 2ll * H + 2 + (strip ? EVAL_STRIP : 0);
  const long long npix = (long long)B * Hp * Wp;
  HWG_REQUIRE(Hp <= 0x7fffffffll && 3 * npix <= 0x7fffffffll - 3, "eval_pairs: %d pictures of %lld x %lld x 3 bytes do not fit int", B, Hp, Wp);
  const long long words = (3 * npix + 3) / 4;
  HWG_REQUIRE(out_bytes >= 4 * words, "eval_pairs: out holds %lld bytes, the pictures rounded up to 4 bytes need %lld", out_bytes, 4 * words);
  HWG_REQUIRE(((uintptr_t)image & 3) == 0 && ((uintptr_t)recon & 3) == 0 && ((uintptr_t)out & 3) == 0,
              "eval_pairs: image, recon and out must be 4-byte aligned");
  EvalGeom g;
  g.B = B; g.H = H; g.Wi = Wi; g.Wr = Wr; g.Wp = (int)Wp; g.Hp = (int)Hp;
  const int dif = Wi > Wr ? Wi - Wr : Wr - Wi;
  g.pr = Wi < Wr ? dif / 2 : 0;
  g.pg = Wr < Wi ? dif / 2 : 0;
  g.S = strip ? EVAL_STRIP : 0;
  g.L = strip ? L : 0; g.G = strip ? G : 0; g.gh = strip ? gh : 1; g.gw = strip ? gw : 1;
  g.gtop = 2 * H + 2 + (EVAL_STRIP - g.gh) / 2;
  g.npix = (int)npix; g.words = (int)words;
  hipLaunchKernelGGL(eval_pairs_kernel, dim3(hwg_cdiv(words, EVAL_BLOCK)), dim3(EVAL_BLOCK), 0, (hipStream_t)stream, image, recon, g, atlas, codes,
                     (unsigned*)out);
  HWG_LAUNCH_CHECK("eval_pairs");
  return HWG_OK;
}
