// What the two executions of the line augmentation share (augment.hip: on the collated fp32 batch; store_warp.hip: on the bytes of the
// device-resident line store): the brightness LUT entry and the mesh warp of one 64-column tile of one line. One source, so that the two
// kernels cannot differ in an operation or in its order - their outputs are compared bit for bit (tests/test_line_store_warp_gpu.py).
#pragma once
#include "hwg_common.h"

constexpr int AUG_STATS = 258;          // per line: threshold, border level, LUT[256]
constexpr int AUG_TILE = 64;            // columns per workgroup of the warp kernels (one wavefront row)
constexpr int AUG_MAXR = 16;            // lattice rows held in LDS
constexpr int AUG_MAXC = 24;            // lattice columns a 64-column tile can touch (interval >= 6 px: 64 / 6 + 1 own + 2 x 2 neighbours)
constexpr float AUG_EPS = 5e-5f;        // a pixel this far (barycentric) outside its best triangle still counts as inside the mesh

__device__ __forceinline__ int aug_level(float v) {
  const int p = __float2int_rn((1.f - v) * 128.f);
  return min(max(p, 0), 255);
}

// LUT q(p) = trunc(clamp(p + scale * draw, 0, 255)), the foreground pair of (scale, draw) for p <= thr and the background pair above it.
// The product and the sum are ONE rounding (a fused multiply-add, written out so that no compiler decides it per kernel).
__device__ __forceinline__ int aug_lut_entry(int p, int thr, const float* __restrict__ lf, const float* __restrict__ dr) {
  const int side = p > thr ? 1 : 0;
  float f = __fmaf_rn(lf[side], dr[side], (float)p);
  f = fminf(fmaxf(f, 0.f), 255.f);
  return (int)f;
}

// border level: the mean of the re-lit line, sq = sum hist[p] * lut[p] over N pixels, saturated to a level (half to even)
__device__ __forceinline__ int aug_border_level(long long sq, long long N) {
  int m = 0;
  if (N > 0) m = (int)rint((double)sq / (double)N);
  return min(max(m, 0), 255);
}

// barycentric coordinates of q in the triangle (p0, p1, p2), all in the cell's local frame (row, column); returns the smallest one
// (no fused multiply-adds here and in aug_warp_tile: the geometry is tested against a numpy restatement that rounds every product and sum)
__device__ __forceinline__ float aug_bary(float qy, float qx, float p0y, float p0x, float p1y, float p1x, float p2y, float p2x, float& l0,
                                          float& l1, float& l2) {
#pragma clang fp contract(off)
  const float e1y = p1y - p0y, e1x = p1x - p0x, e2y = p2y - p0y, e2x = p2x - p0x, ry = qy - p0y, rx = qx - p0x;
  const float det = e1y * e2x - e1x * e2y;
  l1 = (ry * e2x - rx * e2y) / det;
  l2 = (e1y * rx - e1x * ry) / det;
  l0 = (1.f - l1) - l2;
  return fminf(l0, fminf(l1, l2));
}

struct AugTileLds {
  float lut[256];                        // the caller's: written by all 256 threads before aug_warp_tile (its first barrier publishes it)
  float sy[AUG_MAXR], sx[AUG_MAXC];
  float dy[AUG_MAXR][AUG_MAXC], dx[AUG_MAXR][AUG_MAXC];
  int diag[AUG_MAXR][AUG_MAXC];
};

// One workgroup of 256 threads: the columns X0 .. X0 + 63 of output row `yb` [H][W] (and of `mb` [2][H][W], optional) that show a line of w
// columns beginning at column xoff. tap(yy, xx) -> the level (0..255) of pixel (yy, xx) of the line, called for 0 <= yy < H, 0 <= xx < w
// only. m: the border level; warp: lattice gy x gx usable (the caller's test), lf = the line's row of lines_f, dr = its row of draws + 2.
// Every thread of the workgroup calls it (two barriers inside); the tile has at least one valid column.
template <class Tap>
__device__ __forceinline__ void aug_warp_tile(AugTileLds& s, const Tap& tap, float m, bool warp, int gy, int gx, int GY,
                                              const float* __restrict__ lf, const float* __restrict__ dr, int H, int W, int w, int xoff, int X0,
                                              float* __restrict__ yb, float* __restrict__ mb) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int X = X0 + lane;                 // column of the padded batch
  const int xl = X - xoff;                 // column of the line
  const float nanv = __int_as_float(0x7fc00000);
  const int xa = max(X0 - xoff, 0), xb = min(X0 + AUG_TILE - 1 - xoff, w - 1);       // the tile's valid columns, line coordinates
  int jlo = 0, nc = 0;
  float hi = 1.f, wi = 1.f;
  if (warp) {
    hi = lf[4 + 1] - lf[4];
    wi = lf[4 + GY + 1] - lf[4 + GY];
    jlo = max((int)((float)xa / wi) - 1, 0);
    const int jhi = min((int)((float)xb / wi) + 2, gx - 1);
    nc = min(jhi - jlo + 1, AUG_MAXC);
    const float sgy = lf[2], sgx = lf[3];
    if (tid < gy) s.sy[tid] = lf[4 + tid];
    if (tid < nc) s.sx[tid] = lf[4 + GY + jlo + tid];
    for (int k = tid; k < gy * nc; k += 256) {
      const int i = k / nc, j = k - i * nc;
      s.dy[i][j] = sgy * dr[i * gx + jlo + j];
      s.dx[i][j] = sgx * dr[gy * gx + i * gx + jlo + j];
    }
  }
  __syncthreads();
  if (warp) {
    // per cell: the diagonal that is locally Delaunay for its four displaced corners a (i,j), b (i,j+1), c (i+1,j+1), d (i+1,j):
    // a-c unless d lies inside the circumcircle of (a, b, c); evaluated in fp64 in the cell's local frame
    for (int k = tid; k < (gy - 1) * (nc - 1); k += 256) {
      const int i = k / (nc - 1), j = k - i * (nc - 1);
      const double ch = (double)s.sy[i + 1] - (double)s.sy[i], cw = (double)s.sx[j + 1] - (double)s.sx[j];
      const double ay = s.dy[i][j], ax = s.dx[i][j], by = s.dy[i][j + 1], bx = cw + s.dx[i][j + 1];
      const double cy = ch + s.dy[i + 1][j + 1], cx = cw + s.dx[i + 1][j + 1], ddy = ch + s.dy[i + 1][j], ddx = s.dx[i + 1][j];
      const double orient = (by - ay) * (cx - ax) - (bx - ax) * (cy - ay);
      const double a0 = ay - ddy, a1 = ax - ddx, a2 = a0 * a0 + a1 * a1;
      const double b0 = by - ddy, b1 = bx - ddx, b2 = b0 * b0 + b1 * b1;
      const double c0 = cy - ddy, c1 = cx - ddx, c2 = c0 * c0 + c1 * c1;
      const double inc = a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0);
      s.diag[i][j] = (orient > 0.0 ? inc : -inc) > 0.0 ? 1 : 0;
    }
  }
  __syncthreads();
  if (X >= W) return;
  for (int y = wv; y < H; y += 4) {
    const size_t o = (size_t)y * W + X;
    if (xl < 0 || xl >= w) {
      yb[o] = -1.f;
      if (mb) { mb[o] = nanv; mb[o + (size_t)H * W] = nanv; }
      continue;
    }
    if (!warp) {
      yb[o] = 1.f - s.lut[tap(y, xl)] * (1.f / 128.f);
      if (mb) { mb[o] = (float)y; mb[o + (size_t)H * W] = (float)xl; }
      continue;
    }
    const int i0 = min(max((int)((float)y / hi), 0), gy - 2);
    const int j0 = min(max((int)((float)xl / wi), 0), gx - 2);
    float best = -INFINITY, my = 0.f, mx = 0.f;
    for (int c = 0; c < 9 && best < 0.f; ++c) {
      const int ci = c / 3, cj = c - ci * 3;
      const int i = i0 + (ci == 0 ? 0 : ci == 1 ? -1 : 1), j = j0 + (cj == 0 ? 0 : cj == 1 ? -1 : 1) - jlo;
      if (i < 0 || i > gy - 2 || j < 0 || j > nc - 2) continue;
      const float ch = s.sy[i + 1] - s.sy[i], cw = s.sx[j + 1] - s.sx[j];
      const float qy = (float)y - s.sy[i], qx = (float)xl - s.sx[j];
      const float ay = s.dy[i][j], ax = s.dx[i][j], by = s.dy[i][j + 1], bx = cw + s.dx[i][j + 1];
      const float cy = ch + s.dy[i + 1][j + 1], cx = cw + s.dx[i + 1][j + 1], ddy = ch + s.dy[i + 1][j], ddx = s.dx[i + 1][j];
      const int f = s.diag[i][j];
      for (int t = 0; t < 2 && best < 0.f; ++t) {
        // corners 0 a, 1 b, 2 c, 3 d; a-c diagonal: (a,b,c) (a,c,d); b-d diagonal: (a,b,d) (b,c,d)
        const int idx = f * 2 + t;
        const int k0 = idx == 3 ? 1 : 0, k1 = (idx & 1) ? 2 : 1, k2 = idx == 0 ? 2 : 3;
        const float p0y = k0 ? by : ay, p0x = k0 ? bx : ax;
        const float p1y = k1 == 1 ? by : cy, p1x = k1 == 1 ? bx : cx;
        const float p2y = k2 == 2 ? cy : ddy, p2x = k2 == 2 ? cx : ddx;
        float l0, l1, l2;
        const float mn = aug_bary(qy, qx, p0y, p0x, p1y, p1x, p2y, p2x, l0, l1, l2);
        if (mn > best) {
          best = mn;
          // source = destination - displacement at every lattice point, so the interpolated source is the pixel minus the interpolated displacement
          const int r0 = i, c0 = j + k0;
          const int r1 = i + (k1 >> 1), c1 = j + 1;
          const int r2 = i + 1, c2 = j + (k2 == 2 ? 1 : 0);
          my = (float)y - ((l0 * s.dy[r0][c0] + l1 * s.dy[r1][c1]) + l2 * s.dy[r2][c2]);
          mx = (float)xl - ((l0 * s.dx[r0][c0] + l1 * s.dx[r1][c1]) + l2 * s.dx[r2][c2]);
        }
      }
    }
    if (!(best >= -AUG_EPS)) {             // outside the mesh: the border level
      yb[o] = 1.f - m * (1.f / 128.f);
      if (mb) { mb[o] = nanv; mb[o + (size_t)H * W] = nanv; }
      continue;
    }
    if (mb) { mb[o] = my; mb[o + (size_t)H * W] = mx; }
    const float fy0 = floorf(my), fx0 = floorf(mx);
    const float fy = my - fy0, fx = mx - fx0;
    // (maps far outside the line are all border; the clamp keeps the integer conversion defined)
    const int y0 = (int)fminf(fmaxf(fy0, -2.f), (float)H), x0 = (int)fminf(fmaxf(fx0, -2.f), (float)w);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
      v[k] = (yy >= 0 && yy < H && xx >= 0 && xx < w) ? s.lut[tap(yy, xx)] : m;
    }
    const float top = v[0] + fx * (v[1] - v[0]), bot = v[2] + fx * (v[3] - v[2]);
    const float val = top + fy * (bot - top);
    const int level = min(max(__float2int_rn(val), 0), 255);
    yb[o] = 1.f - (float)level * (1.f / 128.f);
  }
}

// the columns X0 .. X0 + 63 of a row that shows no line there: padding, no map
__device__ __forceinline__ void aug_padding_tile(int H, int W, int X0, float* __restrict__ yb, float* __restrict__ mb) {
  const int tid = threadIdx.x, X = X0 + (tid & 63), wv = tid >> 6;
  const float nanv = __int_as_float(0x7fc00000);
  if (X < W)
    for (int y = wv; y < H; y += 4) {
      yb[(size_t)y * W + X] = -1.f;
      if (mb) { mb[(size_t)y * W + X] = nanv; mb[((size_t)H + y) * W + X] = nanv; }
    }
}
