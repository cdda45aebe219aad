// Line augmentation on the collated batch: Tensmeyer brightness (Otsu threshold, foreground / background shifted) and the mesh warp of the
// reference's recogniser pre-training (utils/augmentation.py:5-31, utils/grid_distortion.py:11-66, called from datasets/hw_dataset.py:143-152,
// datasets/author_hw_dataset.py:429-432, datasets/author_rimeslines_dataset.py:428-434), which the reference runs per line in the loader
// workers through OpenCV and scipy.interpolate.griddata. Two launches for the whole ragged batch:
//   1. augment_stats_kernel: one workgroup per line - 256-bin histogram of the valid columns in LDS, Otsu threshold, brightness LUT, border level;
//   2. augment_warp_kernel : one workgroup per 64 columns of a line - the inverse map (piecewise linear over the triangulated control lattice)
//      and the bilinear resample of the LUT-mapped line.
// Image values are levels p = (1 - x) * 128 (integers 0..255; the padding value -1 is level 256, which no pixel has), outputs are 1 - level / 128.
//
// Tables (see include/hwg.h): lines_i [B][4] = {valid width w, lattice rows gy (0 = no warp), lattice columns gx, first valid column x_off},
// lines_f [B][lf_stride] = {foreground scale, background scale, row sigma, column sigma, src_y[GY], src_x[GX]},
// draws [B][draw_stride] = {fg, bg, row displacements [gy][gx], column displacements [gy][gx]} (unit draws, multiplied by the scales / sigmas).
#include "hwg_common.h"

constexpr int AUG_STATS = 258;          // per line: threshold, border level, LUT[256]
constexpr int AUG_TILE = 64;            // columns per workgroup of the warp kernel (one wavefront row)
constexpr int AUG_MAXR = 16;            // lattice rows held in LDS
constexpr int AUG_MAXC = 24;            // lattice columns a 64-column tile can touch (interval >= 6 px: 64 / 6 + 1 own + 2 x 2 neighbours)
constexpr float AUG_EPS = 5e-5f;        // a pixel this far (barycentric) outside its best triangle still counts as inside the mesh

__device__ __forceinline__ int aug_level(float v) {
  const int p = __float2int_rn((1.f - v) * 128.f);
  return min(max(p, 0), 255);
}

__global__ __launch_bounds__(512) void augment_stats_kernel(const float* __restrict__ x, const int* __restrict__ lines_i,
                                                            const float* __restrict__ lines_f, int lf_stride,
                                                            const float* __restrict__ draws, int draw_stride, int H, int W,
                                                            int* __restrict__ stats) {
  __shared__ int whist[8][256];          // one histogram per wavefront: only one lane of a wavefront writes at a time, no atomics
  __shared__ int hist[256];
  __shared__ double var[256];
  __shared__ int lut[256];
  __shared__ int thr;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int xoff = max(lines_i[4 * b + 3], 0);
  const int w = max(min(lines_i[4 * b], W - xoff), 0);
  for (int i = tid; i < 8 * 256; i += 512) (&whist[0][0])[i] = 0;
  __syncthreads();
  const float* img = x + (size_t)b * H * W + xoff;
  for (int y = wv; y < H; y += 8) {
    for (int x0 = 0; x0 < w; x0 += 64) {
      const int xl = x0 + lane;
      const bool valid = xl < w;
      const int p = valid ? aug_level(img[(size_t)y * W + xl]) : -1;
      // lines are mostly paper: most lanes of a wavefront hold the same level. The lanes that share the first pending lane's level are
      // counted with one ballot and added by that lane - a few rounds per wavefront row instead of a 64-way same-address conflict
      unsigned long long pending = __ballot(valid);
      while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int lv = __shfl(p, leader, 64);
        const unsigned long long same = __ballot(p == lv) & pending;
        if (lane == leader) whist[wv][lv] += __popcll(same);
        pending &= ~same;
      }
    }
  }
  __syncthreads();
  if (tid < 256) {
    int s = 0;
    for (int k = 0; k < 8; ++k) s += whist[k][tid];
    hist[tid] = s;
  }
  __syncthreads();
  const long long N = (long long)H * w;
  if (tid < 256) {
    // Otsu: between-class variance of the split {<= tid} / {> tid}, up to the common factor 1 / N^2: (s0 w1 - s1 w0)^2 / (w0 w1), the
    // integer parts exact, the square and the quotient each rounded once in fp64
    long long w0 = 0, s0 = 0, S = 0;
    for (int p = 0; p < 256; ++p) {
      const long long h = hist[p];
      S += h * p;
      if (p <= tid) { w0 += h; s0 += h * p; }
    }
    const long long w1 = N - w0, s1 = S - s0;
    double v = 0.0;
    if (w0 > 0 && w1 > 0) {
      const double d = (double)(s0 * w1 - s1 * w0);
      const double dd = d * d;
      v = dd / (double)(w0 * w1);
    }
    var[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    double best = 0.0;
    for (int p = 0; p < 256; ++p)
      if (var[p] > best) { best = var[p]; t = p; }      // lowest level on ties
    thr = t;
  }
  __syncthreads();
  if (tid < 256) {
    const float shift = lines_f[(size_t)b * lf_stride + (tid > thr ? 1 : 0)] * draws[(size_t)b * draw_stride + (tid > thr ? 1 : 0)];
    float f = (float)tid + shift;
    f = fminf(fmaxf(f, 0.f), 255.f);
    lut[tid] = (int)f;
    stats[(size_t)b * AUG_STATS + 2 + tid] = lut[tid];
  }
  __syncthreads();
  if (tid == 0) {
    long long sq = 0;
    for (int p = 0; p < 256; ++p) sq += (long long)hist[p] * lut[p];
    int m = 0;
    if (N > 0) m = (int)rint((double)sq / (double)N);    // the mean of the re-lit line, saturated to a level (half to even)
    stats[(size_t)b * AUG_STATS] = thr;
    stats[(size_t)b * AUG_STATS + 1] = min(max(m, 0), 255);
  }
}

// no fused multiply-adds below: the geometry is tested against a numpy restatement that rounds every product and sum
#pragma clang fp contract(off)
// barycentric coordinates of q in the triangle (p0, p1, p2), all in the cell's local frame (row, column); returns the smallest one
__device__ __forceinline__ float aug_bary(float qy, float qx, float p0y, float p0x, float p1y, float p1x, float p2y, float p2x, float& l0,
                                          float& l1, float& l2) {
  const float e1y = p1y - p0y, e1x = p1x - p0x, e2y = p2y - p0y, e2x = p2x - p0x, ry = qy - p0y, rx = qx - p0x;
  const float det = e1y * e2x - e1x * e2y;
  l1 = (ry * e2x - rx * e2y) / det;
  l2 = (e1y * rx - e1x * ry) / det;
  l0 = (1.f - l1) - l2;
  return fminf(l0, fminf(l1, l2));
}

__global__ __launch_bounds__(256) void augment_warp_kernel(const float* __restrict__ x, const int* __restrict__ lines_i,
                                                           const float* __restrict__ lines_f, int lf_stride,
                                                           const float* __restrict__ draws, int draw_stride, const int* __restrict__ stats,
                                                           int H, int W, int GY, int GX, float* __restrict__ yout, float* __restrict__ map_out) {
  __shared__ float lut[256];
  __shared__ float sy[AUG_MAXR], sx[AUG_MAXC];
  __shared__ float dy[AUG_MAXR][AUG_MAXC], dx[AUG_MAXR][AUG_MAXC];
  __shared__ int diag[AUG_MAXR][AUG_MAXC];
  const int b = blockIdx.y, X0 = blockIdx.x * AUG_TILE, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int xoff = max(lines_i[4 * b + 3], 0);
  const int w = max(min(lines_i[4 * b], W - xoff), 0);
  int gy = lines_i[4 * b + 1], gx = lines_i[4 * b + 2];
  const bool warp = gy >= 2 && gx >= 2 && gy <= GY && gx <= GX && gy <= AUG_MAXR && H > 5 && w > 5;
  const int X = X0 + lane;                 // column of the padded batch
  const int xl = X - xoff;                 // column of the line
  const float nanv = __int_as_float(0x7fc00000);
  float* yb = yout + (size_t)b * H * W;
  float* mb = map_out ? map_out + (size_t)b * 2 * H * W : nullptr;
  const int xa = max(X0 - xoff, 0), xb = min(X0 + AUG_TILE - 1 - xoff, w - 1);       // the tile's valid columns, line coordinates
  if (xa > xb) {                           // padding only
    if (X < W)
      for (int y = wv; y < H; y += 4) {
        yb[(size_t)y * W + X] = -1.f;
        if (mb) { mb[(size_t)y * W + X] = nanv; mb[((size_t)H + y) * W + X] = nanv; }
      }
    return;
  }
  const int m_i = stats[(size_t)b * AUG_STATS + 1];
  const float m = (float)m_i;
  lut[tid] = (float)stats[(size_t)b * AUG_STATS + 2 + tid];
  int jlo = 0, nc = 0;
  float hi = 1.f, wi = 1.f;
  if (warp) {
    const float* lf = lines_f + (size_t)b * lf_stride;
    const float* dr = draws + (size_t)b * draw_stride + 2;
    hi = lf[4 + 1] - lf[4];
    wi = lf[4 + GY + 1] - lf[4 + GY];
    jlo = max((int)((float)xa / wi) - 1, 0);
    const int jhi = min((int)((float)xb / wi) + 2, gx - 1);
    nc = min(jhi - jlo + 1, AUG_MAXC);
    const float sgy = lf[2], sgx = lf[3];
    if (tid < gy) sy[tid] = lf[4 + tid];
    if (tid < nc) sx[tid] = lf[4 + GY + jlo + tid];
    for (int k = tid; k < gy * nc; k += 256) {
      const int i = k / nc, j = k - i * nc;
      dy[i][j] = sgy * dr[i * gx + jlo + j];
      dx[i][j] = sgx * dr[gy * gx + i * gx + jlo + j];
    }
  }
  __syncthreads();
  if (warp) {
    // per cell: the diagonal that is locally Delaunay for its four displaced corners a (i,j), b (i,j+1), c (i+1,j+1), d (i+1,j):
    // a-c unless d lies inside the circumcircle of (a, b, c); evaluated in fp64 in the cell's local frame
    for (int k = tid; k < (gy - 1) * (nc - 1); k += 256) {
      const int i = k / (nc - 1), j = k - i * (nc - 1);
      const double ch = (double)sy[i + 1] - (double)sy[i], cw = (double)sx[j + 1] - (double)sx[j];
      const double ay = dy[i][j], ax = dx[i][j], by = dy[i][j + 1], bx = cw + dx[i][j + 1];
      const double cy = ch + dy[i + 1][j + 1], cx = cw + dx[i + 1][j + 1], ddy = ch + dy[i + 1][j], ddx = dx[i + 1][j];
      const double orient = (by - ay) * (cx - ax) - (bx - ax) * (cy - ay);
      const double a0 = ay - ddy, a1 = ax - ddx, a2 = a0 * a0 + a1 * a1;
      const double b0 = by - ddy, b1 = bx - ddx, b2 = b0 * b0 + b1 * b1;
      const double c0 = cy - ddy, c1 = cx - ddx, c2 = c0 * c0 + c1 * c1;
      const double inc = a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0);
      diag[i][j] = (orient > 0.0 ? inc : -inc) > 0.0 ? 1 : 0;
    }
  }
  __syncthreads();
  const float* img = x + (size_t)b * H * W + xoff;
  if (X >= W) return;
  for (int y = wv; y < H; y += 4) {
    const size_t o = (size_t)y * W + X;
    if (xl < 0 || xl >= w) {
      yb[o] = -1.f;
      if (mb) { mb[o] = nanv; mb[o + (size_t)H * W] = nanv; }
      continue;
    }
    if (!warp) {
      yb[o] = 1.f - lut[aug_level(img[(size_t)y * W + xl])] * (1.f / 128.f);
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
      const float ch = sy[i + 1] - sy[i], cw = sx[j + 1] - sx[j];
      const float qy = (float)y - sy[i], qx = (float)xl - sx[j];
      const float ay = dy[i][j], ax = dx[i][j], by = dy[i][j + 1], bx = cw + dx[i][j + 1];
      const float cy = ch + dy[i + 1][j + 1], cx = cw + dx[i + 1][j + 1], ddy = ch + dy[i + 1][j], ddx = dx[i + 1][j];
      const int f = diag[i][j];
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
          my = (float)y - ((l0 * dy[r0][c0] + l1 * dy[r1][c1]) + l2 * dy[r2][c2]);
          mx = (float)xl - ((l0 * dx[r0][c0] + l1 * dx[r1][c1]) + l2 * dx[r2][c2]);
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
      v[k] = (yy >= 0 && yy < H && xx >= 0 && xx < w) ? lut[aug_level(img[(size_t)yy * W + xx])] : m;
    }
    const float top = v[0] + fx * (v[1] - v[0]), bot = v[2] + fx * (v[3] - v[2]);
    const float val = top + fy * (bot - top);
    const int level = min(max(__float2int_rn(val), 0), 255);
    yb[o] = 1.f - (float)level * (1.f / 128.f);
  }
}

extern "C" int hwg_augment_stats(const float* x, const int* lines_i, const float* lines_f, int lf_stride, const float* draws, int draw_stride,
                                 int B, int H, int W, int* stats, void* stream) {
  HWG_REQUIRE(x && lines_i && lines_f && draws && stats && B > 0 && H > 0 && W > 0, "augment_stats: bad arguments");
  HWG_REQUIRE(lf_stride >= 4 && draw_stride >= 2, "augment_stats: table strides too small");
  HWG_REQUIRE((long long)H * W <= (1LL << 22), "augment_stats: line of %d x %d pixels is too large for the exact fp64 Otsu sums", H, W);
  hipLaunchKernelGGL(augment_stats_kernel, dim3(B), dim3(512), 0, (hipStream_t)stream, x, lines_i, lines_f, lf_stride, draws, draw_stride, H, W, stats);
  HWG_LAUNCH_CHECK("augment_stats");
  return HWG_OK;
}

extern "C" int hwg_augment_warp(const float* x, const int* lines_i, const float* lines_f, int lf_stride, const float* draws, int draw_stride,
                                const int* stats, int B, int H, int W, int GY, int GX, float* y, float* map_out, void* stream) {
  HWG_REQUIRE(x && lines_i && lines_f && draws && stats && y && y != x && B > 0 && H > 0 && W > 0, "augment_warp: bad arguments");
  HWG_REQUIRE(GY >= 0 && GX >= 0 && GY <= AUG_MAXR, "augment_warp: %d lattice rows (at most %d: lines up to ~190 px high)", GY, AUG_MAXR);
  HWG_REQUIRE(lf_stride >= 4 + GY + GX && (long long)draw_stride >= 2 + 2LL * GY * GX, "augment_warp: table strides too small for a %d x %d lattice", GY, GX);
  HWG_REQUIRE(B <= 65535, "augment_warp: batch too large");
  hipLaunchKernelGGL(augment_warp_kernel, dim3(hwg_cdiv(W, AUG_TILE), B), dim3(256), 0, (hipStream_t)stream, x, lines_i, lines_f, lf_stride, draws,
                     draw_stride, stats, H, W, GY, GX, y, map_out);
  HWG_LAUNCH_CHECK("augment_warp");
  return HWG_OK;
}
