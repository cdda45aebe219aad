"""numpy restatement of the line augmentation (csrc/augment.hip; reference: utils/augmentation.py:5-31, utils/grid_distortion.py:11-66) for
the tests: Otsu threshold / brightness LUT / border level in exact integers + fp64, the inverse map of the mesh warp in a chosen precision
(fp64 = the yardstick; float32 = the same formulas at the kernel's precision, whose distance from fp64 sets the tests' bound), and the fp64
bilinear resample. Test infrastructure, not product code."""
import numpy as np

# a pixel this far (barycentric) outside its best triangle still counts as inside the mesh: rounding must not open holes along the edges
# between triangles. float32: the kernel's constant; fp64: nine orders above the rounding error, far below anything a test resolves
EPS = {np.float32: 5e-5, np.float64: 1e-9}
CELL_ORDER = [(0, 0), (0, -1), (0, 1), (-1, 0), (-1, -1), (-1, 1), (1, 0), (1, -1), (1, 1)]
# corners of a cell: 0 a (i,j), 1 b (i,j+1), 2 c (i+1,j+1), 3 d (i+1,j); triangles of the a-c diagonal, then of the b-d diagonal
TRIANGLES = {0: [(0, 1, 2), (0, 2, 3)], 1: [(0, 1, 3), (1, 2, 3)]}
CORNER_RC = [(0, 0), (0, 1), (1, 1), (1, 0)]


def lattice(h, w, interval=12):
    """grid_distortion.py:25-41: intervals fitted to the image, np.mgrid with a float step -> (src_y, src_x)"""
    w_ratio = max(1, round(w / float(interval)))
    h_ratio = max(1, round(h / float(interval)))
    wi, hi = w / w_ratio, h / h_ratio
    src = np.mgrid[0:h + hi:hi, 0:w + wi:wi]
    return src[0][:, 0].copy(), src[1][0, :].copy()


def levels(x):
    """image values 1 - p/128 -> integer levels p"""
    return np.rint((1.0 - np.asarray(x, dtype=np.float64)) * 128.0).astype(np.int64)


def otsu_variances(hist):
    """between-class variance (times N^2) of every split {<= t} / {> t}: (s0 w1 - s1 w0)^2 / (w0 w1), integers exact, two fp64 roundings"""
    hist = np.asarray(hist, dtype=np.int64)
    p = np.arange(256, dtype=np.int64)
    w0, s0 = np.cumsum(hist), np.cumsum(hist * p)
    w1, s1 = w0[-1] - w0, s0[-1] - s0
    d = (s0 * w1 - s1 * w0).astype(np.float64)
    ok = (w0 > 0) & (w1 > 0)
    return np.where(ok, (d * d) / np.maximum(w0 * w1, 1).astype(np.float64), 0.0), w0


def stats(level_img, fg, bg):
    """-> (t, lut int64[256], m): Otsu threshold (lowest level of the best split), LUT trunc(clamp(p + (p > t ? bg : fg), 0, 255)) in float32
    (augmentation.py:11-22: a float32 image plus the shifts, clamp, astype(uint8)), border level round-half-even(mean of the re-lit line)"""
    hist = np.bincount(np.asarray(level_img).reshape(-1), minlength=256)[:256]
    var, _ = otsu_variances(hist)
    t = int(np.argmax(var))
    p = np.arange(256)
    f = p.astype(np.float32) + np.where(p > t, np.float32(bg), np.float32(fg)).astype(np.float32)
    lut = np.clip(f, np.float32(0), np.float32(255)).astype(np.int64)
    m = int(np.clip(np.rint(float((hist * lut).sum()) / float(hist.sum())), 0, 255))
    return t, lut, m


def split_margin(hist):
    """relative gap between the best between-class variance and the best one among the candidates that split the histogram differently"""
    var, w0 = otsu_variances(hist)
    t = int(np.argmax(var))
    other = var[w0 != w0[t]]
    return float("inf") if not len(other) or var[t] == 0 else float((var[t] - other.max()) / var[t])


def cell_diagonals(sy, sx, dy, dx):
    """[gy-1, gx-1] bool: True where the b-d diagonal is the locally Delaunay one (d inside the circumcircle of a, b, c), fp64, cell-local frame"""
    sy, sx, dy, dx = (np.asarray(v, dtype=np.float64) for v in (sy, sx, dy, dx))
    ch, cw = (sy[1:] - sy[:-1])[:, None], (sx[1:] - sx[:-1])[None, :]
    ay, ax = dy[:-1, :-1], dx[:-1, :-1]
    by, bx = dy[:-1, 1:], cw + dx[:-1, 1:]
    cy, cx = ch + dy[1:, 1:], cw + dx[1:, 1:]
    ddy, ddx = ch + dy[1:, :-1], dx[1:, :-1]
    orient = (by - ay) * (cx - ax) - (bx - ax) * (cy - ay)
    a0, a1 = ay - ddy, ax - ddx
    b0, b1 = by - ddy, bx - ddx
    c0, c1 = cy - ddy, cx - ddx
    a2, b2, c2 = a0 * a0 + a1 * a1, b0 * b0 + b1 * b1, c0 * c0 + c1 * c1
    inc = a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0)
    return np.where(orient > 0, inc, -inc) > 0


def warp_map(H, w, src_y, src_x, disp_y, disp_x, dtype=np.float64):
    """inverse map of the mesh warp for the pixels of an H x w line: piecewise-linear interpolation of (lattice + displacement) -> lattice over
    the lattice cells, each split along its locally Delaunay diagonal; a pixel's triangle is searched among the 3 x 3 cells around its
    undisplaced cell (first triangle that contains it, else the nearest one if within EPS[dtype]). Arithmetic in `dtype`, cell-local frame, the
    source written as pixel - interpolated displacement. -> dict(map_y, map_x (NaN outside the mesh), inside, border = the chosen triangle's
    barycentric coordinate with respect to the mesh border (inf for a triangle without a border edge))"""
    T = dtype
    sy, sx = np.asarray(src_y).astype(T), np.asarray(src_x).astype(T)
    dy, dx = np.asarray(disp_y).astype(T), np.asarray(disp_x).astype(T)
    gy, gx = len(sy), len(sx)
    diag = cell_diagonals(sy, sx, dy, dx)
    hi, wi = sy[1] - sy[0], sx[1] - sx[0]
    Y, X = np.mgrid[0:H, 0:w]
    Yf, Xf = Y.astype(T), X.astype(T)
    i0 = np.clip((Yf / hi).astype(np.int64), 0, gy - 2)
    j0 = np.clip((Xf / wi).astype(np.int64), 0, gx - 2)
    best = np.full((H, w), -np.inf, dtype=T)
    my, mx = np.zeros((H, w), dtype=T), np.zeros((H, w), dtype=T)
    border = np.full((H, w), np.inf, dtype=T)
    one = T(1)
    with np.errstate(all="ignore"):
        for di, dj in CELL_ORDER:
            i, j = i0 + di, j0 + dj
            ok = (i >= 0) & (i <= gy - 2) & (j >= 0) & (j <= gx - 2)
            i, j = np.clip(i, 0, gy - 2), np.clip(j, 0, gx - 2)
            ch, cw = sy[i + 1] - sy[i], sx[j + 1] - sx[j]
            qy, qx = Yf - sy[i], Xf - sx[j]
            cdy = [dy[i, j], dy[i, j + 1], dy[i + 1, j + 1], dy[i + 1, j]]       # corner displacements
            cdx = [dx[i, j], dx[i, j + 1], dx[i + 1, j + 1], dx[i + 1, j]]
            py = [cdy[0], cdy[1], ch + cdy[2], ch + cdy[3]]                      # corner positions, local frame
            px = [cdx[0], cw + cdx[1], cw + cdx[2], cdx[3]]
            f = diag[i, j]
            for t in range(2):
                pick = lambda vals, k: np.where(f, vals[TRIANGLES[1][t][k]], vals[TRIANGLES[0][t][k]])     # noqa: E731
                p0y, p1y, p2y = (pick(py, k) for k in range(3))
                p0x, p1x, p2x = (pick(px, k) for k in range(3))
                e1y, e1x, e2y, e2x, ry, rx = p1y - p0y, p1x - p0x, p2y - p0y, p2x - p0x, qy - p0y, qx - p0x
                det = e1y * e2x - e1x * e2y
                l1 = (ry * e2x - rx * e2y) / det
                l2 = (e1y * rx - e1x * ry) / det
                l0 = (one - l1) - l2
                mn = np.fmin(l0, np.fmin(l1, l2))
                upd = ok & (best < 0) & (mn > best)
                d0y, d1y, d2y = (pick(cdy, k) for k in range(3))
                d0x, d1x, d2x = (pick(cdx, k) for k in range(3))
                my = np.where(upd, Yf - ((l0 * d0y + l1 * d1y) + l2 * d2y), my)
                mx = np.where(upd, Xf - ((l0 * d0x + l1 * d1x) + l2 * d2x), mx)
                # barycentric coordinate l_k belongs to the edge opposite corner k: a border edge when both its ends lie on one side of the lattice
                bc = np.full((H, w), np.inf, dtype=T)
                ls = (l0, l1, l2)
                for k in range(3):
                    ends = [e for e in range(3) if e != k]
                    rr = [i + np.where(f, CORNER_RC[TRIANGLES[1][t][e]][0], CORNER_RC[TRIANGLES[0][t][e]][0]) for e in ends]
                    cc = [j + np.where(f, CORNER_RC[TRIANGLES[1][t][e]][1], CORNER_RC[TRIANGLES[0][t][e]][1]) for e in ends]
                    on_border = ((rr[0] == 0) & (rr[1] == 0)) | ((rr[0] == gy - 1) & (rr[1] == gy - 1)) | ((cc[0] == 0) & (cc[1] == 0)) | ((cc[0] == gx - 1) & (cc[1] == gx - 1))
                    bc = np.where(on_border, np.fmin(bc, ls[k]), bc)
                border = np.where(upd, bc, border)
                best = np.where(upd, mn, best)
    inside = best >= -T(EPS[T])
    return {"map_y": np.where(inside, my, np.nan), "map_x": np.where(inside, mx, np.nan), "inside": inside, "border": border, "best": best}


def bilinear(img, map_y, map_x, m):
    """fp64 bilinear sample of the H x w array `img` at (map_y, map_x); taps outside the array take m"""
    H, w = img.shape
    my, mx = np.asarray(map_y, dtype=np.float64), np.asarray(map_x, dtype=np.float64)
    y0, x0 = np.floor(my), np.floor(mx)
    fy, fx = my - y0, mx - x0

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < w)
        return np.where(ok, img[np.clip(yy, 0, H - 1).astype(np.int64), np.clip(xx, 0, w - 1).astype(np.int64)], float(m))
    top = tap(y0, x0) + fx * (tap(y0, x0 + 1) - tap(y0, x0))
    bot = tap(y0 + 1, x0) + fx * (tap(y0 + 1, x0 + 1) - tap(y0 + 1, x0))
    return top + fy * (bot - top)


def augment(level_img, fg, bg, src_y=None, src_x=None, disp_y=None, disp_x=None):
    """the whole augmentation of one line in fp64 -> (output levels int64 [H, w], t, lut, m, map dict or None)"""
    t, lut, m = stats(level_img, fg, bg)
    q = lut[level_img].astype(np.float64)
    H, w = level_img.shape
    if src_y is None or H <= 5 or w <= 5:
        return q.astype(np.int64), t, lut, m, None
    mp = warp_map(H, w, src_y, src_x, disp_y, disp_x, np.float64)
    v = bilinear(q, np.nan_to_num(mp["map_y"]), np.nan_to_num(mp["map_x"]), m)
    out = np.where(mp["inside"], np.rint(v), m).astype(np.int64)
    return out, t, lut, m, mp
