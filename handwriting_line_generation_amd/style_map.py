"""The host side of umap_styles.py: from the kernel's k nearest rows to the graph the layout kernel walks, and the whole map.

    styles --ops.knn_rows--> (idx, d2) --fuzzy_graph--> CSR (row_ptr, col, period_q) --ops.umap_layout, from pca_init--> embedding [N, 2]

Everything here is fp64 numpy (no scipy, no umap-learn, no numba): the smooth-kNN weights of UMAP (McInnes, Healy, Melville 2018, section 3
and algorithm 3), their symmetrisation, the curve parameters a, b of the low-dimensional similarity 1 / (1 + a x^(2b)), and the starting
positions. What differs from umap-learn is listed in INTEGRATION.md, "Known differences of umap_styles.py"."""
import numpy as np

SMOOTH_K_TOLERANCE = 1e-5
MIN_K_DIST_SCALE = 1e-3
SCHEDULE_ONE = 65536          # period_q is a period in 1 / 65536 epochs


def find_ab(spread=1.0, min_dist=0.2):
    """-> (a, b): the least-squares fit of 1 / (1 + a x^(2b)) at x = linspace(0, 3 spread, 300) to the target 1 for x < min_dist, else
    exp(-(x - min_dist) / spread) (umap-learn's find_ab_params, there scipy's curve_fit). Levenberg-Marquardt from (1, 1) on the analytic
    Jacobian, until a step no longer changes the parameters."""
    x = np.linspace(0.0, 3.0 * spread, 300)
    target = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    logx = np.log(np.where(x > 0, x, 1.0))          # (x = 0: x^(2b) = 0 and its derivative in b is 0)

    def model(p):
        xp = np.where(x > 0, np.exp(2.0 * p[1] * logx), 0.0)
        f = 1.0 / (1.0 + p[0] * xp)
        return f, xp

    p = np.array([1.0, 1.0])
    f, xp = model(p)
    res = f - target
    cost = float(res @ res)
    lam = 1e-3
    for _ in range(500):
        jac = np.stack([-xp * f * f, -p[0] * xp * 2.0 * logx * f * f], axis=1)
        g, h = jac.T @ res, jac.T @ jac
        moved = False
        while lam < 1e12:
            step = np.linalg.solve(h + lam * np.diag(np.diag(h)), -g)
            q = p + step
            if q[0] > 0 and q[1] > 0:
                fq, xq = model(q)
                rq = fq - target
                cq = float(rq @ rq)
                if cq <= cost:
                    moved = True
                    break
            lam *= 10.0
        if not moved:
            break
        small = np.abs(step).max() <= 1e-13 * np.abs(p).max()
        p, f, xp, res, cost = q, fq, xq, rq, cq
        lam = max(lam / 10.0, 1e-12)
        if small:
            break
    return float(p[0]), float(p[1])


def smooth_knn(dist, n_neighbors):
    """dist fp64 [N, K] (a row ascending) -> (rho [N], sigma [N]): the distance to the nearest neighbour that is not a copy, and the
    bandwidth at which the row's weights sum to log2(n_neighbors), by bisection"""
    n, k = dist.shape
    target = np.log2(float(n_neighbors))
    positive = dist > 0
    rho = np.where(positive.any(axis=1), np.where(positive, dist, np.inf).min(axis=1), 0.0)
    d = dist - rho[:, None]
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    running = np.ones(n, dtype=bool)
    for _ in range(64):
        with np.errstate(over="ignore", under="ignore"):
            p = np.where(d > 0, np.exp(-d / mid[:, None]), 1.0).sum(axis=1)
        running &= ~(np.abs(p - target) < SMOOTH_K_TOLERANCE)
        if not running.any():
            break
        above = running & (p > target)
        below = running & ~(p > target)
        hi = np.where(above, mid, hi)
        lo = np.where(below, mid, lo)
        with np.errstate(invalid="ignore"):
            half = (lo + hi) / 2.0
        new_mid = np.where(above, half, np.where(np.isinf(hi), 2.0 * mid, half))
        mid = np.where(running, new_mid, mid)
    floor = np.where(rho > 0, MIN_K_DIST_SCALE * dist.mean(axis=1), MIN_K_DIST_SCALE * dist.mean())
    return rho, np.maximum(mid, floor)


def fuzzy_graph(idx, d2, n_neighbors, n_epochs):
    """the kernel's output for K = n_neighbors - 1 (idx int [N, K], d2 [N, K] squared distances) -> (row_ptr int32 [N + 1], col int32 [E],
    period_q int32 [E], w fp64 [E]): the symmetrised fuzzy graph w_ij + w_ji - w_ij w_ji over the union of the edges, without the edges
    weaker than max(w) / n_epochs (they would never be drawn), sorted by (row, column); period_q = rint(65536 max(w) / w): the strongest
    edge is drawn every epoch, an edge of weight w every max(w) / w epochs."""
    idx = np.asarray(idx).astype(np.int64)
    dist = np.sqrt(np.asarray(d2, dtype=np.float64))
    n, k = idx.shape
    if k != n_neighbors - 1 or dist.shape != (n, k):
        raise ValueError("fuzzy_graph: idx %s and d2 %s must both be [N, n_neighbors - 1 = %d]" % (idx.shape, dist.shape, n_neighbors - 1))
    if not 1 <= n_epochs <= 32767:
        raise ValueError("fuzzy_graph: n_epochs must lie in 1..32767 (a period is at most 65536 n_epochs and has to fit 31 bits), got %r" % (n_epochs,))
    rho, sigma = smooth_knn(dist, n_neighbors)
    d = dist - rho[:, None]
    with np.errstate(under="ignore"):
        w = np.where(d > 0, np.exp(-d / sigma[:, None]), 1.0)
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = idx.reshape(-1)
    w = w.reshape(-1)
    fwd, bwd = rows * n + cols, cols * n + rows
    keys = np.unique(np.concatenate([fwd, bwd]))
    w_ij, w_ji = np.zeros(keys.shape[0]), np.zeros(keys.shape[0])
    w_ij[np.searchsorted(keys, fwd)] = w
    w_ji[np.searchsorted(keys, bwd)] = w
    sym = w_ij + w_ji - w_ij * w_ji
    top = sym.max()
    keep = ~(sym < top / n_epochs)
    keys, sym = keys[keep], sym[keep]
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // n, minlength=n), out=row_ptr[1:])
    period_q = np.rint(SCHEDULE_ONE * top / sym)
    return row_ptr.astype(np.int32), (keys % n).astype(np.int32), period_q.astype(np.int32), sym


def pca_init(styles):
    """-> fp32 [N, 2]: the projections on the two leading principal axes, each axis signed so that its largest projection in magnitude is
    positive, scaled so that the largest coordinate in magnitude is 10"""
    x = np.asarray(styles, dtype=np.float64)
    x = x - x.mean(axis=0)
    d = x.shape[1]
    if d == 1:
        x = np.concatenate([x, np.zeros_like(x)], axis=1)
    _, vec = np.linalg.eigh(x.T @ x / max(x.shape[0] - 1, 1))
    p = x @ vec[:, ::-1][:, :2]
    for axis in range(2):
        if p[np.argmax(np.abs(p[:, axis])), axis] < 0:
            p[:, axis] = -p[:, axis]
    top = np.abs(p).max()
    return (10.0 * p / (top if top > 0 else 1.0)).astype(np.float32)


def check_styles(styles):
    """-> contiguous fp32 [N, D]; ValueError for anything a map cannot be drawn of"""
    styles = np.asarray(styles)
    if styles.ndim == 4 and styles.shape[2:] == (1, 1):
        styles = styles[:, :, 0, 0]
    if styles.ndim != 2 or styles.shape[0] < 1 or styles.shape[1] < 1:
        raise ValueError("style_map: styles must be [n, D] or [n, D, 1, 1] with n, D >= 1, got %s" % (tuple(styles.shape),))
    styles = np.ascontiguousarray(styles, dtype=np.float32)
    finite = np.isfinite(styles).all(axis=1)
    if not finite.all():
        raise ValueError("style_map: style row %d is not finite (a neighbour order with NaN is not defined)" % int(np.argmin(finite)))
    seen = set()
    for row in styles + np.float32(0.0):          # (-0.0 + 0.0 = 0.0: rows at distance 0 are one row)
        seen.add(row.tobytes())
        if len(seen) == 3:
            break
    if len(seen) < 3:
        raise ValueError("style_map: %d distinct style rows; a map needs at least 3" % len(seen))
    return styles


def embed(styles, gpu, n_neighbors=35, min_dist=0.2, n_epochs=None, seed=42, neg=5, info=None):
    """styles [N, D] -> the map, fp32 numpy [N, 2]: exact k nearest rows and the layout epochs on `gpu` (ops.knn_rows, ops.umap_layout), the
    graph in between on the host. n_neighbors / min_dist default to the reference's 35 / 0.2, neg to umap-learn's negative_sample_rate,
    n_epochs to 500 up to 10000 rows and 200 above. The same styles and seed give the same bytes. `info`: a dict that receives the
    parameters used."""
    import torch

    from . import ops
    styles = check_styles(styles)
    n = styles.shape[0]
    n_neighbors = int(n_neighbors)
    if n_neighbors < 2:
        raise ValueError("style_map: n_neighbors must be at least 2, got %d" % n_neighbors)
    if n_neighbors > n - 1:
        print("style_map: n_neighbors %d is more than %d rows allow: using %d" % (n_neighbors, n, n - 1), flush=True)
        n_neighbors = n - 1
    if n_neighbors - 1 > ops.KNN_MAX_K:
        raise ValueError("style_map: n_neighbors is at most %d, got %d" % (ops.KNN_MAX_K + 1, n_neighbors))
    if n_epochs is None:
        n_epochs = 500 if n <= 10000 else 200
    n_epochs = int(n_epochs)
    a, b = find_ab(1.0, float(min_dist))
    styles_d = ops.h2d(styles, gpu)
    idx_d, d2_d = ops.knn_rows(styles_d, n_neighbors - 1)
    fetch_idx, fetch_d2 = ops.AsyncFetch(idx_d), ops.AsyncFetch(d2_d)
    y0 = pca_init(styles)                       # (while the kernel runs)
    row_ptr, col, period_q, _ = fuzzy_graph(fetch_idx.get().numpy(), fetch_d2.get().numpy(), n_neighbors, n_epochs)
    graph = ops.umap_graph(row_ptr, col, period_q, gpu)
    y = ops.h2d(y0, gpu)
    ops.umap_layout(graph, y, n_epochs, a, b, int(neg), int(seed))
    out = y.cpu().numpy()
    if info is not None:
        info.update(n_neighbors=n_neighbors, min_dist=float(min_dist), n_epochs=n_epochs, seed=int(seed), neg=int(neg), a=a, b=b,
                    edges=int(col.shape[0]))
    if not np.isfinite(out).all():
        raise FloatingPointError("style_map: the layout left non-finite positions")
    return out
