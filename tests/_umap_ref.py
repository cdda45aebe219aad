"""Restatement, from the definitions alone, of what umap_styles.py computes - fp64 numpy, written as loops over rows and edges, sharing no
code with the package: the k nearest other rows in the stable order of (distance, column), the curve parameters a, b, the fuzzy graph and
its integer schedule, one layout epoch (optionally evaluated in float32: the yardstick of the device's rounding), and trustworthiness from
its definition. The Philox words are oracle.optim_ref's (philox_blocks, which tests/test_style_map_cpu.py pins to philox4x32).

No umap-learn output can serve as a golden file for any of this: umap-learn is not installed where these tests were written, and its
layout loop is not reproducible from run to run. The numbers the tests compare against are these definitions."""
import math

import numpy as np

from oracle import optim_ref


# ---- k nearest rows -------------------------------------------------------------------------------------------------------------------
def all_d2(styles, dtype=np.float64):
    """squared L2 distances of all pairs, computed in fp64, returned as `dtype` [N, N]"""
    x = np.asarray(styles, dtype=np.float64)
    out = np.empty((x.shape[0], x.shape[0]), dtype=dtype)
    for i in range(x.shape[0]):
        diff = x - x[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def knn(styles, k, dtype=np.float64):
    """-> (idx int32 [N, k], d2 dtype [N, k]): per row the k nearest OTHER rows; the row's own column is taken out by index, the rest is
    the stable order of the distances (ties by column)"""
    d2 = all_d2(styles, dtype)
    n = d2.shape[0]
    idx = np.empty((n, k), dtype=np.int32)
    out = np.empty((n, k), dtype=dtype)
    for i in range(n):
        order = np.argsort(d2[i], kind="stable")
        order = order[order != i][:k]
        idx[i], out[i] = order, d2[i][order]
    return idx, out


# ---- a, b -----------------------------------------------------------------------------------------------------------------------------
def find_ab(spread, min_dist):
    """least squares of 1 / (1 + a x^(2b)) against the target curve at 300 points; Gauss-Newton on a numerical Jacobian with step halving"""
    x = np.linspace(0, 3 * spread, 300)
    want = np.array([1.0 if v < min_dist else math.exp(-(v - min_dist) / spread) for v in x])

    def resid(a, b):
        return 1.0 / (1.0 + a * x ** (2 * b)) - want

    a, b = 1.0, 1.0
    for _ in range(200):
        r = resid(a, b)
        h = 1e-6
        j = np.stack([(resid(a + h, b) - resid(a - h, b)) / (2 * h), (resid(a, b + h) - resid(a, b - h)) / (2 * h)], axis=1)
        step = np.linalg.lstsq(j, -r, rcond=None)[0]
        scale = 1.0
        while scale > 1e-10:
            na, nb = a + scale * step[0], b + scale * step[1]
            if na > 0 and nb > 0 and (resid(na, nb) ** 2).sum() <= (r ** 2).sum():
                break
            scale /= 2
        else:
            break
        done = abs(na - a) + abs(nb - b) < 1e-12
        a, b = na, nb
        if done:
            break
    return a, b


# ---- fuzzy graph ----------------------------------------------------------------------------------------------------------------------
def fuzzy_graph(idx, d2, n_neighbors, n_epochs):
    """-> (row_ptr, col, period_q, w) of the symmetrised graph, edges sorted by (row, column)"""
    n, k = idx.shape
    dist = [[math.sqrt(float(v)) for v in row] for row in d2]
    total = sum(sum(row) for row in dist) / (n * k)
    target = math.log2(n_neighbors)
    weight = {}
    for i in range(n):
        row = dist[i]
        pos = [v for v in row if v > 0]
        rho = min(pos) if pos else 0.0
        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            p = sum(float(np.exp(-(v - rho) / mid)) if v - rho > 0 else 1.0 for v in row)
            if abs(p - target) < 1e-5:
                break
            if p > target:
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = 2 * mid if hi == math.inf else (lo + hi) / 2
        sigma = max(mid, 1e-3 * (sum(row) / k) if rho > 0 else 1e-3 * total)
        for j, v in zip(idx[i], row):
            weight[(i, int(j))] = 1.0 if v - rho <= 0 else float(np.exp(-(v - rho) / sigma))
    sym = {}
    for (i, j), w in weight.items():
        back = weight.get((j, i), 0.0)
        sym[(i, j)] = sym[(j, i)] = w + back - w * back
    top = max(sym.values())
    edges = sorted(e for e, w in sym.items() if not w < top / n_epochs)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    for i, _ in edges:
        row_ptr[i + 1] += 1
    row_ptr = np.cumsum(row_ptr)
    col = np.array([j for _, j in edges], dtype=np.int64)
    w = np.array([sym[e] for e in edges])
    return row_ptr, col, np.rint(65536 * top / w).astype(np.int64), w


def active_edges(period_q, n):
    """which edges epoch n draws: the integer schedule"""
    q = np.asarray(period_q, dtype=np.int64)
    return (n * 65536) // q > ((n - 1) * 65536) // q


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
def negative_samples(n, n_vertices, n_edges, neg, seed):
    """-> int64 [E, neg]: the vertex each repulsion of epoch n pushes away from"""
    blocks = (neg + 3) // 4
    words = optim_ref.philox_blocks(seed, n * n_edges * blocks, n_edges * blocks).reshape(n_edges, 4 * blocks)[:, :neg]
    return ((words.astype(np.uint64) * np.uint64(n_vertices)) >> np.uint64(32)).astype(np.int64)


def layout_epoch(row_ptr, col, period_q, y, n, n_epochs, a, b, neg, seed, dtype=np.float64):
    """positions after epoch n from the positions `y` before it, every operation in `dtype`"""
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    nv, ne = row_ptr.shape[0] - 1, col.shape[0]
    y = np.asarray(y).astype(dtype)
    a, b, two, four, eps = dtype(a), dtype(b), dtype(2), dtype(4), dtype(0.001)
    alpha = dtype(np.float32(1.0 - (n - 1) / float(n_epochs)))
    owner = np.repeat(np.arange(nv), np.diff(row_ptr))
    act = np.flatnonzero(active_edges(period_q, n))
    i, j = owner[act], col[act]
    total = np.zeros((nv, 2), dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = y[i] - y[j]
        s = (d * d).sum(axis=1, dtype=dtype)
        safe = np.where(s > 0, s, dtype(1))
        c = -two * a * b * safe ** (b - dtype(1)) / (a * safe ** b + dtype(1))
        term = two * np.clip(c[:, None] * d, -four, four)
        term[~(s > 0)] = 0
        np.add.at(total, i, term)
        far = negative_samples(n, nv, ne, neg, seed)[act]
        for t in range(neg):
            r = far[:, t]
            d = y[i] - y[r]
            s = (d * d).sum(axis=1, dtype=dtype)
            safe = np.where(s > 0, s, dtype(1))
            c = two * b / ((eps + safe) * (a * safe ** b + dtype(1)))
            term = np.clip(c[:, None] * d, -four, four)
            term[~(s > 0)] = four
            term[r == i] = 0
            np.add.at(total, i, term)
    return (y + alpha * total).astype(dtype)


def layout(row_ptr, col, period_q, y, n_epochs, a, b, neg, seed, begin=0, end=None, dtype=np.float64):
    for n in range(begin + 1, (n_epochs if end is None else end) + 1):
        y = layout_epoch(row_ptr, col, period_q, y, n, n_epochs, a, b, neg, seed, dtype)
    return y


def pca(styles):
    """the projections on the two leading principal axes (sign and scale are the package's business)"""
    x = np.asarray(styles, dtype=np.float64)
    x = x - x.mean(axis=0)
    _, _, vt = np.linalg.svd(x, full_matrices=False)
    return x @ vt[:2].T


# ---- quality --------------------------------------------------------------------------------------------------------------------------
def trustworthiness(x, y, k):
    """1 - 2 / (N k (2N - 3k - 1)) sum_i sum_{j in U_i} (r(i, j) - k): U_i the k nearest of i in the map y that are not among its k nearest
    in the input x, r(i, j) the place of j among the input neighbours of i (1 = nearest)"""
    dx, dy = all_d2(x), all_d2(y)
    n = dx.shape[0]
    penalty = 0
    for i in range(n):
        order_x = np.argsort(dx[i], kind="stable")
        order_x = order_x[order_x != i]
        place = np.empty(n, dtype=np.int64)
        place[order_x] = np.arange(1, n)
        order_y = np.argsort(dy[i], kind="stable")
        order_y = order_y[order_y != i][:k]
        ranks = place[order_y]
        penalty += int((ranks[ranks > k] - k).sum())
    return 1.0 - 2.0 * penalty / (n * k * (2 * n - 3 * k - 1))


def nearest_label_share(y, labels):
    """share of points whose nearest other point in the map carries their label"""
    d = all_d2(y)
    np.fill_diagonal(d, np.inf)
    labels = np.asarray(labels)
    return float((labels[np.argmin(d, axis=1)] == labels).mean())
