"""numpy restatement of writer retrieval as evaluate.writer_id defines it (not a test module): per row, the columns in the stable order of
their distances; first_rank = the first place >= 1 that holds a column of the row's writer; top-n = share of rows with first_rank <= n.
Written from the definitions, with np.argsort(kind="stable") - no code shared with the package."""
import numpy as np


def row_distances(styles, i, metric, dtype):
    s = styles.astype(dtype)
    diff = s[i][None, :] - s
    return np.abs(diff).sum(axis=1, dtype=dtype) if metric == 0 else (diff * diff).sum(axis=1, dtype=dtype)


def first_rank(styles, ids, metric, dtype=np.float32):
    """-> (first_rank int64 [N] (N: no same-writer column at a place >= 1), nearest_same dtype [N] (+inf there), margin [N]: the smallest
    |d[i, k] - nearest_same[i]| / nearest_same[i] over the columns k other than the one at first_rank (inf where undefined))"""
    ids = np.asarray(ids)
    n = len(ids)
    rank = np.full(n, n, dtype=np.int64)
    near = np.full(n, np.inf, dtype=dtype)
    margin = np.full(n, np.inf, dtype=np.float64)
    for i in range(n):
        d = row_distances(styles, i, metric, dtype)
        order = np.argsort(d, kind="stable")
        pos = np.empty(n, dtype=np.int64)
        pos[order] = np.arange(n)
        cand = pos[(ids == ids[i]) & (pos >= 1)]
        if cand.size:
            rank[i] = cand.min()
            j = order[rank[i]]
            near[i] = d[j]
            others = np.delete(d, j).astype(np.float64)
            if others.size and d[j] > 0:
                margin[i] = np.abs(others - float(d[j])).min() / float(d[j])
            elif others.size:
                margin[i] = 0.0 if (others == 0).any() else np.inf
    return rank, near, margin


def summary(rank, n, tops=(1, 5, 20)):
    has = rank < n
    out = {"top%d" % k: int((rank <= min(k, n - 1)).sum()) / n for k in tops}
    out["mean_first_rank"] = int(rank[has].sum()) / int(has.sum()) if has.any() else None
    out["rows_without_match"] = int((~has).sum())
    return out


def ids_of(authors):
    table = {}
    return np.array([table.setdefault(a.item() if isinstance(a, np.generic) else a, len(table)) for a in authors], dtype=np.int32)
