"""numpy restatement of the same-writer / different-writer distances as evaluate.style_distances defines them (not a test module; shares no
code with the package): over all pairs i < j of style vectors, d^2 = sum (a - b)^2 and d = sqrt(float64(d^2)); a pair belongs to the
same-writer set when the two writers are equal, and to the cell (writer of i, writer of j) of the writer x writer matrices, which are
symmetric. Two variants: dtype float32 forms d^2 as the reference does (fp32 differences, fp32 squares, numpy's fp32 sum - exact for the
quarter-valued inputs of the tests, whatever the order), dtype float64 forms it in fp64 from the fp32 inputs. Sums over a set of pairs are
math.fsum, the exactly rounded sum, so a bound on the device's error is not spent on this file's."""
import math

import numpy as np


def ids_of(authors):
    """int32 ids in order of first appearance"""
    table = {}
    return np.array([table.setdefault(a.item() if isinstance(a, np.generic) else a, len(table)) for a in authors], dtype=np.int32)


def distances(styles, ids, dtype=np.float32):
    """-> (d float64 [P], same bool [P], i [P], j [P], d2 dtype [P]) over the P = n (n - 1) / 2 pairs i < j, in the order of the reference's
    double loop"""
    s = np.asarray(styles, dtype=np.float32).astype(dtype)
    ids = np.asarray(ids)
    n = s.shape[0]
    i, j = np.triu_indices(n, 1)
    d2 = np.empty(i.shape[0], dtype=dtype)
    step = max(1, (1 << 22) // max(s.shape[1], 1))
    for k in range(0, i.shape[0], step):
        diff = s[i[k:k + step]] - s[j[k:k + step]]
        d2[k:k + step] = (diff * diff).sum(axis=1, dtype=dtype)
    return np.sqrt(d2.astype(np.float64)), ids[i] == ids[j], i, j, d2


def cell(d, d2, mask):
    """(count, sum of d, sum of float64(d2)) over the pairs of mask"""
    return int(mask.sum()), math.fsum(d[mask].tolist()), math.fsum(d2[mask].astype(np.float64).tolist())


def stats(styles, ids, dtype=np.float32, writers=None):
    """-> dict: "d", "d2", "same" (per pair), "cells0" [(count, sum, sumsq)] * 2 (same writer, different writers), "count" / "sum" /
    "sumsq" [A, A] (symmetric; A = writers or max id + 1), "min_d2", "max_d2" (dtype scalars; +inf / -inf without a pair)"""
    ids = np.asarray(ids)
    d, same, i, j, d2 = distances(styles, ids, dtype)
    A = int(ids.max()) + 1 if writers is None else writers
    count = np.zeros((A, A), dtype=np.int64)
    total = np.zeros((A, A), dtype=np.float64)
    total_sq = np.zeros((A, A), dtype=np.float64)
    key = np.minimum(ids[i], ids[j]).astype(np.int64) * A + np.maximum(ids[i], ids[j])
    order = np.argsort(key, kind="stable")
    bounds = np.flatnonzero(np.diff(np.concatenate([[-1], key[order]]))) if key.size else np.zeros(0, dtype=np.int64)
    for k, lo in enumerate(bounds):
        hi = bounds[k + 1] if k + 1 < len(bounds) else key.size
        sel = order[lo:hi]
        a, b = divmod(int(key[order[lo]]), A)
        n, sd, sq = len(sel), math.fsum(d[sel].tolist()), math.fsum(d2[sel].astype(np.float64).tolist())
        count[a, b] = count[b, a] = n
        total[a, b] = total[b, a] = sd
        total_sq[a, b] = total_sq[b, a] = sq
    return {"d": d, "d2": d2, "same": same, "cells0": [cell(d, d2, same), cell(d, d2, ~same)], "count": count, "sum": total, "sumsq": total_sq,
            "min_d2": d2.min() if d2.size else dtype(np.inf), "max_d2": d2.max() if d2.size else dtype(-np.inf)}


def summary(d):
    """what the reference prints for a list of distances: np.mean and np.std (population) in fp64; None for an empty list"""
    if len(d) == 0:
        return {"pairs": 0, "mean": None, "std": None}
    return {"pairs": int(len(d)), "mean": float(np.mean(d)), "std": float(np.std(d))}


def edges(min_d2, max_d2, bins):
    """-> (edges float64 [bins + 1] in d, edge2 float32 [bins + 1] in d^2): equal-width bins in d between the extremes; the squares are
    taken in fp64 and rounded to fp32 once, then the first is 0 and the last +inf"""
    lo, hi = math.sqrt(float(min_d2)), math.sqrt(float(max_d2))
    e = np.array([lo + (hi - lo) * k / bins for k in range(bins + 1)], dtype=np.float64)
    e[-1] = hi
    e2 = np.array([np.float32(v * v) for v in e], dtype=np.float32)
    e2[0], e2[-1] = np.float32(0), np.float32(np.inf)
    return e, e2


def histogram(d2, same, edge2):
    """-> int64 [2, bins]: pair counts per bin, same-writer pairs then different-writer pairs; bin k iff edge2[k] <= d2 < edge2[k + 1],
    compared in fp32 on d2 itself"""
    d2 = np.asarray(d2, dtype=np.float32)
    edge2 = np.asarray(edge2, dtype=np.float32)
    bins = len(edge2) - 1
    out = np.zeros((2, bins), dtype=np.int64)
    for k in range(bins):
        inside = (d2 >= edge2[k]) & (d2 < edge2[k + 1])
        out[0, k] = int((inside & same).sum())
        out[1, k] = int((inside & ~same).sum())
    return out
