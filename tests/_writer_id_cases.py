"""Style vectors with writer labels for the retrieval and style-distance tests (not collected by pytest): the quarter-valued cases whose
distances are exact in fp32 in any summation order, and Gaussian clusters around per-writer centres."""
import numpy as np


def quarter_case(n, d, variant, seed=0):
    """-> (styles float32 [n, d] in quarters, ids int32 [n]). equal: one writer; distinct: n writers; duplicated: every row is followed by
    an exact copy of itself (n odd: the last row is single), writers drawn at random so that copies fall within and across writers"""
    rs = np.random.RandomState(1000 * n + d + seed)
    styles = np.clip(np.round(rs.randn(n, d) * 12) / 4, -16, 16).astype(np.float32)
    if variant == "equal":
        ids = np.zeros(n, dtype=np.int32)
    elif variant == "distinct":
        ids = np.arange(n, dtype=np.int32)
    else:
        styles = np.repeat(styles[:(n + 1) // 2], 2, axis=0)[:n].copy()
        ids = rs.randint(0, max(n // 5, 2), n).astype(np.int32)
    return styles, ids


def gaussian_case(n, d, seed):
    """Gaussian styles around per-writer centres: -> (styles float32 [n, d], ids int32 [n])"""
    rs = np.random.RandomState(seed)
    writers = max(n // 6, 2)
    ids = rs.randint(0, writers, n).astype(np.int32)
    centres = 0.3 * rs.randn(writers, d)             # clusters that overlap: the nearest same-writer line is often not the nearest line
    return (centres[ids] + rs.randn(n, d)).astype(np.float32), ids
