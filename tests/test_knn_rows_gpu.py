"""GPU: hwg_knn_rows (csrc/style_map.hip through ops.knn_rows) against tests/_umap_ref.py, the restatement with np.argsort(kind="stable").
No umap-learn output serves as a golden file (it is not installed where these tests were written, and its NN-descent is approximate).

Bit-exact block: every style value is a multiple of 1/4 in [-2, 2], so a difference is a multiple of 1/4 <= 4, its square a multiple of
1/16 <= 16, and a sum over D <= 100 of them stays far below 2^24 units of its grid: every distance is exact in fp32 in any summation order,
and idx and d2 must be EQUAL to the restatement's, ties by column. Rows are copied within a row block, across row blocks and across
column blocks: a copy is a neighbour at distance 0, the lower column first.
Real-valued block: against fp64 without leaving out any row. A sequential fp32 sum of D non-negative terms, each rounded once (the
difference) and fused (the square), is within relative gamma = (D + 2) 2^-24 of the exact value; the tests allow 2 gamma. Rows with near
ties exist (the test counts them), so a column may differ from the fp64 order - but its fp64 distance may not."""
import numpy as np
import pytest
import torch

import _umap_ref as ref

pytestmark = pytest.mark.gpu

# the kernel's tiles: 16 rows per workgroup, 256 columns per column block, depth tiles of 32, lists of 64 keys
QUARTER_SHAPES = [(37, 1, 1), (37, 5, 36), (273, 33, 8), (512, 32, 64), (600, 100, 63)]
REAL_SHAPES = [(800, 64, 34), (273, 33, 14)]


def quarter_case(n, d):
    rs = np.random.RandomState(100 * n + d)
    x = (rs.randint(-8, 9, (n, d)) * 0.25).astype(np.float32)
    x[5] = x[3]                         # a copy within a row block
    x[n - 1] = x[2]                     # across row blocks
    x[20] = x[3]                        # a third copy of row 3
    if n > 260:
        x[260] = x[0]                   # across column blocks
        x[261] = x[n - 2]
    return x


def gaussian_case(n, d):
    rs = np.random.RandomState(n + d)
    centres = rs.randn(max(n // 20, 2), d)
    return (centres[rs.randint(0, len(centres), n)] + rs.randn(n, d)).astype(np.float32)


def _run(x, k, cuda, out=None):
    from handwriting_line_generation_amd import ops
    idx, d2 = ops.knn_rows(torch.from_numpy(np.array(x)).to(cuda), k, out=out)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


_want = {}


def _reference(n, d, k):
    """computed once per case, shared by the tests that need it, never changed"""
    if (n, d, k) not in _want:
        x = quarter_case(n, d)
        idx, d2 = ref.knn(x, k, dtype=np.float32)
        for a in (x, idx, d2):
            a.setflags(write=False)
        _want[(n, d, k)] = (x, idx, d2)
    return _want[(n, d, k)]


@pytest.mark.parametrize("n,d,k", QUARTER_SHAPES)
def test_quarter_valued_inputs_are_bit_exact(cuda, n, d, k):
    x, want_idx, want_d2 = _reference(n, d, k)
    idx, d2 = _run(x, k, cuda)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == d2.shape == (n, k)
    bad = np.flatnonzero((idx != want_idx).any(axis=1))
    assert bad.size == 0, (bad[:8], idx[bad[:2]], want_idx[bad[:2]])
    assert np.array_equal(d2.view(np.int32), want_d2.view(np.int32))
    # the copies: row 3's nearest are its copies 5 and 20 at distance 0, lower column first; row 5 sees 3 then 20
    # (D = 1 has 17 values for 37 rows: copies everywhere, the restatement above is the check)
    if d >= 5:
        assert (d2[3, 0] == 0) and idx[3, 0] == 5 and idx[5, 0] == 3 and idx[n - 1, 0] == 2
    if d >= 5 and k >= 2:
        assert idx[3, 1] == 20 and d2[3, 1] == 0 and idx[5, 1] == 20 and idx[20, :2].tolist() == [3, 5]
    if n > 260:
        assert idx[0, 0] == 260 and idx[260, 0] == 0 and d2[260, 0] == 0
    assert (np.diff(d2, axis=1) >= 0).all() and (idx != np.arange(n)[:, None]).all()
    if k == n - 1:                      # every other row, each once
        assert (np.sort(idx, axis=1) == np.array([[c for c in range(n) if c != i] for i in range(n)])).all()


@pytest.mark.parametrize("n,d,k", REAL_SHAPES)
def test_real_valued_inputs_against_fp64(cuda, n, d, k):
    x = gaussian_case(n, d)
    full = ref.all_d2(x)                                     # fp64 [n, n]
    _, want = ref.knn(x, k + 1)                              # (one more than asked for: the near ties at the end of the list count too)
    gap = np.diff(want, axis=1) / want[:, 1:]
    print("N=%d D=%d K=%d: %d rows with a relative gap below 1e-5 among the first %d distances (smallest %.3g)" % (
        n, d, k, int((gap < 1e-5).any(axis=1).sum()), k + 1, gap.min()))
    idx, d2 = _run(x, k, cuda)
    bound = 2 * (d + 2) * 2.0 ** -24
    want = want[:, :k]
    err_a = np.abs(d2.astype(np.float64) - want) / want
    err_b = np.abs(full[np.arange(n)[:, None], idx] - want) / want
    print("N=%d D=%d K=%d: d2 max relative error %.3g, distance of the chosen column %.3g (bound %.3g)" % (n, d, k, err_a.max(), err_b.max(), bound))
    assert err_a.max() <= bound, (err_a.max(), bound)                                                # (a)
    assert err_b.max() <= bound, (err_b.max(), bound)                                                # (b)
    assert (idx != np.arange(n)[:, None]).all() and (idx >= 0).all() and (idx < n).all()               # (c)
    assert all(len(set(row)) == k for row in idx.tolist())
    assert (np.diff(d2, axis=1) >= 0).all()


def test_two_calls_give_the_same_bytes_and_every_entry_is_written(cuda):
    x = gaussian_case(800, 64)
    a = _run(x, 34, cuda)
    b = _run(x, 34, cuda)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    xq, want_idx, want_d2 = _reference(273, 33, 8)
    out = (torch.full((273, 8), -7, dtype=torch.int32, device=cuda), torch.full((273, 8), float("nan"), dtype=torch.float32, device=cuda))
    idx, d2 = _run(xq, 8, cuda, out=out)
    assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)


def test_limits_are_refused_before_a_launch(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    x = torch.zeros(100, 8, device=cuda)
    idx = torch.full((100, 64), -7, dtype=torch.int32, device=cuda)
    d2 = torch.zeros((100, 64), device=cuda)
    for k in (0, 65, 100, -1, 2.0, True):
        with pytest.raises(L.HwgError, match="knn_rows"):
            ops.knn_rows(x, k)
    for args, word in [((x, 100, 8, 65, idx, d2, 0), "limit"), ((x, 100, 8, 100, idx, d2, 0), "limit"), ((x, 100, 8, 0, idx, d2, 0), "bad sizes"),
                       ((x, (1 << 20) + 1, 8, 5, idx, d2, 0), "limit"), ((x, 100, 65537, 5, idx, d2, 0), "limit"),
                       ((x.data_ptr() + 4, 99, 8, 5, idx, d2, 0), "aligned"), ((None, 100, 8, 5, idx, d2, 0), "null")]:
        with pytest.raises(L.HwgError, match=word):
            L.call("hwg_knn_rows", *args)
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all()                   # nothing ran
    with pytest.raises(L.HwgError, match="out must be"):
        ops.knn_rows(x, 5, out=(idx, d2))
