"""GPU: hwg_umap_layout (csrc/style_map.hip through ops.umap_layout) and the whole map (style_map.embed) against tests/_umap_ref.py.
No umap-learn output serves as a golden file: umap-learn is not installed where these tests were written, and its layout loop is not
reproducible from run to run. The references are the restatement of the definitions in fp64, and - as the yardstick of what fp32 can
deliver - the same restatement evaluated in numpy float32: the device's largest error from fp64 may be at most 4 x the float32
restatement's largest error + 4 * 2^-24 * max|Y| (the rule of profiles/crnn_lstm.txt; observed ratios: profiles/umap_styles.txt)."""
import numpy as np
import pytest
import torch

import _umap_ref as ref

pytestmark = pytest.mark.gpu

N, N_EPOCHS = 273, 50
A, B = float(np.float32(1.576943)), float(np.float32(0.895061))          # min_dist 0.1: a fractional exponent on both sides of 1
EPOCHS = (1, 2, N_EPOCHS)
CLUSTER = slice(5, 25)                                                   # vertices at identical coordinates

_graph = {}


def fabricated():
    """-> dict: a CSR graph of 273 vertices with degrees from 1 to 200 (the hub row 0 is longer than the group of 16 lanes, rows 2 and 3 sit
    on its edge), periods from 65536 up, positions with twenty vertices on one point, and the first seed for which, in every tested epoch,
    some repulsion draws its own vertex (r == i) and some draws another vertex at the same point (s == 0)"""
    if _graph:
        return _graph
    rs = np.random.RandomState(7)
    deg = rs.randint(1, 21, N)
    deg[:4] = [200, 1, 17, 16]
    cols = []
    for i in range(N):
        others = np.delete(np.arange(N), i)
        c = set(rs.choice(others, deg[i], replace=False).tolist())
        if i == 5:
            c.add(6)                                                     # an edge between two vertices on one point: s == 0 in the attraction
        cols.append(sorted(c))
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    col = np.concatenate(cols).astype(np.int32)
    e = col.shape[0]
    period_q = np.rint(65536 * rs.uniform(1, N_EPOCHS, e)).astype(np.int32)
    period_q[rs.rand(e) < 0.3] = 65536
    period_q[row_ptr[5]:row_ptr[6]] = 65536                              # vertex 5's edges are drawn every epoch
    period_q[-1] = 65536 * N_EPOCHS                                      # the longest period there is: drawn once, in the last epoch
    y = (rs.randn(N, 2) * 5).astype(np.float32)
    y[CLUSTER] = y[5]
    owner = np.repeat(np.arange(N), np.diff(row_ptr))
    same_point = np.zeros(N, dtype=bool)
    same_point[CLUSTER] = True
    for seed in range(1000):
        ok = True
        for n in EPOCHS:
            act = ref.active_edges(period_q, n)
            far, i = ref.negative_samples(n, N, e, 5, seed)[act], owner[act][:, None]
            ok &= bool((far == i).any()) and bool(((far != i) & same_point[far] & same_point[i]).any())
        if ok:
            break
    else:
        raise AssertionError("no seed draws r == i and a vertex on the same point in every tested epoch")
    for a in (row_ptr, col, period_q, y, owner):
        a.setflags(write=False)
    _graph.update(row_ptr=row_ptr, col=col, period_q=period_q, y=y, owner=owner, seed=seed, e=e)
    return _graph


def _device_epochs(g, cuda, begin, end, neg, y=None, period_q=None):
    from handwriting_line_generation_amd import ops
    graph = ops.umap_graph(g["row_ptr"], g["col"], g["period_q"] if period_q is None else period_q, cuda)
    yd = torch.from_numpy(np.array(g["y"] if y is None else y)).to(cuda)
    ops.umap_layout(graph, yd, N_EPOCHS, A, B, neg, g["seed"], epoch_begin=begin, epoch_end=end)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _against_the_restatement(g, got, n, neg):
    """-> (bound, ratio): asserts the error rule for epoch n from the fabricated positions"""
    args = (g["row_ptr"], g["col"], g["period_q"], g["y"], n, N_EPOCHS, A, B, neg, g["seed"])
    want = ref.layout_epoch(*args)
    want32 = ref.layout_epoch(*args, dtype=np.float32)
    assert want32.dtype == np.float32 and np.isfinite(want).all() and np.isfinite(got).all()
    err, err32 = np.abs(got.astype(np.float64) - want).max(), np.abs(want32.astype(np.float64) - want).max()
    bound = 4 * err32 + 4 * 2.0 ** -24 * np.abs(want).max()
    moved = np.abs(want - g["y"]).max()
    print("epoch %d of %d, neg %d: device max error %.3g, float32 restatement %.3g (ratio %.2f), bound %.3g; largest move %.3g" % (
        n, N_EPOCHS, neg, err, err32, err / err32 if err32 > 0 else float("inf"), bound, moved))
    assert err <= bound, (n, err, bound)
    assert moved > 1000 * bound                                          # the epoch did something the bound can see
    return bound, want


@pytest.mark.parametrize("n", EPOCHS)
def test_single_epochs_against_the_restatement(cuda, n):
    g = fabricated()
    act = ref.active_edges(g["period_q"], n)
    assert act[g["row_ptr"][5]:g["row_ptr"][6]].all() and 0 < act.sum() < g["e"]
    assert act[-1] == (n == N_EPOCHS)
    assert np.diff(g["row_ptr"]).max() >= 200 and np.diff(g["row_ptr"]).min() == 1 and g["period_q"].min() == 65536
    got = _device_epochs(g, cuda, n - 1, n, 5)
    _against_the_restatement(g, got, n, 5)
    # twenty vertices on one point do not stay there: (4, 4) per repulsion from a vertex on the same point, clamped terms elsewhere
    assert len({tuple(r) for r in got[CLUSTER].tolist()}) > 1


@pytest.mark.parametrize("n", (1, 2, 7, N_EPOCHS))
def test_the_schedule_draws_exactly_the_restatements_edges(cuda, n):
    """neg = 16: an edge drawn in the wrong epoch (or not drawn in its own) moves its vertex by an attraction and sixteen repulsions - the
    restatement with one edge's activity flipped differs by far more than the bound, so agreement within the bound is agreement on every
    edge of the sample's kind"""
    g = fabricated()
    got = _device_epochs(g, cuda, n - 1, n, 16)
    bound, want = _against_the_restatement(g, got, n, 16)
    act = ref.active_edges(g["period_q"], n)
    rs = np.random.RandomState(n)
    free = np.flatnonzero(g["owner"] >= 30)
    for e in rs.choice(free, 8, replace=False).tolist() + [int(g["row_ptr"][1]) - 1]:          # (and the last edge of the hub row)
        q = np.array(g["period_q"])
        q[e] = 65536 * n + 1 if act[e] else 65536                        # a period above n epochs is not drawn before epoch n + 1
        assert ref.active_edges(q, n)[e] != act[e]
        flipped = ref.layout_epoch(g["row_ptr"], g["col"], q, g["y"], n, N_EPOCHS, A, B, 16, g["seed"])
        i = g["owner"][e]
        print("edge %d of vertex %d flipped: moves it by %.3g (bound %.3g)" % (e, i, np.abs(flipped[i] - want[i]).max(), bound))
        assert np.abs(flipped[i] - want[i]).max() > 100 * bound, (e, np.abs(flipped[i] - want[i]).max(), bound)
        assert np.abs(got[i] - want[i]).max() <= bound


def test_split_calls_and_repeat_runs_give_the_same_bytes(cuda):
    g = fabricated()
    whole = _device_epochs(g, cuda, 0, 5, 5)
    again = _device_epochs(g, cuda, 0, 5, 5)
    assert whole.tobytes() == again.tobytes()
    part = _device_epochs(g, cuda, 0, 2, 5)
    part = _device_epochs(g, cuda, 2, 5, 5, y=part)
    assert part.tobytes() == whole.tobytes()
    one = _device_epochs(g, cuda, 0, 1, 5)
    for n in range(1, 5):                                                # epoch by epoch: odd and even counts end in the same buffer
        one = _device_epochs(g, cuda, n, n + 1, 5, y=one)
    assert one.tobytes() == whole.tobytes()
    assert _device_epochs(g, cuda, 3, 3, 5).tobytes() == g["y"].tobytes()                  # no epoch: untouched
    # five epochs from the restatement: the runs have not come apart yet
    want = ref.layout(g["row_ptr"], g["col"], g["period_q"], g["y"], N_EPOCHS, A, B, 5, g["seed"], 0, 5)
    assert np.abs(whole - want).max() < 1e-3


def test_the_wrapper_checks_the_graph_before_the_upload(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    g = fabricated()
    bad = np.array(g["row_ptr"])
    bad[10] = bad[11] + 1
    with pytest.raises(L.HwgError, match="step down"):
        ops.umap_graph(bad, g["col"], g["period_q"], cuda)
    col = np.array(g["col"])
    col[3] = N
    with pytest.raises(L.HwgError, match="col must lie"):
        ops.umap_graph(g["row_ptr"], col, g["period_q"], cuda)
    graph = ops.umap_graph(g["row_ptr"], g["col"], g["period_q"], cuda)
    y = torch.from_numpy(np.array(g["y"])).to(cuda)
    for kw, word in [(dict(neg=0), "limit"), (dict(neg=17), "limit"), (dict(epoch_begin=3, epoch_end=2), "bad sizes"), (dict(epoch_end=N_EPOCHS + 1), "bad sizes")]:
        args = dict(dict(neg=5, epoch_begin=0, epoch_end=1), **kw)
        with pytest.raises(L.HwgError, match=word):
            ops.umap_layout(graph, y, N_EPOCHS, A, B, args["neg"], 0, epoch_begin=args["epoch_begin"], epoch_end=args["epoch_end"])
    with pytest.raises(L.HwgError, match="y must be"):
        ops.umap_layout(graph, y[:-1].contiguous(), N_EPOCHS, A, B, 5, 0)
    with pytest.raises(L.HwgError, match="scratch must be"):
        ops.umap_layout(graph, y, N_EPOCHS, A, B, 5, 0, scratch=y)
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == g["y"].tobytes()                 # nothing ran


def test_quality_of_the_whole_map(cuda):
    """800 points: 40 centres drawn N(0, 1) in D = 64, 20 points each with unit noise, seed 0; n_neighbors 15, 200 epochs. The device's
    map must close at least half of the way from the PCA start to the restatement's own 200-epoch map in trustworthiness at 15
    neighbours (0.673 and 0.997 where this was written), and the share of points whose nearest point in the map has their label must be
    the restatement's (1.000) minus at most 0.02 - the two runs come apart in the last bits after a few epochs, so a point on a border can
    fall either way."""
    from handwriting_line_generation_amd import style_map
    rs = np.random.RandomState(0)
    centres = rs.randn(40, 64)
    labels = np.repeat(np.arange(40), 20)
    x = (centres[labels] + rs.randn(800, 64)).astype(np.float32)
    info = {}
    got = style_map.embed(x, cuda, n_neighbors=15, n_epochs=200, info=info)
    assert got.dtype == np.float32 and got.shape == (800, 2) and np.isfinite(got).all()
    assert (info["n_neighbors"], info["n_epochs"], info["neg"], info["seed"], info["min_dist"]) == (15, 200, 5, 42, 0.2)
    # the restatement's own run, from its own neighbours, graph, curve and PCA
    idx, d2 = ref.knn(x, 14)
    row_ptr, col, period_q, _ = ref.fuzzy_graph(idx, d2, 15, 200)
    a, b = ref.find_ab(1.0, 0.2)
    p = ref.pca(x)
    for axis in range(2):
        if p[np.argmax(np.abs(p[:, axis])), axis] < 0:
            p[:, axis] = -p[:, axis]
    y0 = (10 * p / np.abs(p).max()).astype(np.float32)
    want = ref.layout(row_ptr, col, period_q, y0, 200, float(np.float32(a)), float(np.float32(b)), 5, 42)
    assert np.isfinite(want).all()
    t_pca, t_ref, t_got = ref.trustworthiness(x, y0, 15), ref.trustworthiness(x, want, 15), ref.trustworthiness(x, got, 15)
    s_ref, s_got = ref.nearest_label_share(want, labels), ref.nearest_label_share(got, labels)
    print("trustworthiness at 15 neighbours: PCA start %.4f, restatement %.4f, device %.4f; nearest-label share: restatement %.4f, device %.4f; "
          "%d edges" % (t_pca, t_ref, t_got, s_ref, s_got, info["edges"]))
    assert abs(info["edges"] - col.shape[0]) <= 0.01 * col.shape[0]      # (fp32 and fp64 neighbours differ at near ties only)
    assert t_ref > t_pca + 0.1
    assert t_got > t_pca + 0.5 * (t_ref - t_pca), (t_pca, t_ref, t_got)
    assert s_got >= s_ref - 0.02, (s_ref, s_got)
    # the same seed gives the same bytes, another seed another map
    assert style_map.embed(x, cuda, n_neighbors=15, n_epochs=200).tobytes() == got.tobytes()
    assert style_map.embed(x[:200], cuda, n_neighbors=15, n_epochs=20, seed=1).tobytes() != style_map.embed(x[:200], cuda, n_neighbors=15, n_epochs=20, seed=2).tobytes()
