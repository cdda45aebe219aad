"""CPU: the host side of umap_styles.py (handwriting_line_generation_amd/style_map.py, the program's argument handling, picture and
ordered.txt) against tests/_umap_ref.py, the restatement of the definitions. No umap-learn output serves as a golden file: umap-learn is
not installed where these tests were written; the four (a, b) pairs below were computed with scipy.optimize.curve_fit. No device is touched."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import _umap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AB_TABLE = [(0.2, 1.262058, 1.003005), (0.1, 1.576943, 0.895061), (0.0, 1.932808, 0.790495), (0.5, 0.583030, 1.334167)]


@pytest.mark.parametrize("min_dist,a,b", AB_TABLE)
def test_find_ab_against_curve_fit(min_dist, a, b):
    from handwriting_line_generation_amd import style_map
    got = style_map.find_ab(1.0, min_dist)
    assert abs(got[0] - a) <= 1e-4 * a and abs(got[1] - b) <= 1e-4 * b, got
    mine = ref.find_ab(1.0, min_dist)
    assert abs(mine[0] - a) <= 1e-4 * a and abs(mine[1] - b) <= 1e-4 * b, mine


def test_the_restatements_philox_is_philox4x32():
    from oracle import optim_ref
    seed, ctr0 = 0x123456789ABCDEF, (1 << 33) + 5
    blocks = optim_ref.philox_blocks(seed, ctr0, 3)
    for k in range(3):
        c = ctr0 + k
        want = optim_ref.philox4x32((c & 0xFFFFFFFF, c >> 32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
        assert tuple(int(v) for v in blocks[k]) == want
    far = ref.negative_samples(7, 1000, 11, 5, seed)              # 5 repulsions: two blocks per edge, words 0..3 of the first, 0 of the second
    assert far.shape == (11, 5) and far.min() >= 0 and far.max() < 1000
    e, t = 4, 4
    c = (7 * 11 + e) * 2 + t // 4
    word = optim_ref.philox4x32((c & 0xFFFFFFFF, c >> 32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[t % 4]
    assert far[e, t] == (word * 1000) >> 32


def _knn_case(n, d, k, seed):
    """Gaussian clusters with planted copies -> (idx, d2) of the restatement's exact kNN: row 1 copies row 0 (their first neighbour is at
    distance 0), rows 2..2+k are one point (a row of all-zero distances)"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(n // 10 + 1, d)[rs.randint(0, n // 10 + 1, n)] * 2 + rs.randn(n, d)).astype(np.float32)
    x[1] = x[0]
    x[2:3 + k] = x[2]
    return ref.knn(x, k, dtype=np.float32)


@pytest.mark.parametrize("n,d,k,n_epochs", [(120, 7, 14, 200), (60, 3, 5, 500), (40, 4, 1, 50), (300, 16, 34, 200)])
def test_fuzzy_graph_against_the_restatement(n, d, k, n_epochs):
    from handwriting_line_generation_amd import style_map
    idx, d2 = _knn_case(n, d, k, seed=n + k)
    assert (d2[2] == 0).all() and d2[0, 0] == 0 and d2[0, 1 if k > 1 else 0] >= 0
    row_ptr, col, period_q, w = style_map.fuzzy_graph(idx, d2, k + 1, n_epochs)
    want_ptr, want_col, want_q, want_w = ref.fuzzy_graph(idx, d2, k + 1, n_epochs)
    assert row_ptr.dtype == col.dtype == period_q.dtype == np.int32
    assert np.array_equal(row_ptr, want_ptr) and np.array_equal(col, want_col)
    assert np.abs(w - want_w).max() <= 1e-12, np.abs(w - want_w).max()
    near_half = np.abs((65536 * want_w.max() / want_w) % 1 - 0.5) < 1e-6           # a period whose rounding 1e-12 could turn: none here
    assert not near_half.any() and np.array_equal(period_q, want_q)
    # sorted by (row, column), symmetric, no self edge, every vertex has an edge
    e = row_ptr[-1]
    owner = np.repeat(np.arange(n), np.diff(row_ptr))
    keys = owner.astype(np.int64) * n + col
    assert (np.diff(keys) > 0).all() and (owner != col).all() and (np.diff(row_ptr) >= 1).all()
    pairs = dict(zip(zip(owner.tolist(), col.tolist()), w.tolist()))
    assert all(pairs[(j, i)] == v for (i, j), v in pairs.items())
    # the schedule
    assert period_q.min() >= 65536 and period_q.max() <= 65536 * n_epochs and (period_q == 65536).any()
    drawn = np.zeros(e, dtype=np.int64)
    for epoch in range(1, n_epochs + 1):
        drawn += ref.active_edges(period_q, epoch)
    assert np.array_equal(drawn, (n_epochs * 65536) // period_q.astype(np.int64)) and drawn.min() >= 1 and drawn.max() == n_epochs


def test_smooth_knn_by_hand():
    from handwriting_line_generation_amd import style_map
    # K = 1, n_neighbors = 2: the target is log2(2) = 1 and the single neighbour at rho weighs 1: the bisection stops at its start
    rho, sigma = style_map.smooth_knn(np.array([[2.0], [0.0]]), 2)
    assert rho.tolist() == [2.0, 0.0] and sigma.tolist() == [1.0, 1.0]
    # all-zero row: every weight is 1, p = K > target for ever: sigma falls to the floor 1e-3 mean(all)
    dist = np.array([[0.0, 0.0, 0.0, 0.0], [0.0, 1.0, 2.0, 4.0]])
    rho, sigma = style_map.smooth_knn(dist, 5)
    assert rho.tolist() == [0.0, 1.0] and sigma[0] == 1e-3 * dist.mean()
    p = 2 + np.exp(-1 / sigma[1]) + np.exp(-3 / sigma[1])
    assert abs(p - np.log2(5)) < 1e-5


def test_fuzzy_graph_refuses_what_it_cannot_schedule():
    from handwriting_line_generation_amd import style_map
    idx, d2 = _knn_case(40, 4, 3, seed=1)
    with pytest.raises(ValueError, match="n_neighbors - 1"):
        style_map.fuzzy_graph(idx, d2, 5, 100)
    with pytest.raises(ValueError, match="n_epochs"):
        style_map.fuzzy_graph(idx, d2, 4, 40000)


def test_pca_init_sign_and_scale():
    from handwriting_line_generation_amd import style_map
    rs = np.random.RandomState(4)
    x = (rs.randn(200, 6) * np.array([5, 3, 1, 1, 0.5, 0.1])) @ np.linalg.qr(rs.randn(6, 6))[0]
    y0 = style_map.pca_init(x.astype(np.float32))
    assert y0.dtype == np.float32 and y0.shape == (200, 2)
    assert abs(float(np.abs(y0).max()) - 10.0) < 1e-5
    for axis in range(2):
        assert y0[np.argmax(np.abs(y0[:, axis])), axis] > 0
    p = ref.pca(x.astype(np.float32))
    for axis in range(2):                                             # the same axes up to sign, one scale for both
        c = np.corrcoef(p[:, axis], y0[:, axis])[0, 1]
        assert abs(abs(c) - 1) < 1e-6, c
    assert abs(np.abs(y0[:, 0]).max() / np.abs(y0[:, 1]).max() - np.abs(p[:, 0]).max() / np.abs(p[:, 1]).max()) < 1e-4
    # the sign is fixed by the data, not by the solver: mirrored styles give the same map (the row with the largest projection keeps it positive)
    assert np.allclose(style_map.pca_init(-x.astype(np.float32)), y0, atol=1e-5)
    one = style_map.pca_init(np.arange(5, dtype=np.float32)[:, None])  # D = 1: the second axis is empty
    assert one.shape == (5, 2) and (one[:, 1] == 0).all() and one[:, 0].max() == 10


def test_embed_refuses_bad_styles_before_the_device():
    from handwriting_line_generation_amd import style_map
    s = np.random.RandomState(0).randn(6, 3).astype(np.float32)
    bad = s.copy()
    bad[4, 2] = np.nan
    with pytest.raises(ValueError, match="row 4"):
        style_map.embed(bad, None)
    with pytest.raises(ValueError, match="2 distinct"):
        style_map.embed(np.repeat(s[:2], 3, axis=0), None)
    with pytest.raises(ValueError, match="styles must be"):
        style_map.embed(np.zeros((5, 3, 2, 1), dtype=np.float32), None)
    with pytest.raises(ValueError, match="n_neighbors"):
        style_map.embed(s, None, n_neighbors=1)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """the argument checks run on the host side of the entry points, in front of the launches: with arguments they refuse, the call
    returns its status without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20

    def knn(styles=p, N=100, D=8, K=5, idx=p, d2=p):
        return (styles, N, D, K, idx, d2, 0)
    for a, word in [(knn(styles=None), "null"), (knn(idx=None), "null"), (knn(d2=None), "null"), (knn(K=0), "bad sizes"), (knn(D=0), "bad sizes"),
                    (knn(N=1, K=1), "bad sizes"), (knn(K=65), "limit"), (knn(N=50, K=50), "limit"), (knn(N=(1 << 20) + 1), "limit"),
                    (knn(D=65537), "limit"), (knn(styles=p + 4), "aligned"), (knn(styles=p + 8), "aligned"), (knn(idx=p + 2), "aligned"),
                    (knn(d2=p + 1), "aligned")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_knn_rows", *a)
        assert word in str(e.value), (a, str(e.value))

    def lay(row_ptr=p, col=p, q=p, N=100, E=500, y=p, ys=2 * p, e0=0, e1=10, ne=10, a=1.5, b=0.9, neg=5, seed=1):
        return (row_ptr, col, q, N, E, y, ys, e0, e1, ne, a, b, neg, seed, 0)
    for a, word in [(lay(row_ptr=None), "null"), (lay(col=None), "null"), (lay(q=None), "null"), (lay(y=None), "null"), (lay(ys=None), "null"),
                    (lay(ys=p), "two buffers"), (lay(N=0), "bad sizes"), (lay(E=0), "bad sizes"), (lay(e0=-1), "bad sizes"),
                    (lay(e0=5, e1=4), "bad sizes"), (lay(e1=11), "bad sizes"), (lay(ne=0, e1=0), "bad sizes"), (lay(N=(1 << 20) + 1), "limit"),
                    (lay(neg=0), "limit"), (lay(neg=17), "limit"), (lay(ne=32768), "limit"), (lay(a=0.0), "positive"), (lay(b=-1.0), "positive"),
                    (lay(a=float("nan")), "positive"), (lay(y=p + 4), "aligned"), (lay(ys=2 * p + 4), "aligned"), (lay(col=p + 2), "aligned")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_umap_layout", *a)
        assert word in str(e.value), (a, str(e.value))
    assert L.abi_version() == 6


def test_ops_wrappers_refuse_without_a_device():
    import torch
    from handwriting_line_generation_amd import _lib as L, ops
    for styles in (torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.float64), np.zeros((4, 3), dtype=np.float32)):
        with pytest.raises(L.HwgError):
            ops.knn_rows(styles, 2)
    ok = dict(row_ptr=[0, 2, 3, 4], col=[1, 2, 0, 0], period_q=[65536, 70000, 65536, 70000])
    for change, word in [(dict(row_ptr=[0, 3, 2, 4]), "step down"), (dict(row_ptr=[1, 2, 3, 4]), "rise from 0"), (dict(row_ptr=[0, 2, 3, 5]), "rise from 0"),
                         (dict(col=[1, 2, 0, 3]), "col must lie"), (dict(col=[1, -1, 0, 0]), "col must lie"),
                         (dict(period_q=[65536, 0, 65536, 70000]), "period_q must lie"), (dict(period_q=[65536, 65536, 70000]), "bad sizes"),
                         (dict(col=[1.0, 2.0, 0.0, 0.0]), "integer array")]:
        with pytest.raises(L.HwgError, match=word):
            ops.umap_graph(**dict(ok, **change), device="cpu")
    with pytest.raises(L.HwgError, match="umap_graph"):
        ops.umap_layout((1, 2, 3), torch.zeros(3, 2), 10, 1.0, 1.0, 5, 0)


def _dump(path, styles, authors):
    with open(path, "wb") as f:
        pickle.dump({"styles": styles, "authors": authors}, f)


def _program(args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "umap_styles.py")] + args, cwd=cwd, timeout=120, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)


def test_umap_styles_arguments_and_error_exits(tmp_path):
    import umap_styles as cli
    a = cli.parse_args(["some/prefix_"])
    assert (a.style_loc, a.image_dir, a.add, a.gpu, a.dedupe, a.n_neighbors, a.min_dist, a.epochs, a.seed, a.out) == (
        "some/prefix_", None, None, 0, False, 35, 0.2, None, 42, "umap_styles")
    a = cli.parse_args(["p*", "pictures", "add", "-g", "2", "--dedupe", "--n-neighbors", "15", "--min-dist", "0.1", "--epochs", "100", "--seed", "7",
                        "-o", "here/map"])
    assert (a.style_loc, a.image_dir, a.add, a.gpu, a.dedupe, a.n_neighbors, a.min_dist, a.epochs, a.seed, a.out) == (
        "p*", "pictures", "add", 2, True, 15, 0.1, 100, 7, "here/map")
    r = _program([], str(tmp_path))
    assert r.returncode != 0 and "style_loc" in r.stdout, r.stdout[-2000:]
    r = _program([str(tmp_path / "none_styles_")], str(tmp_path))
    assert r.returncode != 0 and "umap_styles.py: no file matches" in r.stdout and "Traceback" not in r.stdout, r.stdout[-2000:]
    g = np.random.RandomState(0)
    s = g.randn(5, 4).astype(np.float32)
    s[3, 1] = np.nan
    _dump(str(tmp_path / "a_styles_1.pkl"), s, list("xyxyz"))
    r = _program([str(tmp_path / "a_styles_")], str(tmp_path))
    assert r.returncode != 0 and "row 3 is not finite" in r.stdout and "Traceback" not in r.stdout, r.stdout[-2000:]
    _dump(str(tmp_path / "b_styles_1.pkl"), np.repeat(g.randn(2, 4).astype(np.float32), 4, axis=0), list("xxxxyyyy"))
    r = _program([str(tmp_path / "b_styles_")], str(tmp_path))
    assert r.returncode != 0 and "2 distinct style rows" in r.stdout and "Traceback" not in r.stdout, r.stdout[-2000:]
    _dump(str(tmp_path / "c_styles_1.pkl"), g.randn(3, 4, 1, 1).astype(np.float32), list("xyx"))
    _dump(str(tmp_path / "c_styles_2.pkl"), g.randn(2, 5).astype(np.float32), list("xy"))
    r = _program([str(tmp_path / "c_styles_")], str(tmp_path))
    assert r.returncode != 0 and "c_styles_2.pkl" in r.stdout and "style_dim" in r.stdout and "Traceback" not in r.stdout, r.stdout[-2000:]
    assert not [n for n in os.listdir(str(tmp_path)) if n.endswith((".npz", ".png"))]


def test_prepare_add_and_dedupe(tmp_path):
    import umap_styles as cli
    g = np.random.RandomState(1)
    base = g.randn(4, 6).astype(np.float32)
    _dump(str(tmp_path / "s_1.pkl"), base[[0, 0, 1, 1, 1]], ["a", "a", "a", "b", "b"])
    _dump(str(tmp_path / "s_2.pkl"), base[[2, 3, 3]][:, :, None, None], np.array(["b", "c", "c"]))
    styles, authors, raw, row_of_raw = cli.prepare(cli.parse_args([str(tmp_path / "s_"), "--dedupe"]))
    # line 1 repeats line 0; line 3 has the style of line 2 but another writer; line 4 repeats 3; line 7 repeats 6
    assert authors == ["a", "a", "b", "b", "c"] and np.array_equal(styles, base[[0, 1, 1, 2, 3]])
    assert raw == ["a", "a", "a", "b", "b", "b", "c", "c"] and row_of_raw.tolist() == [0, 0, 1, 2, 2, 3, 4, 4]
    styles, authors, raw, row_of_raw = cli.prepare(cli.parse_args([str(tmp_path / "s_"), "pictures", "add"]))
    assert styles.shape == (108, 6) and authors[8:] == [cli.EXTRA_AUTHOR] * 100 and row_of_raw.tolist() == list(range(108))
    np.random.seed(42)
    assert np.array_equal(styles[8:], np.random.normal(size=(100, 6)).astype(np.float32))


def test_png_writer_on_a_fixed_embedding(tmp_path):
    import io
    from PIL import Image
    import umap_styles as cli
    emb = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 5.0], [10.0, 5.0], [5.0, 2.5]], dtype=np.float32)
    authors = ["w1", "w2", "w1", 7, cli.EXTRA_AUTHOR]
    thumb = str(tmp_path / "w2_0.png")
    Image.fromarray(np.full((60, 200), 90, dtype=np.uint8)).save(thumb)
    data = cli.draw_map(emb, authors, size=400)
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.mode == "RGB" and im.size == (400, 400)
    px = np.asarray(im)
    pts = cli.map_points(emb, 400)
    assert pts.min() >= 20 - 1 and pts.max() <= 379 + 1 and pts[0, 0] == pts[2, 0] < pts[1, 0] == pts[3, 0]
    assert pts[0, 1] > pts[2, 1]                                                # y grows upwards
    assert abs((pts[1, 0] - pts[0, 0]) - 2 * (pts[0, 1] - pts[2, 1])) <= 2      # one scale for both axes (each point rounded to a pixel)
    colours = cli.writer_colours(authors)
    rs = np.random.RandomState(42)
    want = [tuple(int(v) for v in (rs.rand(3) * 255).astype(np.uint8)) for _ in range(3)]
    assert [colours["w1"], colours["w2"], colours[7]] == want and colours[cli.EXTRA_AUTHOR] == (0, 0, 0)
    for (x, y), a in zip(pts.tolist(), authors):
        assert tuple(px[y, x]) == colours[a], (a, px[y, x])
    assert tuple(px[0, 0]) == (255, 255, 255) and tuple(px[pts[0, 1], pts[0, 0] + cli.DOT + 3]) == (255, 255, 255)
    # a thumbnail: a tenth of 200 x 60, centred on its row's point
    px = np.asarray(Image.open(io.BytesIO(cli.draw_map(emb, authors, size=400, thumbs=[(1, thumb)]))))
    x, y = pts[1].tolist()
    assert (px[y - 3:y + 3, x - 10:x + 10] == 90).all() and tuple(px[y - 3 - cli.DOT - 2, x]) == (255, 255, 255)


def test_ordered_txt_round_trip(tmp_path):
    import umap_styles as cli
    names = [cli.picture_name(a, i) for a in ("a01", 7) for i in range(3)]
    assert names[:4] == ["a01_0.png", "a01_1.png", "a01_2.png", "7_0.png"]
    cli.write_ordered(str(tmp_path), 3, names)
    text = (tmp_path / "ordered.txt").read_text()
    assert text.splitlines() == ["3"] + names and text.endswith("\n")
    assert os.listdir(str(tmp_path)) == ["ordered.txt"]                         # nothing left of the temporary name
    assert cli.read_ordered(str(tmp_path)) == (3, names)
    # picture <author>_<i> is line i of that writer in the files; with --dedupe a dropped line's row is the one it repeats
    raw_authors = ["a01", 7, "a01", "a01", 7, 7, "a01"]
    got = cli.thumbnails(str(tmp_path), raw_authors, [0, 1, 2, 2, 3, 4, 5])
    assert got == [(r, os.path.join(str(tmp_path), n)) for r, n in zip([0, 2, 2, 1, 3, 4], names)]
    with pytest.raises(SystemExit, match="ordered.txt"):
        cli.thumbnails(str(tmp_path), ["a01", 7, "a01"], [0, 1, 2])
    with pytest.raises(SystemExit, match="cannot read"):
        cli.read_ordered(str(tmp_path / "nowhere"))


def test_generate_knows_the_u_action(tmp_path):
    import generate as cli
    assert "u" in cli.CHOICES and cli.PER_AUTHOR == 3
    with pytest.raises(NotImplementedError) as e:
        cli.main(["-c", str(tmp_path / "none.pth"), "-d", str(tmp_path / "out"), "-r", "choice=i"])
    assert all(w in str(e.value) for w in ("'R'", "'f'", "'u'", "'i'"))
