"""CPU: same-writer / different-writer style distances (evaluate.style_distances, play_styles.py) without a device - the numpy restatement
of the definition (tests/_play_styles_ref.py) against the numbers recorded from the unmodified reference script
(tests/golden/play_styles, tools/gen_golden_play_styles.py), the argument checks of hwg_style_pair_stats in front of its launches, the
host-side pieces (summary, histogram edges, the sort by writer, the pictures) and the program's error exits."""
import io
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import _play_styles_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_STYLES = os.path.join(ROOT, "tests", "golden", "writer_id", "styles.pkl")
GOLD = os.path.join(ROOT, "tests", "golden", "play_styles", "expected.json")


def _golden():
    with open(GOLD_STYLES, "rb") as f:
        data = pickle.load(f)
    return data, json.load(open(GOLD))


def test_restatement_reproduces_the_reference_numbers():
    """the reference's `inter` list is the same-writer set (188 pairs), its `intra` list the 1642 different-writer pairs"""
    data, want = _golden()
    d, same = ref.distances(data["styles"][:, :, 0, 0], ref.ids_of(data["authors"]))[:2]
    assert want["same"]["label"] == "inter" and want["different"]["label"] == "intra"
    for key, part in (("same", d[same]), ("different", d[~same])):
        got = ref.summary(part)
        assert got["pairs"] == want[key]["pairs"] == {"same": 188, "different": 1642}[key]
        for k in ("mean", "std"):
            assert abs(got[k] - want[key][k]) <= 1e-12 * abs(want[key][k]), (key, k, got[k], want[key][k])
    assert want["lines"] == ["inter dist mean: %s, stddev: %s" % (want["same"]["mean"], want["same"]["std"]),
                             "intra dist mean: %s, stddev: %s" % (want["different"]["mean"], want["different"]["std"])]
    # the fp64 variant sees the same distances: the golden input is quarter-valued, every d^2 is exact in fp32
    d64 = ref.distances(data["styles"][:, :, 0, 0], ref.ids_of(data["authors"]), np.float64)[0]
    assert np.array_equal(d, d64)
    # the matrices fold back into the two sets
    st = ref.stats(data["styles"][:, :, 0, 0], ref.ids_of(data["authors"]))
    assert int(np.trace(st["count"])) == 188 and int(np.triu(st["count"], 1).sum()) == 1642
    assert np.array_equal(st["count"], st["count"].T) and np.array_equal(st["sum"], st["sum"].T)


def test_restatement_by_hand():
    # three points on a line, writers a a b: one same-writer pair at distance 1, two different-writer pairs at 3 and 2
    s = np.array([[0.0], [1.0], [3.0]], dtype=np.float32)
    st = ref.stats(s, [0, 0, 1])
    assert st["cells0"] == [(1, 1.0, 1.0), (2, 5.0, 13.0)]
    assert st["count"].tolist() == [[1, 2], [2, 0]] and st["sum"].tolist() == [[1.0, 5.0], [5.0, 0.0]]
    assert (st["min_d2"], st["max_d2"]) == (1.0, 9.0)
    e, e2 = ref.edges(1.0, 9.0, 4)
    assert e.tolist() == [1.0, 1.5, 2.0, 2.5, 3.0] and e2.tolist() == [0.0, 2.25, 4.0, 6.25, np.inf] and e2.dtype == np.float32
    # an edge belongs to the bin on its right: d^2 = 4 falls in [4, 6.25)
    assert ref.histogram(st["d2"], st["same"], e2).tolist() == [[1, 0, 0, 0], [0, 0, 1, 1]]
    assert ref.stats(s[:1], [0])["cells0"] == [(0, 0.0, 0.0), (0, 0.0, 0.0)] and ref.summary([]) == {"pairs": 0, "mean": None, "std": None}


def test_summary_and_matrices_on_the_host():
    from handwriting_line_generation_amd import evaluate
    assert evaluate.pair_summary(0, 0.0, 0.0) == {"pairs": 0, "mean": None, "std": None}
    assert evaluate.pair_summary(1, np.sqrt(2.0), 2.0) == {"pairs": 1, "mean": np.sqrt(2.0), "std": 0.0}      # one pair: std 0, not a rounding residue
    d = np.array([1.0, 2.0, 4.0, 8.5])
    got = evaluate.pair_summary(4, d.sum(), (d * d).sum())
    assert got["pairs"] == 4 and abs(got["mean"] - d.mean()) < 1e-15 and abs(got["std"] - d.std()) < 1e-14
    count, mean, std = evaluate.pair_matrices([[0, 1], [1, 3]], [[0.0, 2.0], [2.0, 6.0]], [[0.0, 4.0], [4.0, 14.0]])
    assert count.dtype == np.int64 and np.isnan(mean[0, 0]) and np.isnan(std[0, 0])
    assert mean[0, 1] == mean[1, 0] == 2.0 and std[0, 1] == 0.0 and mean[1, 1] == 2.0 and abs(std[1, 1] - np.sqrt(14 / 3 - 4)) < 1e-15


def test_histogram_edges():
    from handwriting_line_generation_amd import evaluate
    lo2, hi2 = np.float32(3.0625), np.float32(410.5)
    for bins in (1, 2, 7, 64, 256):
        edges, edge2 = evaluate.pair_edges(lo2, hi2, bins)
        assert edges.dtype == np.float64 and edges.shape == (bins + 1,) and edge2.dtype == np.float32 and edge2.shape == (bins + 1,)
        assert edges[0] == np.sqrt(np.float64(lo2)) and edges[-1] == np.sqrt(np.float64(hi2))                 # the unsquared extremes
        width = np.diff(edges)
        assert np.abs(width - (edges[-1] - edges[0]) / bins).max() <= 4 * np.finfo(np.float64).eps * edges[-1]   # equal width in d
        assert edge2[0] == 0 and np.isinf(edge2[-1]) and (np.diff(edge2) >= 0).all()
        assert np.array_equal(edge2[1:-1], (edges[1:-1] * edges[1:-1]).astype(np.float32))                   # squared in fp64, rounded once
        ref_edges, ref_edge2 = ref.edges(lo2, hi2, bins)
        assert np.abs(ref_edges - edges).max() <= 4 * np.finfo(np.float64).eps * edges[-1]
        # the extremes themselves are counted: the smallest d^2 in the first bin, the largest in the last
        h = ref.histogram(np.array([lo2, hi2], dtype=np.float32), np.array([True, False]), edge2)
        assert h[0, 0] == 1 and h[1, -1] == 1 and h.sum() == 2
    edges, edge2 = evaluate.pair_edges(np.float32(4), np.float32(4), 3)                                       # one distance only
    assert edges.tolist() == [2.0] * 4 and edge2.tolist() == [0.0, 4.0, 4.0, np.inf]
    assert ref.histogram(np.array([4], dtype=np.float32), np.array([True]), edge2).tolist() == [[0, 0, 1], [0, 0, 0]]


class _FakeOps:
    """ops.style_pair_stats and ops.h2d on the host, from the restatement: what evaluate.style_distances does around the device calls
    (checks, author ids, dedupe, the sort by writer, folding, edges) runs without a GPU"""
    SP_SAME_DIFFERENT, SP_WRITER_PAIRS, SP_MAX_WRITERS, SP_MAX_BINS = 0, 1, 4096, 256

    def __init__(self):
        self.calls = []

    def h2d(self, host, device, dtype=None):
        import torch
        return torch.as_tensor(host)

    def style_pair_stats(self, styles, writer, mode, edge2=None, out=None, workspace=None):
        import torch
        s, w = styles.numpy(), writer.numpy()
        assert (np.diff(w) >= 0).all() and w[0] == 0, "the rows must arrive sorted by writer"
        self.calls.append((mode, None if edge2 is None else len(edge2) - 1))
        st = ref.stats(s, w)
        if mode == 0:
            cells = [np.array([c[k] for c in st["cells0"]]) for k in range(3)]
        else:
            cells = [st["count"], st["sum"], st["sumsq"]]
        hist = None if edge2 is None else torch.from_numpy(ref.histogram(st["d2"], st["same"], edge2))
        return (torch.from_numpy(cells[0].astype(np.int64)), torch.from_numpy(cells[1].astype(np.float64)),
                torch.from_numpy(cells[2].astype(np.float64)), torch.tensor([st["min_d2"], st["max_d2"]], dtype=torch.float32), hist)


def _same_result(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


def test_style_distances_sorts_by_writer_and_forgets_the_order(monkeypatch):
    from handwriting_line_generation_amd import evaluate
    data, want = _golden()
    fake = _FakeOps()
    monkeypatch.setattr(evaluate, "ops", fake)
    styles, authors = data["styles"], list(data["authors"])
    got = evaluate.style_distances(styles, authors, None)
    assert fake.calls == [(1, None), (0, 64)]                                   # the sums per writer pair, then the histogram
    assert (got["lines"], got["dim"], got["writers"]) == (61, 37, len(set(authors))) and "dropped" not in got
    for key in ("same", "different"):
        assert got[key]["pairs"] == want[key]["pairs"]
        for k in ("mean", "std"):
            assert abs(got[key][k] - want[key][k]) <= 1e-12 * want[key][k]
    assert sum(got["hist"]["same"]) == 188 and sum(got["hist"]["different"]) == 1642 and len(got["hist"]["edges"]) == 65
    assert got["writer_names"] == list(dict.fromkeys(authors)) and got["pair_count"].shape == (got["writers"],) * 2
    solo = got["writer_names"].index("solo")
    assert got["pair_count"][solo, solo] == 0 and np.isnan(got["pair_mean"][solo, solo]) and np.isnan(got["pair_std"][solo, solo])
    assert int(np.triu(got["pair_count"]).sum()) == 1830
    # without the matrices: one call in mode 0 for the sums, the same scalars
    flat = evaluate.style_distances(styles[:, :, 0, 0], authors, None, matrices=False)
    assert fake.calls[2:] == [(0, None), (0, 64)] and "pair_count" not in flat and "writer_names" not in flat
    assert flat["hist"] == got["hist"] and flat["same"]["pairs"] == 188
    for key in ("same", "different"):
        for k in ("mean", "std"):
            assert abs(flat[key][k] - got[key][k]) <= 1e-13 * got[key][k]
    # a shuffled input gives the same dictionary once the writers are put in the same order (they are numbered by first appearance)
    perm = np.random.RandomState(5).permutation(61)
    shuffled = evaluate.style_distances(styles[perm], [authors[i] for i in perm], None)
    to = [shuffled["writer_names"].index(a) for a in got["writer_names"]]
    shuffled["writer_names"] = [shuffled["writer_names"][i] for i in to]
    for k in ("pair_count", "pair_mean", "pair_std"):
        shuffled[k] = shuffled[k][np.ix_(to, to)]
    _same_result(shuffled, got)
    # dedupe drops the two repeated rows of the golden file
    dd = evaluate.style_distances(styles, authors, None, dedupe=True, bins=7)
    assert dd["dropped"] == 2 and dd["lines"] == 59 and dd["same"]["pairs"] + dd["different"]["pairs"] == 59 * 58 // 2 and len(dd["hist"]["same"]) == 7
    # one line: no pair, no histogram call
    del fake.calls[:]
    one = evaluate.style_distances(styles[:1], authors[:1], None)
    assert one["same"] == one["different"] == {"pairs": 0, "mean": None, "std": None} and one["hist"] == {"edges": [], "same": [], "different": []}
    assert fake.calls == [(1, None)] and np.isnan(one["pair_mean"]).all() and one["pair_count"].tolist() == [[0]]


def test_style_distances_leaves_the_matrices_out_above_4096_writers(monkeypatch, capsys):
    from handwriting_line_generation_amd import evaluate

    class Counting(_FakeOps):
        def style_pair_stats(self, styles, writer, mode, edge2=None, out=None, workspace=None):
            import torch
            self.calls.append((mode, None if edge2 is None else len(edge2) - 1))
            n = len(writer)
            hist = None if edge2 is None else torch.zeros((2, len(edge2) - 1), dtype=torch.int64)
            return (torch.tensor([0, n * (n - 1) // 2]), torch.tensor([0.0, 1.0]), torch.tensor([0.0, 1.0]), torch.tensor([1.0, 1.0]), hist)
    fake = Counting()
    monkeypatch.setattr(evaluate, "ops", fake)
    n = 4097
    got = evaluate.style_distances(np.arange(n, dtype=np.float32)[:, None], list(range(n)), None)
    assert fake.calls[0] == (0, None) and "pair_count" not in got and got["writers"] == n          # not an error: a note
    assert "4097 writers" in capsys.readouterr().out


def test_style_distances_refuses_bad_input_before_the_device():
    from handwriting_line_generation_amd import evaluate
    s = np.zeros((5, 3), dtype=np.float32)
    s[3, 1] = np.nan
    with pytest.raises(ValueError, match="row 3"):
        evaluate.style_distances(s, list("abcde"), None)
    with pytest.raises(ValueError, match="authors"):
        evaluate.style_distances(np.zeros((5, 3), dtype=np.float32), list("abcd"), None)
    with pytest.raises(ValueError, match="styles must be"):
        evaluate.style_distances(np.zeros((5, 3, 2, 1), dtype=np.float32), list("abcde"), None)
    with pytest.raises(ValueError, match="styles must be"):
        evaluate.style_distances(np.zeros((0, 3), dtype=np.float32), [], None)
    for bins in (0, 257, 2.5, True):
        with pytest.raises(ValueError, match="bins"):
            evaluate.style_distances(np.zeros((5, 3), dtype=np.float32), list("abcde"), None, bins=bins)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """the argument checks of hwg_style_pair_stats run on the host side of the entry point, in front of every launch and of the memset: with
    arguments they refuse, the call returns its status without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20
    need0 = L.query("hwg_style_pair_stats_workspace", 61, 13, 0)
    need1 = L.query("hwg_style_pair_stats_workspace", 61, 13, 1)
    assert 0 < need0 < need1 and need0 % 16 == 0 and need1 % 16 == 0
    assert need1 >= (4 + 13) * 13 * 20                                             # (row blocks + writers) slots of A cells
    for bad in ((0, 1, 0), (61, 0, 0), (61, 62, 0), (61, 13, 2), ((1 << 20) + 1, 1, 0), (8192, 4097, 1)):
        assert L.query("hwg_style_pair_stats_workspace", *bad) == 0, bad
    assert L.query("hwg_style_pair_stats_workspace", 8192, 4097, 0) > 0              # mode 0 has no limit on the writers

    def args(styles=p, writer=p, N=61, D=37, A=13, mode=1, edge2=None, bins=0, count=p, total=p, sq=p, rng=p, hist=None, ws=p, ws_bytes=None):
        return (styles, writer, N, D, A, mode, edge2, bins, count, total, sq, rng, hist, ws, need1 if ws_bytes is None else ws_bytes, 0)
    cases = [(args(styles=None), "null"), (args(writer=None), "null"), (args(count=None), "null"), (args(total=None), "null"),
             (args(sq=None), "null"), (args(rng=None), "null"), (args(ws=None), "null"),
             (args(edge2=p, bins=4), "come together"), (args(hist=p, bins=4), "come together"), (args(bins=4), "come together"),
             (args(N=0), "bad sizes"), (args(D=0), "bad sizes"), (args(A=0), "bad sizes"), (args(A=62), "bad sizes"), (args(mode=2), "bad sizes"),
             (args(mode=-1), "bad sizes"), (args(edge2=p, hist=p, bins=0), "bad sizes"),
             (args(N=(1 << 20) + 1), "limit"), (args(D=65537), "limit"), (args(edge2=p, hist=p, bins=257), "limit"),
             (args(N=8192, A=4097), "limit"),
             (args(styles=p + 8), "aligned"), (args(writer=p + 2), "aligned"), (args(count=p + 4), "aligned"), (args(total=p + 4), "aligned"),
             (args(sq=p + 4), "aligned"), (args(rng=p + 2), "aligned"), (args(ws=p + 8), "aligned"), (args(edge2=p + 2, hist=p, bins=4), "aligned"),
             (args(edge2=p, hist=p + 4, bins=4), "aligned"),
             (args(ws_bytes=need1 - 1), "workspace"), (args(ws_bytes=0), "workspace"), (args(mode=0, ws_bytes=need0 - 16), "workspace")]
    for a, word in cases:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_style_pair_stats", *a)
        assert word in str(e.value), (a, str(e.value))


def test_ops_wrapper_refuses_wrong_tensors_without_a_device():
    import torch
    from handwriting_line_generation_amd import _lib as L, ops
    ids = torch.zeros(4, dtype=torch.int32)
    good = torch.zeros(4, 3)
    for styles in (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, 1), torch.zeros(0, 3), np.zeros((4, 3), dtype=np.float32)):
        with pytest.raises(L.HwgError, match="styles must be"):
            ops.style_pair_stats(styles, ids, 0)
    for writer in (torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), [0, 0, 0, 0]):
        with pytest.raises(L.HwgError, match="writer must be"):
            ops.style_pair_stats(good, writer, 0)
    with pytest.raises(L.HwgError, match="mode"):
        ops.style_pair_stats(good, ids, 2)
    # the order of the writers is checked on the host: not sorted, negative, ids beyond the number of rows
    for writer, word in (([0, 1, 0, 1], "never decrease"), ([-1, 0, 0, 1], "never decrease"), ([0, 0, 1, 9], "number the writers")):
        with pytest.raises(L.HwgError, match=word):
            ops.style_pair_stats(good, torch.tensor(writer, dtype=torch.int32), 0)
    for edge2 in (np.array([0.0, 2.0, 1.0, np.inf], dtype=np.float32), np.array([0.0, 1.0], dtype=np.float64), np.zeros(1, dtype=np.float32),
                  np.array([0.0, np.nan, 2.0], dtype=np.float32), np.zeros(258, dtype=np.float32)):
        with pytest.raises(L.HwgError, match="edge2"):
            ops.style_pair_stats(good, ids, 0, edge2=edge2)
    with pytest.raises(L.HwgError, match="GPU"):                                  # a missing device is an error, never a host computation
        ops.style_pair_stats(good, ids, 0)


def test_pictures():
    import play_styles as cli
    from PIL import Image
    assert [cli.cell_pixels(a) for a in (1, 13, 64, 65, 100, 1024, 1025, 4096)] == [16, 16, 16, 15, 10, 1, 1, 1]
    m = np.array([[1.0, 2.0, np.nan], [2.0, 5.0, 3.0], [np.nan, 3.0, 4.0]])
    px = cli.heat_pixels(m)
    assert px.shape == (48, 48, 3) and px.dtype == np.uint8
    assert (px[0:16, 32:48] == cli.GREY).all() and (px[32:48, 0:16] == cli.GREY).all()               # NaN cells are grey
    assert tuple(px[0, 0]) == cli.RAMP_LIGHT and tuple(px[16, 16]) == cli.RAMP_DARK                  # the smallest and the largest value
    assert (px[:16, :16] == px[0, 0]).all()                                                          # one square per cell
    shade = [int(px[16 * r, 16 * c].astype(int).sum()) for r, c in ((0, 0), (0, 1), (1, 2), (2, 2), (1, 1))]   # values 1, 2, 3, 4, 5
    assert shade == sorted(shade, reverse=True) and len(set(shade)) == 5                             # larger values come out darker
    im = Image.open(io.BytesIO(cli.heat_map(m)))
    assert im.size == (48, 48) and im.mode == "RGB" and np.array_equal(np.asarray(im), px)
    assert cli.heat_pixels(np.full((2, 2), np.nan)).reshape(-1, 3).tolist() == [list(cli.GREY)] * (32 * 32)
    assert (cli.heat_pixels(np.full((2, 2), 7.0)) == cli.RAMP_LIGHT).all()                           # a constant matrix: no division by zero
    assert cli.heat_pixels(np.zeros((2000, 2000))).shape == (2000, 2000, 3)
    im = Image.open(io.BytesIO(cli.hist_picture([0, 5, 10, 0], [1, 0, 0, 30])))
    assert im.size == cli.HIST_SIZE and im.mode == "RGB"
    got = np.asarray(im).reshape(-1, 3)
    for name in ("same", "different"):
        assert (got == cli.HIST_COLOURS[name]).all(axis=1).sum() > 50, name                          # both outlines are there
    assert Image.open(io.BytesIO(cli.hist_picture([], []))).size == cli.HIST_SIZE                    # no pair: an empty frame


def test_npz_and_json_parts():
    import play_styles as cli
    result = {"lines": 3, "dim": 2, "writers": 2, "same": {"pairs": 1, "mean": 1.0, "std": 0.0}, "different": {"pairs": 0, "mean": None, "std": None},
              "hist": {"edges": [1.0, 1.0], "same": [1], "different": [0]}, "writer_names": ["a", 7], "pair_count": np.zeros((2, 2), dtype=np.int64),
              "pair_mean": np.zeros((2, 2)), "pair_std": np.zeros((2, 2))}
    assert json.loads(json.dumps(cli.scalar_part(result))) == {k: result[k] for k in ("lines", "dim", "writers", "same", "different", "hist")}
    arrays = cli.npz_arrays(result)
    assert set(arrays) == {"lines", "dim", "writers", "pair_count", "pair_mean", "pair_std", "same_pairs", "same_mean", "same_std", "different_pairs",
                           "different_mean", "different_std", "hist_edges", "hist_same", "hist_different", "writer_names"}
    assert np.isnan(arrays["different_mean"]) and arrays["writer_names"].tolist() == ["a", "7"] and arrays["hist_same"].dtype == np.int64


def _program(args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "play_styles.py")] + args, cwd=cwd, timeout=120, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)


def test_play_styles_arguments_and_error_exits(tmp_path):
    import play_styles as cli
    a = cli.parse_args(["some/prefix_", "-g", "2", "--dedupe", "--bins", "32", "-o", "out/p", "--json", "o.json"])
    assert (a.style_loc, a.gpu, a.dedupe, a.bins, a.out, a.json) == ("some/prefix_", 2, True, 32, "out/p", "o.json")
    a = cli.parse_args(["p*"])
    assert (a.style_loc, a.gpu, a.dedupe, a.bins, a.out, a.json) == ("p*", 0, False, 64, None, None)
    r = _program([], str(tmp_path))
    assert r.returncode != 0 and "style_loc" in r.stdout, r.stdout[-2000:]
    # a prefix that matches nothing: a message under this program's name, before torch or the device are touched
    r = _program([str(tmp_path / "none_styles_")], str(tmp_path))
    assert r.returncode != 0 and "play_styles.py: no file matches" in r.stdout and "none_styles_*" in r.stdout, r.stdout[-2000:]
    assert "Traceback" not in r.stdout and "eval_writer_id.py" not in r.stdout
    r = _program([str(tmp_path / "none_styles_"), "--bins", "0"], str(tmp_path))
    assert r.returncode != 0 and "--bins" in r.stdout, r.stdout[-2000:]
    with open(str(tmp_path / "c_styles_1.pkl"), "wb") as f:
        f.write(b"not a pickle")
    r = _program([str(tmp_path / "c_styles_")], str(tmp_path))
    assert r.returncode != 0 and "c_styles_1.pkl" in r.stdout and "Traceback" not in r.stdout, r.stdout[-2000:]


def test_get_styles_has_the_distances_flag():
    import get_styles as cli
    assert cli.parse_args(["-c", "x.pth", "-d", "o", "--distances"]).distances is True
    assert cli.parse_args(["-c", "x.pth", "-d", "o"]).distances is False


def test_golden_tool_writes_nothing_without_the_reference(tmp_path):
    before = open(GOLD).read()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_play_styles.py")], cwd=str(tmp_path), timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "nothing written" in r.stdout, r.stdout[-2000:]
    assert open(GOLD).read() == before and os.listdir(str(tmp_path)) == []
