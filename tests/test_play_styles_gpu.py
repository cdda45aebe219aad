"""GPU: same-writer / different-writer style distances on the device (csrc/style_pairs.hip through ops.style_pair_stats,
evaluate.style_distances, play_styles.py and get_styles.py --distances) against tests/_play_styles_ref.py, the numpy restatement that
tests/test_play_styles_cpu.py pins to the reference's recorded numbers.

Exact block: every style value is a multiple of 1/4 with |value| <= 16 and D <= 129, so every d^2 is exact in fp32 in any summation order
(tests/test_writer_id_gpu.py): count, hist, min_d2 and max_d2 must be EQUAL to the restatement's. A cell's sum and sumsq are fp64 sums of n
non-negative terms (each term correctly rounded: the fp64 root, the exact conversion of d^2) in the kernel's order, against the
restatement's exactly rounded sum: any order of n - 1 additions is within (n - 1) 2^-53 relative of the exact sum, the bound is that
doubled and rounded up: n 2^-52. The variance q / n - m^2 then carries at most n 2^-52 rms^2 (rms^2 = q / n), i.e. the standard deviation
n 2^-52 rms^2 / std (where std is 0: sqrt(n 2^-52 rms^2)).
Real-valued block: against the restatement in fp64. d^2 is one sequential fp32 chain of D fused steps on once-rounded differences: within
relative gamma = (D + 2) 2^-24 of the exact value, d = sqrt(d^2) within 0.5 gamma (+ second order: 0.51 gamma)."""
import io
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import _play_styles_ref as ref
from _get_styles_program import _child, program  # noqa: F401  (the fabricated IAM directory + checkpoint fixture of the get_styles.py test)
from _writer_id_cases import gaussian_case, quarter_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_STYLES = os.path.join(ROOT, "tests", "golden", "writer_id", "styles.pkl")
GOLD = os.path.join(ROOT, "tests", "golden", "play_styles", "expected.json")

# the kernel's tiles (csrc/style_pairs.hip: SP_BR rows per workgroup, SP_BC columns per column block, SP_DK depth per tile; SP_GROUP columns
# per first-level group of the segmented sums)
BR, BC, DK, GROUP = 16, 256, 32, 8
EDGE_SHAPES = [(BR - 1, DK - 1), (BR, DK), (BR + 1, DK + 1),              # one workgroup, one column block: row-block and depth-tile edges
               (BC - 1, 2 * DK - 1), (BC, 2 * DK), (BC + 1, 2 * DK + 1),  # the column-block edge
               (2 * BC + 1, 3)]                                           # three column blocks, the last one with a single column
SHAPES = [(1, 1), (2, 3), (21, 5), (61, 37), (300, 128)] + EDGE_SHAPES
LAYOUTS = ["one", "distinct", "grouped", "shuffled"]
U = 2.0 ** -52


def writer_layout(n, layout, seed=0):
    """-> int32 [n] writer labels 0 .. A-1, every label used. one: a single writer; distinct: n writers; grouped: runs of one writer each
    - single-line writers, one writer longer than a row block and one longer than a column block where n has room for them, the rest 1 .. 12
    lines, in random order, so that runs start anywhere in a row block and writers straddle row and column blocks; shuffled: the rows of
    `grouped` in random order (the same multiset of pairs per cell)"""
    rs = np.random.RandomState(77 * n + seed)
    if layout == "one":
        return np.zeros(n, dtype=np.int32)
    if layout == "distinct":
        return np.arange(n, dtype=np.int32)
    picked, left = [], n
    for s in (BC + 5, BR + 3, 1, 1):
        if s <= left:
            picked.append(s)
            left -= s
    while left > 0:
        s = min(int(rs.randint(1, 13)), left)
        picked.append(s)
        left -= s
    picked = [picked[i] for i in rs.permutation(len(picked))]
    ids = np.repeat(np.arange(len(picked), dtype=np.int32), picked)
    return ids[rs.permutation(n)] if layout == "shuffled" else ids


def _run(styles, ids, mode, cuda, edge2=None, out=None, workspace=None):
    """rows sorted by writer label (stable), as evaluate.style_distances hands them over -> numpy (count, sum, sumsq, d2_range, hist)"""
    from handwriting_line_generation_amd import ops
    order = np.argsort(ids, kind="stable")
    got = ops.style_pair_stats(torch.from_numpy(np.ascontiguousarray(styles[order])).to(cuda), torch.from_numpy(np.ascontiguousarray(ids[order])).to(cuda),
                               mode, edge2=edge2, out=out, workspace=workspace)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in got)


_want = {}


def _reference(n, d, layout):
    """computed once per case, shared by the tests that need it, never changed"""
    key = (n, d, layout)
    if key not in _want:
        styles, _ = quarter_case(n, d, "equal")
        ids = writer_layout(n, layout)
        st = ref.stats(styles, ids)
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[key] = (styles, ids, st)
    return _want[key]


def _close_sums(got, want, n, what):
    got, want, n = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, want, n))
    err = np.abs(got - want)
    bad = np.flatnonzero(err > n * U * np.abs(want))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], n[bad[:8]])
    return float((err / np.maximum(np.abs(want), 1e-300))[n > 0].max()) if (n > 0).any() else 0.0


def _check_std(count, total, total_sq, d, masks, what):
    """the package's mean / std of the kernel's sums against np.mean / np.std of the restatement's distances, per cell of masks"""
    from handwriting_line_generation_amd import evaluate
    for k, mask in enumerate(masks):
        got, want = evaluate.pair_summary(count[k], total[k], total_sq[k]), ref.summary(d[mask])
        assert got["pairs"] == want["pairs"], (what, k)
        if want["pairs"] == 0:
            assert got["mean"] is None and got["std"] is None
            continue
        n, rms2 = want["pairs"], float(np.mean(d[mask] ** 2))
        assert abs(got["mean"] - want["mean"]) <= n * U * want["mean"], (what, k, got, want)
        bound = n * U * rms2 / want["std"] if want["std"] > 0 else np.sqrt(n * U * rms2)
        assert abs(got["std"] - want["std"]) <= bound, (what, k, got, want, bound)
        if n == 1:
            assert got["std"] == 0.0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_quarter_valued_inputs(cuda, n, d, layout):
    styles, ids, st = _reference(n, d, layout)
    A = int(ids.max()) + 1
    pairs = n * (n - 1) // 2
    n_same = st["cells0"][0][0]
    for mode, bins in ((0, 64), (1, 5), (0, None), (1, None)):
        edge2 = want_hist = None
        if bins is not None and pairs:
            edge2 = ref.edges(st["min_d2"], st["max_d2"], bins)[1]
            want_hist = ref.histogram(st["d2"], st["same"], edge2)
        count, total, total_sq, d2_range, hist = _run(styles, ids, mode, cuda, edge2=edge2)
        assert count.dtype == np.int64 and total.dtype == total_sq.dtype == np.float64 and d2_range.dtype == np.float32
        assert d2_range.tolist() == [float(st["min_d2"]), float(st["max_d2"])], (mode, d2_range, st["min_d2"], st["max_d2"])
        if mode == 0:
            assert count.shape == (2,) and count.tolist() == [c[0] for c in st["cells0"]], (count, st["cells0"])
            _close_sums(total, [c[1] for c in st["cells0"]], count, "sum")
            _close_sums(total_sq, [c[2] for c in st["cells0"]], count, "sumsq")
            _check_std(count, total, total_sq, st["d"], [st["same"], ~st["same"]], (n, d, layout, mode))
        else:
            assert count.shape == (A, A)
            bad = np.argwhere(count != st["count"])
            assert bad.size == 0, (bad[:8], count[tuple(bad[:8].T)], st["count"][tuple(bad[:8].T)])
            _close_sums(total, st["sum"], st["count"], "sum")
            _close_sums(total_sq, st["sumsq"], st["count"], "sumsq")
            assert np.array_equal(total, total.T) and np.array_equal(total_sq, total_sq.T)                  # (b, a) mirrors (a, b), bit for bit
            if layout != "distinct" or n <= 61:
                i, j = np.triu_indices(n, 1)
                lo, hi = np.minimum(ids[i], ids[j]), np.maximum(ids[i], ids[j])
                some = [(0, 0), (0, A - 1), (A // 2, A // 2), (A // 2, A - 1), (A - 1, A - 1)]
                cells = sorted(set(some)) if A > 6 else [(a, b) for a in range(A) for b in range(a, A)]
                _check_std([count[c] for c in cells], [total[c] for c in cells], [total_sq[c] for c in cells], st["d"],
                           [(lo == a) & (hi == b) for a, b in cells], (n, d, layout, mode))
        if edge2 is None:
            assert hist is None
        else:
            assert hist.dtype == np.int64 and hist.shape == (2, bins)
            assert np.array_equal(hist, want_hist), (mode, bins, np.argwhere(hist != want_hist)[:8])
            assert hist[0].sum() == n_same and hist[1].sum() == pairs - n_same                              # every pair is in a bin
    if n == 1:
        from handwriting_line_generation_amd import evaluate
        assert count.tolist() == [[0]] and np.isinf(d2_range).all() and d2_range[0] > 0 > d2_range[1]
        assert evaluate.pair_summary(count[0, 0], total[0, 0], total_sq[0, 0]) == {"pairs": 0, "mean": None, "std": None}


def test_few_bins_and_uneven_edges(cuda):
    """1 and 2 bins (no guess to start from), edges that are not equal-width in d, equal edges, and edges that leave pairs outside"""
    styles, ids, st = _reference(61, 37, "grouped")
    lo, hi = float(st["min_d2"]), float(st["max_d2"])
    mid = np.float32(np.median(st["d2"]))
    for edge2 in ([0.0, np.inf], [0.0, mid, np.inf], [0.0, lo, lo, mid, mid, 0.75 * hi, hi, np.inf], [lo + 1, mid, 0.9 * hi],
                  [0.0, 1.0, 2.0, 3.0, mid, np.inf], sorted(set(st["d2"].tolist()))[:200] + [np.inf]):
        edge2 = np.sort(np.array(edge2, dtype=np.float32))
        for mode in (0, 1):
            hist = _run(styles, ids, mode, cuda, edge2=edge2)[4]
            assert np.array_equal(hist, ref.histogram(st["d2"], st["same"], edge2)), (edge2[:8], mode)


REAL_CASES = {(96, 40): 0, (257, 129): 28}       # shape -> seed of test_writer_id_gpu.py's cases
BAND_CAP = 1e-3                                   # pairs within gamma of an inner edge, summed over the edges, as a share of all pairs


@pytest.mark.parametrize("n,d", sorted(REAL_CASES))
def test_real_valued_inputs_against_fp64(cuda, n, d):
    styles, ids = gaussian_case(n, d, REAL_CASES[(n, d)])
    A = int(ids.max()) + 1
    gamma = (d + 2) * 2.0 ** -24
    st = ref.stats(styles, ids, np.float64, writers=A)
    d64, d2_64, same = st["d"], st["d2"], st["same"]
    pairs = n * (n - 1) // 2
    assert 0 < same.sum() < pairs                                                # both sets
    bins = 64
    for mode in (0, 1):
        count, total, total_sq, d2_range, _ = _run(styles, ids, mode, cuda)
        assert abs(float(d2_range[0]) - d2_64.min()) <= gamma * d2_64.min() and abs(float(d2_range[1]) - d2_64.max()) <= gamma * d2_64.max()
        if mode == 0:
            cells = [(count[k], total[k], total_sq[k], m) for k, m in ((0, same), (1, ~same))]
            assert count.tolist() == [int(same.sum()), int((~same).sum())]
        else:
            assert np.array_equal(count, st["count"])
            i, j = np.triu_indices(n, 1)
            lo, hi = np.minimum(ids[i], ids[j]), np.maximum(ids[i], ids[j])
            cells = [(count[a, b], total[a, b], total_sq[a, b], (lo == a) & (hi == b)) for a in range(A) for b in range(a, A) if count[a, b] >= 2]
        from handwriting_line_generation_amd import evaluate
        worst_mean = worst_std = 0.0
        for c, s, q, mask in cells:
            got, want = evaluate.pair_summary(c, s, q), ref.summary(d64[mask])
            k, rms2 = want["pairs"], float(np.mean(d64[mask] ** 2))
            assert got["pairs"] == k
            mean_err = abs(got["mean"] - want["mean"]) / want["mean"]
            assert mean_err <= 0.51 * gamma + k * U, (mode, got, want)
            worst_mean = max(worst_mean, mean_err / (0.51 * gamma + k * U))
            if want["std"] > 0:
                bound = 0.51 * gamma * np.sqrt(rms2) + k * U * rms2 / want["std"]
                assert abs(got["std"] - want["std"]) <= bound, (mode, got, want, bound)
                worst_std = max(worst_std, abs(got["std"] - want["std"]) / bound)
        print("N=%d D=%d mode=%d: %d cells, worst mean error %.3g of its bound, worst std error %.3g of its bound (gamma %.3g)" % (
            n, d, mode, len(cells), worst_mean, worst_std, gamma))
        # the histogram between the extremes the kernel found
        edges, edge2 = ref.edges(d2_range[0], d2_range[1], bins)
        inner = edge2[1:-1].astype(np.float64)
        in_band = sum(int(((d2_64 >= e / (1 + gamma)) & (d2_64 < e / (1 - gamma))).sum()) for e in inner)
        assert in_band <= BAND_CAP * pairs, "seed %d leaves %d of %d pairs within gamma of an edge" % (REAL_CASES[(n, d)], in_band, pairs)
        hist = _run(styles, ids, mode, cuda, edge2=edge2)[4]
        assert hist[0].sum() == same.sum() and hist[1].sum() == (~same).sum()
        moved = 0
        for row, mask in ((0, same), (1, ~same)):
            cum = np.cumsum(hist[row])[:-1]
            low = np.array([int((d2_64[mask] < e / (1 + gamma)).sum()) for e in inner])
            high = np.array([int((d2_64[mask] < e / (1 - gamma)).sum()) for e in inner])
            assert (low <= cum).all() and (cum <= high).all(), (mode, row, np.flatnonzero((cum < low) | (cum > high))[:8])
            moved += int(np.abs(cum - np.array([int((d2_64[mask] < e).sum()) for e in inner])).sum())
        print("N=%d D=%d mode=%d: %d of %d pairs within gamma of one of %d inner edges; cumulative counts differ from fp64's by %d in all" % (
            n, d, mode, in_band, pairs, len(inner), moved))


def test_repeat_runs_poisoned_buffers_and_mode_agreement(cuda):
    from handwriting_line_generation_amd import _lib as L
    styles, ids = gaussian_case(257, 129, 3)
    n, A = 257, int(ids.max()) + 1
    edge2 = ref.edges(1.0, 700.0, 33)[1]
    clean = {}
    for mode in (0, 1):
        a = _run(styles, ids, mode, cuda, edge2=edge2)
        b = _run(styles, ids, mode, cuda, edge2=edge2)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), mode                                  # two runs: the same bits
        clean[mode] = a
        # outputs and workspace pre-filled with NaN and with 0x7f bytes: every entry is written, nothing stale is read
        cells = (2,) if mode == 0 else (A, A)
        need = L.query("hwg_style_pair_stats_workspace", n, A, mode)
        for fill in ("nan", 0x7F):
            out = [torch.empty(cells, dtype=torch.int64, device=cuda), torch.empty(cells, dtype=torch.float64, device=cuda),
                   torch.empty(cells, dtype=torch.float64, device=cuda), torch.empty((2,), dtype=torch.float32, device=cuda),
                   torch.empty((2, 33), dtype=torch.int64, device=cuda)]
            ws = torch.empty((need + 64,), dtype=torch.uint8, device=cuda)
            for t in out + [ws]:
                if fill == "nan" and t.dtype.is_floating_point:
                    t.fill_(float("nan"))
                elif fill == "nan":
                    t.view(torch.uint8).fill_(0xFF)                                                          # (as fp64: NaN)
                else:
                    t.view(torch.uint8).fill_(fill)
            got = _run(styles, ids, mode, cuda, edge2=edge2, out=out, workspace=ws)
            for x, y in zip(got, a):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (mode, fill)
            assert (ws[need:].cpu().numpy() == (0xFF if fill == "nan" else fill)).all()                      # nothing written past the stated size
    # mode 1 folded over a <= b is mode 0: counts and histogram equal, sums within the bound for fp64 sums of n terms in two orders
    c0, s0, q0, r0, h0 = clean[0]
    c1, s1, q1, r1, h1 = clean[1]
    assert np.array_equal(r0.view(np.int32), r1.view(np.int32)) and np.array_equal(h0, h1)
    upper = np.triu(np.ones((A, A), dtype=bool), 1)
    for k, mask in ((0, np.eye(A, dtype=bool)), (1, upper)):
        assert int(c1[mask].sum()) == int(c0[k])
        for m1, m0 in ((s1, s0), (q1, q0)):
            folded = float(np.sum(m1[mask].astype(np.longdouble)))
            assert abs(folded - m0[k]) <= int(c0[k]) * U * m0[k], (k, folded, m0[k])        # each within (n - 1) 2^-53 of the exact sum


def _golden():
    with open(GOLD_STYLES, "rb") as f:
        data = pickle.load(f)
    return data, json.load(open(GOLD))


def _play(args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "play_styles.py")] + args, cwd=cwd, timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def test_golden_through_evaluate_and_the_program(cuda, tmp_path):
    from PIL import Image
    from handwriting_line_generation_amd import evaluate
    data, want = _golden()
    got = evaluate.style_distances(data["styles"], data["authors"], cuda)
    writers = len(set(data["authors"].tolist()))
    assert (got["lines"], got["dim"], got["writers"]) == (61, 37, writers) and "dropped" not in got
    for key in ("same", "different"):
        assert got[key]["pairs"] == want[key]["pairs"]
        for k in ("mean", "std"):
            assert abs(got[key][k] - want[key][k]) <= 1e-12 * want[key][k], (key, k, got[key][k], want[key][k])
    st = ref.stats(data["styles"][:, :, 0, 0], ref.ids_of(data["authors"]))
    assert np.array_equal(got["pair_count"], st["count"]) and got["writer_names"] == list(dict.fromkeys(data["authors"].tolist()))
    edges, edge2 = evaluate.pair_edges(st["min_d2"], st["max_d2"], 64)
    assert got["hist"]["edges"] == edges.tolist()
    assert [got["hist"]["same"], got["hist"]["different"]] == ref.histogram(st["d2"], st["same"], edge2).tolist()
    flat = evaluate.style_distances(data["styles"], data["authors"], cuda, matrices=False)
    assert flat["hist"] == got["hist"] and set(flat) == {"lines", "dim", "writers", "same", "different", "hist"}
    for key in ("same", "different"):
        for k in ("mean", "std"):
            assert abs(flat[key][k] - want[key][k]) <= 1e-12 * want[key][k]
    # the program: the reference's two lines (parsed: the fp64 sums are taken in another order than numpy's), then the plain ones
    prefix = str(tmp_path / "golden")
    out_json = str(tmp_path / "d.json")
    lines = _play([os.path.join(os.path.dirname(GOLD_STYLES), "styles"), "-g", "0", "-o", prefix, "--json", out_json], str(tmp_path))
    assert lines[0] == "styles: (61, 37)"
    for line, label, key in ((lines[1], "inter", "same"), (lines[2], "intra", "different")):
        head, mean, std = line.replace(", stddev: ", " ").rsplit(" ", 2)
        assert head == "%s dist mean:" % label and line.startswith(want["lines"][0 if key == "same" else 1][:20])
        assert abs(float(mean) - want[key]["mean"]) <= 1e-12 * want[key]["mean"] and abs(float(std) - want[key]["std"]) <= 1e-12 * want[key]["std"]
    assert lines[3] == "same writer: pairs 188, mean %s, std %s" % (got["same"]["mean"], got["same"]["std"])
    assert lines[4] == "different writers: pairs 1642, mean %s, std %s" % (got["different"]["mean"], got["different"]["std"])
    saved = json.load(open(out_json))
    assert saved == json.loads(json.dumps({k: got[k] for k in ("lines", "dim", "writers", "same", "different", "hist")}))
    z = np.load(prefix + ".npz")
    assert int(np.triu(z["pair_count"]).sum()) == 1830 and z["pair_count"].shape == (writers, writers)
    assert np.array_equal(z["pair_mean"], got["pair_mean"], equal_nan=True) and np.array_equal(z["pair_std"], got["pair_std"], equal_nan=True)
    assert int(z["same_pairs"]) == 188 and float(z["same_mean"]) == got["same"]["mean"] and z["hist_same"].tolist() == got["hist"]["same"]
    assert z["writer_names"].tolist() == [str(a) for a in got["writer_names"]] and not bool(z["dedupe"])
    side = writers * max(1, min(16, 1024 // writers))
    assert Image.open(prefix + "_mean.png").size == Image.open(prefix + "_std.png").size == (side, side)
    assert Image.open(prefix + "_hist.png").size == (640, 400)
    solo = got["writer_names"].index("solo") * (side // writers)
    assert Image.open(prefix + "_mean.png").convert("RGB").getpixel((solo, solo)) == (128, 128, 128)        # a single-line writer: no pair, grey
    # --dedupe drops the two repeated rows
    lines = _play([GOLD_STYLES, "--dedupe", "--bins", "16"], str(tmp_path))
    assert lines[1] == "dropped 2 repeated lines, 59 left"
    dd = evaluate.style_distances(data["styles"], data["authors"], cuda, dedupe=True, matrices=False, bins=16)    # what the program ran
    assert dd["dropped"] == 2 and dd["lines"] == 59 and len(dd["hist"]["same"]) == 16
    assert lines[4] == "same writer: pairs %d, mean %s, std %s" % (dd["same"]["pairs"], dd["same"]["mean"], dd["same"]["std"])
    assert dd["same"]["pairs"] + dd["different"]["pairs"] == 59 * 58 // 2
    # one line: no pair
    one = evaluate.style_distances(data["styles"][:1], data["authors"][:1], cuda)
    assert one["same"] == one["different"] == {"pairs": 0, "mean": None, "std": None} and one["hist"]["edges"] == []


def test_get_styles_distances(cuda, program):  # noqa: F811
    from handwriting_line_generation_amd import evaluate
    out = str(program["dir"] / "out_distances")
    stdout = _child(["-c", program["ckpt"], "-f", program["cfg"], "-d", out, "-g", "0", "-T", "--distances"], str(program["dir"]))
    it = program["iteration"]
    assert sorted(os.listdir(out)) == ["test_distances_%s.json" % it, "test_styles_%s.pkl" % it], stdout[-2000:]
    with open(os.path.join(out, "test_styles_%s.pkl" % it), "rb") as f:
        data = pickle.load(f)
    got = json.load(open(os.path.join(out, "test_distances_%s.json" % it)))
    assert got["lines"] + got["dropped"] == len(data["authors"]) and got["lines"] >= 1
    assert got == json.loads(json.dumps(evaluate.style_distances(data["styles"], data["authors"], cuda, dedupe=True, matrices=False)))
    assert set(got) == {"lines", "dim", "writers", "dropped", "same", "different", "hist"}
