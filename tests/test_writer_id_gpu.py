"""GPU: writer retrieval on the device (csrc/writer_id.hip through ops.writer_first_rank, evaluate.writer_id, eval_writer_id.py and
get_styles.py --writer-id) against tests/_writer_id_ref.py, the numpy restatement that tests/test_writer_id_cpu.py pins to the reference's
recorded numbers.

Bit-exact block: every style value is a multiple of 1/4 with |value| <= 16, so a difference is a multiple of 1/4 <= 32, its square a multiple
of 1/16 <= 1024, and a sum over D <= 129 of either stays below 2^24 units of its grid: every distance is exact in fp32 in any summation
order, numpy's and the kernel's alike, and first_rank and nearest_same must be EQUAL to the restatement's.
Real-valued block: against the restatement in fp64. A sequential fp32 sum of D non-negative terms, each rounded once (the difference) or
fused (the square), is within relative gamma = (D + 2) 2^-24 of the exact value; first_rank may differ only where fp64 sees another column
within 2 gamma of the target distance - and the seeds are chosen so that there is no such row, which the test asserts first."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import _writer_id_ref as ref
from _writer_id_cases import gaussian_case, quarter_case
from _get_styles_program import _child, program  # noqa: F401  (the fabricated IAM directory + checkpoint fixture of the get_styles.py test)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "writer_id")

# the kernel's tiles (csrc/writer_id.hip: WID_BR rows per workgroup, WID_BC columns per column block, WID_DK depth per tile)
BR, BC, DK = 16, 256, 32
EDGE_SHAPES = [(BR - 1, DK - 1), (BR, DK), (BR + 1, DK + 1),              # one workgroup, one column block: row-block and depth-tile edges
               (BC - 1, 2 * DK - 1), (BC, 2 * DK), (BC + 1, 2 * DK + 1),  # the column-block edge (and 16 | 255 + 1, 256, 257: row blocks again)
               (2 * BC + 1, 3)]                                           # three column blocks, the last one with a single column
SHAPES = [(1, 1), (2, 3), (21, 5), (61, 37)] + EDGE_SHAPES + [(300, 128)]
VARIANTS = ["equal", "distinct", "duplicated"]


REAL_CASES = {(96, 40): 0, (257, 129): 28}       # shape -> seed at which fp64 finds no near tie at the target (searched on the host)


def _run(styles, ids, metric, cuda, out=None):
    from handwriting_line_generation_amd import ops
    rank, near = ops.writer_first_rank(torch.from_numpy(styles).to(cuda), torch.from_numpy(ids).to(cuda), metric, out=out)
    torch.cuda.synchronize()
    return rank.cpu().numpy(), near.cpu().numpy()


_want = {}


def _reference(n, d, variant, metric):
    """computed once per case, shared by the tests that need it, never changed"""
    key = (n, d, variant, metric)
    if key not in _want:
        styles, ids = quarter_case(n, d, variant)
        rank, near, _ = ref.first_rank(styles, ids, metric)
        rank.setflags(write=False)
        near.setflags(write=False)
        _want[key] = (styles, ids, rank, near)
    return _want[key]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_quarter_valued_inputs_are_bit_exact(cuda, n, d, variant):
    for metric in (0, 1):
        styles, ids, want_rank, want_near = _reference(n, d, variant, metric)
        rank, near = _run(styles, ids, metric, cuda)
        assert rank.dtype == np.int32 and near.dtype == np.float32 and rank.shape == near.shape == (n,)
        bad = np.flatnonzero(rank != want_rank)
        assert bad.size == 0, (metric, bad[:8], rank[bad[:8]], want_rank[bad[:8]])
        assert np.array_equal(near, want_near), (metric, np.flatnonzero(near != want_near)[:8])
        if variant == "distinct":
            # nobody shares a writer: only the row's own column can count, and only behind an exact copy with a lower index
            assert ((rank == n) | (near == 0)).all() and np.array_equal(rank == n, np.isinf(near))
        if variant == "equal" and n > 1:
            assert (rank == 1).all()                                    # everybody does: place 1 is a hit whoever holds it


def test_two_rows_two_writers_and_one_writer(cuda):
    s = np.array([[1.0, -2.0, 0.25], [0.5, 4.0, 0.25]], dtype=np.float32)
    for metric, dist in ((0, 6.5), (1, 36.25)):
        rank, near = _run(s, np.array([0, 1], dtype=np.int32), metric, cuda)
        assert rank.tolist() == [2, 2] and np.isinf(near).all()
        rank, near = _run(s, np.array([5, 5], dtype=np.int32), metric, cuda)
        assert rank.tolist() == [1, 1] and near.tolist() == [dist, dist]
        # identical rows of two writers: row 1's own column sits at place 1 behind its copy and counts
        rank, near = _run(np.stack([s[0], s[0]]), np.array([0, 1], dtype=np.int32), metric, cuda)
        assert rank.tolist() == [2, 1] and near.tolist() == [np.inf, 0.0]


@pytest.mark.parametrize("n,d", sorted(REAL_CASES))
def test_real_valued_inputs_against_fp64(cuda, n, d):
    styles, ids = gaussian_case(n, d, REAL_CASES[(n, d)])
    gamma = (d + 2) * 2.0 ** -24
    for metric in (0, 1):
        want_rank, want_near, margin = ref.first_rank(styles, ids, metric, dtype=np.float64)
        has = want_rank < n
        assert has.sum() > n // 2 and len(set(want_rank[has].tolist())) > 3               # the case is not trivial
        exempt = has & (margin <= 2 * gamma)
        assert not exempt.any(), "seed %d leaves fp64 near ties at rows %s" % (REAL_CASES[(n, d)], np.flatnonzero(exempt))
        rank, near = _run(styles, ids, metric, cuda)
        rel = np.abs(near[has].astype(np.float64) - want_near[has]) / want_near[has]
        print("N=%d D=%d metric=%d: nearest_same max relative error %.3g (bound %.3g), smallest fp64 margin %.3g" % (
            n, d, metric, rel.max(), gamma, margin[has].min()))
        assert np.array_equal(np.isinf(near), ~has)
        assert rel.max() <= gamma, (metric, rel.max(), gamma)
        assert np.array_equal(rank, want_rank), (metric, np.flatnonzero(rank != want_rank)[:8])


def test_repeat_runs_and_poisoned_outputs(cuda):
    styles, ids = gaussian_case(257, 129, 3)
    styles_q, ids_q, want_rank, want_near = _reference(300, 128, "duplicated", 1)
    for metric in (0, 1):
        a = _run(styles, ids, metric, cuda)
        b = _run(styles, ids, metric, cuda)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    # outputs pre-filled with garbage (ranks that look like "no target" and like huge counts, NaN distances): every entry is overwritten
    for fill_rank, fill_near in ((-1, float("nan")), (2 ** 31 - 1, -1.0)):
        out = (torch.full((300,), fill_rank, dtype=torch.int32, device=cuda), torch.full((300,), fill_near, dtype=torch.float32, device=cuda))
        rank, near = _run(styles_q, ids_q, 1, cuda, out=out)
        assert np.array_equal(rank, want_rank) and np.array_equal(near, want_near)


def test_golden_through_evaluate_and_the_program(cuda, tmp_path):
    """the reference's six printed numbers come out of evaluate.writer_id and of eval_writer_id.py, the two top-n lines character for character"""
    from handwriting_line_generation_amd import evaluate
    with open(os.path.join(GOLD, "styles.pkl"), "rb") as f:
        data = pickle.load(f)
    want = json.load(open(os.path.join(GOLD, "expected.json")))
    got = evaluate.writer_id(data["styles"], data["authors"], cuda)
    assert (got["lines"], got["dim"], got["writers"]) == (61, 37, len(set(data["authors"].tolist()))) and "dropped" not in got
    ids = ref.ids_of(data["authors"])
    for name, metric in (("l1", 0), ("l2", 1)):
        for k in ("top1", "top5", "top20"):
            assert got[name][k] == want[name][k], (name, k, got[name][k], want[name][k])
        rank, _, _ = ref.first_rank(data["styles"][:, :, 0, 0], ids, metric)
        assert got[name] == ref.summary(rank, 61)
    # short inputs: the tops are clamped to n - 1 where the reference raises IndexError
    short = evaluate.writer_id(data["styles"][:4], data["authors"][:4], cuda)
    rank, _, _ = ref.first_rank(data["styles"][:4, :, 0, 0], ids[:4], 1)
    assert short["l2"] == ref.summary(rank, 4) and short["lines"] == 4
    # dedupe: the run of three collapses to one row, the pair across writers stays
    dd = evaluate.writer_id(data["styles"], data["authors"], cuda, dedupe=True)
    keep = evaluate.dedupe_rows(data["styles"][:, :, 0, 0], ids)
    assert dd["dropped"] == 2 == int((~keep).sum()) and dd["lines"] == 59
    rank, _, _ = ref.first_rank(data["styles"][keep][:, :, 0, 0], ids[keep], 0)
    assert dd["l1"] == ref.summary(rank, 59)
    # the program
    out_json = str(tmp_path / "scores.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_writer_id.py"), os.path.join(GOLD, "styles"), "-g", "0", "--json", out_json],
                       cwd=str(tmp_path), timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0] == want["shape_line"] == "styles: (61, 37)"
    assert [l for l in lines if "\ttop1:" in l] == want["top_lines"]
    assert lines[1] == "l2 mean first rank: %s (rows without a same-writer line: %d)" % (got["l2"]["mean_first_rank"], got["l2"]["rows_without_match"])
    assert lines[3] == "l1 mean first rank: %s (rows without a same-writer line: %d)" % (got["l1"]["mean_first_rank"], got["l1"]["rows_without_match"])
    assert not any(l.startswith(("l1 rank", "l2 rank")) for l in lines)
    assert json.load(open(out_json)) == got


def test_get_styles_writer_id(cuda, program):  # noqa: F811
    from handwriting_line_generation_amd import evaluate
    out = str(program["dir"] / "out_writer_id")
    stdout = _child(["-c", program["ckpt"], "-f", program["cfg"], "-d", out, "-g", "0", "-T", "--writer-id"], str(program["dir"]))
    it = program["iteration"]
    assert sorted(os.listdir(out)) == ["test_styles_%s.pkl" % it, "test_writer_id_%s.json" % it], stdout[-2000:]
    with open(os.path.join(out, "test_styles_%s.pkl" % it), "rb") as f:
        data = pickle.load(f)
    scores = json.load(open(os.path.join(out, "test_writer_id_%s.json" % it)))
    assert scores["lines"] + scores["dropped"] == len(data["authors"]) and scores["lines"] >= 1
    assert scores == evaluate.writer_id(data["styles"], data["authors"], cuda, dedupe=True)
    assert set(scores["l1"]) == set(scores["l2"]) == {"top1", "top5", "top20", "mean_first_rank", "rows_without_match"}
