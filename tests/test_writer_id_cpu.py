"""CPU: writer retrieval (evaluate.writer_id, eval_writer_id.py) without a device - the numpy restatement of the definition against numbers
recorded from the unmodified reference script (tests/golden/writer_id, tools/gen_golden_writer_id.py), the argument checks of
hwg_writer_first_rank in front of its launches, the program's argument handling and error exits, and the host-side pieces (dedupe, author ids,
the refusal of non-finite styles)."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import _writer_id_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "writer_id")


def _golden():
    with open(os.path.join(GOLD, "styles.pkl"), "rb") as f:
        data = pickle.load(f)
    return data, json.load(open(os.path.join(GOLD, "expected.json")))


def test_golden_input_holds_what_it_was_made_for():
    data, _ = _golden()
    s4, authors = data["styles"], list(data["authors"])
    assert s4.dtype == np.float32 and s4.ndim == 4 and s4.shape[2:] == (1, 1)
    n, d = s4.shape[:2]
    s = s4[:, :, 0, 0]
    assert 40 <= n <= 80 and d % 4 != 0 and len(authors) == n
    assert np.array_equal(s * 4, np.round(s * 4)) and np.abs(s).max() <= 16           # every distance exact in fp32, in any order
    same = [(s[i] == s[i + 1]).all() for i in range(n - 1)]
    assert any(same[i] and same[i + 1] and authors[i] == authors[i + 1] == authors[i + 2] for i in range(n - 2))     # a run of three
    assert any(same[i] and authors[i] != authors[i + 1] for i in range(n - 1))                                       # a pair across writers
    assert min(authors.count(a) for a in set(authors)) == 1                                                          # a single-line writer


def test_restatement_reproduces_the_reference_numbers():
    """the definition (stable order, own column in the list, places 1..n) gives the six top-n numbers the reference printed, exactly"""
    data, want = _golden()
    s = data["styles"][:, :, 0, 0]
    ids = ref.ids_of(data["authors"])
    for name, metric in (("l1", 0), ("l2", 1)):
        rank, near, _ = ref.first_rank(s, ids, metric)
        got = ref.summary(rank, len(ids))
        for k in ("top1", "top5", "top20"):
            assert got[k] == want[name][k], (name, k, got[k], want[name][k])
        assert got[k] < 1 and got["rows_without_match"] >= 1              # the single-line writer has no match
        assert np.isinf(near[rank == len(ids)]).all() and np.isfinite(near[rank < len(ids)]).all()
    assert want["l1"]["top1"] < want["l1"]["top5"] < want["l1"]["top20"] < 1 and want["l2"]["top1"] < want["l2"]["top5"] < want["l2"]["top20"] < 1
    assert all(want["l1"][k] != want["l2"][k] for k in ("top1", "top5", "top20"))


def test_restatement_by_hand():
    # three points on a line, writers a a b: row 0 sees [0, 1, 3] -> its writer at place 1; row 2 (writer b alone) has none
    s = np.array([[0.0], [1.0], [3.0]], dtype=np.float32)
    rank, near, _ = ref.first_rank(s, [0, 0, 1], 0)
    assert rank.tolist() == [1, 1, 3] and near.tolist() == [1.0, 1.0, np.inf]
    # an exact duplicate with a lower index takes place 0: the row's own column is then a hit at place 1
    s = np.array([[2.0], [2.0], [5.0]], dtype=np.float32)
    rank, near, _ = ref.first_rank(s, [0, 1, 2], 1)
    assert rank.tolist() == [3, 1, 3] and near.tolist() == [np.inf, 0.0, np.inf]
    assert ref.summary(rank, 3) == {"top1": 1 / 3, "top5": 1 / 3, "top20": 1 / 3, "mean_first_rank": 1.0, "rows_without_match": 2}


def test_writer_first_rank_entry_point_refuses_bad_arguments_before_any_launch():
    """the argument checks of hwg_writer_first_rank run on the host side of the entry point, in front of both launches: with arguments they
    refuse, the call returns its status without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20

    def args(styles=p, ids=p, N=61, D=37, metric=0, rank=p, near=p):
        return (styles, ids, N, D, metric, rank, near, 0)
    for a, word in [(args(styles=None), "null"), (args(ids=None), "null"), (args(rank=None), "null"), (args(near=None), "null"),
                    (args(N=0), "bad sizes"), (args(D=0), "bad sizes"), (args(N=-5), "bad sizes"), (args(metric=2), "bad sizes"),
                    (args(metric=-1), "bad sizes"), (args(N=(1 << 20) + 1), "limit"), (args(D=65537), "limit"),
                    (args(styles=p + 4), "aligned"), (args(styles=p + 8), "aligned"), (args(ids=p + 2), "aligned"),
                    (args(rank=p + 1), "aligned"), (args(near=p + 2), "aligned")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_writer_first_rank", *a)
        assert word in str(e.value), (a, str(e.value))


def test_ops_wrapper_refuses_wrong_tensors_without_a_device():
    import torch
    from handwriting_line_generation_amd import _lib as L, ops
    ids = torch.zeros(4, dtype=torch.int32)
    for styles in (torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, 1), np.zeros((4, 3), dtype=np.float32)):
        with pytest.raises(L.HwgError):
            ops.writer_first_rank(styles, ids, 0)


def test_author_ids_with_strings_and_integers():
    from handwriting_line_generation_amd import evaluate
    ids, writers = evaluate.author_ids(["b", "a", "b", "c", "a"])
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1, 0, 2, 1] and writers == 3
    ids, writers = evaluate.author_ids(np.array(["b", "a", "b"]))                 # what get_styles.py pickles
    assert ids.tolist() == [0, 1, 0] and writers == 2
    ids, writers = evaluate.author_ids([7, 3, 7, np.int64(3), 3])
    assert ids.tolist() == [0, 1, 0, 1, 1] and writers == 2
    ids, writers = evaluate.author_ids(["3", 3])                                  # equality as Python sees it, as the reference's ==
    assert ids.tolist() == [0, 1] and writers == 2
    ids, writers = evaluate.author_ids([])
    assert ids.shape == (0,) and writers == 0
    assert ref.ids_of(["b", "a", "b", "c", "a"]).tolist() == [0, 1, 0, 2, 1]


def test_dedupe_rows_on_the_host():
    from handwriting_line_generation_amd import evaluate
    s = np.array([[1, 2], [1, 2], [1, 2], [1, 2], [3, 4], [1, 2], [0.0, 5], [-0.0, 5]], dtype=np.float32)
    ids = np.array([0, 0, 0, 1, 1, 1, 2, 2], dtype=np.int32)
    keep = evaluate.dedupe_rows(s, ids)
    # rows 1, 2 repeat row 0; row 3 has the same bytes but another writer; row 5 repeats row 0 but not the row above; -0.0 is other bytes
    assert keep.tolist() == [True, False, False, True, True, True, True, True]
    assert evaluate.dedupe_rows(s[:1], ids[:1]).tolist() == [True]


def test_writer_id_refuses_bad_input_before_the_device():
    from handwriting_line_generation_amd import evaluate
    s = np.zeros((5, 3), dtype=np.float32)
    s[3, 1] = np.nan
    s[4, 0] = np.inf
    with pytest.raises(ValueError, match="row 3"):
        evaluate.writer_id(s, list("abcde"), None)
    with pytest.raises(ValueError, match="authors"):
        evaluate.writer_id(np.zeros((5, 3), dtype=np.float32), list("abcd"), None)
    with pytest.raises(ValueError, match="styles must be"):
        evaluate.writer_id(np.zeros((5, 3, 2, 1), dtype=np.float32), list("abcde"), None)
    with pytest.raises(ValueError, match="styles must be"):
        evaluate.writer_id(np.zeros((0, 3), dtype=np.float32), [], None)


def _program(args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "eval_writer_id.py")] + args, cwd=cwd, timeout=120, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)


def _dump(path, styles, authors):
    with open(path, "wb") as f:
        pickle.dump({"styles": styles, "authors": authors}, f)


def test_eval_writer_id_arguments_and_error_exits(tmp_path):
    import eval_writer_id as cli
    a = cli.parse_args(["some/prefix_", "-g", "2", "--dedupe", "--json", "o.json"])
    assert (a.style_loc, a.gpu, a.dedupe, a.json) == ("some/prefix_", 2, True, "o.json")
    a = cli.parse_args(["p*"])
    assert (a.style_loc, a.gpu, a.dedupe, a.json) == ("p*", 0, False, None)
    r = _program([], str(tmp_path))
    assert r.returncode != 0 and "style_loc" in r.stdout, r.stdout[-2000:]
    r = _program([str(tmp_path / "none_styles_")], str(tmp_path))
    assert r.returncode != 0 and "no file matches" in r.stdout and "none_styles_*" in r.stdout, r.stdout[-2000:]
    _dump(str(tmp_path / "a_styles_1.pkl"), np.zeros((3, 4), dtype=np.float32), ["x", "y", "x"])
    _dump(str(tmp_path / "a_styles_2.pkl"), np.zeros((0, 4), dtype=np.float32), [])
    r = _program([str(tmp_path / "a_styles_")], str(tmp_path))
    assert r.returncode != 0 and "a_styles_2.pkl" in r.stdout and "no styles" in r.stdout, r.stdout[-2000:]
    _dump(str(tmp_path / "b_styles_1.pkl"), np.zeros((3, 4, 1, 1), dtype=np.float32), ["x", "y", "x"])
    _dump(str(tmp_path / "b_styles_2.pkl"), np.zeros((2, 5), dtype=np.float32), ["x", "y"])
    r = _program([str(tmp_path / "b_styles_*")], str(tmp_path))
    assert r.returncode != 0 and "b_styles_2.pkl" in r.stdout and "style_dim" in r.stdout, r.stdout[-2000:]
    with open(str(tmp_path / "c_styles_1.pkl"), "wb") as f:
        f.write(b"not a pickle")
    r = _program([str(tmp_path / "c_styles_")], str(tmp_path))
    assert r.returncode != 0 and "c_styles_1.pkl" in r.stdout and "Traceback" not in r.stdout, r.stdout[-2000:]


def test_load_styles_concatenates_in_sorted_order(tmp_path):
    import eval_writer_id as cli
    _dump(str(tmp_path / "s_2.pkl"), np.full((2, 3), 2, dtype=np.float32), ["c", "d"])
    _dump(str(tmp_path / "s_10.pkl"), np.full((1, 3, 1, 1), 10, dtype=np.float32), np.array(["a"]))
    _dump(str(tmp_path / "s_1.pkl"), np.full((2, 3), 1, dtype=np.float64), ["b", "b"])
    for loc in (str(tmp_path / "s_"), str(tmp_path / "s_*")):
        styles, authors = cli.load_styles(loc)
        assert styles.dtype == np.float32 and styles.shape == (5, 3)
        assert styles[:, 0].tolist() == [1, 1, 10, 2, 2] and authors == ["b", "b", "a", "c", "d"]       # s_1, s_10, s_2: sorted() of the names


def test_get_styles_has_the_writer_id_flag():
    import get_styles as cli
    assert cli.parse_args(["-c", "x.pth", "-d", "o", "--writer-id"]).writer_id is True
    assert cli.parse_args(["-c", "x.pth", "-d", "o"]).writer_id is False
