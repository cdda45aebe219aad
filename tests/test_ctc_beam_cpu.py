"""CPU: the host side of the CTC prefix beam search - string_utils.prefix_beam_decode against known answers and against the dictionary-loop
restatement of tests/_ctc_beam_ref.py, the shortest-CTC-path encoding the kernel hands to the greedy collapse, the argument checks of
hwg_ctc_beam_error_rates in front of its launches, and get_styles.py's --beam handling. No device is touched."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _ctc_beam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf

HAND_CASES = ref.HAND_CASES


def _probability_by_enumeration(p, text):
    """the sum over every alignment of T frames that collapses to `text` (the definition the beam search approximates from below)"""
    p = np.asarray(p, dtype=np.float64)
    T, C = p.shape
    total = 0.0
    for code in range(C ** T):
        path = [(code // C ** t) % C for t in range(T)]
        collapsed = [c for i, c in enumerate(path) if c != 0 and not (i > 0 and c == path[i - 1])]
        if collapsed == list(text):
            total += float(np.prod([p[t, c] for t, c in enumerate(path)]))
    return total


@pytest.mark.parametrize("case", range(len(HAND_CASES)))
def test_known_answers_by_hand(case):
    from handwriting_line_generation_amd.utils import string_utils as su
    p, beam, text, prob, greedy = HAND_CASES[case]
    lp = np.log(np.array(p))
    assert abs(_probability_by_enumeration(p, text) - prob) < 1e-12                # the hand-computed sum is the enumeration's
    ids, score, totals = su.prefix_beam_decode(lp, beam)
    assert ids == text and abs(score - math.log(prob)) < 1e-12, (ids, score, math.log(prob))
    assert totals.shape == (beam,) and totals[0] == score and (np.diff(totals[np.isfinite(totals)]) <= 0).all()
    assert [int(c) for c in su.naive_decode(lp)[0]] == greedy
    r = ref.search(lp, beam)
    assert list(r["text"]) == text and abs(float(r["score"]) - math.log(prob)) < 1e-12
    # a beam wide enough for every text of these sizes: each total is that text's exact probability, and they sum to 1
    wide = ref.search(lp, 16)
    assert abs(np.exp(wide["totals"][np.isfinite(wide["totals"])]).sum() - 1.0) < 1e-12


def test_degenerate_rows():
    from handwriting_line_generation_amd.utils import string_utils as su
    lp = np.full((4, 3), NINF)
    ids, score, totals = su.prefix_beam_decode(lp, 3)                              # nothing has an alignment: the empty beam
    assert ids == [] and score == NINF and (totals == NINF).all()
    path = [2, 2, 0, 1, 1, 2]
    lp = np.full((6, 3), NINF)
    lp[np.arange(6), path] = 0.0
    ids, score, totals = su.prefix_beam_decode(lp, 3)                              # one path of probability 1
    assert ids == [2, 1, 2] and score == 0.0 and totals.tolist() == [0.0, NINF, NINF]
    nan = np.log(np.array(HAND_CASES[0][0]))
    nan = np.concatenate([nan, np.full((2, 1), np.nan)], axis=1)                   # a NaN class is a class of probability 0
    ids, score, _ = su.prefix_beam_decode(nan, 4)
    assert ids == [1] and abs(score - math.log(0.64)) < 1e-12
    ids, score, totals = su.prefix_beam_decode(np.array([[0.0, NINF]] * 3), 2)      # all blank
    assert ids == [] and score == 0.0 and totals.tolist() == [0.0, NINF]


@pytest.mark.parametrize("shape", [(17, 3, 2, 1), (24, 6, 4, 1), (24, 6, 4, 3), (40, 12, 8, 3), (20, 30, 32, 4), (12, 5, 1, 2)])
def test_prefix_beam_decode_is_the_restatement(shape):
    from handwriting_line_generation_amd.utils import string_utils as su
    T, C, K, sigma = shape
    for seed in range(3):
        lp = ref.log_softmax_rows(T, C, sigma, seed)
        want = ref.search(lp, K)
        ids, score, totals = su.prefix_beam_decode(lp, K)
        assert tuple(ids) == want["text"] and score == float(want["score"])
        assert np.array_equal(totals, want["totals"])                              # fp64 on both sides, the same sums: the same bits
        assert want["gap"] > 0


def test_the_restatement_counts_re_entries():
    """the statistics the GPU tests select their trap cases by: a prefix that left the beam and came back while its extension stayed"""
    r = ref.search(ref.log_softmax_rows(20, 3, 1.0, 1), 2)
    assert r["reentries"] >= r["trap"] >= 1
    assert ref.search(np.log(np.array(HAND_CASES[0][0])), 4)["reentries"] == 0


@pytest.mark.parametrize("text,T", [([1, 1, 2], 5), ([1, 1, 1], 5), ([], 4), ([3], 1), ([1, 2, 1, 2], 4), ([2, 2], 3)])
def test_shortest_ctc_path_round_trips_through_the_greedy_decode(text, T):
    from handwriting_line_generation_amd.utils import string_utils as su
    path = su.shortest_ctc_path(text, T)
    assert path == ref.shortest_path(text, T) and len(path) == T
    doubles = sum(a == b for a, b in zip(text, text[1:]))
    assert path[:len(text) + doubles].count(0) == doubles and not any(path[len(text) + doubles:])
    onehot = np.full((T, 4), -5.0)
    onehot[np.arange(T), path] = 0.0
    assert [int(c) for c in su.naive_decode(onehot)[0]] == text


def test_shortest_ctc_path_that_does_not_fit():
    from handwriting_line_generation_amd.utils import string_utils as su
    with pytest.raises(ValueError):
        su.shortest_ctc_path([1, 1, 1], 4)
    assert ref.shortest_path([1, 1, 1], 4) is None


def test_ctc_beam_entry_point_refuses_bad_arguments_before_any_launch():
    """with arguments they refuse, both entries return their status without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20

    def args(pred=p, T=40, B=6, C=80, beam=16, table=p, codes=p, offsets=p, longest=19, out=p, scores=p, ws=p, ws_bytes=None):
        need = L.query("hwg_ctc_beam_workspace", T, B, C, beam)
        return (pred, T, B, C, beam, table, codes, offsets, longest, out, scores, ws, need if ws_bytes is None else ws_bytes, 0)
    need = L.query("hwg_ctc_beam_workspace", 40, 6, 80, 16)
    assert need > 0 and need % 8 == 0 and L.query("hwg_ctc_beam_workspace", 40, 12, 80, 16) == 2 * need
    for bad in ((0, 6, 80, 16), (40, 0, 80, 16), (40, 6, 1, 16), (40, 6, 80, 0), (40, 6, 80, 33), (2049, 6, 80, 16), (40, 6, 1025, 16)):
        assert L.query("hwg_ctc_beam_workspace", *bad) == 0
    for a, word in [(args(pred=None), "null"), (args(table=None), "null"), (args(codes=None), "null"), (args(offsets=None), "null"),
                    (args(out=None), "null"), (args(scores=None), "null"), (args(T=0), "bad sizes"), (args(B=0), "bad sizes"),
                    (args(C=1), "bad sizes"), (args(longest=-1), "bad sizes"), (args(beam=0), "limit"), (args(beam=33), "limit"),
                    (args(beam=-1), "limit"), (args(T=2049), "limit"), (args(C=1025), "limit"), (args(longest=2048), "limit"),
                    (args(pred=p + 2), "aligned"), (args(out=p + 1), "aligned"), (args(scores=p + 3), "aligned"), (args(ws=p + 4), "aligned")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_ctc_beam_error_rates", *a)
        assert word in str(e.value) and "(-1)" in str(e.value), (a, str(e.value))
    for a in (args(ws=None), args(ws_bytes=need - 1), args(ws_bytes=0)):
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_ctc_beam_error_rates", *a)
        assert "workspace" in str(e.value) and "(-3)" in str(e.value), (a, str(e.value))


def test_get_styles_refuses_beam_without_cer(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "get_styles.py"), "-c", str(tmp_path / "none.pth"), "-d", str(tmp_path / "out"),
                        "--beam", "4"], cwd=str(tmp_path), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0 and "--beam" in r.stdout and "--cer" in r.stdout, r.stdout[-2000:]
    assert os.listdir(str(tmp_path)) == []                   # nothing was created
    import get_styles as cli
    a = cli.parse_args(["-c", "x.pth", "-d", "o", "--cer", "--beam", "4"])
    assert (a.cer, a.beam) == (True, 4) and cli.parse_args(["-c", "x.pth", "-d", "o", "--cer"]).beam == 0
    with pytest.raises(SystemExit):
        cli.main(["-c", "x.pth", "-d", str(tmp_path / "out"), "--cer", "--beam", "-2"])
    assert os.listdir(str(tmp_path)) == []


def test_new_eval_beam_key(capsys):
    """-a beam=K: an integer width in the config and a header line; without the key neither; a width that is none is refused"""
    import new_eval

    def cfg():
        return {"trainer": {}, "model": {}, "data_loader": {"char_file": __file__, "batch_size": 2}, "optimizer_type": "Adam"}
    got = new_eval.prepare_config(cfg(), new_eval.parse_args(["-c", "x", "-a", "beam=8,by_author"]))
    assert got["beam"] == 8 and "prefix beam search, beam 8" in capsys.readouterr().out
    got = new_eval.prepare_config(cfg(), new_eval.parse_args(["-c", "x"]))
    assert "beam" not in got and "beam" not in capsys.readouterr().out
    for bad in ("beam=0", "beam=-3", "beam=wide", "beam=2.5", "beam"):
        with pytest.raises(SystemExit) as e:
            new_eval.prepare_config(cfg(), new_eval.parse_args(["-c", "x", "-a", bad]))
        assert "beam" in str(e.value)
