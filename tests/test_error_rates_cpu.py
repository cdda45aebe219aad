"""CPU: the host side of the device error rates - what string_utils prepares for and makes of the kernel's integers, the argument checks of
hwg_ctc_error_rates in front of its launches, and get_styles.py's argument handling. No device is touched."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _idx_to_char():
    pkg = os.path.join(ROOT, "handwriting_line_generation_amd", "data", "IAM_char_set.json")
    return {int(k): v for k, v in json.load(open(pkg))["idx_to_char"].items()}


def _host_counts(ref_text, hyp_text, casesensitive):
    """the integers the kernel leaves, computed with string_utils' own Levenshtein: hypothesis normalised as cer does it"""
    from handwriting_line_generation_amd.utils import string_utils as su
    ref = su.normalise_ref(ref_text, casesensitive)
    hyp = " ".join(hyp_text.split())
    if not casesensitive:
        hyp = hyp.lower()
    hyp = [ord(c) for c in hyp]

    def words(codes):
        return [tuple(w) for w in "".join(chr(c) for c in codes).split(" ")] if codes else []
    rw, hw = words(ref), words(hyp)
    return (su._levenshtein(ref, hyp), len(ref), len(hyp)), (su._levenshtein(rw, hw), len(rw), len(hw))


HAND_CASES = [("", "abc def"), ("", ""), (" \t  ", "x"), (" \t ", ""), ("a\tb  c", "a b c"), ("tabs\tand  double   spaces ", " tabs and double spaces"),
              ("naïve café 中文", "naive cafe"), ("Hello World", "hello world"), ("MiXeD Case words", "mixed case Words"),
              ("one two three two", "two one two"), ("same", "same"), ("a", "")]


def test_rates_from_counts_over_the_host_counts_is_cer_and_wer():
    from oracle import cer_kats
    from handwriting_line_generation_amd.utils import string_utils as su
    idx_to_char = _idx_to_char()
    pairs = list(HAND_CASES)
    cases = cer_kats.cases(idx_to_char, len(idx_to_char) + 1)
    assert len(cases) == 6
    for pred, texts, _ in cases:
        for b, text in enumerate(texts):
            ids, _ = su.naive_decode(pred[:, b])
            pairs.append((text, su.label2str_single(ids, idx_to_char, False)))
    for ref_text, hyp_text in pairs:
        for casesensitive in (True, False):
            chars, words = _host_counts(ref_text, hyp_text, casesensitive)
            got_c, got_w = su.rates_from_counts(*chars), su.rates_from_counts(*words)
            want_c, want_w = su.cer(ref_text, hyp_text, casesensitive), su.wer(ref_text, hyp_text, casesensitive)
            assert got_c == want_c and type(got_c) is type(want_c), (ref_text, hyp_text, casesensitive, got_c, want_c)
            assert got_w == want_w and type(got_w) is type(want_w), (ref_text, hyp_text, casesensitive, got_w, want_w)
    assert su.rates_from_counts(3, 0, 7) == 7 and su.rates_from_counts(3, 4, 7) == 0.75


def test_normalise_ref():
    from handwriting_line_generation_amd.utils import string_utils as su
    assert su.normalise_ref("  Ab\t c  ", True) == [ord(c) for c in "Ab c"]
    assert su.normalise_ref("  Ab\t c  ", False) == [ord(c) for c in "ab c"]
    assert su.normalise_ref(" \n ", True) == [] and su.normalise_ref("", False) == []
    assert su.normalise_ref("İx", False) == [ord(c) for c in "İx".lower()]          # the whole string is lower-cased, as cer does


def test_class_code_table():
    import numpy as np
    from handwriting_line_generation_amd.utils import string_utils as su
    idx_to_char = _idx_to_char()
    C = len(idx_to_char) + 1
    t = su.class_code_table(idx_to_char, C, True)
    assert t.dtype == np.int32 and t.shape == (C,)
    assert all(t[c] == ord(ch) for c, ch in idx_to_char.items())
    low = su.class_code_table(idx_to_char, C, False)
    assert all(low[c] == ord(ch.lower()) for c, ch in idx_to_char.items()) and (low != t).any()
    small = {1: "a", 2: "\t", 3: " ", 4: "B"}
    assert su.class_code_table(small, 5, True).tolist() == [0, 97, 32, 32, 66]
    assert su.class_code_table(small, 5, False).tolist() == [0, 97, 32, 32, 98]
    for bad in ("İ", "Σ"):                        # 'İ' lower-cases to two characters, 'Σ' by its place in the word
        assert su.class_code_table({1: "a", 2: bad}, 3, False) is None and su.class_code_table({1: "a", 2: bad}, 3, True) is None
    assert su.class_code_table({1: "a", 2: "σ", 3: "é"}, 4, False).tolist() == [0, 97, ord("σ"), ord("é")]
    assert su.class_code_table({1: "a", 2: "bc"}, 3, True) is None and su.class_code_table({1: "a"}, 3, True) is None


def test_ctc_error_rates_entry_point_refuses_bad_arguments_before_any_launch():
    """the argument checks of hwg_ctc_error_rates run on the host side of the entry point, in front of both launches: with arguments they
    refuse, the call returns its status without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20

    def args(pred=p, T=40, B=6, C=80, table=p, codes=p, offsets=p, longest=19, out=p):
        return (pred, T, B, C, table, codes, offsets, longest, out, 0)
    for a, word in [(args(pred=None), "null"), (args(table=None), "null"), (args(codes=None), "null"), (args(offsets=None), "null"),
                    (args(out=None), "null"), (args(T=0), "bad sizes"), (args(B=0), "bad sizes"), (args(C=1), "bad sizes"),
                    (args(T=-3), "bad sizes"), (args(longest=-1), "bad sizes"), (args(T=8193), "limit"), (args(C=1025), "limit"),
                    (args(longest=2048), "limit"), (args(pred=p + 2), "aligned"), (args(out=p + 1), "aligned")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_ctc_error_rates", *a)
        assert word in str(e.value), (a, str(e.value))


def _get_styles(args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "get_styles.py")] + args, cwd=cwd, timeout=120, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)


def test_get_styles_arguments(tmp_path):
    out = tmp_path / "out"
    r = _get_styles(["-d", str(out)], str(tmp_path))
    assert r.returncode != 0 and "must provide a checkpoint" in r.stdout, r.stdout[-2000:]
    r = _get_styles(["-c", str(tmp_path / "none.pth"), "-d", str(out), "-S"], str(tmp_path))
    assert r.returncode != 0 and "-S" in r.stdout and "not built" in r.stdout, r.stdout[-2000:]
    r = _get_styles(["-c", str(tmp_path / "none.pth")], str(tmp_path))
    assert r.returncode != 0 and "-d" in r.stdout, r.stdout[-2000:]
    assert os.listdir(str(tmp_path)) == []                   # nothing was created
    import get_styles as cli
    with pytest.raises(SystemExit):
        cli.main(["-f", str(tmp_path / "cfg.json"), "-d", str(out)])
    a = cli.parse_args(["-c", "x.pth", "-d", "o", "-g", "2", "-b", "8", "-f", "c.json", "-a", "model=style_dim=64", "-T", "--cer"])
    assert (a.checkpoint, a.savedir, a.gpu, a.batchsize, a.config, a.addtoconfig, a.test, a.cer) == ("x.pth", "o", 2, 8, "c.json", "model=style_dim=64", True, True)
    assert os.listdir(str(tmp_path)) == []
