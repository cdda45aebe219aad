"""GPU: CER / WER counted on the device (csrc/error_rate.hip through ops.ctc_error_rates) against the host path - string_utils.naive_decode,
cer and wer, which tests/golden/valid_gan.json pins to the unmodified reference -, in the trainer (trainer.device_cer) and in the get_styles.py
program. Every comparison is exact: integers, or floats that must be the same bits."""
import json
import os
import pickle
import random
import string

import numpy as np
import pytest
import torch

from _get_styles_program import _child, program  # noqa: F401  (the fixture is used by name)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
POOL = "a " + "".join(c for c in string.ascii_letters + string.digits + string.punctuation if c != "a")      # class 1 'a', class 2 ' '


def _iam_idx_to_char():
    pkg = os.path.join(ROOT, "handwriting_line_generation_amd", "data", "IAM_char_set.json")
    return {int(k): v for k, v in json.load(open(pkg))["idx_to_char"].items()}


def _char_set(C):
    return {c: POOL[c - 1] for c in range(1, C)}


def _host_counts(pred, gt, idx_to_char, casesensitive):
    """per line, with string_utils' own decode and Levenshtein: ([decoded length, character distance, hypothesis characters, word distance,
    hypothesis words], decoded ids)"""
    from handwriting_line_generation_amd.utils import string_utils as su
    rows, ids_all = [], []
    for b, text in enumerate(gt):
        ids, _ = su.naive_decode(pred[:, b])
        hyp = " ".join(su.label2str_single(ids, idx_to_char, False).split())
        ref = " ".join(text.split())
        if not casesensitive:
            hyp, ref = hyp.lower(), ref.lower()
        rows.append([len(ids), su._levenshtein(ref, hyp), len(hyp), su._levenshtein(ref.split(), hyp.split()), len(hyp.split())])
        ids_all.append([int(i) for i in ids])
    return rows, ids_all


def _check(pred, gt, idx_to_char, casesensitive, cuda):
    """device == host on one batch: the integers, the decoded ids, the rates (same bits and types) and the strings; never the fallback"""
    from handwriting_line_generation_amd import ops
    before = ops.error_rate_fallbacks
    handle = ops.ctc_error_rates(torch.from_numpy(pred).to(cuda), gt, idx_to_char, casesensitive)
    assert ops.error_rate_fallbacks == before and handle.counts() is not None, "the host fallback was taken"
    stats, decoded = handle.counts()
    want, ids = _host_counts(pred, gt, idx_to_char, casesensitive)
    T = pred.shape[0]
    for b in range(len(gt)):
        assert stats[b].tolist() == want[b] + [0, 0, 0], (b, gt[b][:40], stats[b].tolist(), want[b])
        assert decoded[b].tolist() == ids[b] + [0] * (T - len(ids[b])), b
    cers, wers, strs = handle.result()
    h_cers, h_wers, h_strs = ops.host_error_rates(pred, gt, idx_to_char, casesensitive)
    assert strs == h_strs
    assert cers == h_cers and wers == h_wers and [type(v) for v in cers + wers] == [type(v) for v in h_cers + h_wers]
    return stats


def _pred_from_raw(raw, C, seed):
    """scores [T,B,C] whose arg-max path is raw [T,B]"""
    raw = np.asarray(raw)
    pred = np.random.RandomState(seed).randn(raw.shape[0], raw.shape[1], C).astype(np.float32)
    t, b = np.meshgrid(np.arange(raw.shape[0]), np.arange(raw.shape[1]), indexing="ij")
    pred[t, b, raw] += 12.0
    assert (pred.argmax(2) == raw).all()
    return pred


def _raw_from_text(text, T, char_to_idx, drop=None, swap=None, C=None):
    """the text written into T steps, a blank between two characters; `drop`: leave out every drop-th character, `swap`: replace every swap-th"""
    raw, t = np.zeros(T, dtype=np.int64), 0
    for j, ch in enumerate(text):
        if t >= T or ch not in char_to_idx or (drop and j % drop == 2):
            continue
        ci = char_to_idx[ch]
        if swap and j % swap == 1:
            ci = ci % (C - 1) + 1
        raw[t] = ci
        t += 2
    return raw


def test_reference_known_answers_on_the_device(cuda):
    """oracle/cer_kats.py's six cases: the strings are the unmodified reference's (tests/golden/valid_gan.json), cer and wer are getCER's"""
    from oracle import cer_kats
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.trainer.hw_with_style_trainer import HWWithStyleTrainer
    gold = json.load(open(os.path.join(GOLD, "valid_gan.json")))["cer_kats"]
    idx_to_char = _iam_idx_to_char()
    cases = cer_kats.cases(idx_to_char, len(idx_to_char) + 1)
    assert len(cases) == len(gold) == 6
    stub = type("T", (), {"idx_to_char": idx_to_char, "casesensitive": True})()
    for (pred, texts, casesens), ref in zip(cases, gold):
        _check(pred, texts, idx_to_char, casesens, cuda)
        cers, wers, strs = ops.ctc_error_rates(torch.from_numpy(pred).to(cuda), texts, idx_to_char, casesens).result()
        assert strs == ref["strs"]
        stub.casesensitive = casesens
        cer, wer, _ = HWWithStyleTrainer.getCER(stub, texts, pred)
        assert HWWithStyleTrainer._mean_rates(ops.ctc_error_rates(torch.from_numpy(pred).to(cuda), texts, idx_to_char, casesens)) == (cer, wer)
        assert abs(cer - ref["cer"]) < 1e-12 and abs(wer - ref["wer"]) < 1e-12
    assert any(r["cer"] > 0 for r in gold)


@pytest.mark.parametrize("C", [2, 3, 80, 81])
def test_small_shapes(cuda, C):
    """T in {1, 2, 65}, B in {1, 3}, C on both sides of the 16-byte load rule (C % 4) and of one pass over a row (64 classes), random
    arg-max paths with many blanks, repeats and spaces"""
    idx_to_char = _char_set(C)
    rs = np.random.RandomState(C)
    for T in (1, 2, 65):
        for B in (1, 3):
            weights = np.ones(C)
            weights[0] = max(C // 3, 1)                         # blanks
            if C > 2:
                weights[2] = max(C // 6, 1)                     # spaces
            raw = rs.choice(C, size=(T, B), p=weights / weights.sum())
            raw[1:] = np.where(rs.rand(T - 1, B) < 0.25, raw[:-1], raw[1:])        # repeats
            gt = ["".join(idx_to_char[c] for c in rs.choice(np.arange(1, C), size=rs.randint(0, T + 3))) for _ in range(B)]
            for casesens in (True, False):
                _check(_pred_from_raw(raw, C, seed=T * 10 + B), gt, idx_to_char, casesens, cuda)


def test_reference_lengths_and_hypothesis_lengths(cuda):
    """reference lengths on both sides of every columns-per-lane step (64, 128) and the longest allowed (2047), against hypotheses that are
    shorter, longer and (corrupted) copies; characters outside the set in the reference; T = 200: more than one 64-wide pass of each
    in-place compaction"""
    C = 80
    idx_to_char = _char_set(C)
    char_to_idx = {v: k for k, v in idx_to_char.items()}
    rnd = random.Random(4)
    words = ["".join(rnd.choice(POOL[2:40]) for _ in range(rnd.randint(1, 7))) for _ in range(30)]

    def text(n):
        s = ""
        while len(s) < n:
            s += rnd.choice(words) + " "
        s = s[:n]
        return s[:-1] + "x" if s.endswith(" ") else s
    lengths = [0, 1, 63, 64, 65, 128, 129, 2047]
    gt = [text(n) for n in lengths]
    assert [len(" ".join(g.split())) for g in gt] == lengths
    gt += ["café naïve 中文 " + text(20), "MiXeD " + text(30).upper()]
    for T in (65, 200):
        raws = []
        for b, g in enumerate(gt):
            source = g if b % 2 == 0 else text(40) + " " + g               # even lines: the reference's start; odd: other words first
            raws.append(_raw_from_text(source, T, char_to_idx, drop=5 if b % 3 == 0 else None, swap=4 if b % 3 == 1 else None, C=C))
        pred = _pred_from_raw(np.stack(raws, axis=1), C, seed=T)
        for casesens in (True, False):
            stats = _check(pred, gt, idx_to_char, casesens, cuda)
        hyp_chars = stats[:, 2].tolist()
        assert any(h > n for h, n in zip(hyp_chars, lengths)) and any(h < n for h, n in zip(hyp_chars, lengths))
        assert (stats[:, 1] > 0).any() and (stats[:, 3] > 0).any()
    assert max(hyp_chars) > 64


def test_decode_and_argmax_edges(cuda):
    """all-blank lines, a repeat separated by a blank, space - blank - space, leading and trailing spaces, exact ties in the maximum, NaN
    rows, all -inf rows"""
    C = 80
    idx_to_char = _char_set(C)
    a, sp, b = 1, 2, 3
    T = 12
    lines = [
        [0] * T,                                                # all blank
        [a, 0, a, a, 0, 0, b, b, b, 0, a, 0],                   # repeats with and without a blank between
        [a, sp, 0, sp, b, 0, 0, 0, 0, 0, 0, 0],                 # space, blank, space: two spaces decoded, one compared
        [sp, sp, 0, sp, a, b, sp, 0, sp, 0, 0, 0],              # leading and trailing spaces
        [sp, 0, sp, 0, sp, 0, sp, 0, 0, 0, 0, 0],               # nothing but spaces
        [a, b, a, b, a, b, a, b, a, b, a, b],                   # full length
    ]
    gt = ["", "aab a", "a b", "ab", "", "abababababab"]
    raw = np.array(lines).T
    pred = _pred_from_raw(raw, C, seed=1)
    stats = _check(pred, gt, idx_to_char, True, cuda)
    assert stats[:, 0].tolist() == [0, 4, 4, 6, 4, 12] and stats[:, 2].tolist() == [0, 4, 3, 2, 0, 12]
    assert stats[:, 1].tolist() == [0, 1, 0, 0, 0, 0] and stats[:, 3].tolist() == [0, 2, 0, 0, 0, 0] and stats[:, 4].tolist() == [0, 1, 2, 1, 0, 1]
    # ties, NaN, -inf: the host path reads the same array with np.argmax
    pred = _pred_from_raw(raw, C, seed=2)
    pred[0, 0, :] = 3.0                                          # every class ties: the first (the blank)
    pred[1, 1, :] = -1.0
    pred[1, 1, [b, 70]] = 5.0                                    # two classes tie: the lower one
    pred[2, 1, [79, 5]] = 20.0                                   # a tie across the two passes over a row of 80
    pred[3, 2, :] = np.nan                                       # a NaN row: the first NaN (the blank)
    pred[4, 2, 7] = np.nan                                       # one NaN beats every number
    pred[5, 2, [66, 9]] = np.nan                                 # the first NaN wins
    pred[5, 2, 30] = np.inf
    pred[6, 3, :] = -np.inf                                      # all -inf: the first
    pred[7, 3, :] = -np.inf
    pred[7, 3, 41] = -3e38
    pred[8, 4, :] = 0.0
    pred[8, 4, 6] = -0.0                                         # -0 == +0: still the first
    got = pred.argmax(2)
    assert got[0, 0] == 0 and got[1, 1] == b and got[2, 1] == 5 and got[3, 2] == 0 and got[4, 2] == 7 and got[5, 2] == 9
    assert got[6, 3] == 0 and got[7, 3] == 41 and got[8, 4] == 0
    _check(pred, gt, idx_to_char, True, cuda)
    _check(pred, gt, idx_to_char, False, cuda)
    # the same with a class count that takes the scalar loads
    _check(np.ascontiguousarray(np.concatenate([pred, pred[:, :, 1:2] - 1.0], axis=2)), gt, _char_set(81), True, cuda)


def test_beyond_a_limit_the_host_path_answers(cuda, capfd):
    from handwriting_line_generation_amd import ops
    C = 80
    idx_to_char = _char_set(C)
    char_to_idx = {v: k for k, v in idx_to_char.items()}
    gt = ["ab " * 682 + "ab", "ab cd"]
    assert len(gt[0]) == 2048
    pred = _pred_from_raw(np.stack([_raw_from_text("ab ab cd", 30, char_to_idx), _raw_from_text("ab cx", 30, char_to_idx)], axis=1), C, seed=3)
    before = ops.error_rate_fallbacks
    handle = ops.ctc_error_rates(torch.from_numpy(pred).to(cuda), gt, idx_to_char, True)
    assert ops.error_rate_fallbacks == before + 1 and handle.counts() is None
    assert handle.result() == ops.host_error_rates(pred, gt, idx_to_char, True)
    # a character set that does not compare class by class
    odd = dict(idx_to_char)
    odd[5] = "İ"
    handle = ops.ctc_error_rates(torch.from_numpy(pred).to(cuda), gt[1:] * 2, odd, False)
    assert ops.error_rate_fallbacks == before + 2
    assert handle.result() == ops.host_error_rates(pred, gt[1:] * 2, odd, False)
    assert capfd.readouterr().err.count("scored on the host") <= 1                       # said once
    with pytest.raises(ops.L.HwgError):
        ops.ctc_error_rates(torch.from_numpy(pred).to(cuda), gt[:1], idx_to_char, True)


@pytest.mark.parametrize("async_log", [False, 1])
def test_trainer_device_cer_changes_nothing(cuda, tmp_path, async_log):
    """two recogniser pre-training trainers from the same seeds, trainer.device_cer off and on: three iterations and flush_log give the same
    logs (CER and WER included), bit-identical weights, and _valid_epoch the same dictionary"""
    from oracle import torch_ref
    from handwriting_line_generation_amd import ops, rng
    from handwriting_line_generation_amd.harness import build_simple_trainer
    from handwriting_line_generation_amd.model import HWWithStyle
    cfgm = {"num_class": 80, "hwr": "CNNOnly batchnorm", "generator": "none", "style": "none"}
    msd = torch_ref.seeded_state_dict(HWWithStyle(cfgm), 41)
    runs = []
    before = ops.error_rate_fallbacks
    try:
        for device_cer in (False, True):
            rng.set_mode("device", seed=9)
            torch.manual_seed(0); np.random.seed(0); random.seed(0)
            workdir = tmp_path / ("on" if device_cer else "off")
            workdir.mkdir()
            trainer, _ = build_simple_trainer("iam_hwr", batch_size=4, width=128, label_len=5, workdir=str(workdir), model_state=msd)
            trainer.device_cer, trainer.async_log = device_cer, async_log
            logs = [trainer._train_iteration(it) for it in range(3)] + [trainer.flush_log()]
            trainer.valid_data_loader = [trainer.data_loader.dataset.batch(k) for k in (50, 51, 52)]
            val = trainer._valid_epoch()
            torch.cuda.synchronize()
            runs.append((logs, val, {k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items()}))
    finally:
        rng.set_mode("device")
    (logs_a, val_a, sd_a), (logs_b, val_b, sd_b) = runs
    assert ops.error_rate_fallbacks == before
    assert logs_a == logs_b and val_a == val_b
    assert sum("CER" in log for log in logs_a) >= 3 and all(np.isfinite(v) for log in logs_a for v in log.values())
    assert any(log.get("CER", 0) > 0 for log in logs_a) and val_a["val_CER"] > 0
    assert set(sd_a) == set(sd_b) and all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)


# ---- get_styles.py on a fabricated IAM directory and the reduced reference checkpoint (tests/_get_styles_program.py) ------------------------
def _in_process(program, split, cuda):
    """the same model and loader in this process -> (lines the loader hands out, first batch's styles, host-path cer / wer per real line)"""
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.data.author_hw_dataset import getDataLoader
    from handwriting_line_generation_amd.generate import load_for_generation
    model, config, _ = load_for_generation(program["ckpt"], program["cfg"], gpu=0)
    config["data_loader"]["shuffle"] = config["validation"]["shuffle"] = False
    idx_to_char = _iam_idx_to_char()
    first, cers, wers, authors = None, [], [], []
    if split == "test":
        loaders = {"test": getDataLoader(config, "test")[0]}
    else:
        loaders = dict(zip(("train", "val"), getDataLoader(config, "train")))
    out = {}
    with torch.no_grad():
        for name, loader in loaders.items():
            first, cers, wers, authors = None, [], [], []
            for inst in loader:
                image, label = ops.h2d(inst["image"], cuda), ops.h2d(inst["label"], cuda)
                model.pred = model.spaced_label = model.spaced_label_index = None
                style = model.extract_style(image, label, inst["a_batch_size"])
                if first is None:
                    first = style.cpu().numpy()
                c, w, _ = ops.host_error_rates(model.pred.cpu().numpy(), inst["gt"], idx_to_char, True)
                cers += c
                wers += w
                authors += list(inst["author"])
            model.pred = model.spaced_label = model.spaced_label_index = None
            out[name] = (authors, first, cers, wers)
    return out


def _mean(values):
    total = 0
    for v in values:
        total += v
    return total / max(len(values), 1)


@pytest.mark.parametrize("split", ["train", "test"])
def test_get_styles_program(cuda, program, split):
    from handwriting_line_generation_amd.generate import load_style_file, sample_styles
    out = str(program["dir"] / ("out_" + split))
    stdout = _child(["-c", program["ckpt"], "-f", program["cfg"], "-d", out, "-g", "0", "--cer"] + (["-T"] if split == "test" else []),
                    str(program["dir"]))
    it = program["iteration"]
    names = ["test"] if split == "test" else ["train", "val"]
    assert sorted(os.listdir(out)) == sorted(["%s_styles_%s.pkl" % (n, it) for n in names] + ["%s_cer_%s.json" % (n, it) for n in names])
    want = _in_process(program, split, cuda)
    for n in names:
        authors, first, cers, wers = want[n]
        assert len(authors) > 0 and "%s: lines %d " % (n, len(authors)) in stdout and "lines/s" in stdout, stdout[-2000:]
        got = pickle.load(open(os.path.join(out, "%s_styles_%s.pkl" % (n, it)), "rb"))
        assert set(got) == {"styles", "authors"}
        assert got["styles"].dtype == np.float32 and got["styles"].shape == (len(authors), first.shape[1])      # one row per line
        assert list(got["authors"]) == authors
        assert np.array_equal(got["styles"][:len(first)], first)
        scores = json.load(open(os.path.join(out, "%s_cer_%s.json" % (n, it))))
        assert set(scores) >= {"cer_real", "wer_real", "cer_gen", "wer_gen", "lines"} and scores["lines"] == len(authors)
        assert scores["cer_real_lines"] == cers and scores["wer_real_lines"] == wers
        assert scores["cer_real"] == _mean(cers) and scores["wer_real"] == _mean(wers)
        assert len(scores["cer_gen_lines"]) == len(scores["wer_gen_lines"]) == len(authors)
        assert all(np.isfinite(v) and v >= 0 for v in scores["cer_gen_lines"] + scores["wer_gen_lines"])
        assert scores["cer_gen"] == _mean(scores["cer_gen_lines"])
    styles = load_style_file(os.path.join(out, "%s_styles_" % names[0]))
    assert sum(len(v) for v in styles.values()) == len(want[names[0]][0])
    assert sample_styles(styles, 4, random.Random(2)).shape == (4, want[names[0]][1].shape[1])
