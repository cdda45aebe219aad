"""CPU: what recogniser training on generated lines decides on the host - the argument checks of hwg_lines_from_u8 in front of its launch,
the pool's bookkeeping (data/synth_lines.py, with a stub renderer in the generator's place), label merging against `collate`, the config
refusals of HWRWithSynthTrainer and its resolution by name."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 64
CHARS = {c: i + 1 for i, c in enumerate("abcdefghij ")}


def test_lines_from_u8_entry_point_refuses_bad_arguments_before_any_launch():
    """the argument checks run on the host side of the entry point, in front of the launch: with arguments they refuse, the call returns its
    status without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20          # any 16-byte aligned address
    good = dict(pixels=p, n=4096, offsets=p, widths=p, n_lines=1, select=p, min_select=0, real=None, Br=0, Wr=0, B=1, H=64, W=44, out=p, stream=0)

    def args(**kw):
        return tuple(kw.get(k, v) for k, v in good.items())
    for a, word in [(args(pixels=None), "null"), (args(offsets=None), "null"), (args(widths=None), "null"), (args(select=None), "null"),
                    (args(out=None), "null"), (args(B=0), "bad sizes"), (args(H=0), "bad sizes"), (args(W=0), "bad sizes"), (args(B=70000), "bad sizes"),
                    (args(n_lines=-1), "bad sizes"), (args(W=42), "multiple of 4"), (args(out=p + 4), "aligned"), (args(pixels=p + 2), "aligned"),
                    (args(min_select=-1), "negative select"), (args(real=p, Br=2, Wr=45), "real batch"), (args(real=p, Br=0, Wr=40), "real batch"),
                    (args(real=p + 2, Br=2, Wr=37), "aligned"), (args(real=p, Br=2, Wr=37, min_select=-3), "behind")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_lines_from_u8", *a)
        assert word in str(e.value), (a, str(e.value))


# ---- the pool, with a stub in the generator's place ------------------------------------------------------------------------------------------
def _files(tmp_path, text="abc def ghij abcdefghij hgfedcba jihg fedcba abcabc defdef"):
    styles = str(tmp_path / "styles_")
    with open(styles + "1.pkl", "wb") as f:
        pickle.dump({"authors": ["x", "x", "y", "z"], "styles": np.random.RandomState(1).randn(4, 8).astype(np.float32)}, f)
    corpus = str(tmp_path / "corpus.txt")
    open(corpus, "w").write(text)
    return styles, corpus


def _stub(rendered=None, batch_lines=3):
    """render(texts, styles) like generate.render_lines_device: buckets by label length, a line of 4 columns per character, host tensors"""
    from handwriting_line_generation_amd.generate import bucket_by_length

    def render(texts, styles):
        assert len(texts) == styles.shape[0]
        batches, _ = bucket_by_length(texts, CHARS, batch_lines)
        for n, idx in batches:
            widths = [4 * len(texts[i]) for i in idx]
            offsets = np.zeros(len(idx) + 1, dtype=np.int64)
            np.cumsum(H * np.asarray(widths), out=offsets[1:])
            if rendered is not None:
                rendered.append(list(idx))
            yield idx, torch.full((int(offsets[-1]),), len(idx), dtype=torch.uint8), offsets, widths
    return render


def _pool(tmp_path, render=None, rank=0, start=0, **synth):
    from handwriting_line_generation_amd.data.synth_lines import SynthLinePool
    styles, corpus = _files(tmp_path) if "text_data" not in synth else (_files(tmp_path)[0], synth.pop("text_data"))
    cfg = dict(dict(checkpoint="unused", styles=styles, text_data=corpus, per_batch=2, pool=8, seed=5, max_len=6), **synth)
    return SynthLinePool(cfg, CHARS, rank=rank, start=start, render=render or _stub())


def test_no_index_twice_before_a_refill_and_a_refill_at_exhaustion(tmp_path):
    pool = _pool(tmp_path)
    assert pool.refills == [] and pool.pixels is None                     # nothing is rendered before the first draw
    seen = []
    for _ in range(4):
        seen += pool.draw(2)
        assert pool.refills == [0]
    assert sorted(seen) == list(range(8))
    first = (list(pool.texts), pool.offsets.copy())
    again = pool.draw(2)
    assert pool.refills == [0, 1] and len(again) == 2 and (list(pool.texts), pool.offsets.tolist()) != (first[0], first[1].tolist())
    # tables of the kept lines: inside the one buffer, multiples of 4, labels as str2label_single encodes the text
    from handwriting_line_generation_amd.utils.string_utils import str2label_single
    assert pool.pixels.dtype == torch.uint8 and pool.pixels.dim() == 1
    assert (pool.offsets % 4 == 0).all() and (pool.widths % 4 == 0).all() and (pool.offsets + H * pool.widths <= pool.pixels.numel()).all()
    assert len(set(pool.offsets.tolist())) == len(pool.offsets)
    for text, label, w in zip(pool.texts, pool.labels, pool.widths):
        assert w == 4 * len(text) and np.array_equal(label, str2label_single(text, CHARS))
    # fewer than n left: the remainder is dropped, the next pool is drawn
    pool.draw(5)
    assert pool.refills == [0, 1]
    pool.draw(2)
    assert pool.refills == [0, 1, 2]
    assert pool.name(pool.draw(1)[0]).startswith("synth_") and 16 <= int(pool.name(0)[6:]) < 24


def test_seed_rank_and_refill_number_make_the_pool(tmp_path):
    def state(pool, k):
        pool.refill(k)
        return pool.drawn_texts, pool.drawn_styles.tobytes(), [pool.draw(2) for _ in range(4)]
    a, b = _pool(tmp_path), _pool(tmp_path)
    assert state(a, 3) == state(b, 3)
    assert state(a, 0) == state(b, 0)                     # whatever was rendered before
    other_rank, other_seed = _pool(tmp_path, rank=1), _pool(tmp_path, seed=6)
    s0 = state(a, 3)
    for other in (state(other_rank, 3), state(other_seed, 3), state(b, 4)):
        assert other[0] != s0[0] and other[1] != s0[1]
    assert len(s0[0]) == 8 and all(3 <= len(t) <= 6 or t == "" for t in s0[0])


def test_left_out_lines_are_not_counted(tmp_path):
    corpus = str(tmp_path / "digits.txt")
    open(corpus, "w").write("abc 0123456789012 def 98765432109876 ghij 5555555555555 abcdefghij")
    pool = _pool(tmp_path, text_data=corpus, pool=32)
    pool.refill(0)
    from handwriting_line_generation_amd.utils.string_utils import str2label_single
    empty = [i for i, t in enumerate(pool.drawn_texts) if len(str2label_single(t, CHARS)) == 0]
    assert 0 < len(empty) < 32 and pool.left_out == len(empty)
    assert len(pool.texts) == len(pool.labels) == len(pool.offsets) == len(pool.widths) == 32 - len(empty)
    assert sorted(pool.ids) == [i for i in range(32) if i not in empty] and all(len(l) > 0 for l in pool.labels)
    n = 0
    while pool.refills == [0]:
        drawn = pool.draw(1)
        n += pool.refills == [0]
    assert n == 32 - len(empty)
    # lines wider than max_width are left out too
    wide = _pool(tmp_path, pool=32, max_width=16)
    wide.refill(0)
    assert 0 < len(wide.texts) < 32 and (wide.widths <= 16).all() and wide.left_out == 32 - len(wide.texts)
    assert sum(1 for t in wide.drawn_texts if 0 < 4 * len(str2label_single(t, CHARS)) <= 16) == len(wide.texts)
    # a pool that keeps fewer lines than one batch draws says why
    none = _pool(tmp_path, pool=8, max_width=4)
    with pytest.raises(RuntimeError, match="fewer than"):
        none.draw(8)


def test_resume_refill_number(tmp_path):
    from handwriting_line_generation_amd.data.synth_lines import first_refill
    assert [first_refill(i, 2, 4) for i in range(6)] == [0, 0, 1, 1, 2, 2]
    assert first_refill(1000, 16, 2048) == 7 and first_refill(0, 16, 2048) == 0 and first_refill(128, 16, 2048) == 1
    # a run of 3 iterations at per_batch 2, pool 4 used pools 0 and 1; resumed behind iteration 2 the first pool is number 1, never 0 again
    fresh = _pool(tmp_path, pool=4)
    for _ in range(3):
        fresh.draw(2)
    assert fresh.refills == [0, 1]
    resumed = _pool(tmp_path, pool=4, start=first_refill(2, 2, 4))
    resumed.draw(2)
    assert resumed.refills == [1] and resumed.drawn_texts == fresh.drawn_texts
    resumed.draw(2), resumed.draw(2)
    assert resumed.refills == [1, 2]


def test_label_merging_equals_collate():
    from handwriting_line_generation_amd.data.hw_dataset import collate
    from handwriting_line_generation_amd.data.synth_lines import SYNTH_AUTHOR, merge_labels

    def item(w, gt, lab, name, author):
        return {"image": np.zeros((H, w, 1), dtype=np.float32), "gt": gt, "gt_label": np.asarray(lab, dtype=np.uint32), "name": name,
                "center": False, "author": author}
    real = [item(37, "abc", [1, 2, 3], "x_0", "x"), item(21, "de", [4, 5], "y_3", "y")]
    for synth in ([("fghi", [6, 7, 8, 9]), ("j", [10])], [("a", [1])], []):          # longer than, shorter than the real labels; none
        want = collate(real + [item(8, t, l, "synth_%d" % k, SYNTH_AUTHOR) for k, (t, l) in enumerate(synth)])
        inst = collate(real)
        got = merge_labels(inst, [t for t, _ in synth], [np.asarray(l, dtype=np.uint32) for _, l in synth], ["synth_%d" % k for k in range(len(synth))])
        assert got["label"].dtype == torch.int32 and torch.equal(got["label"], want["label"])
        assert got["label_lengths"].dtype == want["label_lengths"].dtype and torch.equal(got["label_lengths"], want["label_lengths"])
        assert got["gt"] == want["gt"] and got["name"] == want["name"] and got["author"] == want["author"]
        assert got["image"] is inst["image"] and inst["label"].shape[1] == 2            # the real instance itself is left as it was


# ---- the trainer's configuration -------------------------------------------------------------------------------------------------------------
def _config(tmp_path, **synth):
    cfg = json.load(open(os.path.join(ROOT, "configs", "cf_IAM_hwr_cnnOnly_batchnorm_aug_synth.json")))
    styles, corpus = _files(tmp_path)
    ckpt = str(tmp_path / "gen.pth")
    open(ckpt, "wb").write(b"")
    cfg["trainer"]["synth"].update(checkpoint=ckpt, styles=styles, text_data=corpus)
    cfg["trainer"]["synth"].update(synth)
    cfg["trainer"]["save_dir"] = str(tmp_path / "saved")
    return cfg


def test_shipped_config_is_pretraining_plus_the_synth_block(tmp_path):
    from handwriting_line_generation_amd.data.synth_lines import SYNTH_KEYS, validate_synth_config
    base = json.load(open(os.path.join(ROOT, "configs", "cf_IAM_hwr_cnnOnly_batchnorm_aug.json")))
    cfg = json.load(open(os.path.join(ROOT, "configs", "cf_IAM_hwr_cnnOnly_batchnorm_aug_synth.json")))
    assert cfg["name"] == "IAM_hwr_cnnOnly_batchnorm_aug_synth" and cfg["trainer"]["class"] == "HWRWithSynthTrainer"
    assert set(cfg["trainer"]["synth"]) == set(SYNTH_KEYS)
    cfg["trainer"].pop("synth")
    cfg["trainer"]["class"], cfg["name"] = base["trainer"]["class"], base["name"]
    assert cfg == base
    assert cfg["model"]["generator"] == "none" and cfg["model"]["style"] == "none"          # checkpoints hold the recogniser alone
    assert validate_synth_config(_config(tmp_path)) == (16, 2048)


@pytest.mark.parametrize("change,word", [
    (dict(per_batch=-1), "negative"),
    (dict(per_batch=4, pool=3), "smaller than per_batch"),
    (dict(checkpoint="/nowhere/gen.pth"), "generator checkpoint"),
    (dict(styles="/nowhere/styles_"), "style file"),
    (dict(text_data="/nowhere/text.txt"), "text file"),
    (dict(checkpoint=None), "is missing"),
    (dict(pol=4), "unknown key"),
    ("center_pad", "center_pad"),
])
def test_config_refusals_say_why(tmp_path, change, word):
    """refused by validate_synth_config and by the trainer's constructor alike - before a model moves, a pool loads or a directory is made"""
    from handwriting_line_generation_amd.data.synth_lines import validate_synth_config
    from handwriting_line_generation_amd.trainer import HWRWithSynthTrainer
    cfg = _config(tmp_path)
    if change == "center_pad":
        cfg["data_loader"]["center_pad"] = True
    else:
        cfg["trainer"]["synth"].update(change)
    with pytest.raises(ValueError, match=word):
        validate_synth_config(cfg)
    with pytest.raises(ValueError, match=word):
        HWRWithSynthTrainer(None, {}, [], None, cfg, None)
    assert not os.path.exists(cfg["trainer"]["save_dir"])


def test_per_batch_zero_needs_no_files(tmp_path):
    from handwriting_line_generation_amd.data.synth_lines import validate_synth_config
    cfg = _config(tmp_path, per_batch=0, checkpoint="/nowhere/gen.pth", styles="/nowhere/s", text_data="/nowhere/t")
    cfg["data_loader"]["center_pad"] = True
    assert validate_synth_config(cfg) == (0, 0)
    cfg["trainer"].pop("synth")
    assert validate_synth_config(cfg) == (0, 0)


def test_trainer_resolves_by_name():
    """train.py: getattr(trainers, config["trainer"]["class"])"""
    import handwriting_line_generation_amd.trainer as trainers
    from handwriting_line_generation_amd.trainer.hw_with_style_trainer import HWWithStyleTrainer
    cfg = json.load(open(os.path.join(ROOT, "configs", "cf_IAM_hwr_cnnOnly_batchnorm_aug_synth.json")))
    cls = getattr(trainers, cfg["trainer"]["class"])
    assert cls.__name__ == "HWRWithSynthTrainer" and issubclass(cls, HWWithStyleTrainer)
