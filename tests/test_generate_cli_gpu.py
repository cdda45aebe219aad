"""GPU: from a checkpoint to pictures - generate.load_for_generation, render_lines, style_from_images and the generate.py program, on the
REFERENCE-written (width-reduced) checkpoint tests/golden/ref_ckpt_gan.pth.xz.

That checkpoint's spacer predicts ~0 blanks and ~0 repeats for every character (spacer.mean = spacer.std ~ -0.09 / 0.03: a line would be
empty), so every test but the loading one reads a copy of the file in which only spacer.mean = (3, 1) and spacer.std = (1.5, 0.5) are
replaced: lines are ~4 columns per character wide and their spacing depends on text and style."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _reference_checkpoint import unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = ["hello", "world", "abcde", "hi", "no", "ok"]
STYLE_SEED = 1          # no spacer count of TEXTS in these styles is within 1e-3 of a rounding tie (closest: 0.067; checked in the test below)


def _numpy_u8(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return ((np.float32(1.0) - x) * np.float32(127.5)).astype(np.uint8)


@pytest.fixture(scope="module")
def spread(cuda, tmp_path_factory):
    """-> dict(path, model, config, char_to_idx, state): the spread-out copy of the reference checkpoint, loaded for generation"""
    from handwriting_line_generation_amd.generate import load_for_generation
    from handwriting_line_generation_amd.logger import load_checkpoint
    d = tmp_path_factory.mktemp("gen_ckpt")
    ck = load_checkpoint(unpack("gan", d))
    ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
    ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
    path = os.path.join(str(d), "spread.pth")
    torch.save(ck, path)
    model, config, char_to_idx = load_for_generation(path, gpu=0)
    return {"path": path, "model": model, "config": config, "char_to_idx": char_to_idx, "state": ck["state_dict"]}


def _styles(n=len(TEXTS), seed=STYLE_SEED):
    return torch.randn(n, 128, generator=torch.Generator().manual_seed(seed))


def test_load_for_generation_builds_the_model_alone(cuda, tmp_path, monkeypatch):
    from handwriting_line_generation_amd.base import base_trainer
    from handwriting_line_generation_amd.generate import load_for_generation
    from handwriting_line_generation_amd.logger import load_checkpoint
    from handwriting_line_generation_amd.model import HWWithStyle

    def no_trainer(self, *a, **k):
        raise AssertionError("load_for_generation built a trainer")
    monkeypatch.setattr(base_trainer.BaseTrainer, "__init__", no_trainer)
    monkeypatch.setattr(torch.optim.Adam, "__init__", no_trainer)
    path = unpack("gan", tmp_path)
    model, config, char_to_idx = load_for_generation(path, gpu=0)
    assert isinstance(model, HWWithStyle) and not model.training and all(not m.training for m in model.modules())
    want = {k: v for k, v in load_checkpoint(path)["state_dict"].items() if "style_from_normal" not in k}
    got = model.state_dict()
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].is_cuda and torch.equal(got[k].cpu(), v), k
    assert config["model"]["RUN"] is True and all(v is None for k, v in config.items() if "pretrained" in k)
    packaged = json.load(open(os.path.join(ROOT, "handwriting_line_generation_amd", "data", "IAM_char_set.json")))["char_to_idx"]
    assert char_to_idx == packaged
    # a char_file that does not exist falls back to the packaged file of the same name; -a style additions reach the model's config
    ck = load_checkpoint(path)
    ck["config"]["data_loader"]["char_file"] = "/nowhere/at/all/IAM_char_set.json"
    torch.save(ck, str(tmp_path / "moved.pth"))
    model2, config2, cti2 = load_for_generation(str(tmp_path / "moved.pth"), gpu=0, add_to_config=[["model", "max_gen_length", "300"]])
    assert cti2 == packaged and model2.max_gen_length == 300 and config2["model"]["max_gen_length"] == 300


def _reference_render(model, texts, styles, char_to_idx, batches, cuda):
    """generate_stream over `batches`, downloaded as fp32, converted with numpy, cropped to 4 * (T - round(padded * T))"""
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.generate import generate_stream
    from handwriting_line_generation_amd.utils.string_utils import str2label_single

    def requests():
        for n, idx in batches:
            label = np.stack([str2label_single(texts[i], char_to_idx).astype(np.int32) for i in idx], axis=1)
            yield torch.from_numpy(label), torch.IntTensor([n] * len(idx)), ops.h2d(styles[idx].contiguous(), cuda)
    out, widths_of_batch = {}, []
    with torch.no_grad():
        for (n, idx), (image, padded) in zip(batches, generate_stream(model, requests(), cuda)):
            img = image.cpu().numpy()
            assert img.shape[:3] == (len(idx), 1, 64) and img.shape[3] % 4 == 0
            T = img.shape[3] // 4
            for b, i in enumerate(idx):
                w = min(max(4 * (T - int(round(padded[b] * T))), 4), img.shape[3])
                out[i] = _numpy_u8(img[b, 0, :, :w])
            widths_of_batch.append(img.shape[3])
    return out, widths_of_batch


def test_render_lines_is_the_models_output_cropped_and_converted(cuda, spread):
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.generate import bucket_by_length, render_lines
    model, cti = spread["model"], spread["char_to_idx"]
    styles = _styles()
    model.count_std, model.dup_std = 0.25, 0.125          # what the run must put back
    try:
        rng.set_mode("device", seed=41)
        got = list(render_lines(model, TEXTS, styles, cti, cuda, batch_lines=4))
        assert (model.count_std, model.dup_std) == (0.25, 0.125)
        batches, skipped = bucket_by_length(TEXTS, cti, 4)
        assert skipped == [] and [(n, idx) for n, idx in batches] == [(5, [0, 1, 2]), (2, [3, 4, 5])]
        rng.set_mode("device", seed=41)
        model.count_std = model.dup_std = 0
        want, image_widths = _reference_render(model, TEXTS, styles, cti, batches, cuda)
        assert sorted(i for i, _ in got) == list(range(len(TEXTS)))          # every index exactly once
        for i, line in got:
            assert line.dtype == np.uint8 and line.shape[0] == 64 and line.shape[1] % 4 == 0
            assert 4 <= line.shape[1] <= image_widths[0 if i < 3 else 1]
            assert line.shape == want[i].shape and np.array_equal(line, want[i]), i
        assert min(line.shape[1] for _, line in got) >= 16 and len({line.tobytes() for _, line in got}) == len(TEXTS)     # real, distinct lines
        # a consumer that stops early: the stds are 0 while the generator is open and come back when it is closed
        model.count_std, model.dup_std = 0.25, 0.125
        it = render_lines(model, TEXTS, styles, cti, cuda, batch_lines=2)
        next(it)
        assert (model.count_std, model.dup_std) == (0, 0) and torch.is_grad_enabled()
        it.close()
        assert (model.count_std, model.dup_std) == (0.25, 0.125)
    finally:
        model.count_std, model.dup_std = 1e-8, 1e-9
        rng.set_mode("device")
        torch.cuda.synchronize()


def test_a_lines_width_is_its_own_in_a_bucket_or_alone(cuda, spread):
    """count_std = dup_std = 0: the width of a line rendered in its bucket is its width rendered alone at batch 1 - with equal label lengths
    no line sees padding, so the spacing depends on the line's own text and style only. Integer widths are compared; the CPU oracle's
    spacer counts show that no chosen line sits within 1e-3 of a rounding tie (where the batched and the single pass could round apart)."""
    import torch.nn.functional as F
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.generate import render_lines
    from handwriting_line_generation_amd.utils.string_utils import str2label_single
    from oracle import torch_ref
    model, cti = spread["model"], spread["char_to_idx"]
    styles = _styles()
    sub = {k[len("spacer."):]: v for k, v in spread["state"].items() if k.startswith("spacer.")}
    oracle_widths = []
    for i, text in enumerate(TEXTS):
        lab = torch.from_numpy(str2label_single(text, cti).astype(np.int64))[:, None]
        counts = torch_ref.spacer(sub, F.one_hot(lab, 80).float(), styles[i:i + 1], training=False)
        tie = float((counts - torch.floor(counts) - 0.5).abs().min())
        assert tie > 1e-3, (text, tie)
        oracle_widths.append(4 * int(torch.round(counts).clamp_min(0).sum()))
    try:
        rng.set_mode("device", seed=5)
        bucketed = {i: line.shape[1] for i, line in render_lines(model, TEXTS, styles, cti, cuda, batch_lines=4)}
        alone = {i: line.shape[1] for i, line in render_lines(model, TEXTS, styles, cti, cuda, batch_lines=1)}
    finally:
        rng.set_mode("device")
    assert bucketed == alone
    assert [bucketed[i] for i in range(len(TEXTS))] == oracle_widths
    assert len(set(oracle_widths[:3])) > 1 or len(set(oracle_widths[3:])) > 1        # the spacing does depend on text and style


def _child(args, timeout=300):
    """one generate.py process; a non-zero or timed-out child fails the test at once (nothing more is started on the GPU)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py")] + args, cwd=ROOT, timeout=timeout, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def _read_pngs(d, names):
    from PIL import Image
    out = []
    for n in names:
        im = Image.open(os.path.join(d, n))
        assert im.mode == "L" and im.size[1] == 64 and im.size[0] > 0 and im.size[0] % 4 == 0, (n, im.mode, im.size)
        out.append(np.asarray(im).copy())
    return out


def test_cli_R(cuda, spread, tmp_path):
    import generate as cli
    from handwriting_line_generation_amd.evaluate import dump_styles
    g = np.random.RandomState(3)
    dump_styles({"styles": g.randn(6, 128).astype(np.float32), "authors": ["a", "a", "b", "b", "c", "c"]}, str(tmp_path / "styles.pkl"))
    lines = ["the quick brown fox", "jumps over", "the lazy dog and", "then it sleeps", "for a while in", "the warm sun", "until the evening",
             "comes again"]
    (tmp_path / "texts.txt").write_text("\n".join(lines) + "\n")
    corpus = " ".join(lines) + " "          # TextData collapses white space, the final newline included
    names = ["sample_%d.png" % i for i in range(5)]

    def run(out, seed, extra=()):
        stdout = _child(["-c", spread["path"], "-d", str(tmp_path / out), "-g", "0", "-s", str(tmp_path / "styles.pkl"),
                         "-r", "choice=R,num=5,text=%s" % (tmp_path / "texts.txt"), "--seed", str(seed)] + list(extra))
        assert "lines 5 " in stdout and "lines/s" in stdout, stdout[-2000:]
        return str(tmp_path / out)
    a = run("a", 7)
    assert sorted(os.listdir(a)) == sorted(names + ["OUT.txt"])
    px_a = _read_pngs(a, names)
    out_a = open(os.path.join(a, "OUT.txt")).read()
    rows = out_a.splitlines()
    assert len(rows) == 5
    for i, row in enumerate(rows):
        head, text = row.split(":", 1)
        assert head == str(i) and len(text) > 0 and text in corpus
    b = run("b", 7)
    px_b = _read_pngs(b, names)
    assert open(os.path.join(b, "OUT.txt")).read() == out_a
    assert all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(px_a, px_b))
    c = run("c", 8)
    px_c = _read_pngs(c, names)
    assert open(os.path.join(c, "OUT.txt")).read() != out_a or any(p.shape != q.shape or not np.array_equal(p, q) for p, q in zip(px_a, px_c))
    s = run("s", 7, ["--shard", "3"])
    assert sorted(os.listdir(s)) == ["OUT.txt", "lines_00000.npz", "lines_00001.npz"]
    first, second = cli.read_shard(os.path.join(s, "lines_00000.npz")), cli.read_shard(os.path.join(s, "lines_00001.npz"))
    assert len(first) == 3 and len(second) == 2
    assert sorted(i for i, _ in first + second) == list(range(5))
    with np.load(os.path.join(s, "lines_00000.npz")) as z:
        assert z["pixels"].dtype == np.uint8 and z["pixels"].ndim == 1 and z["offsets"].dtype == np.int64 and z["offsets"].shape == (4,)
        assert z["widths"].dtype == np.int32 and z["index"].dtype == np.int64 and z["offsets"][-1] == z["pixels"].size == 64 * z["widths"].sum()
    for i, line in first + second:
        assert line.shape == px_a[i].shape and np.array_equal(line, px_a[i]), i


def _noise_line(path, h, w, seed):
    """seeded grey noise blurred along x"""
    from PIL import Image
    x = np.random.RandomState(seed).uniform(0, 255, (h, w + 8))
    x = np.stack([x[:, k:k + w] for k in range(9)]).mean(0)
    Image.fromarray(x.astype(np.uint8)).save(path)


def test_cli_f(cuda, spread, tmp_path):
    import generate as cli
    from PIL import Image
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.generate import generate, style_from_images
    model, cti = spread["model"], spread["char_to_idx"]
    p1, p2 = str(tmp_path / "one.png"), str(tmp_path / "two.png")
    _noise_line(p1, 64, 160, 1)
    _noise_line(p2, 80, 200, 2)          # 80 rows: resized to 64 x 160
    out = str(tmp_path / "out")
    _child(["-c", spread["path"], "-d", out, "-g", "0", "-r", "choice=f,path1=%s,path2=%s,text=hello" % (p1, p2)])
    names = ["gen0_%d.png" % i for i in range(20)]
    assert sorted(os.listdir(out)) == sorted(names)
    px = _read_pngs(out, names)
    assert len({p.shape for p in px[:1] + px[-1:]}) > 1 or not np.array_equal(px[0], px[-1])
    try:
        # the same steps in this process, from the same seed: styles of the two images, then the first interpolation step = style 1 itself
        cli.seed_everything(1234)
        style = style_from_images(model, [p1, p2], cuda)
        assert style.shape == (2, 128)
        model.count_std = model.dup_std = 0
        with torch.no_grad():
            first = generate(model, style[0:1].contiguous(), "hello", cti, cuda).cpu().numpy()
        want = _numpy_u8(first[0, 0])
        assert px[0].shape == want.shape and np.array_equal(px[0], want)
        # style_from_images = extract_style on the tensor built here with the same PIL calls
        im1 = Image.open(p1).convert("L")
        im2 = Image.open(p2).convert("L")
        assert im2.size == (200, 80)
        im2 = im2.resize((160, 64), Image.BICUBIC)
        stack = torch.stack([torch.from_numpy(1.0 - np.asarray(im, dtype=np.float32)[None] / 128.0) for im in (im1, im2)], dim=0)
        old = model.use_hwr_pred_for_style
        model.use_hwr_pred_for_style = True
        model.pred = model.spaced_label = model.spaced_label_index = None
        try:
            with torch.no_grad():
                direct = model.extract_style(ops.h2d(stack, cuda), None, 1)
        finally:
            model.use_hwr_pred_for_style = old
            model.pred = model.spaced_label = model.spaced_label_index = None
        assert torch.equal(direct, style)
        assert float((style[0] - style[1]).abs().max()) > 0
    finally:
        model.count_std, model.dup_std = 1e-8, 1e-9
        from handwriting_line_generation_amd import rng
        rng.set_mode("device")
