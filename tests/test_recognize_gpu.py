"""GPU: recognize.py as a child process on a temporary directory of fabricated line images of differing heights and widths, with the reduced
reference checkpoints (the GAN checkpoint and the recogniser pre-training checkpoint; their recognisers' periodic fixture weights read the
same few characters off every picture, so the convolution and recurrent weights are redrawn from a seeded generator first - every other
entry of the files is kept) and a CRNN pre-training checkpoint of this package built on the spot. The program's output file is compared byte for byte
with the host path run in this process on the same batches - `_resize` (PIL), 1 - p / 128, padding -1, the recogniser,
ops.host_error_rates - so the device fit, the batching, the device decode and the order of the output are all held to the loaders'
arithmetic. A failed or timed-out child fails the test at once and nothing more is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)
from _reference_checkpoint import unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, BUCKET = 5, 32
SIZES = [(40, 60), (64, 200), (150, 700), (47, 333), (64, 64), (90, 410), (128, 512), (55, 61), (100, 700), (73, 150), (41, 97), (149, 301)]


def _strokes(h, w, seed):
    """a white picture with a few dark wavy strokes of differing thickness and grey level"""
    g = np.random.RandomState(seed)
    img = np.full((h, w), 255, dtype=np.uint8)
    xs = np.arange(w)
    for _ in range(4 + seed % 3):
        y = h * (0.5 + 0.3 * np.sin(xs / g.uniform(3.0, 25.0) + g.uniform(0, 6.28))) + g.uniform(-0.15, 0.15) * h
        lo, hi = sorted(g.randint(0, w, 2))
        t = g.randint(1, 4)
        for x in range(lo, hi + 1):
            y0 = int(np.clip(y[x], 0, h - 1))
            img[max(y0 - t, 0):y0 + t, x] = g.randint(0, 90)
    for _ in range(3):                                              # upright strokes
        x0 = g.randint(0, w)
        img[g.randint(0, h // 2):g.randint(h // 2, h), max(x0 - 1, 0):x0 + 2] = g.randint(0, 60)
    return img


def _redrawn(path, dst, seed):
    """the checkpoint at `path` with the recogniser's weight matrices and filters redrawn (He-scaled normal values): what it reads now
    depends on the picture"""
    from handwriting_line_generation_amd.logger import load_checkpoint
    ck = load_checkpoint(path)
    g = torch.Generator().manual_seed(seed)
    n = 0
    for k, v in ck["state_dict"].items():
        if k.startswith("hwr.") and v.dtype.is_floating_point and v.dim() >= 2:
            v.copy_(torch.randn(v.shape, generator=g) * (2.0 / v[0].numel()) ** 0.5)
            n += 1
    assert n >= 5, n
    torch.save(ck, dst)
    return dst


def _crnn_checkpoint(hwr_path, dst, seed):
    """a recogniser pre-training checkpoint of this package with a CRNN: the reference file's config with `hwr` = "CRNN batchnorm", the
    keys of a freshly initialised HWWithStyle of that config (whose small default weights read the same two characters off every
    picture: the caller redraws them as well)"""
    from handwriting_line_generation_amd.logger import load_checkpoint
    from handwriting_line_generation_amd.model import HWWithStyle
    ck = load_checkpoint(hwr_path)
    config = ck["config"]
    config["model"] = dict(config["model"], hwr="CRNN batchnorm", pretrained_hwr=None)
    torch.manual_seed(seed)
    state = HWWithStyle(dict(config["model"])).state_dict()
    assert state and all(k.startswith("hwr.") for k in state)
    torch.save({"arch": "HWWithStyle", "iteration": 1, "config": config, "state_dict": state}, dst)
    return dst


def _child(args, cwd, timeout=300):
    """one recognize.py process; a non-zero or timed-out child fails the test at once (nothing more is started on the GPU)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "recognize.py")] + args, cwd=cwd, timeout=timeout, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def lines(cuda, tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("recognize")
    os.makedirs(str(d / "lines"))
    names = ["line_%02d.png" % i for i in range(len(SIZES))]
    images = [_strokes(h, w, i) for i, (h, w) in enumerate(SIZES)]
    for name, im in zip(names, images):
        Image.fromarray(im).save(str(d / "lines" / name))
    (d / "lines" / "notes.txt").write_text("not a line\n")
    gt = ["the %s line, no. %d" % ("quick brown", i) for i in range(len(SIZES))]
    with open(str(d / "gt.tsv"), "w") as f:
        for i in (3, 0, 7, 1, 2, 4, 5, 6, 8, 9, 10, 11):
            f.write("%s\t%s\n" % (names[i], gt[i]))
    hwr = unpack("hwr", d)
    return dict(dir=d, names=names, images=images, gt=gt, gan=_redrawn(unpack("gan", d), str(d / "gan.pth"), 1),
                hwr=_redrawn(hwr, str(d / "hwr.pth"), 2), crnn=_redrawn(_crnn_checkpoint(hwr, str(d / "crnn0.pth"), 3), str(d / "crnn.pth"), 4))


def _host_path(lines, which, cuda, beam=0, order=None):
    """the expected texts (and cer / wer against the references) in the order `order` of the input: the host path on the program's batches"""
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.data.author_hw_dataset import _resize
    from handwriting_line_generation_amd.recognize import load_recogniser, plan_batches
    from handwriting_line_generation_amd.utils import string_utils
    hwr, idx_to_char, config = load_recogniser(lines[which], 0)
    H = int(config["data_loader"].get("img_height", 64))
    cs = config.get("trainer", {}).get("casesensitive", True)
    order = list(range(len(SIZES))) if order is None else order
    images, gt = [lines["images"][i] for i in order], [lines["gt"][i] for i in order]
    fitted = [im if im.shape[0] == H else _resize(im, float(H) / im.shape[0]) for im in images]
    texts = [None] * len(images)
    with torch.no_grad():
        for idx, W in plan_batches([f.shape[1] for f in fitted], BATCH, BUCKET):
            x = np.full((len(idx), 1, H, W), -1.0, dtype=np.float32)
            for j, i in enumerate(idx):
                x[j, 0, :, :fitted[i].shape[1]] = np.float32(1.0) - fitted[i].astype(np.float32) / np.float32(128.0)
            pred = hwr(ops.h2d(torch.from_numpy(x), cuda), None)
            refs = [gt[i] for i in idx]
            if beam:
                _, _, strs = ops.ctc_beam_error_rates(pred, refs, idx_to_char, cs, beam).result()
            else:
                _, _, strs = ops.host_error_rates(pred.cpu().numpy(), refs, idx_to_char, cs)
            for j, i in enumerate(idx):
                texts[i] = strs[j]
    del hwr
    cers = [string_utils.cer(g, t, cs) for g, t in zip(gt, texts)]
    wers = [string_utils.wer(g, t, cs) for g, t in zip(gt, texts)]
    return texts, cers, wers


def _file(names, texts):
    return "".join("%s\t%s\n" % (n, t) for n, t in zip(names, texts)).encode("utf-8")


def test_program_writes_the_host_paths_texts_and_scores(cuda, lines):
    d = lines["dir"]
    texts, cers, wers = _host_path(lines, "gan", cuda)
    print("\nrecognize texts: %r" % (texts,))
    assert len(set(texts)) >= 6, "the fabricated lines read alike: the comparison below would not see a line out of place"
    common = ["-c", lines["gan"], "-i", "lines", "-g", "0", "--batch", str(BATCH), "--bucket", str(BUCKET)]
    out = _child(common + ["-o", "device.txt", "--gt", "gt.tsv"], str(d))
    assert "fallbacks 0" in out and "fit device" in out, out[-2000:]
    assert open(str(d / "device.txt"), "rb").read() == _file(lines["names"], texts)
    got = json.load(open(str(d / "device.txt.json")))
    assert got["lines"] == got["scored"] == len(SIZES) and got["fit_fallbacks"] == 0 and got["beam"] == 0
    assert [p["name"] for p in got["per_line"]] == lines["names"] and [p["text"] for p in got["per_line"]] == texts
    assert [p["cer"] for p in got["per_line"]] == cers and [p["wer"] for p in got["per_line"]] == wers         # bit for bit string_utils.cer / wer
    total_c = total_w = 0
    for c, w in zip(cers, wers):
        total_c, total_w = total_c + c, total_w + w
    assert got["cer"] == total_c / len(cers) and got["wer"] == total_w / len(wers)
    # --host-fit: the program's own cross-check writes the same bytes
    out = _child(common + ["-o", "host.txt", "--host-fit"], str(d))
    assert "fit host" in out
    assert open(str(d / "host.txt"), "rb").read() == open(str(d / "device.txt"), "rb").read()
    assert not os.path.exists(str(d / "host.txt.json"))


def test_beam_and_a_shuffled_list_keep_the_lists_order(cuda, lines):
    d = lines["dir"]
    order = [int(i) for i in np.random.RandomState(7).permutation(len(SIZES))]
    assert order != sorted(order)
    listed = [os.path.join("lines", lines["names"][i]) for i in order]
    with open(str(d / "list.txt"), "w") as f:
        f.write("\n".join(listed) + "\n")
    texts, _, _ = _host_path(lines, "gan", cuda, beam=4, order=order)
    out = _child(["-c", lines["gan"], "-i", "list.txt", "-o", "beam.txt", "--beam", "4", "--batch", str(BATCH), "--bucket", str(BUCKET)], str(d))
    assert "fallbacks 0" in out
    assert open(str(d / "beam.txt"), "rb").read() == _file(listed, texts)


@pytest.mark.parametrize("which", ["hwr", "crnn"])
def test_recogniser_pretraining_checkpoints_read_the_same_lines(cuda, lines, which):
    """the reference's CNN-only pre-training checkpoint and a CRNN one of this package"""
    d = lines["dir"]
    texts, _, _ = _host_path(lines, which, cuda)
    print("\nrecognize texts (%s): %r" % (which, texts))
    assert len(set(texts)) >= 6
    out = _child(["-c", lines[which], "-i", "lines", "-o", which + ".txt", "--batch", str(BATCH), "--bucket", str(BUCKET), "--timing"], str(d))
    assert "fallbacks 0" in out and "timing (synchronised)" in out
    assert open(str(d / (which + ".txt")), "rb").read() == _file(lines["names"], texts)
