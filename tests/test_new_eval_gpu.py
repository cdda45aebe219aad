"""GPU: the new_eval.py program and handwriting_line_generation_amd/evaluators.py on the fabricated IAM directory (oracle.collate_items.fake_iam)
and the reduced REFERENCE-written checkpoints of tests/golden (the GAN one with its spacer spread out as tests/test_error_rates_gpu.py explains).
Pictures are compared byte for byte with the numpy restatement (tests/_eval_pictures_ref.py) of the device tensors the evaluator's hook shows;
scores with ops.host_error_rates on the hooked predictions."""
import csv
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _eval_pictures_ref as ref
from _gpu_tidy import leave_nothing_behind  # noqa: F401
from _reference_checkpoint import unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 64


@pytest.fixture(scope="module")
def program(cuda, tmp_path_factory):
    """-> {kind: (checkpoint path, config path, name, iteration)} for the GAN, recogniser and autoencoder checkpoints, on one dataset"""
    from oracle import collate_items
    from handwriting_line_generation_amd.harness import CHAR_FILES
    from handwriting_line_generation_amd.logger import load_checkpoint
    d = tmp_path_factory.mktemp("new_eval")
    root = str(d / "iam")
    os.makedirs(root)
    collate_items.fake_iam(root, n_pages=6, with_images=True)
    out = {"dir": d}
    for kind in ("gan", "hwr", "auto"):
        ck = load_checkpoint(unpack(kind, d))
        path = str(d / ("%s.pth" % kind))
        if kind == "gan":
            ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
            ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
        torch.save(ck, path)
        cfg = ck["config"]
        cfg["data_loader"].update(data_dir=root, batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"], augmentation=None)
        cfg["validation"] = dict(cfg.get("validation", {}), batch_size=2, num_workers=0, augmentation=None)
        if kind != "hwr":
            cfg["data_loader"].update(a_batch_size=2 if kind == "gan" else 1, max_width=640)
            cfg["validation"].update(a_batch_size=2 if kind == "gan" else 1)
        cfg["trainer"]["save_dir"] = str(d / "saved")
        cfg_path = str(d / ("%s.json" % kind))
        json.dump(cfg, open(cfg_path, "w"))
        out[kind] = (path, cfg_path, cfg["name"], ck["iteration"])
    return out


class Hooked:
    """collects what evaluators.hook is shown, tensors copied to the host"""

    def __init__(self):
        self.calls = []

    def __call__(self, kind, names, tensors):
        self.calls.append((kind, list(names), {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in tensors.items()}))

    def of(self, kind):
        return [(n, t) for k, n, t in self.calls if k == kind]


def _main(argv, capsys):
    """new_eval.main in this process under the hook -> (stdout, Hooked)"""
    import new_eval
    from handwriting_line_generation_amd import evaluators, rng
    hooked = Hooked()
    evaluators.hook = hooked
    rng.set_mode("device", seed=3)
    try:
        capsys.readouterr()
        new_eval.main(argv)
        evaluators.wait()
    finally:
        evaluators.hook = None
        rng.set_mode("device")
    return capsys.readouterr().out, hooked


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.mode, np.asarray(im).copy()


def _iam_idx_to_char():
    pkg = os.path.join(ROOT, "handwriting_line_generation_amd", "data", "IAM_char_set.json")
    return {int(k): v for k, v in json.load(open(pkg))["idx_to_char"].items()}


def _check_pair_pictures(hooked, prefixed=False):
    """every picture the hook saw is on disk as the restatement of the hooked tensors and captions (a line name that repeats - an author's
    left-over line is handed out twice - is written again: the last one stays); -> the files seen"""
    last = {}
    for names, t in hooked.of("recon"):
        want = ref.eval_pairs(t["image"], t["recon"], t["codes"], t["atlas"])
        assert np.array_equal(t["pictures"], want)
        for k, name in enumerate(names):
            fname = "%s_recon.png" % name
            if prefixed:
                fname = re.match(r"CER: (\d+\.\d{3}), ", t["captions"][k]).group(1) + "_" + fname
            last[os.path.join(t["outDir"], fname)] = want[k]
    for path, want in last.items():
        mode, pixels = _png(path)
        assert mode == "RGB" and np.array_equal(pixels, want), path
    return set(last)


def test_program_in_a_child_process(cuda, program):
    ckpt, cfg, name, iteration = program["gan"]
    out = str(program["dir"] / "child")
    r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, os.path.join(ROOT, "new_eval.py"), "-c", ckpt, "-f", cfg, "-d", out, "-g", "0",
                        "-n", "4", "-e", "[recon,pred]"], cwd=str(program["dir"]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    text = r.stdout
    valid_dir, train_dir = os.path.join(out, "valid_" + name), os.path.join(out, "train_" + name)
    assert os.path.exists(os.path.join(valid_dir, "z_iter_%d.txt" % iteration))
    assert open(os.path.join(valid_dir, "z_iter_%d.txt" % iteration)).read() == str(iteration)
    saved = re.findall(r"^saved: (.*)$", text, flags=re.M)
    lines = re.findall(r"^(\S+) GT:      ", text, flags=re.M)
    assert len(lines) >= 8 and len(saved) == len(lines)             # two batches of each split, at least two lines each
    # (an author's left-over line is handed out twice by the loader: a name may repeat, its picture is written again)
    on_disk = {os.path.join(d, f) for d in (valid_dir, train_dir) for f in os.listdir(d) if f.endswith(".png")}
    assert on_disk == set(saved) and {os.path.basename(p) for p in saved} == {"%s_recon.png" % n for n in lines}
    assert not [f for d in (valid_dir, train_dir) for f in os.listdir(d) if ".tmp" in f]
    assert any(f.endswith(".png") for f in os.listdir(valid_dir)) and any(f.endswith(".png") for f in os.listdir(train_dir))
    for path in saved:
        mode, px = _png(path)
        assert mode == "RGB" and px.shape[0] == 2 * H + 52 and px.shape[2] == 3
        top, bottom = px[0], px[2 * H + 1]
        first_top, first_bottom = int(np.flatnonzero(top.any(axis=1))[0]), int(np.flatnonzero(bottom.any(axis=1))[0])
        assert tuple(top[first_top]) == (0, 255, 0) and tuple(bottom[first_bottom]) == (0, 0, 255)
        assert min(first_top, first_bottom) == 0                      # the wider of the two starts at the picture's left edge
        assert not px[H, :first_top].any() and tuple(px[H, first_top]) == (0, 255, 0) and tuple(px[H + 1, first_bottom]) == (0, 0, 255)
    assert "valid metrics" in text
    number = r"[-+0-9.e]+|nan"
    assert re.search(r"^cer overall mean: (%s), std (%s)$" % (number, number), text, flags=re.M), text[-1500:]
    assert re.search(r"^wer overall mean: (%s), std (%s)$" % (number, number), text, flags=re.M)
    assert text.index("valid metrics") > max(text.rindex("saved: "), text.rindex(" pred:    "))


def test_pictures_scores_and_files_in_process(cuda, program, capsys):
    from handwriting_line_generation_amd import evaluate, ops
    from handwriting_line_generation_amd.data.author_hw_dataset import getDataLoader
    from handwriting_line_generation_amd.generate import load_for_generation
    import new_eval
    ckpt, cfg, name, iteration = program["gan"]
    d = program["dir"]
    out, preds, style = str(d / "inproc"), str(d / "preds.csv"), str(d / "styles.pkl")
    argv = ["-c", ckpt, "-f", cfg, "-d", out, "-g", "0", "-n", "4", "-v", "1", "-e", "[recon,pred]",
            "-a", "by_author,save_preds=%s,save_style=%s" % (preds, style)]
    text, hooked = _main(argv, capsys)
    dirs = [os.path.join(out, "valid_" + name), os.path.join(out, "train_" + name)]
    seen = _check_pair_pictures(hooked)
    on_disk = {os.path.join(p, f) for p in dirs for f in os.listdir(p) if f.endswith(".png")}
    assert seen == on_disk and len(seen) >= 6
    assert [t["outDir"] for _, t in hooked.of("recon")] == dirs * 2
    for names, t in hooked.of("recon"):                                  # captions: the reference's text, through the atlas' codes
        assert all(re.fullmatch(r"CER: \d+\.\d{3}, T: .*", c) for c in t["captions"]) and len(t["codes"]) == len(names)
        assert t["pictures"].shape[1] == 2 * H + 52 and t["atlas"].shape[0] >= 95
    # scores: the host path on the hooked predictions
    idx_to_char = _iam_idx_to_char()
    batches = []                                                          # (names, gt, cer, strings) per scored batch: valid, train, valid, train
    for names, t in hooked.of("pred"):
        c, w, s = ops.host_error_rates(t["pred"], t["gt"], idx_to_char, True)
        batches.append((names, t["gt"], c, s))
    assert len(batches) == 4
    all_names = [n for bt in batches for n in bt[0]]
    gts = [g for bt in batches for g in bt[1]]
    cers = [c for bt in batches for c in bt[2]]
    strs = [s for bt in batches for s in bt[3]]
    assert re.findall(r"^(\S+) pred:    (.*)$", text, flags=re.M) == list(zip(all_names, strs))
    assert re.findall(r"^(\S+) GT:      (.*)$", text, flags=re.M) == list(zip(all_names, gts))
    assert len(re.findall(r"^(\S+) aligned: (.*)$", text, flags=re.M)) == len(all_names)
    assert "[[" not in text                                               # the raw prediction arrays are printed at -v 3 only
    for (names, t), bt in zip(hooked.of("recon"), batches):
        assert names == bt[0] and t["captions"] == ["CER: {:.3f}, T: {}".format(c, s) for c, s in zip(bt[2], bt[3])]
    # save_preds: the training batches
    rows = list(csv.reader(open(preds)))
    want_rows = [[n, g, s, str(c)] for k, bt in enumerate(batches) if k % 2 == 1 for n, g, c, s in zip(*bt)]
    assert rows == want_rows and len(rows) >= 4
    # by_author: a list per writer of the validation split, and the overall numbers in the reference's format
    prepared = new_eval.prepare_config(json.load(open(cfg)), new_eval.parse_args(["-c", ckpt]))
    train_loader, valid_loader = getDataLoader(prepared, "train")
    valid_authors = [a for k, inst in enumerate(valid_loader) if k < 2 for a in inst["author"]]
    valid_cers = [c for k, bt in enumerate(batches) if k % 2 == 0 for c in bt[2]]
    assert len(valid_cers) == len(valid_authors)
    for author in set(valid_authors):
        mine = [c for c, a in zip(valid_cers, valid_authors) if a == author]
        assert "cer_{} overall mean: {}, std {}".format(author, np.mean(mine, axis=0), np.std(mine, axis=0)) in text
    batch_means = []
    for k, bt in enumerate(batches):
        if k % 2 == 0:
            total = 0
            for c in bt[2]:
                total += c
            batch_means.append(total / len(bt[2]))
    assert "cer overall mean: {}, std {}".format(np.mean(batch_means, axis=0), np.std(batch_means, axis=0)) in text
    # save_style: what evaluate.extract_styles gives on the same loaders, the batches that were run
    model, _, _ = load_for_generation(ckpt, cfg, gpu=0)
    for loc, loader in ((style + ".%d" % len(train_loader), train_loader), (os.path.join(str(d), "val_styles.pkl") + ".%d" % len(valid_loader), valid_loader)):
        got = pickle.load(open(loc, "rb"))
        assert set(got) == {"styles", "authors"}
        want = evaluate.extract_styles(model, loader, cuda)
        n = len(got["authors"])
        assert n >= 4 and list(got["authors"]) == list(want["authors"][:n])
        assert got["styles"].dtype == np.float32 and np.array_equal(got["styles"], want["styles"][:n])

    # cer_thresh: lines below it get no picture, the others their CER in front of the name
    thresh = max(cers)                                                    # (the reduced checkpoint reads little: most lines sit at one value)
    out2 = str(d / "thresh")
    text2, hooked2 = _main(["-c", ckpt, "-f", cfg, "-d", out2, "-g", "0", "-n", "4", "-v", "1", "-e", "[recon,pred]", "-a", "cer_thresh=%r" % thresh], capsys)
    dirs2 = [os.path.join(out2, "valid_" + name), os.path.join(out2, "train_" + name)]
    seen2 = _check_pair_pictures(hooked2, prefixed=True)
    want2 = {os.path.join(dirs2[k % 2], "{:.3f}_{}_recon.png".format(c, n)) for k, bt in enumerate(batches) for n, c in zip(bt[0], bt[2]) if not c < thresh}
    assert seen2 == want2 and want2
    assert {os.path.join(p, f) for p in dirs2 for f in os.listdir(p) if f.endswith(".png")} == want2
    for names, t in hooked2.of("recon"):
        assert t["image"].shape[0] == len(names) == len(t["lines"])
    n_below = sum(c < thresh for c in cers)
    assert sum(len(names) for names, _ in hooked2.of("recon")) == len(cers) - n_below
    # ... and above every line's CER nothing is composed and nothing written, while every line is still scored
    out3 = str(d / "thresh_all")
    text3, hooked3 = _main(["-c", ckpt, "-f", cfg, "-d", out3, "-g", "0", "-n", "4", "-v", "1", "-e", "[recon,pred]", "-a", "cer_thresh=%r" % (thresh + 1.0)], capsys)
    assert not hooked3.of("recon") and len(hooked3.of("pred")) == 4 and "saved: " not in text3
    assert not [f for sub in os.listdir(out3) for f in os.listdir(os.path.join(out3, sub)) if f.endswith(".png")]
    assert re.findall(r"^(\S+) pred:    (.*)$", text3, flags=re.M) == list(zip(all_names, strs))


def test_run_gen_on_device(cuda, program):
    import new_eval
    from handwriting_line_generation_amd import rng
    ckpt, cfg, name, iteration = program["gan"]
    config, trainer, train_loader, valid_loader, to_eval, _ = new_eval.setup(new_eval.parse_args(["-c", ckpt, "-f", cfg, "-v", "1"]))
    assert to_eval == ["recon", "pred"]
    instance = next(iter(valid_loader))
    get = ["recon", "pred", "style", "gen", "spaced_label", "name", "author", "gt"]
    runs = []
    try:
        with torch.no_grad():
            for on_device in (False, True):
                rng.set_mode("device", seed=5)
                torch.manual_seed(0); np.random.seed(0)
                losses, got = trainer.run_gen(dict(instance), trainer.curriculum.getEval(), list(get), **({"on_device": True} if on_device else {}))
                runs.append(got)
    finally:
        rng.set_mode("device")
    host, dev = runs
    for k in ("recon", "pred", "style", "gen", "spaced_label"):
        assert not host[k].is_cuda and dev[k].is_cuda and not dev[k].requires_grad
        assert torch.equal(dev[k].cpu(), host[k]), k
    assert host["spaced_label"].dtype == torch.int64 and host["spaced_label"].shape[1] == len(instance["gt"])
    assert host["name"] == dev["name"] == instance["name"] and host["author"] == instance["author"] and host["gt"] == instance["gt"]
    with pytest.raises(ValueError, match="Unknown get"):
        with torch.no_grad():
            trainer.run_gen(dict(instance), trainer.curriculum.getEval(), ["recon", "nothing"])


def test_gen_alone(cuda, program, capsys):
    ckpt, cfg, name, iteration = program["gan"]
    out = str(program["dir"] / "gen")
    text, hooked = _main(["-c", ckpt, "-f", cfg, "-d", out, "-g", "0", "-n", "2", "-v", "1", "-e", "[gen]"], capsys)
    dirs = [os.path.join(out, "valid_" + name), os.path.join(out, "train_" + name)]
    assert not hooked.of("recon") and not hooked.of("pred") and len(hooked.of("gen")) == 2
    files = sorted(f for p in dirs for f in os.listdir(p) if f.endswith(".png"))
    assert files and not [f for f in files if f.endswith("_recon.png")]
    want_files = []
    for (names, t), p in zip(hooked.of("gen"), dirs):
        x = t["gen"]
        want = np.clip((np.float32(1) - x) * np.float32(127.5), 0, 255).astype(np.uint8)[:, 0]      # lines_to_u8's arithmetic
        for b, n in enumerate(names):
            mode, px = _png(os.path.join(p, "gen_%s.png" % n))
            assert mode == "L" and np.array_equal(px, want[b])
            want_files.append("gen_%s.png" % n)
    assert files == sorted(want_files)
    assert " pred:    " not in text and "valid metrics" in text


def test_recogniser_and_autoencoder_checkpoints(cuda, program, capsys):
    from handwriting_line_generation_amd import ops
    idx_to_char = _iam_idx_to_char()
    # recogniser pre-training: run_hwr, scores, no pictures
    ckpt, cfg, name, iteration = program["hwr"]
    out = str(program["dir"] / "hwr_out")
    text, hooked = _main(["-c", ckpt, "-f", cfg, "-d", out, "-g", "0", "-n", "4", "-v", "1"], capsys)
    dirs = [os.path.join(out, "valid_" + name), os.path.join(out, "train_" + name)]
    assert sorted(f for p in dirs for f in os.listdir(p)) == ["z_iter_%d.txt" % iteration]
    assert not hooked.of("recon") and len(hooked.of("pred")) == 4
    strs = [s for names, t in hooked.of("pred") for s in ops.host_error_rates(t["pred"], t["gt"], idx_to_char, True)[2]]
    assert [s for _, s in re.findall(r"^(\S+) pred:    (.*)$", text, flags=re.M)] == strs
    assert re.search(r"^cer overall mean: \S+, std \S+$", text, flags=re.M) and re.search(r"^recogLoss overall mean: \S+, std \S+$", text, flags=re.M)
    # autoencoder: pair pictures through AutoTrainer, no strip without `pred`
    ckpt, cfg, name, iteration = program["auto"]
    out = str(program["dir"] / "auto_out")
    text, hooked = _main(["-c", ckpt, "-f", cfg, "-d", out, "-g", "0", "-n", "2", "-v", "1", "-e", "[recon]"], capsys)
    dirs = [os.path.join(out, "valid_" + name), os.path.join(out, "train_" + name)]
    seen = _check_pair_pictures(hooked)
    assert len(seen) >= 2 and {os.path.dirname(p) for p in seen} == set(dirs) and not hooked.of("pred") and " pred:    " not in text
    for names, t in hooked.of("recon"):
        assert t["captions"] is None and t["codes"] is None and t["pictures"].shape[1] == 2 * H + 2
