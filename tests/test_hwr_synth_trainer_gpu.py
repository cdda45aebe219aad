"""GPU: HWRWithSynthTrainer - recogniser training on real lines from a (fabricated) IAM directory plus lines generated on the device by the
REFERENCE-written (width-reduced) GAN checkpoint tests/golden/ref_ckpt_gan.pth.xz. As in test_generate_cli_gpu.py the checkpoint is read
through a copy in which only spacer.mean / spacer.std are replaced (the original's spacer predicts empty lines)."""
import json
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from _reference_checkpoint import unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_CFG = "cf_IAM_hwr_cnnOnly_batchnorm_aug_synth.json"
H = 64
TEXT = """the quick brown fox
jumps over the lazy dog
a line of text
hello world
some more words here
and yet another one
short
handwriting lines
generated on the device
never leave it
mixed with real ones
a dozen short lines
"""


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    """-> dict(dir, iam, synth): a fabricated IAM directory and the `trainer.synth` block (spread generator checkpoint, style file, text file)"""
    from handwriting_line_generation_amd.logger import load_checkpoint
    from oracle import collate_items
    d = tmp_path_factory.mktemp("synth_world")
    iam = os.path.join(str(d), "iam")
    os.makedirs(iam)
    collate_items.fake_iam(iam, n_pages=6, with_images=True)
    ck = load_checkpoint(unpack("gan", d))
    ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
    ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
    gen = os.path.join(str(d), "spread.pth")
    torch.save(ck, gen)
    styles = os.path.join(str(d), "train_styles_")
    with open(styles + "25000.pkl", "wb") as f:
        pickle.dump({"authors": ["000", "000", "017", "230", "230", "017"],
                     "styles": torch.randn(6, 128, generator=torch.Generator().manual_seed(1)).numpy()}, f)
    text = os.path.join(str(d), "text.txt")
    open(text, "w").write(TEXT)
    synth = dict(checkpoint=gen, styles=styles, text_data=text, per_batch=2, pool=4, gen_batch=3, seed=11, max_len=8, max_width=None, spacing_noise=False)
    return {"dir": str(d), "iam": iam, "synth": synth}


def _config(world, save_dir, augmentation=None, **synth):
    from handwriting_line_generation_amd.harness import CHAR_FILES
    cfg = json.load(open(os.path.join(ROOT, "configs", BASE_CFG)))
    cfg["data_loader"].update(data_dir=world["iam"], batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"], augmentation=augmentation)
    cfg["validation"].update(batch_size=2, num_workers=0)
    cfg["trainer"].update(save_dir=str(save_dir), save_step=10 ** 6, save_step_minor=10 ** 6, log_step=10 ** 6, val_step=10 ** 6, iterations=3)
    cfg["trainer"]["synth"] = dict(world["synth"], **synth)
    cfg["seed"] = 5
    cfg["cuda"], cfg["gpu"] = True, 0
    return cfg


def _trainer(cfg, cls=None):
    from handwriting_line_generation_amd import model as M, rng, trainer as T
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.model import loss as loss_fns
    rng.seed_process(cfg["seed"])
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    loader, vloader = D.getDataLoader(cfg, "train")
    model = M.HWWithStyle(cfg["model"])
    losses = {k: getattr(loss_fns, v) for k, v in cfg["loss"].items()}
    return (cls or getattr(T, cfg["trainer"]["class"]))(model, losses, [], None, cfg, loader, vloader, None)


def _levels(p):
    return np.float32(1.0) - p.astype(np.float32) / np.float32(128.0)


def test_pool_holds_the_bytes_generate_py_writes(cuda, world):
    """process seeded identically: the pool's bytes for its (texts, styles) are render_lines' output for the same arguments"""
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.data.synth_lines import SynthLinePool
    from handwriting_line_generation_amd.generate import render_lines
    from handwriting_line_generation_amd.harness import CHAR_FILES
    cti = json.load(open(CHAR_FILES["iam"]))["char_to_idx"]
    try:
        rng.seed_process(7)
        pool = SynthLinePool(dict(world["synth"], pool=7), cti, gpu=0)
        assert pool.model.hwr is None and pool.model.style_extractor is None and not pool.model.training
        std = (pool.model.count_std, pool.model.dup_std)
        pool.refill(0)
        torch.cuda.synchronize()
        assert (pool.model.count_std, pool.model.dup_std) == std and pool.pixels.is_cuda and pool.pixels.dtype == torch.uint8
        host = pool.pixels.cpu().numpy()
        rng.seed_process(7)
        want = dict(render_lines(pool.model, pool.drawn_texts, torch.from_numpy(pool.drawn_styles), pool.gen_char_to_idx, cuda, batch_lines=3))
        assert len(pool.ids) == 7 and sorted(want) == sorted(pool.ids)
        for j, i in enumerate(pool.ids):
            w = int(pool.widths[j])
            line = host[pool.offsets[j]:pool.offsets[j] + H * w].reshape(H, w)
            assert line.shape == want[i].shape and np.array_equal(line, want[i]), i
            assert pool.texts[j] == pool.drawn_texts[i]
        assert len({int(w) for w in pool.widths}) > 1 and min(pool.widths) >= 8          # real, different lines
    finally:
        rng.set_mode("device")


def _run_three(world, tmp_path, tag, **trainer_keys):
    """three iterations at batch_size 2, per_batch 2, pool 4 (a refill at the third), no augmentation -> what run_hwr was handed, what the
    loader and the pool handed out, the logs and the trainer"""
    cfg = _config(world, tmp_path / ("saved_" + tag))
    cfg["trainer"].update(trainer_keys)
    trainer = _trainer(cfg)
    pool = trainer.pool
    real, drawn, consumed = [], [], []

    def rec(items, _orig=trainer.data_loader._collate):
        inst = _orig(items)
        real.append({k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in inst.items()})
        return inst
    trainer.data_loader._collate = rec
    trainer.data_loader_iter = iter(trainer.data_loader)          # (the constructor's iterator was built around the unhooked collate)
    draw = pool.draw

    def draw_rec(n):
        idx = draw(n)
        px = pool.pixels.cpu().numpy()
        drawn.append([(px[pool.offsets[i]:pool.offsets[i] + H * pool.widths[i]].reshape(H, pool.widths[i]).copy(), pool.texts[i], pool.labels[i],
                       pool.name(i)) for i in idx])
        return idx
    pool.draw = draw_rec
    run_hwr = trainer.run_hwr

    def run_rec(instance):
        consumed.append(dict(instance, image=instance["image"].cpu()))
        return run_hwr(instance)
    trainer.run_hwr = run_rec
    gen_before = {k: v.clone() for k, v in pool.model.state_dict().items()}
    hwr_before = {k: v.clone() for k, v in trainer.model.state_dict().items()}
    logs = [trainer._train_iteration(it) for it in range(1, 4)]
    logs.append(trainer.flush_log())
    torch.cuda.synchronize()
    return dict(trainer=trainer, pool=pool, real=real, drawn=drawn, consumed=consumed, logs=logs, gen_before=gen_before, hwr_before=hwr_before)


def test_three_iterations_mix_real_and_generated_lines(cuda, world, tmp_path):
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.data.hw_dataset import collate
    from handwriting_line_generation_amd.data.synth_lines import SYNTH_AUTHOR
    try:
        r = _run_three(world, tmp_path, "host_cer")
        trainer, pool = r["trainer"], r["pool"]
        assert type(trainer).__name__ == "HWRWithSynthTrainer" and pool.refills == [0, 1]          # pool 4 / per_batch 2: a refill at the third
        assert len(r["consumed"]) == len(r["real"]) == len(r["drawn"]) == 3
        seen = set()
        for inst, real, drawn in zip(r["consumed"], r["real"], r["drawn"]):
            Br, Wr = real["image"].shape[0], real["image"].shape[3]
            assert Br == 2 and len(drawn) == 2
            image = inst["image"].numpy()
            W = -(-max([Wr] + [l.shape[1] for l, _, _, _ in drawn]) // 4) * 4
            want = np.full((4, 1, H, W), -1.0, dtype=np.float32)
            want[:2, :, :, :Wr] = real["image"].numpy()
            for j, (line, _, _, _) in enumerate(drawn):
                want[2 + j, 0, :, :line.shape[1]] = _levels(line)
            assert image.shape == want.shape and np.array_equal(image.view(np.int32), want.view(np.int32))
            # labels and the rest: `collate` of the real batch's items followed by one item per generated line
            items = [{"image": np.zeros((H, 4, 1), np.float32), "gt": real["gt"][b], "gt_label": real["label"][:int(real["label_lengths"][b]), b].numpy(),
                      "name": real["name"][b], "center": False, "author": real["author"][b]} for b in range(Br)]
            items += [{"image": np.zeros((H, 4, 1), np.float32), "gt": t, "gt_label": l, "name": n, "center": False, "author": SYNTH_AUTHOR}
                      for _, t, l, n in drawn]
            ref = collate(items)
            assert torch.equal(inst["label"], ref["label"]) and inst["label"].dtype == torch.int32
            assert inst["label_lengths"].tolist() == ref["label_lengths"].tolist()
            assert inst["gt"] == ref["gt"] and inst["name"] == ref["name"] and inst["author"] == ref["author"]
            assert all(n.startswith("synth_") for n in inst["name"][2:]) and not seen & set(inst["name"][2:])
            seen |= set(inst["name"][2:])
        for log in r["logs"][:3]:
            assert log and all(np.isfinite(v) for v in log.values()) and "recogLoss" in log and "CER" in log, log
        after = trainer.model.state_dict()
        assert all(k.startswith("hwr.") for k in after)
        moved = sum(1 for k, v in after.items() if v.dtype.is_floating_point and not torch.equal(v, r["hwr_before"][k]))
        assert moved > 10
        # the generator: bit-unchanged, no gradient anywhere, in no optimizer
        gen_after = pool.model.state_dict()
        assert set(gen_after) == set(r["gen_before"]) and all(torch.equal(v, r["gen_before"][k]) for k, v in gen_after.items())
        assert all(p.grad is None and not p.requires_grad for p in pool.model.parameters()) and not pool.model.training
        mine = {p.data_ptr() for p in trainer.model.parameters()}
        assert not mine & {p.data_ptr() for p in pool.model.parameters()}
        # CER / WER counted on the device: the same logs
        r2 = _run_three(world, tmp_path, "device_cer", device_cer=True)
        assert r2["logs"][:3] == r["logs"][:3]
        # pipelined logging: the same values, one iteration late
        r3 = _run_three(world, tmp_path, "async", device_cer=True, async_log=1)
        assert r3["logs"][0] == {} and r3["logs"][1:] == r["logs"][:3]
    finally:
        rng.set_mode("device")


def test_mixed_batch_is_augmented_once_with_the_loaders_variant(cuda, world, tmp_path):
    """the shipped `augmentation: true`: the trainer reads the un-augmented inner loader and augments the mixed batch - padding stays exactly
    -1 outside every row's own extent (real: line_extents, generated: the pool's widths), pixels stay on the 256-level grid and change"""
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.data.device_augment import DeviceAugment
    try:
        trainer = _trainer(_config(world, tmp_path / "saved", augmentation=True))
        assert isinstance(trainer._augment, DeviceAugment) and not isinstance(trainer.data_loader, DeviceAugment)
        assert isinstance(trainer.valid_data_loader, DeviceAugment)                     # validation: real lines only, as before
        plain, consumed, widths = [], [], []

        def rec(items, _orig=trainer.data_loader._collate):
            inst = _orig(items)
            plain.append(inst["image"].clone())
            return inst
        trainer.data_loader._collate = rec
        trainer.data_loader_iter = iter(trainer.data_loader)
        run_hwr, draw = trainer.run_hwr, trainer.pool.draw

        def draw_rec(n):
            idx = draw(n)
            widths.append([int(trainer.pool.widths[i]) for i in idx])
            return idx
        trainer.pool.draw = draw_rec

        def run_rec(instance):
            consumed.append(instance["image"].cpu())
            return run_hwr(instance)
        trainer.run_hwr = run_rec
        offset0 = rng.device_rng().offset
        for it in range(1, 3):
            log = trainer._train_iteration(it)
            assert log and all(np.isfinite(v) for v in log.values()), log
        torch.cuda.synchronize()
        assert rng.device_rng().offset > offset0 and len(consumed) == len(plain) == len(widths) == 2
        for got, src, w in zip(consumed, plain, widths):
            assert got.shape[0] == 4 and got.shape[3] % 4 == 0 and got.shape[3] >= max([src.shape[3]] + w)
            pad = torch.ones(got.shape, dtype=torch.bool)
            pad[:2, :, :, :src.shape[3]] = src == -1
            for j, wj in enumerate(w):
                pad[2 + j, :, :, :wj] = False
            assert torch.equal(got == -1, pad)
            k = (1.0 - got[~pad].double()) * 128.0
            assert torch.equal(k, k.round()) and float(k.min()) >= 0 and float(k.max()) <= 255
        val = trainer._valid_epoch()
        assert val and all(np.isfinite(v) for v in val.values()) and "val_CER" in val, val
    finally:
        rng.set_mode("device")


def test_per_batch_zero_is_the_pretraining_trainer_bit_for_bit(cuda, world, tmp_path):
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.trainer import HWRWithSynthTrainer, HWWithStyleTrainer
    try:
        out = []
        for cls in (HWRWithSynthTrainer, HWWithStyleTrainer):
            cfg = _config(world, tmp_path / cls.__name__, augmentation=True, per_batch=0, checkpoint="/nowhere/gen.pth")
            trainer = _trainer(cfg, cls)
            if cls is HWRWithSynthTrainer:
                assert trainer.pool is None
            logs = [trainer._train_iteration(it) for it in range(1, 4)]
            torch.cuda.synchronize()
            out.append((logs, {k: v.cpu() for k, v in trainer.model.state_dict().items()}, rng.device_rng().offset))
        (logs_a, sd_a, off_a), (logs_b, sd_b, off_b) = out
        assert logs_a == logs_b and off_a == off_b and set(sd_a) == set(sd_b)
        assert all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    finally:
        rng.set_mode("device")


def test_train_cli_saves_a_recogniser_checkpoint_and_resumes(cuda, world, tmp_path):
    """`train.py -c <cfg>` as a child process: the checkpoint holds the recogniser's keys alone and loads through model.pretrained_hwr; a -r
    resume runs one more step"""
    from handwriting_line_generation_amd.logger import load_checkpoint
    from handwriting_line_generation_amd.model import HWWithStyle
    cfg = _config(world, tmp_path / "saved", augmentation=True)
    cfg["trainer"].update(save_step=3, save_step_minor=1, iterations=3)
    path = str(tmp_path / BASE_CFG)
    json.dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(args):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        return r.stdout + r.stderr
    out = run(["-c", path])
    ckdir = os.path.join(cfg["trainer"]["save_dir"], cfg["name"])
    first = os.path.join(ckdir, "checkpoint-iteration3.pth")
    assert os.path.exists(first), out[-2000:]
    ck = load_checkpoint(first)
    assert ck["iteration"] == 3 and ck["arch"] == "HWWithStyle" and ck["config"]["trainer"]["class"] == "HWRWithSynthTrainer"
    assert ck["state_dict"] and all(k.startswith("hwr.") for k in ck["state_dict"])
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.dtype.is_floating_point)
    gan_model = dict(ck["config"]["model"], pretrained_hwr=first)                      # what a GAN config's model.pretrained_hwr does with it
    loaded = HWWithStyle(gan_model).state_dict()
    assert all(torch.equal(loaded[k], v) for k, v in ck["state_dict"].items())
    out2 = run(["-r", first, "--iterations", "4"])
    ck2 = load_checkpoint(os.path.join(ckdir, "checkpoint-latest.pth"))               # (save_step_minor 1: written behind every iteration)
    assert ck2["iteration"] == 4 and all(k.startswith("hwr.") for k in ck2["state_dict"])
    assert sum(1 for k, v in ck2["state_dict"].items() if v.dtype.is_floating_point and not torch.equal(v, ck["state_dict"][k])) > 10
    assert ck2["rng"]["offset"] > ck["rng"]["offset"]
    # pool 4, per_batch 2: the first run rendered pools 0 and 1; behind 3 iterations the resumed run starts with pool 3 * 2 // 4 = 1
    assert "pool 0:" in out and "pool 1:" in out and "pool 2:" not in out
    assert "pool 1:" in out2 and "pool 0:" not in out2 and "pool 2:" not in out2
