"""GPU: weight averaging (trainer.swa, reference base/base_trainer.py:180-186, 233-237, 287-297, 362-366, 441-442) through
BaseTrainer.train() of the width-reduced GAN set-up the reference-checkpoint tests build (tests/golden/ref_ckpt_reduced_model.json, two
128-pixel lines per batch): schedule, the `swa_`-prefixed validation entries, `swa_state_dict` in every checkpoint, resume, and
generate.load_for_generation(averaged=True).

Three runs are made once for the whole module: A (averaging on, iterations 1..6), B (the same run with averaging off) and R (a trainer
resumed from A's checkpoint of iteration 4, run to iteration 6). A checkpoint keeps the weights, both optimizers and the device generator;
what else a run's future depends on lives on the host and is handed to R by the fixture as A had it behind iteration 4: the position of the
training loader, the three host generators (torch, numpy, random) and the trainer's bank of earlier styles (the conditions under which a
resumed run of this trainer continues the uninterrupted one; the curriculum below adds the last one)."""
import json
import os
import random

import numpy as np
import pytest
import torch

from _reference_checkpoint import GOLD

pytestmark = pytest.mark.gpu

SWA = {"swa": True, "swa_start": 2, "swa_c_iters": 2}
# Lesson of iteration i is CURRICULUM[i % 6]: count, disc, no-step gen, auto + auto-gen, disc, auto + auto-gen - every kind of lesson of the shipped
# curriculum, with the stepping lessons on the saved iterations 2, 4 and 6. A "no-step" lesson leaves its gradients (the trainer's stashed
# sets) for the lesson behind it, and a checkpoint does not hold them: neither here nor in the reference does a run resumed between the two
# continue the uninterrupted one.
CURRICULUM = [["auto", "auto-gen"], ["count"], ["disc"], ["no-step", "gen"], ["auto", "auto-gen"], ["disc"]]


def _counting_dataset(first, *args, **kwargs):
    """SyntheticAuthorDataset that starts `first` batches in and counts the batches it hands out (`.calls`)"""
    from handwriting_line_generation_amd.data.synthetic import SyntheticAuthorDataset

    class Counting(SyntheticAuthorDataset):
        calls = 0

        def batch(self, step):
            self.calls += 1
            return super().batch(step + first)
    return Counting(*args, **kwargs)


def _trainer(workdir, extra, resume=None, first_batch=0):
    from handwriting_line_generation_amd import harness
    from handwriting_line_generation_amd.data.synthetic import SyntheticAuthorDataset, SyntheticLoader
    from handwriting_line_generation_amd.logger import Logger
    from handwriting_line_generation_amd.model import Autoencoder, HWWithStyle
    from handwriting_line_generation_amd.model import loss as loss_fns
    from handwriting_line_generation_amd.trainer import HWWithStyleTrainer
    os.makedirs(workdir, exist_ok=True)
    cfg, _ = harness.synthetic_gan_config("iam_gan", 1, 2, workdir=workdir)
    cfg["model"].update(json.load(open(os.path.join(GOLD, "ref_ckpt_reduced_model.json"))))
    tr = cfg["trainer"]
    tr.update(iterations=6, save_step=2, val_step=2, log_step=1, save_step_minor=None)
    tr["curriculum"] = {"0": CURRICULUM}
    tr.update(extra)
    dl = cfg["data_loader"]
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    if not os.path.exists(tr["encoder_weights"]):
        ae = Autoencoder({"type": tr.get("encoder_type", "2tight"), "hwr": cfg["model"]["num_class"]})
        torch.save({"state_dict": ae.state_dict()}, tr["encoder_weights"])
    model = HWWithStyle(cfg["model"])
    ds = _counting_dataset(first_batch, dl["char_file"], 1, 2, width=128, label_len=6)
    vds = SyntheticAuthorDataset(dl["char_file"], 1, 2, width=128, label_len=6, num_batches=1, seed=900)
    losses = {name: getattr(loss_fns, fn) for name, fn in cfg["loss"].items()}
    return HWWithStyleTrainer(model, losses, [], resume, cfg, SyntheticLoader(ds), SyntheticLoader(vds), Logger()), cfg


def _run(workdir, extra, snapshot_at=None):
    """a fresh run of six iterations -> (trainer, checkpoint directory, host state behind iteration `snapshot_at`)"""
    from handwriting_line_generation_amd import rng
    rng.set_mode("device", seed=5)
    trainer, cfg = _trainer(workdir, extra)
    torch.manual_seed(1); np.random.seed(1); random.seed(1)
    host = {}
    save = trainer._save_checkpoint

    def save_and_snapshot(iteration, *a, **k):
        if iteration == snapshot_at:
            host.update(torch=torch.get_rng_state(), numpy=np.random.get_state(), random=random.getstate(),
                        batches=trainer.data_loader.dataset.calls, prev_styles=[s.clone() for s in trainer.prev_styles])
        return save(iteration, *a, **k)
    trainer._save_checkpoint = save_and_snapshot
    trainer.train()
    torch.cuda.synchronize()
    return trainer, os.path.join(cfg["trainer"]["save_dir"], cfg["name"]), host


@pytest.fixture(scope="module")
def runs(cuda, tmp_path_factory):
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.logger import load_checkpoint
    root = tmp_path_factory.mktemp("swa_runs")
    try:
        a, dir_a, host = _run(str(root / "a"), SWA, snapshot_at=4)
        live_a = {k: v.detach().cpu().clone() for k, v in a.model.state_dict().items()}
        b, dir_b, _ = _run(str(root / "b"), {})
        live_b = {k: v.detach().cpu().clone() for k, v in b.model.state_dict().items()}
        # R: resumed behind iteration 4 into another directory, the host-side state put where A had it
        r, cfg_r = _trainer(str(root / "r"), SWA, resume=os.path.join(dir_a, "checkpoint-iteration4.pth"), first_batch=host["batches"])
        assert r.start_iteration == 5 and r.flat.avg is not None
        r.prev_styles = [s.clone() for s in host["prev_styles"]]
        torch.set_rng_state(host["torch"]); np.random.set_state(host["numpy"]); random.setstate(host["random"])
        r.train()
        torch.cuda.synchronize()
        dir_r = os.path.join(cfg_r["trainer"]["save_dir"], cfg_r["name"])
        out = {"a": a, "dir_a": dir_a, "dir_b": dir_b, "live_a": live_a, "live_b": live_b,
               "ck_a": {i: load_checkpoint(os.path.join(dir_a, "checkpoint-iteration%d.pth" % i)) for i in (2, 4, 6)},
               "ck_b6": load_checkpoint(os.path.join(dir_b, "checkpoint-iteration6.pth")),
               "ck_r6": load_checkpoint(os.path.join(dir_r, "checkpoint-iteration6.pth"))}
        return out
    finally:
        rng.set_mode("device")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_full_run_writes_the_running_mean_and_does_not_perturb_training(runs):
    ck = runs["ck_a"]
    param_keys = {n for n, _ in runs["a"].model.named_parameters(remove_duplicate=False)}      # (generator blocks are registered under two names)
    for i in (2, 4, 6):
        assert "swa_state_dict" in ck[i] and set(ck[i]["swa_state_dict"]) == set(ck[i]["state_dict"]), i
    assert "swa_state_dict" not in runs["ck_b6"]
    # the reference's recurrence (moving_average, alpha = 1 / (n + 1)) over the three checkpoints' own weights, on the CPU
    moved = 0
    for k in sorted(param_keys):
        avg = torch.zeros_like(ck[2]["state_dict"][k])
        for n, i in enumerate((2, 4, 6)):
            alpha = 1.0 / (n + 1)
            avg *= (1.0 - alpha)
            avg += ck[i]["state_dict"][k] * alpha
        assert torch.equal(_bits(ck[6]["swa_state_dict"][k]), _bits(avg)), k
        moved += int(not torch.equal(ck[6]["swa_state_dict"][k], ck[6]["state_dict"][k]))
    assert moved > 100                                                   # (the frozen recogniser's mean is the recogniser)
    buffer_keys = set(ck[6]["state_dict"]) - param_keys
    assert buffer_keys
    for k in buffer_keys:
        assert torch.equal(ck[6]["swa_state_dict"][k], ck[6]["state_dict"][k]), k
    # the training log: every validated iteration from swa_start on carries the averaged model's validation next to the live one's
    entries = {e["iteration"]: e for e in runs["a"].train_logger.entries.values() if any(k.startswith("swa_") for k in e)}
    assert sorted(entries) == [2, 4, 6]
    for e in entries.values():
        val = {k for k in e if k.startswith("val_")}
        assert val and {"swa_" + k for k in val} == {k for k in e if k.startswith("swa_")}
        assert all(np.isfinite(e[k]) for k in e)
    assert entries[2]["swa_val_loss"] == entries[2]["val_loss"]          # the first snapshot IS the live model (same weights, same noise)
    # averaging does not perturb training: the live weights are those of the run without it, bit for bit
    assert set(runs["live_a"]) == set(runs["live_b"])
    for k, v in runs["live_a"].items():
        assert torch.equal(_bits(v), _bits(runs["live_b"][k])), k
        assert torch.equal(_bits(v), _bits(ck[6]["state_dict"][k])), k


def test_resumed_run_continues_the_same_average(runs):
    want, got = runs["ck_a"][6], runs["ck_r6"]
    assert got["iteration"] == 6 and set(got["swa_state_dict"]) == set(want["swa_state_dict"])
    for k, v in want["state_dict"].items():
        assert torch.equal(_bits(got["state_dict"][k]), _bits(v)), "live %s: the resumed run is not the uninterrupted one" % k
    for k, v in want["swa_state_dict"].items():
        assert torch.equal(_bits(got["swa_state_dict"][k]), _bits(v)), k


def test_load_for_generation_averaged(runs, cuda):
    from handwriting_line_generation_amd.generate import load_for_generation
    path = os.path.join(runs["dir_a"], "checkpoint-iteration6.pth")
    model, _, _ = load_for_generation(path, gpu=0, averaged=True)
    want = runs["ck_a"][6]["swa_state_dict"]
    got = model.state_dict()
    assert set(got) == set(want) and not model.training
    for k, v in want.items():
        assert torch.equal(_bits(got[k].cpu()), _bits(v)), k
    live, _, _ = load_for_generation(path, gpu=0)
    assert any(not torch.equal(p.cpu(), want[n]) for n, p in live.named_parameters())
    with pytest.raises(KeyError, match="swa_state_dict"):
        load_for_generation(os.path.join(runs["dir_b"], "checkpoint-iteration6.pth"), gpu=0, averaged=True)
