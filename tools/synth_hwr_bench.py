#!/usr/bin/env python
"""Measurements behind profiles/synth_hwr.txt (needs an MI355X):
  --what steps     recogniser pre-training steps/s at batch 16 on synthetic real lines (as `train.py -c ... --synthetic` builds them):
                   HWWithStyleTrainer (the pre-training trainer as it stands) against HWRWithSynthTrainer with per_batch 0, 8 and 16, in
                   alternating windows so that the spread between equal windows stands next to the differences. The generator is the
                   full-size model of the shipped GAN config with random-init weights (spacer.mean / spacer.std set so that lines are
                   ~16 columns per character wide)
  --what compose   hwg_lines_from_u8 for 16 real + 16 pool lines of ~1200 columns in a loop: time per launch between device events
                   (upload of the 32-row table included) and the bytes it moves
  --what refill    SynthLinePool.refill at pool 2048 (gen_batch 64): seconds and lines/s, to hold against gen_lines_per_sec of bench.py
"""
import argparse
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _world(workdir):
    """-> the `trainer.synth` block around a full-size random-init generator checkpoint, a style file and a text file in `workdir`"""
    import numpy as np
    import torch
    from handwriting_line_generation_amd.data.synthetic import write_synthetic_corpus
    from handwriting_line_generation_amd.harness import CHAR_FILES, build_gan_trainer
    trainer, cfg = build_gan_trainer("iam_gan", 2, 2, width=128, label_len=6, workdir=os.path.join(workdir, "gan"))
    sd = {k: v.cpu() for k, v in trainer.model.state_dict().items()}
    sd["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(sd["spacer.mean"])
    sd["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(sd["spacer.std"])
    ckpt = os.path.join(workdir, "gen.pth")
    torch.save({"state_dict": sd, "config": cfg, "iteration": 0}, ckpt)
    style_dim = trainer.model.style_dim
    del trainer
    torch.cuda.empty_cache()
    styles = os.path.join(workdir, "train_styles_")
    with open(styles + "0.pkl", "wb") as f:
        pickle.dump({"authors": ["a%d" % (i // 4) for i in range(64)], "styles": np.random.RandomState(1).randn(64, style_dim).astype(np.float32)}, f)
    text = os.path.join(workdir, "text.txt")
    write_synthetic_corpus(text, CHAR_FILES["iam"])
    return dict(checkpoint=ckpt, styles=styles, text_data=text, per_batch=0, pool=2048, gen_batch=64, seed=0, max_len=55, max_width=None, spacing_noise=False)


def _trainer(cls, synth, workdir, tag):
    import copy
    import random

    import numpy as np
    import torch
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.data.synthetic import SyntheticAuthorDataset, SyntheticLoader
    from handwriting_line_generation_amd.harness import CHAR_FILES, load_config
    from handwriting_line_generation_amd.model import HWWithStyle, loss as loss_fns
    cfg = copy.deepcopy(load_config("iam_hwr"))
    cfg["cuda"], cfg["gpu"] = True, 0
    dl = cfg["data_loader"]
    dl["char_file"] = CHAR_FILES["iam"]
    cfg["trainer"]["save_dir"] = os.path.join(workdir, "saved_" + tag)
    if synth is not None:
        cfg["trainer"]["synth"] = synth
    rng.set_mode("device", seed=3)
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    ds = SyntheticAuthorDataset(dl["char_file"], dl["batch_size"], 1, width=512, label_len=30, seed=100)
    losses = {name: getattr(loss_fns, fn) for name, fn in cfg["loss"].items()}
    trainer = cls(HWWithStyle(cfg["model"]), losses, [], None, cfg, SyntheticLoader(ds), None, None)
    trainer.data_loader.make_resident(8, trainer.gpu)
    for inst in trainer.data_loader._resident:          # the labels stay on the host, where a real loader leaves them
        inst["label"] = inst["label"].cpu()
    trainer.data_loader_iter = iter(trainer.data_loader)
    return trainer


def steps(args):
    import torch
    from handwriting_line_generation_amd.trainer import HWRWithSynthTrainer, HWWithStyleTrainer
    torch.set_num_threads(1)
    workdir = tempfile.mkdtemp(prefix="hwg_synth_")
    synth = _world(workdir)
    kinds = [("HWWithStyleTrainer", HWWithStyleTrainer, None)] + [("per_batch=%d" % n, HWRWithSynthTrainer, dict(synth, per_batch=n)) for n in (0, 8, 16)]
    for device_cer, async_log in ((False, False), (True, 1)):
        trainers = []
        for name, cls, block in kinds:
            t = _trainer(cls, block, workdir, name)
            t.device_cer, t.async_log = device_cer, async_log
            trainers.append([name, t, 0, []])
        for window in range(args.windows + 1):
            for entry in trainers:
                name, t, it, rates = entry
                n = args.warmup if window == 0 else args.steps
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    t._train_iteration(it)
                    it += 1
                t.flush_log()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                entry[2] = it
                if window:
                    rates.append(n / dt)
        for name, t, it, rates in trainers:
            extra = "" if getattr(t, "pool", None) is None else "  (pools rendered: %d, mean line width %.0f columns)" % (len(t.pool.refills), float(t.pool.widths.mean()))
            print("device_cer=%s async_log=%s %-20s steps/s per window of %d steps: %s  median %.2f%s" % (
                device_cer, async_log, name, args.steps, " ".join("%.2f" % v for v in rates), sorted(rates)[len(rates) // 2], extra), flush=True)
        del trainers
        torch.cuda.empty_cache()


def compose(args):
    import numpy as np
    import torch
    from handwriting_line_generation_amd import ops
    dev = torch.device("cuda:0")
    H, n, Br, Wr = 64, 16, 16, 1200
    widths = (np.random.RandomState(0).randint(270, 301, size=n) * 4).astype(np.int32)        # 1080 .. 1200 columns
    offsets = np.zeros(n, dtype=np.int64)
    offsets[1:] = np.cumsum(H * widths.astype(np.int64))[:-1]
    pixels = torch.randint(0, 256, (int(H * widths.sum()),), dtype=torch.uint8, device=dev)
    real = torch.rand(Br, 1, H, Wr, device=dev) * 2 - 1
    select = [-1 - r for r in range(Br)] + list(range(n))
    out = ops.lines_from_u8(pixels, offsets, widths, select, real=real)
    B, W = out.shape[0], out.shape[3]
    moved = real.numel() * 4 + int(H * widths.sum()) + out.numel() * 4
    for _ in range(20):
        ops.lines_from_u8(pixels, offsets, widths, select, real=real, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        ops.lines_from_u8(pixels, offsets, widths, select, real=real, out=out)
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    us = e0.elapsed_time(e1) * 1e3 / args.steps
    print("compose: %d real rows of %d columns + %d pool lines of %d..%d columns -> [%d,1,%d,%d]; %.2f MB moved per launch; %d calls: %.1f us per call "
          "between device events (table upload + launch) = %.2f TB/s, %.1f us per call host wall clock" % (
              Br, Wr, n, widths.min(), widths.max(), B, H, W, moved / 1e6, args.steps, us, moved / us / 1e6, wall * 1e6 / args.steps), flush=True)


def refill(args):
    import json

    import torch
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.data.synth_lines import SynthLinePool
    from handwriting_line_generation_amd.harness import CHAR_FILES
    workdir = tempfile.mkdtemp(prefix="hwg_synth_")
    synth = _world(workdir)
    rng.set_mode("device", seed=3)
    pool = SynthLinePool(synth, json.load(open(CHAR_FILES["iam"]))["char_to_idx"], gpu=0)
    for k in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool.refill(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print("refill %d: pool %d, gen_batch %d: %.1f ms = %.0f lines/s; %d lines kept, mean width %.0f columns, %.1f MB of pixels%s" % (
            k, pool.size, pool.gen_batch, dt * 1e3, pool.size / dt, len(pool.texts), float(pool.widths.mean()), pool.pixels.numel() / 1e6,
            "  (first call: plans and allocations)" if k == 0 else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("steps", "compose", "refill"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    {"steps": steps, "compose": compose, "refill": refill}[args.what](args)


if __name__ == "__main__":
    main()
