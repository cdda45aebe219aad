#!/usr/bin/env python
"""Measurements behind profiles/line_store.txt (needs an MI355X):
  --what kernel    ops.store_batch against ops.lines_from_u8 (the yardstick: same output bytes, same 16-byte stores, no warp) back to back in
                   one process at 8 x 64 x 512 and 16 x 64 x 1216: time per call between device events (table upload + launch) in alternating
                   windows, so that the spread between equal windows stands next to the ratio. store_batch at rest (strech 1, m 0: f = 0), with
                   the loader's draws (strech in [0.6, 1.4], |skew| <= 45 degrees), and with masks.
  --what steps     GAN training steps/s of the shipped IAM config from a fabricated IAM directory (oracle.collate_items.fake_iam, the form
                   pictures put on white canvases of --page W,H pixels - IAM's forms are 2479 x 3542 - so that a page decode costs what it
                   costs there), through data.getDataLoader as train.py builds it: --loader host (DataLoader workers) or store
                   (data_loader.device_store). --root: the tree to import the package from (the parent commit's, for the before / after of the
                   host path); this file itself needs nothing of the new code with --loader host.
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel(args):
    import math

    import numpy as np
    import torch
    from handwriting_line_generation_amd import ops
    dev = torch.device("cuda:0")
    H = 64
    for B, W in ((8, 512), (16, 1216)):
        rs = np.random.RandomState(B)
        n = 2 * B
        widths = np.full(n, W, dtype=np.int64)
        widths[B:] = (int(W / 1.4) // 4) * 4                   # the second half leaves room for strech 1.4 inside W columns
        offsets = np.zeros(n, dtype=np.int64)
        offsets[1:] = np.cumsum(H * widths)[:-1]
        nbytes = int(H * widths.sum())
        pixels = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev)
        masks = (torch.randint(0, 2, (nbytes,), dtype=torch.uint8, device=dev) * 255).to(torch.uint8)
        pool = ops.LinePool(pixels, offsets, widths, height=H, masks=masks)
        rest = [(k, W, 1.0, 0.0) for k in range(B)]
        drawn = []
        for k in range(B, 2 * B):
            s = 0.6 + 0.8 * rs.random_sample()
            drawn.append((k, int(widths[k] * s), s, math.tan((2 * rs.random_sample() - 1) * math.pi / 4)))
        out = torch.empty(B * H * W, dtype=torch.float32, device=dev)
        out2 = torch.empty(B * H * W, dtype=torch.float32, device=dev)
        kinds = [("lines_from_u8 (yardstick)", lambda: ops.lines_from_u8(pixels, offsets, widths, list(range(B)), out=out, height=H)),
                 ("store_batch at rest", lambda: ops.store_batch(pool, rest, W=W, out=out)),
                 ("store_batch drawn", lambda: ops.store_batch(pool, drawn, W=W, out=out)),
                 ("store_batch drawn + masks", lambda: ops.store_batch(pool, drawn, W=W, want_mask=True, out=(out, out2)))]
        times = {name: [] for name, _ in kinds}
        for window in range(args.windows + 1):
            for name, fn in kinds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if window:                                     # window 0: warm-up
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        base = sorted(times[kinds[0][0]])[len(times[kinds[0][0]]) // 2]
        print("[%d,1,%d,%d] = %.2f MB of fp32 per tensor; us per call between device events, %d windows of %d calls:" % (B, H, W, B * H * W * 4 / 1e6, args.windows, args.calls))
        for name, _ in kinds:
            med = sorted(times[name])[len(times[name]) // 2]
            print("  %-28s %s  median %.1f us  = %.2f x the yardstick" % (name, " ".join("%.1f" % t for t in times[name]), med, med / base), flush=True)


def _fabricate(root, n_pages, page):
    """fake_iam's directory with every form on a white canvas of `page` = (W, H) pixels (boxes unchanged: the crop is the same)"""
    from PIL import Image
    from oracle import collate_items
    pages, _ = collate_items.fake_iam(root, n_pages=n_pages, with_images=True)
    for name in pages:
        path = os.path.join(root, "forms", name + ".png")
        form = Image.open(path).convert("L")
        canvas = Image.new("L", (max(page[0], form.size[0]), max(page[1], form.size[1])), 255)
        canvas.paste(form, (0, 0))
        canvas.save(path)
    sets = {"train": pages, "valid": pages[:2], "test": pages[:2]}
    json.dump(sets, open(os.path.join(root, "sets.json"), "w"))


def steps(args):
    import random

    import numpy as np
    import torch
    torch.set_num_threads(1)
    from handwriting_line_generation_amd import model as M, rng
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.synthetic import write_synthetic_corpus
    from handwriting_line_generation_amd.harness import CHAR_FILES, load_config
    from handwriting_line_generation_amd.model import loss as loss_fns
    from handwriting_line_generation_amd.trainer import HWWithStyleTrainer
    work = tempfile.mkdtemp(prefix="hwg_store_")
    root = os.path.join(work, "iam")
    os.makedirs(root)
    _fabricate(root, args.pages, tuple(int(v) for v in args.page.split(",")))
    cfg = copy.deepcopy(load_config("iam_gan"))
    dl, tr = cfg["data_loader"], cfg["trainer"]
    dl.update(data_dir=root, char_file=CHAR_FILES["iam"], width_bucket=128)
    if args.loader == "store":
        dl["device_store"] = True
    cfg["validation"] = dict(cfg.get("validation", {}), num_workers=0)
    tr.update(save_dir=os.path.join(work, "saved"), print_dir=None, encoder_weights=os.path.join(work, "encoder.pth"), text_data=os.path.join(work, "corpus.txt"))
    cfg["model"]["pretrained_hwr"] = None
    cfg["cuda"], cfg["gpu"] = True, 0
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    rng.set_mode("device", seed=3)
    torch.save({"state_dict": M.Autoencoder({"type": tr.get("encoder_type", "2tight"), "hwr": cfg["model"]["num_class"]}).state_dict()}, tr["encoder_weights"])
    write_synthetic_corpus(tr["text_data"], dl["char_file"])
    t0 = time.perf_counter()
    loader, _ = D.getDataLoader(cfg, "train")
    built = time.perf_counter() - t0
    losses = {k: getattr(loss_fns, v) for k, v in cfg["loss"].items()}
    trainer = HWWithStyleTrainer(M.HWWithStyle(cfg["model"]), losses, [], None, cfg, loader, None, None)
    rates, it = [], 0
    for window in range(args.windows + 1):
        n = args.warmup if window == 0 else args.steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            trainer._train_iteration(it)
            it += 1
        torch.cuda.synchronize()
        if window:
            rates.append(n / (time.perf_counter() - t0))
    print("steps: tree %s  loader %-5s (%s, %d items of %d lines, batch_size %d, num_workers %s, pages %s, built in %.2f s): steps/s per window of %d steps: %s  median %.2f" % (
        args.root or HERE, args.loader, type(loader).__name__, len(loader.dataset), dl["a_batch_size"], dl["batch_size"], dl.get("num_workers"), args.page, built,
        args.steps, " ".join("%.2f" % r for r in rates), sorted(rates)[len(rates) // 2]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "steps"), required=True)
    ap.add_argument("--loader", choices=("host", "store"), default="host")
    ap.add_argument("--root", default=None, help="import the package (and oracle/) from this tree instead of the one this file is in")
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--pages", type=int, default=12)
    ap.add_argument("--page", default="2479,3542")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else HERE)
    {"kernel": kernel, "steps": steps}[args.what](args)


if __name__ == "__main__":
    main()
