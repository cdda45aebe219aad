#!/usr/bin/env python
"""Measurements behind profiles/line_store_warp.txt (needs an MI355X):
  --what kernel    B = 16 lines of the widths of tests/test_augment_gpu.py's `ragged16` (W = 1216): ops.store_warp_batch against the path it
                   replaces - the upload of the collated fp32 batch (ops.h2d) + ops.augment_lines - back to back in ONE process, alternating
                   windows, time per call between device events, device draws on both sides; the median over the windows and every window,
                   so that the spread of the old path's own repeats stands next to the difference. The two outputs are compared bit for bit
                   on the same generator state first.
  --what steps     recogniser pre-training steps/s of the shipped cf_IAM_hwr_cnnOnly_batchnorm_aug.json (batch 16, its num_workers) from a
                   fabricated IAM directory (oracle.collate_items.fake_iam, every form on a white canvas of --page W,H pixels - IAM's forms
                   are 2479 x 3542 - so that a page decode costs what it costs there), through data.getDataLoader as train.py builds it:
                   --loader host (DataLoader workers + DeviceAugment) or store (data_loader.device_store: "warp"). --root: the tree to import
                   the package from (the parent commit's); this file needs nothing of the new code with --loader host.
  --what digest    sha256 of ops.augment_lines' output, map and statistics on seeded lines with device draws, from the tree given by
                   --root: the path without the key, to be compared between the parent commit's tree and this one.
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 64
RAGGED16 = [1216, 161, 1003, 640, 333, 1100, 87, 950, 512, 777, 1211, 240, 405, 868, 699, 1150]


def _text_line(rs, w):
    img = rs.randint(190, 256, size=(H, w))
    for _ in range(max(w // 14, 1)):
        x, y = int(rs.randint(0, max(w - 3, 1))), int(rs.randint(4, 40))
        img[y:y + int(rs.randint(6, 22)), x:x + int(rs.randint(2, 9))] = rs.randint(10, 110)
    return img


def kernel(args):
    import numpy as np
    import torch
    from handwriting_line_generation_amd import ops
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(21)
    lines = [_text_line(rs, w) for w in RAGGED16]
    B, W = len(lines), max(RAGGED16)
    widths = np.array(RAGGED16, dtype=np.int64)
    offsets = np.zeros(B, dtype=np.int64)
    np.cumsum(H * widths[:-1], out=offsets[1:])
    pool = ops.LinePool(torch.from_numpy(np.concatenate([l.astype(np.uint8).reshape(-1) for l in lines])).to(dev), offsets, widths, height=H)
    t0 = time.perf_counter()
    ops.store_line_stats(pool)
    torch.cuda.synchronize()
    print("store_line_stats, first call (code object load included): %.1f ms for %d lines, %d bytes" % ((time.perf_counter() - t0) * 1e3, B, pool.pixels.numel()))
    host = np.full((B, 1, H, W), -1.0, dtype=np.float32)
    for b, l in enumerate(lines):
        host[b, 0, :, :l.shape[1]] = 1.0 - l.astype(np.float32) / 128.0
    host = torch.from_numpy(host)
    mesh = ops.LineMesh(H, RAGGED16, sigma=1.5)
    rows = list(range(B))
    out = torch.empty(B * H * W, dtype=torch.float32, device=dev)
    g = ops.DeviceRNG(5)

    def old():
        return ops.augment_lines(ops.h2d(host, dev), mesh, rng=g)

    def new():
        return ops.store_warp_batch(pool, rows, mesh, W, rng=g, out=out)
    g.offset = 0
    a = old()
    g.offset = 0
    b = new()
    torch.cuda.synchronize()
    same = torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    print("same generator state: old and new outputs %s ([%d,1,%d,%d])" % ("equal bit for bit" if same else "DIFFER", B, H, W))
    assert same
    kinds = [("old: h2d fp32 batch + augment_lines", old), ("new: store_warp_batch", new)]
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
    print("[%d,1,%d,%d] = %.2f MB of fp32; us per call between device events (host side of the call included), %d windows of %d calls:"
          % (B, H, W, B * H * W * 4 / 1e6, args.windows, args.calls))
    med = {}
    for name, _ in kinds:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        print("  %-38s %s  median %.1f us  (min %.1f, max %.1f)" % (name, " ".join("%.1f" % v for v in times[name]), med[name], t[0], t[-1]), flush=True)
    print("  new / old = %.2f" % (med[kinds[1][0]] / med[kinds[0][0]]))


def digest(args):
    import hashlib

    import numpy as np
    import torch
    from handwriting_line_generation_amd import ops
    widths = RAGGED16 + [5, 6, 63, 64, 65]
    rs = np.random.RandomState(21)
    x = np.full((len(widths), 1, H, max(widths)), -1.0, dtype=np.float32)
    for b, w in enumerate(widths):
        x[b, 0, :, :w] = 1.0 - rs.randint(0, 256, size=(H, w)).astype(np.float32) / 128.0
    x = torch.from_numpy(x).cuda()
    out = []
    for sigma, seed in ((1.5, 5), (0.7, 6)):
        g = ops.DeviceRNG(seed)
        g.offset = 17
        mesh = ops.LineMesh(H, widths, sigma=sigma, bright=[b % 3 != 1 for b in range(len(widths))], warp=[b % 4 != 2 for b in range(len(widths))])
        y, mp, st = ops.augment_lines(x, mesh, rng=g, want_map=True)
        torch.cuda.synchronize()
        out.append(hashlib.sha256(y.cpu().numpy().tobytes() + mp.cpu().numpy().tobytes() + st.cpu().numpy().tobytes()).hexdigest()[:20])
    print("augment_lines digests, tree %s: %s" % (args.root or HERE, " ".join(out)))


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
    json.dump({"train": pages, "valid": pages[:2], "test": pages[:2]}, open(os.path.join(root, "sets.json"), "w"))


def steps(args):
    import random

    import numpy as np
    import torch
    torch.set_num_threads(1)
    from handwriting_line_generation_amd import model as M, rng
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.harness import CHAR_FILES
    from handwriting_line_generation_amd.model import loss as loss_fns
    from handwriting_line_generation_amd.trainer import HWWithStyleTrainer
    work = tempfile.mkdtemp(prefix="hwg_warp_store_")
    root = os.path.join(work, "iam")
    os.makedirs(root)
    _fabricate(root, args.pages, tuple(int(v) for v in args.page.split(",")))
    cfg = copy.deepcopy(json.load(open(os.path.join(HERE, "configs", "cf_IAM_hwr_cnnOnly_batchnorm_aug.json"))))
    dl, tr = cfg["data_loader"], cfg["trainer"]
    dl.update(data_dir=root, char_file=CHAR_FILES["iam"])
    if args.loader == "store":
        dl["device_store"] = "warp"
    cfg["validation"] = dict(cfg.get("validation", {}), num_workers=0)
    tr.update(save_dir=os.path.join(work, "saved"))
    cfg["cuda"], cfg["gpu"] = True, 0
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    rng.set_mode("device", seed=3)
    t0 = time.perf_counter()
    loader, _ = D.getDataLoader(cfg, "train")
    torch.cuda.synchronize()
    built = time.perf_counter() - t0
    extra = ""
    if hasattr(loader, "store"):
        extra = ", pool of %d lines = %d bytes (+ %d bytes of statistics), statistics launch %.3f s" % (
            len(loader.store.widths), loader.store.pixels.size, 4 * 257 * len(loader.store.widths), loader.stats_s)
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
    print("steps: tree %s  loader %-5s (%s, %d lines, batch_size %d, num_workers %s, %d pages of %s, loaders built in %.2f s%s): steps/s per window of %d steps: %s  median %.2f" % (
        args.root or HERE, args.loader, type(loader).__name__, len(loader.dataset), dl["batch_size"], dl.get("num_workers"), args.pages, args.page, built, extra,
        args.steps, " ".join("%.2f" % r for r in rates), sorted(rates)[len(rates) // 2]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "steps", "digest"), required=True)
    ap.add_argument("--loader", choices=("host", "store"), default="host")
    ap.add_argument("--root", default=None, help="import the package (and oracle/) from this tree instead of the one this file is in")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--pages", type=int, default=48)
    ap.add_argument("--page", default="2479,3542")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else HERE)
    {"kernel": kernel, "steps": steps, "digest": digest}[args.what](args)


if __name__ == "__main__":
    main()
