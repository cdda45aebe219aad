#!/usr/bin/env python
"""Measurements behind profiles/sample_sheets.txt (needs an MI355X):
  --what kernels   hwg_sheet_minmax and hwg_sheet_compose (csrc/sample_sheet.hip), each in a loop between device events, for batches of
                   8 x 64 x 512 and 16 x 64 x 1216, with the bytes each launch moves
  --what steps     steps/s of the synthetic IAM GAN config (the package's own trainer on harness.build_gan_trainer, the shipped batch and
                   512-column lines) over --windows windows of --steps iterations after --warmup; --sheets N switches sample sheets on at
                   print_every N (0 = print_dir null; this mode uses nothing a commit without sample sheets lacks)
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels(args):
    import torch
    from handwriting_line_generation_amd import ops
    dev = torch.device("cuda:0")
    for B, H, W in ((8, 64, 512), (16, 64, 1216)):
        x = torch.rand(B, 1, H, W, device=dev) * 2 - 1
        hs, ws, nrow = ops.sample_sheet_shape(B, H, W)
        out = torch.empty((-(-hs * ws // 4) * 4,), dtype=torch.uint8, device=dev)
        n = x.numel()
        parts = ops.L.query("hwg_sheet_parts", n)
        partials = torch.empty((parts, 2), dtype=torch.float32, device=dev)
        st = ops._stream()
        calls = {"minmax": lambda: ops.L.call("hwg_sheet_minmax", x, n, partials, parts, st),
                 "compose": lambda: ops.L.call("hwg_sheet_compose", x, B, H, W, nrow, partials, parts, out, out.numel(), st)}
        moved = {"minmax": 4 * n + 8 * parts, "compose": 4 * n + hs * ws}
        for name in ("minmax", "compose"):
            for _ in range(20):
                calls[name]()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                calls[name]()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.steps
            print("%d x %d x %d (sheet %d x %d, nrow %d, %d partials) hwg_sheet_%-8s %7.2f us per launch in a loop of %d (back to back: launch "
                  "gaps included), %.2f MB moved = %.2f TB/s" % (B, H, W, hs, ws, nrow, parts, name, us, args.steps, moved[name] / 1e6, moved[name] / us / 1e6),
                  flush=True)


def steps(args):
    import random

    import numpy as np
    import torch
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.harness import build_gan_trainer
    torch.set_num_threads(1)
    workdir = tempfile.mkdtemp(prefix="hwg_sheets_")
    rng.set_mode("device", seed=1)
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    trainer, cfg = build_gan_trainer("iam_gan", workdir=workdir)
    trainer.async_log = 1
    label = "print_dir null"
    if args.sheets:
        out = os.path.join(workdir, "sheets")
        trainer.enable_sample_sheets(out, print_every=args.sheets, serperate_print_every=10 ** 9)
        label = "sheets at print_every %d" % args.sheets
    it, rates = 0, []
    for window in range(args.windows + 1):
        n = args.warmup if window == 0 else args.steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            trainer._train_iteration(it)
            it += 1
        trainer.flush_log()
        if args.sheets:
            trainer.finish_sample_sheets()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if window:
            rates.append(n / dt)
    dl = cfg["data_loader"]
    extra = ""
    if args.sheets:
        files = sorted(os.listdir(out))
        extra = "  files: %s (%d bytes)" % (" ".join(files), sum(os.path.getsize(os.path.join(out, f)) for f in files))
    print("%s [%s, batch %d x %d, 512 columns, async_log 1]: steps/s per window of %d steps after %d warm-up: %s  all %d steps: %.2f%s" % (
        args.tag, label, dl["batch_size"], dl.get("a_batch_size", 1), args.steps, args.warmup, " ".join("%.2f" % v for v in rates),
        args.steps * args.windows, args.steps * args.windows / sum(args.steps / v for v in rates), extra), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernels", "steps"), required=True)
    ap.add_argument("--steps", type=int, default=140)
    ap.add_argument("--warmup", type=int, default=70)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sheets", type=int, default=0)
    ap.add_argument("--tag", type=str, default="this commit")
    args = ap.parse_args()
    {"kernels": kernels, "steps": steps}[args.what](args)


if __name__ == "__main__":
    main()
