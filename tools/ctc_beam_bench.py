#!/usr/bin/env python
"""Measurements behind profiles/ctc_beam.txt (needs an MI355X; one process):
  1. ops.ctc_beam_error_rates at T = 304, B = 16, C = 80 with beam 4, 16 and 32 on random scores (every class alive in every frame: the
     worst case) next to ops.ctc_error_rates on the same input (the yardstick of profiles/error_rates.txt) and to
     string_utils.prefix_beam_decode on the host (one line timed, a batch is 16 of them).
  2. The same on the real predictions of the reduced reference checkpoint (tests/golden/ref_ckpt_gan.pth.xz) over a fabricated IAM
     directory, and the CER / WER difference, beam minus greedy, over those lines.
Time per call: device events around --calls calls (upload + launches + the fetch's enqueue), after --warmup calls."""
import argparse
import json
import lzma
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEAMS = (4, 16, 32)


def per_call_us(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn().result()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    handles = [fn() for _ in range(calls)]
    e1.record()
    for h in handles:
        h.result()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def compare(name, pred, gt, idx_to_char, args, host_lines=1):
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.utils import string_utils
    T, B, C = pred.shape
    greedy = per_call_us(lambda: ops.ctc_error_rates(pred, gt, idx_to_char), args.calls, args.warmup)
    print("%s: T=%d B=%d C=%d" % (name, T, B, C), flush=True)
    print("    greedy (ops.ctc_error_rates)          %9.1f us per call" % greedy, flush=True)
    pred_h = pred.cpu().numpy()
    for beam in BEAMS:
        us = per_call_us(lambda: ops.ctc_beam_error_rates(pred, gt, idx_to_char, beam=beam), args.calls, args.warmup)
        t0 = time.perf_counter()
        for b in range(host_lines):
            string_utils.prefix_beam_decode(pred_h[:, b], beam)
        host = (time.perf_counter() - t0) / host_lines
        print("    beam %2d (ops.ctc_beam_error_rates)    %9.1f us per call = %5.2f us per frame, %6.1f x greedy; host prefix_beam_decode "
              "%.2f s per line = %.1f s per batch (%d line(s) timed), %.0f x the device" % (
                  beam, us, us / T, us / greedy, host, host * B, host_lines, host * B * 1e6 / us), flush=True)


def random_scores(args, idx_to_char):
    import numpy as np
    import torch
    T, B, C = 304, 16, 80
    rs = np.random.RandomState(0)
    gt = ["".join(idx_to_char[int(c)] for c in rs.randint(1, C, size=n)) for n in rs.randint(40, 91, size=B)]
    pred = torch.from_numpy(rs.randn(T, B, C).astype(np.float32)).cuda()
    compare("random scores", pred, gt, idx_to_char, args)


def checkpoint_predictions(args, idx_to_char):
    import torch
    from oracle import collate_items
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.data.author_hw_dataset import getDataLoader
    from handwriting_line_generation_amd.generate import load_for_generation
    from handwriting_line_generation_amd.harness import CHAR_FILES
    from handwriting_line_generation_amd.logger import load_checkpoint
    d = tempfile.mkdtemp(prefix="hwg_beam_")
    try:
        root = os.path.join(d, "iam")
        os.makedirs(root)
        collate_items.fake_iam(root, n_pages=args.pages, with_images=True)
        raw = os.path.join(d, "ref.pth")
        with open(raw, "wb") as f:
            f.write(lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "ref_ckpt_gan.pth.xz"), "rb").read()))
        ck = load_checkpoint(raw)
        cfg = ck["config"]
        cfg["data_loader"].update(data_dir=root, batch_size=8, a_batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"], max_width=640,
                                  augmentation=None, shuffle=False)
        cfg["validation"] = dict(cfg.get("validation", {}), batch_size=8, a_batch_size=2, num_workers=0, augmentation=None, shuffle=False)
        cfg_path = os.path.join(d, "cfg.json")
        json.dump(cfg, open(cfg_path, "w"))
        model, config, _ = load_for_generation(raw, cfg_path, gpu=0)
        gpu = torch.device("cuda", 0)
        batches = []
        with torch.no_grad():
            for inst in getDataLoader(config, "train")[1]:
                model.pred = model.spaced_label = model.spaced_label_index = None
                batches.append((model.hwr(ops.h2d(inst["image"], gpu), None).detach().contiguous(), list(inst["gt"])))
        model.pred = None
    finally:
        shutil.rmtree(d, ignore_errors=True)
    pred, gt = max(batches, key=lambda b: b[0].shape[0])
    compare("checkpoint predictions (the widest validation batch)", pred, gt, idx_to_char, args)
    for beam in BEAMS:
        sums, n, changed = [0.0, 0.0, 0.0, 0.0], 0, 0
        for pred, gt in batches:
            g = ops.ctc_error_rates(pred, gt, idx_to_char).result()
            k = ops.ctc_beam_error_rates(pred, gt, idx_to_char, beam=beam).result()
            for i, part in enumerate((g[0], g[1], k[0], k[1])):
                sums[i] += sum(part)
            n += len(gt)
            changed += sum(a != b for a, b in zip(g[2], k[2]))
        print("    %d lines, beam %2d: CER greedy %.4f beam %.4f (beam - greedy %+.4f), WER greedy %.4f beam %.4f (%+.4f), %d texts differ" % (
            n, beam, sums[0] / n, sums[2] / n, (sums[2] - sums[0]) / n, sums[1] / n, sums[3] / n, (sums[3] - sums[1]) / n, changed), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pages", type=int, default=60)
    args = ap.parse_args()
    import torch
    torch.set_num_threads(1)
    idx_to_char = {int(k): v for k, v in json.load(open(os.path.join(ROOT, "handwriting_line_generation_amd", "data", "IAM_char_set.json")))["idx_to_char"].items()}
    random_scores(args, idx_to_char)
    checkpoint_predictions(args, idx_to_char)


if __name__ == "__main__":
    main()
