#!/usr/bin/env python
"""Measurements behind profiles/error_rates.txt (needs an MI355X):
  --what steps      recogniser pre-training steps/s (configs/cf_IAM_hwr_cnnOnly_batchnorm_aug.json on synthetic batches, as `train.py -c ...
                    --synthetic` builds them), trainer.device_cer off against on, in alternating windows so that the spread between equal
                    windows stands next to the difference; once with the reference's per-step log and once with async_log = 1
  --what kernels    hwg_ctc_error_rates at T = 304, B = 16, C = 80 in a loop: run it under `rocprofv3 --kernel-trace --stats` for the
                    two launches' kernel times; it prints the device-event time of the pair and the host path's time itself
  --what get_styles get_styles.py with and without --cer on a fabricated IAM directory of --pages pages and the reduced reference
                    checkpoint (tests/golden/ref_ckpt_gan.pth.xz, spacer spread as in tests/test_generate_cli_gpu.py), twice each
"""
import argparse
import json
import lzma
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def steps(args):
    import random

    import numpy as np
    import torch
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.harness import build_simple_trainer
    torch.set_num_threads(1)
    for async_log in (False, 1):
        trainers = {}
        for device_cer in (False, True):
            rng.set_mode("device", seed=3)
            torch.manual_seed(0); np.random.seed(0); random.seed(0)
            trainer, _ = build_simple_trainer("iam_hwr", width=512, label_len=30)          # batch 16, as the config
            trainer.device_cer, trainer.async_log = device_cer, async_log
            trainer.data_loader.make_resident(8, trainer.gpu)
            trainer.data_loader_iter = iter(trainer.data_loader)
            trainers[device_cer] = [trainer, 0]
        rates = {False: [], True: []}
        for window in range(2 * args.windows + 2):
            device_cer = bool(window % 2)
            trainer, it = trainers[device_cer]
            n = args.warmup if window < 2 else args.steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                trainer._train_iteration(it)
                it += 1
            trainer.flush_log()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            trainers[device_cer][1] = it
            if window >= 2:
                rates[device_cer].append(n / dt)
        for device_cer in (False, True):
            r = rates[device_cer]
            print("async_log=%s device_cer=%s steps/s per window of %d steps: %s  median %.2f" % (
                async_log, device_cer, args.steps, " ".join("%.2f" % v for v in r), sorted(r)[len(r) // 2]), flush=True)
        print("async_log=%s ratio of medians on/off: %.3f" % (async_log, sorted(rates[True])[len(rates[True]) // 2] / sorted(rates[False])[len(rates[False]) // 2]),
              flush=True)


def kernels(args):
    import numpy as np
    import torch
    from handwriting_line_generation_amd import ops
    T, B, C = 304, 16, 80
    idx_to_char = {int(k): v for k, v in json.load(open(os.path.join(ROOT, "handwriting_line_generation_amd", "data", "IAM_char_set.json")))["idx_to_char"].items()}
    rs = np.random.RandomState(0)
    gt = ["".join(idx_to_char[int(c)] for c in rs.randint(1, C, size=n)) for n in rs.randint(40, 91, size=B)]
    pred_h = rs.randn(T, B, C).astype(np.float32)
    pred = torch.from_numpy(pred_h).cuda()
    for _ in range(10):
        ops.ctc_error_rates(pred, gt, idx_to_char).result()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    handles = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        handles.append(ops.ctc_error_rates(pred, gt, idx_to_char))
    e1.record()
    for h in handles:
        h.result()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print("device: T=%d B=%d C=%d, %d calls: %.1f us per call between device events (upload + two launches + fetch enqueue), %.1f us per call "
          "host wall clock including .result()" % (T, B, C, args.steps, e0.elapsed_time(e1) * 1e3 / args.steps, wall * 1e6 / args.steps), flush=True)
    t0 = time.perf_counter()
    for _ in range(20):
        ops.host_error_rates(pred.cpu().numpy(), gt, idx_to_char)
    print("host path (pred.cpu() + naive_decode + cer + wer): %.1f us per call" % ((time.perf_counter() - t0) * 1e6 / 20), flush=True)


def get_styles(args):
    import torch
    from oracle import collate_items
    from handwriting_line_generation_amd.harness import CHAR_FILES
    from handwriting_line_generation_amd.logger import load_checkpoint
    d = tempfile.mkdtemp(prefix="hwg_styles_")
    root = os.path.join(d, "iam")
    os.makedirs(root)
    collate_items.fake_iam(root, n_pages=args.pages, with_images=True)
    raw = os.path.join(d, "ref.pth")
    with open(raw, "wb") as f:
        f.write(lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "ref_ckpt_gan.pth.xz"), "rb").read()))
    ck = load_checkpoint(raw)
    ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
    ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
    path = os.path.join(d, "spread.pth")
    torch.save(ck, path)
    cfg = ck["config"]
    cfg["data_loader"].update(data_dir=root, batch_size=args.batch, a_batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"], max_width=640, augmentation=None)
    cfg["validation"] = dict(cfg.get("validation", {}), batch_size=args.batch, a_batch_size=2, num_workers=0, augmentation=None)
    cfg_path = os.path.join(d, "cfg.json")
    json.dump(cfg, open(cfg_path, "w"))
    import atexit
    import shutil
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    for k in range(2):
        for extra in ([], ["--cer"]):
            cmd = [sys.executable, os.path.join(ROOT, "get_styles.py"), "-c", path, "-f", cfg_path, "-d", os.path.join(d, "out%d%s" % (k, "".join(extra))), "-g", "0"] + extra
            r = subprocess.run(cmd, cwd=d, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                raise SystemExit("get_styles.py failed:\n" + r.stdout[-3000:])
            print("run %d %s" % (k, " ".join(extra) or "(styles only)"), flush=True)
            print("\n".join("    " + l for l in r.stdout.splitlines() if "lines/s" in l or "cer_real" in l), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("steps", "kernels", "get_styles"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--pages", type=int, default=60)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    {"steps": steps, "kernels": kernels, "get_styles": get_styles}[args.what](args)


if __name__ == "__main__":
    main()
