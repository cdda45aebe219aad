#!/usr/bin/env python
"""python tools/generate_film_bench.py [--warmup 3] [--calls 10] [--repeats 20] [--runs 20] [--out profiles/generate_film.txt]
Times the stretch film's labels on one MI355X:
 * hwg_stretch_onehot (csrc/stretch.hip), the entry point alone: the 79 frames of generate.stretch_scales() in one launch, at T=130, B=2,
   ncls=80 and at T=400, B=8, ncls=80; windows of `calls` back-to-back launches between two device events, `repeats` windows, median and
   spread; achieved bytes per second next to the write bound 2 * sum T_out * B * ncls * 4 bytes over the peak HBM write rate;
 * ops.stretch_onehot, the whole call (label download and check, table upload, launch), host clock around a device synchronise;
 * the same frames by the torch chain of the reference (ops.onehot_both, permute, F.interpolate, permute - 79 times), same clock;
 * the whole `generate.py -r choice=s` action both ways (the second with ops.stretch_onehot replaced by that chain), `runs` runs each,
   alternating, on the fabricated dataset and the reduced checkpoint of the tests - lines of some 60 steps, two per batch: a toy size that
   measures the action's fixed costs (79 generator passes, 158 PNGs), not the label kernel."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_HBM = 8.0e12          # bytes / s, the MI355X's HBM3E specification


def spread(xs):
    return "median %.4f ms (min %.4f, max %.4f, n=%d)" % (1e3 * statistics.median(xs), 1e3 * min(xs), 1e3 * max(xs), len(xs))


def torch_chain(label, ncls, scales):
    import torch.nn.functional as F
    from handwriting_line_generation_amd import ops
    frames = []
    for s in scales:
        onehot = ops.onehot_both(label, ncls)
        frames.append(F.interpolate(onehot.permute(1, 2, 0), scale_factor=s, mode="linear").permute(2, 0, 1))
    return frames


def time_labels(T, B, ncls, args, say):
    import numpy as np
    import torch
    from handwriting_line_generation_amd import _lib as L, ops
    from handwriting_line_generation_amd.generate import stretch_scales
    dev = torch.device("cuda", 0)
    scales = stretch_scales()
    g = np.random.RandomState(T)
    lab = g.randint(1, ncls, (T, B)).astype(np.int32)
    lab[g.rand(T, B) < 0.5] = 0
    label = ops.h2d(torch.from_numpy(lab), dev)
    nbytes = 2 * sum(f[0] for f in ops.stretch_frames(T, scales)) * B * ncls * 4
    say("T=%d B=%d ncls=%d: 79 frames, %d bytes written (both layouts); write bound %.4f ms at %.1f TB/s" % (
        T, B, ncls, nbytes, 1e3 * nbytes / PEAK_HBM, PEAK_HBM / 1e12))
    # the entry point alone: record the arguments of one wrapper call, launch them again
    recorded = []
    call = L.call

    def recording(name, *a):
        if name == "hwg_stretch_onehot":
            recorded.append(a)
        return call(name, *a)
    L.call = recording
    try:
        keep = ops.stretch_onehot(label, ncls, scales)
    finally:
        L.call = call
    (entry_args,) = recorded
    for _ in range(args.warmup):
        L.call("hwg_stretch_onehot", *entry_args)
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            L.call("hwg_stretch_onehot", *entry_args)
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) / 1e3 / args.calls)
    med = statistics.median(windows)
    say("  hwg_stretch_onehot, per launch in windows of %d back-to-back launches: %s; %.3f TB/s written = %.1f %% of the write bound" % (
        args.calls, spread(windows), nbytes / med / 1e12, 100 * nbytes / PEAK_HBM / med))
    del keep

    def host_timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out
    whole = host_timed(lambda: ops.stretch_onehot(label, ncls, scales))
    chain = host_timed(lambda: torch_chain(label, ncls, scales))
    say("  ops.stretch_onehot, whole call (label check on the host, table upload, 1 launch), host clock: %s" % spread(whole))
    say("  torch chain (onehot_both, permute, F.interpolate, permute; 79 times), host clock:          %s" % spread(chain))
    say("  chain / call = %.1f x" % (statistics.median(chain) / statistics.median(whole)))


def time_action(args, say):
    import torch
    import generate as cli
    from oracle import collate_items
    from _reference_checkpoint import unpack
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.harness import CHAR_FILES
    from handwriting_line_generation_amd.logger import load_checkpoint
    import pathlib
    d = pathlib.Path(tempfile.mkdtemp(prefix="film_bench_"))
    root = str(d / "iam")
    os.makedirs(root)
    collate_items.fake_iam(root, n_pages=8, with_images=True)
    ck = load_checkpoint(unpack("gan", d))
    ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
    ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
    path = str(d / "gan.pth")
    torch.save(ck, path)
    cfg = ck["config"]
    cfg["data_loader"].update(data_dir=root, batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"], augmentation=None, a_batch_size=2, max_width=640)
    cfg["validation"] = dict(cfg.get("validation", {}), batch_size=2, num_workers=0, augmentation=None, a_batch_size=2)
    cfg["trainer"]["style_together"] = True
    cfg_path = str(d / "gan.json")
    json.dump(cfg, open(cfg_path, "w"))
    kernel_path = ops.stretch_onehot

    def chain_path(label, ncls, scales):
        return [f.contiguous() for f in torch_chain(label, ncls, scales)]

    def run(which, k):
        import contextlib
        import io
        ops.stretch_onehot = kernel_path if which == "kernel" else chain_path
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                cli.main(["-c", path, "-f", cfg_path, "-d", str(d / ("%s_%d" % (which, k))), "-g", "0", "-r", "choice=s,batch=1"])
        finally:
            ops.stretch_onehot = kernel_path
        m = re.search(r"^lines (\d+)  seconds (\S+)", buf.getvalue(), flags=re.M)
        return int(m.group(1)), float(m.group(2))
    for which in ("kernel", "chain"):
        run(which, -1)
    times = {"kernel": [], "chain": []}
    lines = 0
    for k in range(args.runs):
        for which in ("kernel", "chain"):
            lines, seconds = run(which, k)
            times[which].append(seconds)
    say("generate.py -r choice=s,batch=1 on the fabricated dataset (2 lines, %d pictures), the action's own `seconds` (checkpoint loading excluded), runs alternating:" % lines)
    say("  labels by hwg_stretch_onehot: %s" % spread(times["kernel"]))
    say("  labels by the torch chain:    %s" % spread(times["chain"]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("generate_film_bench.py measures on the GPU: no HIP device is visible")
    torch.set_num_threads(1)
    rows = []

    def say(text):
        print(text, flush=True)
        rows.append(text)
    say("stretch film labels on one MI355X - tools/generate_film_bench.py --warmup %d --calls %d --repeats %d --runs %d" % (
        args.warmup, args.calls, args.repeats, args.runs))
    say("device: %s" % torch.cuda.get_device_name(0))
    time_labels(130, 2, 80, args, say)
    time_labels(400, 8, 80, args, say)
    time_action(args, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
