"""Measure recognize.py end to end on fabricated line images and print what profiles/recognize.txt quotes (not wired into bench.py).

    python tools/recognize_bench.py --lines 2000 --dir /tmp/recognize_bench            # fabricate, then four runs of the program
    python tools/recognize_bench.py --lines 2000 --dir /tmp/recognize_bench --only-prepare

Fabricates `--lines` PNG line images (seeded strokes on white; heights 40 .. 150, widths 60 .. 1400, each picture its own size) and unpacks
the reduced recogniser pre-training checkpoint of tests/golden. Then runs recognize.py as child processes, one at a time, each under its
own time limit, and stops at the first that fails: the default (device fit) and --host-fit, each once as it is (lines/s end to end) and
once with --timing (the device synchronised around every stage: the share of fit, recogniser and decode). The kernel's own time per batch
comes from a separate `rocprofv3 --kernel-trace --stats -- python recognize.py ...` run on the prepared directory."""
import argparse
import lzma
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def strokes(h, w, seed):
    g = np.random.RandomState(seed)
    img = np.full((h, w), 255, dtype=np.uint8)
    xs = np.arange(w)
    for _ in range(5):
        y = h * (0.5 + 0.3 * np.sin(xs / g.uniform(3.0, 25.0) + g.uniform(0, 6.28))) + g.uniform(-0.15, 0.15) * h
        t = g.randint(1, 4)
        yi = np.clip(y.astype(np.int64), t, h - 1 - t)
        for dy in range(-t, t):
            img[yi + dy, xs] = g.randint(0, 90)
    return img


def prepare(d, n):
    from PIL import Image
    lines = os.path.join(d, "lines")
    os.makedirs(lines, exist_ok=True)
    g = np.random.RandomState(0)
    for i in range(n):
        path = os.path.join(lines, "line_%05d.png" % i)
        if not os.path.exists(path):
            h = int(g.randint(40, 151))
            Image.fromarray(strokes(h, int(g.randint(60, 1401)), i)).save(path)
        else:
            g.randint(40, 151), g.randint(60, 1401)
    ck = os.path.join(d, "hwr.pth")
    if not os.path.exists(ck):
        with open(ck, "wb") as f:
            f.write(lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "ref_ckpt_hwr.pth.xz"), "rb").read()))
    return lines, ck


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2000)
    ap.add_argument("--dir", type=str, required=True)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--only-prepare", action="store_true")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per child")
    a = ap.parse_args()
    t0 = time.time()
    lines, ck = prepare(a.dir, a.lines)
    print("prepared %d lines in %s (%.1f s)" % (a.lines, lines, time.time() - t0), flush=True)
    if a.only_prepare:
        return
    outs = []
    for tag, extra in [("device", []), ("host-fit", ["--host-fit"]), ("device --timing", ["--timing"]), ("host-fit --timing", ["--host-fit", "--timing"])]:
        out = os.path.join(a.dir, "out_%s.txt" % tag.replace(" ", "").replace("-", ""))
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "recognize.py"), "-c", ck, "-i", lines, "-o", out, "--batch", str(a.batch)] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
        wall = time.time() - t0
        if r.returncode != 0:
            raise SystemExit("%s failed (%d):\n%s" % (tag, r.returncode, r.stdout[-3000:]))
        print("== %s: process wall %.2f s (interpreter start, torch import and checkpoint load included)" % (tag, wall))
        print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("lines ", "timing "))), flush=True)
        outs.append(open(out, "rb").read())
    print("output files identical: %s" % all(o == outs[0] for o in outs))


if __name__ == "__main__":
    main()
