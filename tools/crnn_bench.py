"""Measure the CRNN recogniser's LSTM kernels on the GPU and write profiles/crnn_lstm.txt (not wired into bench.py).

  python tools/crnn_bench.py [--out profiles/crnn_lstm.txt] [--reps 20] [--steps 30]

Per layer (H = 512, both directions) at T = 126 and 302 (line widths 512 / 1216), B = 8 and 16:
  * hwg_lstm_fwd / hwg_lstm_bwd: the stream's span per call from device events around `reps` back-to-back calls, and the host's enqueue time
    per call (a host clock around the same calls, before the synchronise). One launch per time step: where the enqueue time is the larger of
    the two, the loop is bound by the host's launch rate, not by the kernels.
  * the same two layers through torch.nn.LSTM on the same GPU (MIOpen): what a user has without these kernels. Recorded, not a gate.
  * recogniser pre-training steps/s, CRNN beside CNN-only, same visit, synthetic lines of width 512 at the configs' batch size.
Every shape is warmed up before its timed window. There is no CPU fallback: without a GPU this tool fails.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def span_and_enqueue(fn, reps):
    """-> (device span per call, host enqueue time per call), microseconds"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, (t1 - t0) * 1e6 / reps


def lstm_rows(reps, dev):
    from handwriting_line_generation_amd import ops
    H = 512
    rows = []
    for T in (126, 302):
        for B in (8, 16):
            g = torch.Generator().manual_seed(T + B)
            s = 1.0 / np.sqrt(H)
            xp = [torch.randn(T, B, 4 * H, generator=g).to(dev).requires_grad_(True) for _ in range(2)]
            w = [((torch.rand(4 * H, H, generator=g) * 2 - 1) * s).to(dev) for _ in range(2)]
            b = [((torch.rand(4 * H, generator=g) * 2 - 1) * s).to(dev) for _ in range(2)]
            dy = torch.randn(T, B, 2 * H, generator=g).to(dev)
            with torch.no_grad():           # (no_grad: the kernel's ping-pong path, no gates written)
                fwd_eval = span_and_enqueue(lambda: ops.lstm_layer(xp, w, b, False), reps)
            fwd_train = span_and_enqueue(lambda: ops.lstm_layer(xp, w, b, True), reps)
            y = ops.lstm_layer(xp, w, b, True)
            bwd = span_and_enqueue(lambda: torch.autograd.grad(y, xp, dy, retain_graph=True), reps)     # dxproj only: the step loop alone
            m = torch.nn.LSTM(H, H, bidirectional=True, num_layers=1).to(dev)
            x = torch.randn(T, B, H, generator=g).to(dev).requires_grad_(True)
            with torch.no_grad():
                t_fwd = span_and_enqueue(lambda: m(x), reps)
            yt = m(x)[0]
            t_bwd = span_and_enqueue(lambda: torch.autograd.grad(yt, x, dy, retain_graph=True), reps)
            rows.append((T, B, fwd_eval, fwd_train, bwd, t_fwd, t_bwd))
    return rows


def steps_per_second(which, steps):
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.harness import build_simple_trainer
    rng.set_mode("device", seed=1)
    trainer, cfg = build_simple_trainer(which, width=512, label_len=30)
    for it in range(5):
        trainer._train_iteration(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(5, 5 + steps):
        trainer._train_iteration(it)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0), cfg["data_loader"]["batch_size"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crnn_lstm.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("crnn_bench needs the GPU (there is no CPU fallback and a CPU timing would say nothing)")
    dev = torch.device("cuda:0")
    lines = ["CRNN LSTM kernels (csrc/lstm.hip), one layer = both directions, H = 512; %s; reps %d" % (torch.cuda.get_device_name(0), a.reps),
             "span = device events around back-to-back calls, per call; enqueue = host clock around the same calls before the synchronise; microseconds",
             "%4s %3s | %-23s | %-23s | %-23s | %-23s | %-23s" % ("T", "B", "hwg fwd no_grad span/enq", "hwg fwd train span/enq", "hwg bwd (dxproj) span/enq",
                                                                    "nn.LSTM fwd span/enq", "nn.LSTM bwd span/enq")]
    for T, B, fe, ft, bw, tf, tb in lstm_rows(a.reps, dev):
        lines.append("%4d %3d | %10.0f / %-10.0f | %10.0f / %-10.0f | %10.0f / %-10.0f | %10.0f / %-10.0f | %10.0f / %-10.0f"
                     % ((T, B) + fe + ft + bw + tf + tb))
        lines.append("         per time step: fwd no_grad %.2f us, fwd train %.2f us, bwd %.2f us" % (fe[0] / T, ft[0] / T, bw[0] / T))
    for which in ("iam_hwr", "iam_hwr_crnn"):
        sps, bs = steps_per_second(which, a.steps)
        lines.append("pre-training %-13s width 512, batch %d: %.1f steps/s (%d timed steps after 5 warm-up)" % (which, bs, sps, a.steps))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
