#!/usr/bin/env python
"""Measurements behind profiles/writer_id.txt (needs an MI355X): hwg_writer_first_rank (both launches of one call: targets, counts) at
D = 128 for N = 2048, 8192 and --iam-lines (default 6161, the training lines of the IAM line-level partition), L1 and squared L2.

Per size and metric: --warmup untimed calls, then --repeats windows of --calls calls each between two device events; the median window
over the calls is the time of one call. Next to it the VALU bound: one call computes every distance twice (once per sweep), 2 lane
operations per (row, column, d) - subtract, then add-absolute or fused multiply-add -, i.e. 4 N^2 D lane operations, against the part's
fp32 vector rate (157.3 TFLOP/s counts a fused multiply-add as two: 78.6e12 lane operations per second). For N = 2048 only, the numpy
restatement (tests/_writer_id_ref.py) is timed on the host on the same input, once per metric, and its result is compared with the device's.
Under `rocprofv3 --kernel-trace --stats` the two launches' kernel times come apart (wid_sweep_kernel<metric, sweep>)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LANE_OPS_PER_S = 157.3e12 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iam-lines", type=int, default=6161)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement at N = 2048")
    args = ap.parse_args()
    import numpy as np
    import torch
    from handwriting_line_generation_amd import ops
    import _writer_id_ref as ref
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    gpu = torch.device("cuda:0")
    print("command: %s" % " ".join(sys.argv))
    for n in (2048, 8192, args.iam_lines):
        rs = np.random.RandomState(n)
        writers = max(n // 20, 2)
        ids = rs.randint(0, writers, n).astype(np.int32)
        styles = (0.3 * rs.randn(writers, args.dim)[ids] + rs.randn(n, args.dim)).astype(np.float32)
        styles_d, ids_d = torch.from_numpy(styles).to(gpu), torch.from_numpy(ids).to(gpu)
        out = (torch.empty(n, dtype=torch.int32, device=gpu), torch.empty(n, dtype=torch.float32, device=gpu))
        for name, metric in (("l1", ops.WID_L1), ("l2", ops.WID_L2)):
            for _ in range(args.warmup):
                ops.writer_first_rank(styles_d, ids_d, metric, out=out)
            torch.cuda.synchronize()
            windows = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    ops.writer_first_rank(styles_d, ids_d, metric, out=out)
                e1.record()
                e1.synchronize()
                windows.append(e0.elapsed_time(e1) / args.calls)
            ms = statistics.median(windows)
            bound_ms = 4.0 * n * n * args.dim / LANE_OPS_PER_S * 1e3
            print("N=%d D=%d %s: %.4f ms per call (median of %d windows of %d calls, min %.4f max %.4f); VALU bound %.4f ms -> %.1f %% of the "
                  "fp32 vector rate" % (n, args.dim, name, ms, args.repeats, args.calls, min(windows), max(windows), bound_ms,
                                        100.0 * bound_ms / ms), flush=True)
            if n == 2048 and not args.no_host:
                rank = out[0].cpu().numpy()
                t0 = time.perf_counter()
                want, _, _ = ref.first_rank(styles, ids, metric)
                dt = time.perf_counter() - t0
                print("N=%d D=%d %s: numpy restatement on the host %.1f ms (fp32; ranks differ from the device's on %d of %d rows: numpy sums "
                      "pairwise, near ties may fall the other way)" % (n, args.dim, name, dt * 1e3, int((want != rank).sum()), n), flush=True)


if __name__ == "__main__":
    main()
