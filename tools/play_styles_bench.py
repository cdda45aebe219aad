#!/usr/bin/env python
"""Measurements behind profiles/play_styles.txt (needs an MI355X): hwg_style_pair_stats against hwg_writer_first_rank (metric 1: squared
L2, both launches of one call) on the same input, in the same process, at D = 256 for N = 8192 and 16384.

Writer layouts: `iam` - sizes like those of an IAM split: mean 12 lines, a few single-line writers, one writer of 300 lines -, `distinct`
(every line its own writer: above 4096 writers only the two-cell mode runs, as in evaluate.style_distances) and `one` (a single writer).
Per layout the calls evaluate.style_distances makes: the sums (mode 1, the writer x writer cells; mode 0, the two cells) and the histogram
call (mode 0 with 64 bins between the extremes the first call found).

Per call kind: --warmup untimed calls, then --repeats rounds; a round times one window of --calls calls of EVERY kind, one kind after the
other, between two device events, so that a drift of the machine falls on all kinds alike; the median window over the calls is the time
of one call. The entry points are called as ops.style_pair_stats calls them, with the outputs and the workspace allocated once (the
wrapper's host-side check of the writer order is a device-to-host copy per call and is not part of the kernel's time).
The expectation under test: hwg_writer_first_rank sweeps all N^2 pairs twice, a style_pair_stats call visits N^2 / 2, so sums + histogram
together should cost no more than one hwg_writer_first_rank call, a quarter allowed on top for the fp64 root and the segmented sums:
ratio = (sums + histogram) / writer_first_rank <= 1.25. Next to each time the VALU bound of the distance part (2 lane operations per
(pair, d) against the fp32 vector rate)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANE_OPS_PER_S = 157.3e12 / 2


def writer_sizes(n, layout, rs):
    if layout == "one":
        return [n]
    if layout == "distinct":
        return [1] * n
    sizes, left = [300, 1, 1, 1, 1, 1], n - 305
    while left > 0:
        s = min(int(rs.randint(2, 23)), left)           # uniform 2 .. 22: mean 12
        sizes.append(s)
        left -= s
    return [sizes[i] for i in rs.permutation(len(sizes))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 16384])
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    from handwriting_line_generation_amd import _lib as L, evaluate, ops
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    gpu = torch.device("cuda:0")
    print("command: %s" % " ".join(sys.argv))
    for n in args.sizes:
        for layout in ("iam", "distinct", "one"):
            rs = np.random.RandomState(n)
            sizes = writer_sizes(n, layout, rs)
            A = len(sizes)
            ids = np.repeat(np.arange(A, dtype=np.int32), sizes)
            styles = (0.3 * rs.randn(A, args.dim)[ids] + rs.randn(n, args.dim)).astype(np.float32)
            styles_d, ids_d = torch.from_numpy(styles).to(gpu), torch.from_numpy(ids).to(gpu)
            stream = torch.cuda.current_stream().cuda_stream
            rank_out = (torch.empty(n, dtype=torch.int32, device=gpu), torch.empty(n, dtype=torch.float32, device=gpu))
            kinds = {"writer_first_rank l2": lambda: L.call("hwg_writer_first_rank", styles_d, ids_d, n, args.dim, 1, rank_out[0], rank_out[1], stream)}
            d2_range = ops.style_pair_stats(styles_d, ids_d, 0)[3].cpu().numpy()
            edge2 = ops.h2d(evaluate.pair_edges(d2_range[0], d2_range[1], args.bins)[1], gpu)
            keep = []

            def pair_call(mode, with_hist):
                cells = (2,) if mode == 0 else (A, A)
                need = int(L.query("hwg_style_pair_stats_workspace", n, A, mode))
                out = [torch.empty(cells, dtype=torch.int64, device=gpu), torch.empty(cells, dtype=torch.float64, device=gpu),
                       torch.empty(cells, dtype=torch.float64, device=gpu), torch.empty(2, dtype=torch.float32, device=gpu),
                       torch.empty((2, args.bins), dtype=torch.int64, device=gpu), torch.empty(need, dtype=torch.uint8, device=gpu)]
                keep.append(out)
                return need, lambda: L.call("hwg_style_pair_stats", styles_d, ids_d, n, args.dim, A, mode, edge2 if with_hist else None,
                                            args.bins if with_hist else 0, out[0], out[1], out[2], out[3], out[4] if with_hist else None, out[5],
                                            need, stream)
            workspace = {}
            workspace["sums mode 0"], kinds["sums mode 0"] = pair_call(0, False)
            if A <= ops.SP_MAX_WRITERS:
                workspace["sums mode 1"], kinds["sums mode 1"] = pair_call(1, False)
            workspace["histogram mode 0"], kinds["histogram mode 0"] = pair_call(0, True)
            for call in kinds.values():
                for _ in range(args.warmup):
                    call()
            torch.cuda.synchronize()
            windows = {k: [] for k in kinds}
            for _ in range(args.repeats):
                for k, call in kinds.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.calls):
                        call()
                    e1.record()
                    e1.synchronize()
                    windows[k].append(e0.elapsed_time(e1) / args.calls)
            ms = {k: statistics.median(w) for k, w in windows.items()}
            print("N=%d D=%d layout=%s writers=%d" % (n, args.dim, layout, A))
            for k in kinds:
                pairs = float(n) * n if k.startswith("writer") else 0.5 * n * (n - 1)
                sweeps = 2 if k.startswith("writer") else 1
                bound_ms = sweeps * 2.0 * pairs * args.dim / LANE_OPS_PER_S * 1e3
                print("  %-22s %8.4f ms per call (median of %d windows of %d calls, min %.4f max %.4f); VALU bound of the distances %.4f ms -> %.1f %%%s" % (
                    k, ms[k], args.repeats, args.calls, min(windows[k]), max(windows[k]), bound_ms, 100.0 * bound_ms / ms[k],
                    "" if k.startswith("writer") else "; workspace %.1f MB" % (workspace[k] / 1e6)))
            for sums in ("sums mode 1", "sums mode 0"):
                if sums in ms:
                    both = ms[sums] + ms["histogram mode 0"]
                    print("  %s + histogram = %.4f ms = %.3f x writer_first_rank (expected <= 1.25)" % (sums, both, both / ms["writer_first_rank l2"]),
                          flush=True)


if __name__ == "__main__":
    main()
