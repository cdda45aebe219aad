#!/usr/bin/env python
"""Measurements behind profiles/umap_styles.txt (needs an MI355X): the two kernels of umap_styles.py at D = 128 (the shipped configs'
style_dim), n_neighbors = 35 (K = 34), for N = 2048 and 8192 rows of clustered Gaussian styles (N / 20 writers).

  * hwg_knn_rows: --warmup untimed calls, then --repeats windows of --calls calls each between two device events; the median window over
    the calls is the time of one call. Next to it the VALU bound: 2 lane operations per (row, column, d) - subtract, fused multiply-add -,
    2 N^2 D in all, against the part's fp32 vector rate (157.3 TFLOP/s counts a fused multiply-add as two: 78.6e12 lane operations per
    second). The merge is not in the bound.
  * hwg_umap_layout over the graph style_map.fuzzy_graph builds from those neighbours: one call of 500 epochs (500 launches) between two
    device events, median of --repeats; per epoch = that / 500.
  * the whole program, file to PNG: `umap_styles.py` as a child process on a style file of N = 2048 lines, wall clock (interpreter
    start, torch import and device initialisation included), next to style_map.embed alone in this process.
  * the only baseline there is: the numpy restatement (tests/_umap_ref.py) on the host at N = 2048 - neighbours, graph and --host-epochs
    layout epochs timed, the 500 epochs extrapolated from those. umap-learn is not installed, so there is no time of the reference's own
    path to compare with."""
import argparse
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LANE_OPS_PER_S = 157.3e12 / 2


def case(n, dim):
    import numpy as np
    rs = np.random.RandomState(n)
    writers = max(n // 20, 2)
    ids = rs.randint(0, writers, n)
    return (2.0 * rs.randn(writers, dim)[ids] + rs.randn(n, dim)).astype(np.float32), ids


def timed(fn, repeats):
    import torch
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--host-epochs", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement at N = 2048")
    ap.add_argument("--no-program", action="store_true", help="skip the child process")
    args = ap.parse_args()
    import numpy as np
    import torch
    from handwriting_line_generation_amd import ops, style_map
    import _umap_ref as ref
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    gpu = torch.device("cuda:0")
    print("command: %s" % " ".join(sys.argv))
    k, nn = 34, 35
    a, b = style_map.find_ab(1.0, 0.2)
    for n in (2048, 8192):
        styles, ids = case(n, args.dim)
        styles_d = torch.from_numpy(styles).to(gpu)
        out = (torch.empty((n, k), dtype=torch.int32, device=gpu), torch.empty((n, k), dtype=torch.float32, device=gpu))
        for _ in range(args.warmup):
            ops.knn_rows(styles_d, k, out=out)
        torch.cuda.synchronize()
        windows = [t / args.calls for t in timed(lambda: [ops.knn_rows(styles_d, k, out=out) for _ in range(args.calls)], args.repeats)]
        ms = statistics.median(windows)
        bound_ms = 2.0 * n * n * args.dim / LANE_OPS_PER_S * 1e3
        print("knn_rows N=%d D=%d K=%d: %.4f ms per call (median of %d windows of %d calls, min %.4f max %.4f); VALU bound %.4f ms -> %.1f %% of "
              "the fp32 vector rate" % (n, args.dim, k, ms, args.repeats, args.calls, min(windows), max(windows), bound_ms, 100.0 * bound_ms / ms),
              flush=True)
        row_ptr, col, period_q, _ = style_map.fuzzy_graph(out[0].cpu().numpy(), out[1].cpu().numpy(), nn, args.epochs)
        graph = ops.umap_graph(row_ptr, col, period_q, gpu)
        y0 = torch.from_numpy(style_map.pca_init(styles)).to(gpu)
        y, scratch = y0.clone(), torch.empty_like(y0)
        ops.umap_layout(graph, y, args.epochs, a, b, 5, 42, scratch=scratch)
        torch.cuda.synchronize()

        def whole():
            y.copy_(y0)
            ops.umap_layout(graph, y, args.epochs, a, b, 5, 42, scratch=scratch)
        runs = timed(whole, args.repeats)
        ms = statistics.median(runs)
        deg = np.diff(row_ptr)
        print("umap_layout N=%d E=%d (degrees %d..%d) neg=5: %d epochs %.3f ms (median of %d, min %.3f max %.3f) -> %.2f us per epoch" % (
            n, col.shape[0], deg.min(), deg.max(), args.epochs, ms, args.repeats, min(runs), max(runs), 1e3 * ms / args.epochs), flush=True)
        t0 = time.perf_counter()
        emb = style_map.embed(styles, gpu, n_epochs=args.epochs)
        dt = time.perf_counter() - t0
        print("style_map.embed N=%d: %.1f ms wall (upload, neighbours, graph on the host, %d epochs, download); finite %s" % (
            n, dt * 1e3, args.epochs, bool(np.isfinite(emb).all())), flush=True)
        if n == 2048 and not args.no_program:
            with tempfile.TemporaryDirectory() as d:
                with open(os.path.join(d, "bench_styles_1.pkl"), "wb") as f:
                    pickle.dump({"styles": styles[:, :, None, None], "authors": np.array(["w%d" % i for i in ids])}, f)
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, os.path.join(ROOT, "umap_styles.py"), os.path.join(d, "bench_styles_"), "-o",
                                    os.path.join(d, "map"), "--epochs", str(args.epochs)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                   text=True, timeout=600)
                dt = time.perf_counter() - t0
                assert r.returncode == 0 and os.path.exists(os.path.join(d, "map.png")), r.stdout[-2000:]
                print("umap_styles.py N=%d, file to PNG: %.2f s wall (one child process: interpreter, torch import, device initialisation, "
                      "the map, the %d-byte PNG)" % (n, dt, os.path.getsize(os.path.join(d, "map.png"))), flush=True)
        if n == 2048 and not args.no_host:
            t0 = time.perf_counter()
            idx, d2 = ref.knn(styles, k)
            t1 = time.perf_counter()
            g = ref.fuzzy_graph(idx, d2, nn, args.epochs)
            t2 = time.perf_counter()
            ref.layout(g[0], g[1], g[2], y0.cpu().numpy(), args.epochs, a, b, 5, 42, 0, args.host_epochs)
            t3 = time.perf_counter()
            per_epoch = (t3 - t2) / args.host_epochs
            print("numpy restatement on the host N=%d: neighbours %.2f s, graph %.2f s, layout %.1f ms per epoch over the first %d epochs -> %.1f s "
                  "for %d epochs extrapolated (%.1f s in all; the early epochs draw no fewer edges than the later ones)" % (
                      n, t1 - t0, t2 - t1, per_epoch * 1e3, args.host_epochs, per_epoch * args.epochs, args.epochs,
                      t2 - t0 + per_epoch * args.epochs), flush=True)


if __name__ == "__main__":
    main()
