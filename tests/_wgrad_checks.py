"""The conditions of the weight-gradient kernels' fp64 tests (not collected by pytest): the restatement of each engine, T of the bound and the
cached fp64 references with their yardsticks and bounds. tests/test_wgrad_fp64_gpu.py holds the device to them (its docstring derives them),
tests/test_wgrad_ref_cpu.py measures its seeded flaws against them."""
import torch

from oracle import conv_ref as R
from oracle import wgrad_cases as WC
from _fp64 import _rel, cpu_threads


def restate(c, u, v, dw0, absolute=False):
    """the engine's own algorithm in the dtype of the operands: -> dw [R,S,K,C]"""
    fn = R.wino_wgrad if c["engine"] in ("wino", "s2") else R.wgrad_direct
    return fn(u, v, WC.geom(c), dw0, absolute=absolute)


def terms(c):
    """T of the bound: [R,S,1,1] pixels whose tap falls inside the image; the Winograd forms contract over the tiles"""
    N, H, W, C, K, Rr, S = c["shape"]
    if c["engine"] in ("wino", "s2"):
        mt = 3 if c["engine"] == "s2" else 2
        return torch.full((Rr, S, 1, 1), float(N * WC.cdiv(c["P"], mt) * WC.cdiv(c["Q"], mt)), dtype=torch.float64)
    return R.wgrad_terms(WC.geom(c), N, c["P"], c["Q"], H, W)


def reference_of(c, u, v, dw0, db0, T=None):
    """per set: (fp64 dw, yardstick, bound, fp64 bias gradient, its yardstick, its bound) - the bias entries None without a fused bias gradient"""
    cpu_threads()
    d = lambda t: None if t is None else t.double()
    p = WC.plan(c)
    T = terms(c) if T is None else T
    out = []
    for s in range(c["sets"]):
        us, vs = WC.operands(c, u, v, s)
        w0 = None if dw0 is None else dw0[s]
        ref = R.wgrad_direct(d(us), d(vs), WC.geom(c), d(w0))
        yard = _rel(restate(c, us, vs, w0), ref)
        bound = R.sum_bound(T + p["extra"], restate(c, d(us), d(vs), d(w0), absolute=True))
        rb = yb = bb = None
        if c["bias"]:
            b0 = None if db0 is None else db0[s]
            rb = R.colsum(d(us), d(b0))
            yb = _rel(R.colsum(us, b0), rb)
            bb = R.sum_bound(WC.pixels(c) + p["bias_extra"], R.colsum(d(us), d(b0), absolute=True))
        out.append((ref, yard, bound, rb, yb, bb))
    return out


_REF = {}


def reference(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = reference_of(c, *WC.inputs(c))
    return _REF[c["name"]]
