"""The conditions of the forward convolution engines' fp64 tests (not collected by pytest): the bound's operation counts, the fp32 / absolute
restatement of each engine, the cached fp64 reference and check(), which turns a device output into |err| / bound and the yardstick ratio.
tests/test_conv_fp64_gpu.py holds the device to them (its docstring derives them), tests/test_conv_ref_cpu.py measures its seeded flaws
against them, tests/test_wgrad_fp64_gpu.py prints and asserts with the same check()."""
from oracle import conv_cases as CC
from oracle import conv_ref as R
from _fp64 import YARDSTICK_FACTOR, _ratio, _rel, cpu_threads

WINO_C = {"wino": 2 + 4 + 4, "s2": 2 + 2 + 4}


def extra_ops(c):
    """c of the bound: rounded operations past the contraction on the longest path to an output element"""
    return WINO_C.get(c["engine"], 0) + int(c["bias"]) + int(c["acc"]) + CC.pieces(c) - 1


def restate(c, x, w, b, y0, absolute=False):
    """the engine's own algorithm in the dtype of the operands"""
    fn = {"wino": R.wino_conv, "s2": R.wino_s2_conv}.get(c["engine"], R.conv_direct)
    return fn(x, w, CC.geom(c), b, y0, absolute=absolute)


def reference_of(c, x, w, b, y0, terms=None):
    """(fp64 direct form, relative L2 of the fp32 restatement of the engine's algorithm against it, per-element bound)"""
    cpu_threads()
    d = lambda t: None if t is None else t.double()
    ref = R.conv_direct(d(x), d(w), CC.geom(c), d(b), d(y0))
    yard = _rel(restate(c, x, w, b, y0), ref)
    A = restate(c, d(x), d(w), d(b), d(y0), absolute=True)
    return ref, yard, R.sum_bound((CC.contraction(c) if terms is None else terms) + extra_ops(c), A)


_REF = {}


def reference(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = reference_of(c, *CC.inputs(c))
    return _REF[c["name"]]


def check(c, y, ref, yard, bound, tag=""):
    rel = _rel(y, ref)
    ratio = _ratio(y, ref, bound)
    print("\nconv_fp64 %-34s %-5s rel %.3e yard %.3e (x%.2f) e/b %.3g%s" % (c["name"], c["engine"], rel, yard, rel / yard if yard > 0 else 0.0, ratio, tag))
    bad = []
    if not ratio <= 1.0:
        bad.append("|err| is %.3g x the derived bound" % ratio)
    if yard > 0 and rel > YARDSTICK_FACTOR * yard:
        bad.append("rel L2 %.3e is %.1f x the fp32 yardstick %.3e" % (rel, rel / yard, yard))
    assert not bad, "%s: %s" % (c["name"], "; ".join(bad))
