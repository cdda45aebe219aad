"""The shared arithmetic of the comparisons against fp64 (not collected by pytest): the project's constants, the casts, and the error
measures the *_fp64_gpu, *_abi_* and *_ref_cpu tests hold outputs to."""
import os
import zlib

import torch

YARDSTICK_FACTOR = 10.0      # the project's constant: a result this many times worse than the fp32 CPU restatement of the same algorithm is a
                             # finding, not something a bound absorbs (it absorbs summation-order differences between a kernel's chains and torch's sums)
U = 2.0 ** -24               # one fp32 rounding, relative
SECOND = 1 + 2.0 ** -16      # second-order terms of a first-order error sum


def cpu_threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _d(t):
    return t.double()


def _f(t):
    return t.float()


def _a(t):
    return t.double().abs()


def _f32(v):
    """a Python float as the kernels receive it"""
    return float(torch.tensor(v, dtype=torch.float32))


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _rel(got, want):
    d = got.detach().cpu().double() - want.double()
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    return float(d.norm()) / max(float(want.double().norm()), 1e-300)


def entry(ref, yard32=None, bound=None):
    """one output of a reference: the fp64 value, the yardstick (relative L2 of the fp32 CPU restatement, None: not a sum), the bound"""
    return (ref, None if yard32 is None else _rel(yard32, ref), bound)


def _ratio(got, want, bound):
    """worst |err| / bound over the elements (an element with a bound of 0 must be exact)"""
    err = (got.detach().cpu().double() - want).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _ratio_rows(got, want, bound):
    """_ratio, but a bound with one dimension less than the output holds the L2 norm of the error of every row (_ratio would broadcast it)"""
    err = (got.detach().cpu().double() - want).abs()
    if bound.dim() == err.dim() - 1:
        err = err.norm(dim=-1)
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def ratios(got, want, bound, size=None):
    """(relative L2 / its bound, max|err| / max|ref| / its bound); inf for a non-finite output. `size`: the float64 tensor whose size the
    error is measured against instead of want's (where want is the small difference of large terms)"""
    got = got.detach().cpu().double().reshape(want.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    d = got - want
    size = want if size is None else size
    return (float(d.norm()) / max(float(size.norm()), 1e-300) / bound[0], float(d.abs().max()) / max(float(size.abs().max()), 1e-300) / bound[1])


def report(entry, shape, ws_bytes, checks):
    """checks: [(name, got, want float64, bound[, size])], or (name, ratio) for an error-to-bound ratio the caller formed itself (per-element
    bounds, yardsticks) -> prints the case's line, returns what is over its bound"""
    parts, bad = [], []
    for name, got, *rest in checks:
        if not rest:
            parts.append("%s %.2f" % (name, got))
            if not got <= 1.0:
                bad.append("%s: %.3g x what it is held to" % (name, got))
            continue
        want, bound, *size = rest
        r = ratios(got, want, bound, *size)
        parts.append("%s %.2f/%.2f" % (name, r[0], r[1]))
        if not (r[0] <= 1.0 and r[1] <= 1.0):
            bad.append("%s: relative L2 %.3g x, max/max %.3g x its bound (%.1e, %.1e)" % (name, r[0], r[1], bound[0], bound[1]))
    print("\nabi %-22s %-34s ws %-9d e/b %s" % (entry, shape, ws_bytes, "  ".join(parts) if parts else "-"))
    return bad
