"""The references of the pool / resample / pad / layout / glue kernels' fp64 tests (not collected by pytest): per case the outputs held to
torch.equal and the outputs that are sums, with yardstick and bound, cached. tests/test_resample_glue_fp64_gpu.py holds the device to them,
tests/test_resample_glue_ref_cpu.py seeds its flaws against them."""
import torch

from oracle import resample_cases as SC
from oracle import resample_ref as R
from _fp64 import _a, _d, _f, cpu_threads, entry


def same(got, want):
    """torch.equal with the NaN positions compared apart; the dtype has to match (int32 indices)"""
    got = got.detach().cpu()
    if got.dtype != want.dtype or tuple(got.shape) != tuple(want.shape):
        return False
    if want.dtype.is_floating_point:
        gn, wn = torch.isnan(got), torch.isnan(want)
        return torch.equal(gn, wn) and torch.equal(got.masked_fill(gn, 0), want.masked_fill(wn, 0))
    return torch.equal(got, want)


_REF = {}


def _cached(key, fn):
    if key not in _REF:
        cpu_threads()
        _REF[key] = fn()
    return _REF[key]


def sums_of(fn, K):
    """fn(cast) -> {name: value}; K: {name: terms}; -> {name: entry} with the bound from the same restatement on absolute values"""
    ref, yard, absv = fn(_d), fn(_f), fn(_a)
    return {k: entry(v, yard[k], R.sum_bound(K[k], absv[k])) for k, v in ref.items()}


def nhwc_K(case):
    name, op, shape, prm = case
    if op == "avgpool":
        return {"y": prm["k"][0] * prm["k"][1] + 1, "dx": 1}
    if op in ("maxpool", "maxpool_relu"):
        (kh, kw), (sh, sw), _ = prm["geom"]
        return {"dx": -(-kh // sh) * -(-kw // sw)}
    if op == "upsample":
        return {"dx": prm["f"][0] * prm["f"][1]}
    if op == "blur":
        return {"y": 9, "dx": 9}
    if op == "pad" and prm["pad"][4] == 1:
        pt, pb, pl, pr = prm["pad"][:4]
        return {"dx": (max(pt, pb) + 1) * (max(pl, pr) + 1)}
    return {}


def nhwc_sum_values(case, cast, M=R):
    """the outputs of the case that are sums, in the dtype of `cast`"""
    name, op, (N, H, W, C), prm = case
    x, dy, mask = SC.nhwc_inputs(case)
    K = nhwc_K(case)
    if op == "avgpool":
        return {"y": M.avgpool_fwd(cast(x), *prm["k"]), "dx": M.avgpool_bwd(cast(dy), H, W, *prm["k"])}
    if op in ("maxpool", "maxpool_relu") and K["dx"] > 1:
        y, idx = M.maxpool_fwd(x, *prm["geom"], relu=op == "maxpool_relu")
        return {"dx": M.maxpool_bwd(cast(dy), idx, H, W, y if op == "maxpool_relu" else None)}
    if op == "upsample":
        return {"dx": M.upsample_bwd(cast(dy), *prm["f"])}
    if op == "blur":
        return {"y": M.blur3(cast(x)), "dx": M.blur3(cast(dy))}
    if op == "pad" and prm["pad"][4] == 1:
        return {"dx": M.pad2d_bwd(cast(dy), H, W, *prm["pad"][:5])}
    return {}


def nhwc_exact_values(case, M=R):
    """the outputs of the case that are held to torch.equal"""
    name, op, (N, H, W, C), prm = case
    x, dy, mask = SC.nhwc_inputs(case)
    if op == "act_avgpool":
        return {"y": M.act_avgpool_fwd_f32(x, mask, prm["act"], SC.SLOPE, *prm["k"]),
                "dx": M.act_avgpool_bwd_f32(dy, x, mask, prm["act"], SC.SLOPE, *prm["k"])}
    if op in ("maxpool", "maxpool_relu"):
        y, idx = M.maxpool_fwd(x, *prm["geom"], relu=op == "maxpool_relu")
        out = {"y": y, "idx": idx}
        if nhwc_K(case)["dx"] == 1:
            out["dx"] = M.maxpool_bwd(dy, idx, H, W, y if op == "maxpool_relu" else None)
        return out
    if op == "upsample":
        return {"y": M.upsample_fwd(x, *prm["f"])}
    if op == "pad":
        out = {"y": M.pad2d_fwd(x, *prm["pad"])}
        if prm["pad"][4] == 0:
            out["dx"] = M.pad2d_bwd(dy, H, W, *prm["pad"][:5])
        return out
    return {}


def nhwc_reference(case):
    return _cached(("nhwc", case[0]), lambda: (nhwc_exact_values(case), sums_of(lambda cast: nhwc_sum_values(case, cast), nhwc_K(case))))


def copy_values(case, cast, M=R):
    name, rows, Cs, soff, Cd, doff, Cn, HW, bcast, acc = case
    src, dst = SC.copy_inputs(case)
    return {"dst": M.copy_channels(cast(src), soff, cast(dst), doff, Cn, HW, bcast, acc)}


def reduce_values(case, cast, M=R):
    name, N, HW, Cs, soff, Cn, acc = case
    g = SC.gen("reduce_" + name)
    src, prev = torch.randn(N * HW, Cs, generator=g), torch.randn(N, Cn, generator=g)
    return {"out": M.reduce_rows(cast(src), soff, Cn, N, HW, cast(prev) if acc else None)}, src, prev


def fused_inputs(AB):
    g = SC.gen("fused_%dx%d" % AB)
    return torch.randn(*AB, 3, 3, generator=g), torch.randn(*AB, 4, 4, generator=g), torch.randn(*AB, 3, 3, generator=g)


def col2im_reference(case):
    name, N, H, W, R_, S, ph, pw, dh, dw = case
    t = SC.col2im_inputs(case)
    return _cached(("col2im", name), lambda: sums_of(lambda cast: {"dx": R.col2im_taps(cast(t), H, W, R_, S, ph, pw, dh, dw)}, {"dx": R_ * S}))
