"""The references of the style-path and expert-bank kernels' fp64 tests (not collected by pytest): per family the values in fp64, in fp32
(the yardstick) and in absolute value (the bound's A), cached per case. tests/test_style_expert_fp64_gpu.py holds the device to them (its
docstring lists the bounds), tests/test_style_expert_ref_cpu.py seeds its flaws against them."""
import numpy as np
import torch

from oracle import style_cases as SC
from oracle import style_ref as R
from _fp64 import _a, _d, _f, cpu_threads, entry

_REF = {}


def _cached(key, fn):
    if key not in _REF:
        cpu_threads()
        _REF[key] = fn()
    return _REF[key]


def conv_values(case, cast, fwd=R.grouped_conv_fwd, wgrad=R.grouped_conv_wgrad):
    name, Cin, Cout, S, R_, plan, bias = case
    x, dy, Ws, bs, gW, gb = SC.conv_inputs(case)
    cls = SC.plan_cls(plan, R_)
    X, DY, W = cast(x), cast(dy), [cast(w) for w in Ws]
    out = {"y": fwd(X, cls, W, [cast(b) for b in bs] if bias else None, S), "dx": R.grouped_conv_dgrad(DY, cls, W, S)}
    for e, (dW, db) in wgrad(DY, X, cls, S).items():
        out["dW%d" % e] = cast(gW[e]) + dW
        if bias:
            out["db%d" % e] = cast(gb[e]) + db
    return out


def conv_reference(case):
    def make():
        name, Cin, Cout, S, R_, plan, bias = case
        ref, yard, absv = conv_values(case, _d), conv_values(case, _f), conv_values(case, _a)
        rows = {e: n * R_ for e, n in SC.PLANS[plan][R_].items()}
        K = {"y": Cin * S + 1, "dx": Cout * S}
        return {k: entry(v, yard[k], R.sum_bound(K[k] if k in K else rows[int(k[2:])] + 1, absv[k])) for k, v in ref.items()}
    return _cached(("conv", case[0]), make)


def accumulate_reference(C):
    def make():
        g = SC.gen("accumulate_%d" % C)
        cls = np.concatenate([np.full(n, e, dtype=np.int64) for e, n in sorted(SC.ACCUMULATE_RUNS.items())])
        rows = torch.randn(cls.size, C, generator=g)
        pre = torch.randn(SC.E, C, generator=g) * 3
        vals = [{e: cast(pre[e]) + s for e, s in R.segment_accumulate(cast(rows), cls).items()} for cast in (_d, _f, _a)]
        refs = {"g%d" % e: entry(vals[0][e], vals[1][e], R.sum_bound(SC.ACCUMULATE_RUNS[e] + 1, vals[2][e])) for e in vals[0]}
        return cls, rows, pre, refs
    return _cached(("acc", C), make)


def window_reference(case, scatter=R.scatter_windows):
    def make():
        name, B, Wx, C, w = case
        x, ib, ip, dp, n_in = SC.window_inputs(case)
        vals = [scatter(cast(dp), ib, ip, w, B, Wx) for cast in (_d, _f, _a)]
        return R.gather_windows(x, ib, ip, w), {"dx": entry(vals[0], vals[1], R.sum_bound(2 * w + 1, vals[2]))}
    return _cached(("win", case[0], scatter), make)


def seg_reference(case, fwd=R.segment_mean):
    def make():
        name, n, B, C, kind = case
        v, wgt, seg, dout = SC.seg_inputs(case)
        out64, ws64 = fwd(_d(v), _d(wgt), seg, B)
        out32, ws32 = fwd(v, wgt, seg, B)
        out_b, ws_rel = R.segment_mean_bound(_d(v), _d(wgt), seg, B)
        dv64 = R.segment_mean_bwd(_d(dout), _d(wgt), seg, ws64)
        dv32 = R.segment_mean_bwd(dout, wgt, seg, ws32)
        # dv = wgt / wsum * dout: the kernel's wsum carries its relative error, the division and the product one rounding each
        dv_b = dv64.abs() * (2 * ws_rel[seg.long()] + 3 * R.U)[:, None]
        return {"out": entry(out64, out32, out_b), "dv": entry(dv64, dv32, dv_b)}
    return _cached(("seg", case[0], fwd), make)


def bank_values(case, cast, fwd=R.linear_bank_fwd, bwd=R.linear_bank_bwd):
    name, B, I, O, halves, unused, frozen, xgrad, backward = case
    x, Ws, bs, dys, gW, gb = SC.bank_inputs(case)
    X, W = cast(x), [cast(w) for w in Ws]
    out = {"y%d_%d" % (l, h): t for l, parts in enumerate(fwd(X, W, [cast(b) for b in bs], halves)) for h, t in enumerate(parts)}
    if backward:
        dx, dWs, dbs = bwd(X, W, [[cast(p) if p is not None else None for p in parts] for parts in dys], halves)
        if xgrad:
            out["dx"] = dx
        for l in range(len(O)):
            if l not in frozen:
                out["dW%d" % l] = cast(gW[l]) + dWs[l]
            if frozen.get(l) != "all":
                out["db%d" % l] = cast(gb[l]) + dbs[l]
    return out


def bank_reference(case):
    def make():
        name, B, I, O, halves, unused, frozen, xgrad, backward = case
        ref, yard, absv = bank_values(case, _d), bank_values(case, _f), bank_values(case, _a)
        K = lambda k: I + 1 if k[0] == "y" else sum(O) if k == "dx" else B + 1
        return {k: entry(v, yard[k], R.sum_bound(K(k), absv[k])) for k, v in ref.items()}
    return _cached(("bank", case[0]), make)


def chain_values(case, cast, passes=2, fwd=R.mlp_chain_fwd, bwd=R.mlp_chain_bwd):
    """forward output, and after `passes` backward passes in a row: d x and the parameter gradients added to their pre-filled values"""
    name, D, B, L, frozen, backward = case
    x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
    W, Bv = [cast(w) for w in Ws], [cast(b) for b in bs]
    acts = fwd(cast(x), W, Bv, SC.CHAIN_SLOPE)
    out = {"h": acts[-1]}
    if backward:
        dx, dWs, dbs = bwd(cast(dout), acts, W, SC.CHAIN_SLOPE)
        out["dx"] = passes * dx
        for l in range(L):
            if l != frozen:
                out["dW%d" % l] = cast(gW[l]) + passes * dWs[l]
                out["db%d" % l] = cast(gb[l]) + passes * dbs[l]
    return out, acts


def chain_reference(case):
    def make():
        x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
        (ref, acts), (yard, _) = chain_values(case, _d), chain_values(case, _f)
        hb = R.chain_fwd_bound(acts, [_d(w) for w in Ws], [_d(b) for b in bs])
        return {k: entry(v, yard[k], hb if k == "h" else None) for k, v in ref.items()}
    return _cached(("chain", case[0]), make)
