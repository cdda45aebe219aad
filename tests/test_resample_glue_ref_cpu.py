"""CPU: the restatements of the pool / resample / pad / layout / glue kernels (oracle/resample_ref.py) against torch's own ops and autograd
in fp64, their fp32 fixed-order twins against the fp64 ones, the bookkeeping of the GPU case tables (oracle/resample_cases.py: together the
tables reach every regime the kernels have, the second trip of the grid-stride loops included), and the sensitivity of those tables:
eighteen plausible kernel flaws, seeded into copies of the restatements that live in this file only, each move some case past the bound
tests/test_resample_glue_fp64_gpu.py holds that case to by SENSITIVITY_FACTOR or more, or flip one of its exact comparisons."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resample_cases as SC
from oracle import resample_ref as R
import _resample_glue_checks as G  # the references and bounds the GPU file holds the device to
from _fp64 import _d, _f, _ratio, cpu_threads
from _guarded import CANARY

SENSITIVITY_FACTOR = 10.0
TOL = 1e-10


cpu_threads()


def _leaf(t):
    return t.double().clone().requires_grad_(True)


def _close(a, b, what=""):
    assert tuple(a.shape) == tuple(b.shape), (what, tuple(a.shape), tuple(b.shape))
    torch.testing.assert_close(a.double(), b.double(), rtol=TOL, atol=TOL, equal_nan=True, msg=lambda m: "%s: %s" % (what, m))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _case(name):
    return [c for c in SC.NHWC_CASES if c[0] == name][0]


# ---- the restatements against torch --------------------------------------------------------------------------------------------------------
def _torch_nhwc(case):
    """-> {name: value} of the case from torch's own ops in fp64 (NCHW inside), the adjoint from autograd"""
    name, op, (N, H, W, C), prm = case
    x, dy, mask = SC.nhwc_inputs(case)
    xl = _leaf(_nchw(x))
    src = xl
    out = {}
    if op == "avgpool":
        y = F.avg_pool2d(src, prm["k"])
    elif op == "act_avgpool":
        z = src if mask is None else src * mask.double()[:, :, None, None]
        z = F.relu(z) if prm["act"] == SC.RELU else F.leaky_relu(z, SC.SLOPE) if prm["act"] == SC.LRELU else z
        y = F.avg_pool2d(z, prm["k"])
    elif op in ("maxpool", "maxpool_relu"):
        k, s, p = prm["geom"]
        y, idx = F.max_pool2d(src, k, s, p, return_indices=True)
        out["idx"] = _nhwc(idx).to(torch.int32)
        if op == "maxpool_relu":
            y = F.relu(y)
    elif op == "upsample":
        y = F.interpolate(src, scale_factor=tuple(float(f) for f in prm["f"]), mode="nearest")
    elif op == "blur":
        k1 = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
        k = (k1[:, None] * k1[None, :] / 16).expand(C, 1, 3, 3)
        y = F.conv2d(src, k, padding=1, groups=C)
    elif op == "pad":
        pt, pb, pl, pr, mode, value = prm["pad"]
        y = F.pad(src, (pl, pr, pt, pb), mode="replicate") if mode == 1 else F.pad(src, (pl, pr, pt, pb), value=value)
    y.backward(_nchw(dy.double()))
    out["y"], out["dx"] = _nhwc(y.detach()), _nhwc(xl.grad)
    return out


def _restated_nhwc(case):
    name, op, (N, H, W, C), prm = case
    x, dy, mask = SC.nhwc_inputs(case)
    X, DY = x.double(), dy.double()
    if op == "avgpool":
        return {"y": R.avgpool_fwd(X, *prm["k"]), "dx": R.avgpool_bwd(DY, H, W, *prm["k"])}
    if op == "act_avgpool":
        m = None if mask is None else mask.double()
        return {"y": R.act_avgpool_fwd(X, m, prm["act"], SC.SLOPE, *prm["k"]), "dx": R.act_avgpool_bwd(DY, X, m, prm["act"], SC.SLOPE, *prm["k"])}
    if op in ("maxpool", "maxpool_relu"):
        relu = op == "maxpool_relu"
        y, idx = R.maxpool_fwd(X, *prm["geom"], relu=relu)
        return {"y": y, "idx": idx, "dx": R.maxpool_bwd(DY, idx, H, W, y if relu else None)}
    if op == "upsample":
        return {"y": R.upsample_fwd(X, *prm["f"]), "dx": R.upsample_bwd(DY, *prm["f"])}
    if op == "blur":
        return {"y": R.blur3(X), "dx": R.blur3(DY)}
    return {"y": R.pad2d_fwd(X, *prm["pad"]), "dx": R.pad2d_bwd(DY, H, W, *prm["pad"][:5])}


@pytest.mark.parametrize("case", SC.NHWC_CASES, ids=[c[0] for c in SC.NHWC_CASES])
def test_nhwc_restatement_matches_torch(case):
    """values, adjoints (autograd) and, on every max-pool case, the saved indices: ties, NaN and infinities follow ATen"""
    name, op, shape, prm = case
    want, got = _torch_nhwc(case), _restated_nhwc(case)
    if prm.get("fill") == "special":
        # ATen's backward routes the gradient to the saved index: compare through the restated indices as well, NaN in y compared apart
        assert torch.equal(torch.isnan(got["y"]), torch.isnan(want["y"]))
    for k in want:
        if k == "idx":
            assert got[k].dtype == torch.int32 and torch.equal(got[k], want[k]), "%s: indices differ from ATen's" % name
        else:
            _close(got[k], want[k], "%s %s" % (name, k))
    # the outputs the GPU file holds to torch.equal and to bounds come from the same restatements: the fp32 twins stay within the sum bound
    exact, sums = G.nhwc_reference(case)
    if op == "act_avgpool":
        kk = prm["k"][0] * prm["k"][1]
        x, dy, mask = SC.nhwc_inputs(case)
        m = None if mask is None else mask.double().abs()
        by = R.sum_bound(kk + 3, R.act_avgpool_fwd(x.double().abs(), m, SC.NONE, 0.0, *prm["k"]))
        bx = R.sum_bound(4, R.act_avgpool_bwd(dy.double().abs(), x.double().abs() + 1, m, SC.NONE, 0.0, *prm["k"]))
        assert _ratio(exact["y"], got["y"], by) <= 1.0 and _ratio(exact["dx"], got["dx"], bx) <= 1.0, "%s: fp32 twin off the fp64 value" % name
    for k, v in exact.items():
        if op != "act_avgpool":
            assert G.same(v, got[k].to(v.dtype)), "%s %s: the exact reference is not the fp64 restatement rounded" % (name, k)
    for k, (ref, yard, bound) in sums.items():
        _close(ref, got[k], "%s %s" % (name, k))
        assert yard is not None and bool((bound >= 0).all())


def test_channel_and_layout_restatements_match_torch():
    for case in SC.COPY_CASES:
        name, rows, Cs, soff, Cd, doff, Cn, HW, bcast, acc = case
        src, dst = (t.double() for t in SC.copy_inputs(case))
        v = src[:, soff:soff + Cn]
        if bcast:
            v = v[:, None, :].expand(rows // HW, HW, Cn).reshape(rows, Cn)
        mid = dst[:, doff:doff + Cn] + v if acc else v
        _close(R.copy_channels(src, soff, dst, doff, Cn, HW, bcast, acc), torch.cat([dst[:, :doff], mid, dst[:, doff + Cn:]], 1), "copy " + name)
    for rows, C, Cpad in SC.PAD_CHANNEL_CASES:
        src = torch.randn(rows, C, dtype=torch.float64)
        _close(R.pad_channels(src, Cpad), F.pad(src, (0, Cpad - C)), "pad_channels")
    for case in SC.REDUCE_CASES:
        name, N, HW, Cs, soff, Cn, acc = case
        out, src, prev = G.reduce_values(case, _d)
        want = src.double().view(N, HW, Cs)[:, :, soff:soff + Cn].sum(1) + (prev.double() if acc else 0)
        _close(out["out"], want, "reduce " + name)
    for case in SC.ONEHOT_CASES:
        name, Lr, B, ncls, Cd, doff = case
        lab, prev = SC.onehot_labels(case)
        ok = (lab >= 0) & (lab < ncls)
        oh = F.one_hot(lab.long().clamp(0, ncls - 1), ncls).double() * ok[:, :, None]           # [L, B, ncls]
        blc, lbc = R.onehot_both(lab, ncls)
        _close(lbc, oh, "onehot lbc " + name)
        _close(blc, oh.transpose(0, 1), "onehot blc " + name)
        want = prev.double().clone()
        want[:, :, doff:doff + ncls] = oh.transpose(0, 1)
        _close(R.onehot(lab, ncls, Cd, doff, prev.double()), want, "onehot " + name)
        assert bool((~ok).any()) and float(blc.sum()) == float(ok.sum())
    x = torch.randn(SC.PERMUTE_DIMS, dtype=torch.float64)
    for perm in R.all_perms4():
        _close(R.permute4(x, [x.shape[p] for p in perm], [x.stride(p) for p in perm]), x.permute(perm), "permute %s" % (perm,))
    assert len(set(R.all_perms4())) == 24 and len(set(SC.PERMUTE_DIMS)) == 4


def _fused_weight_module(w3, mult):
    """the FusedUpsample weight as the module forms it: pad the scaled filter by one, average its four one-step shifts"""
    w = F.pad(w3 * mult, [1, 1, 1, 1])
    return (w[:, :, 1:, 1:] + w[:, :, :-1, 1:] + w[:, :, 1:, :-1] + w[:, :, :-1, :-1]) / 4


def test_fused_weight_and_col2im_restatements_match_torch():
    for AB in SC.FUSED_WEIGHT_CASES:
        w3, dw4, prev = G.fused_inputs(AB)
        wl = _leaf(w3)
        w4 = _fused_weight_module(wl, SC.FUSED_MULT)
        w4.backward(dw4.double())
        _close(R.fused_weight_fwd(w3.double(), SC.FUSED_MULT), w4.detach(), "fused fwd")
        _close(R.fused_weight_bwd(dw4.double(), SC.FUSED_MULT), wl.grad, "fused bwd")
        _close(R.fused_weight_bwd(dw4.double(), SC.FUSED_MULT, prev.double()), wl.grad + prev.double(), "fused bwd acc")
        mult = float(np.float32(SC.FUSED_MULT))
        absd = R.fused_weight_bwd(dw4.double().abs(), mult, prev.double().abs())
        assert _ratio(R.fused_weight_bwd_f32(dw4, mult, prev), R.fused_weight_bwd(dw4.double(), mult, prev.double()), R.sum_bound(7, absd)) <= 1.0
    for case in SC.COL2IM_CASES:
        name, N, H, W, R_, S, ph, pw, dh, dw = case
        t = SC.col2im_inputs(case).double()
        taps = torch.zeros(R_ * S, 1, R_, S, dtype=torch.float64)
        for r in range(R_):
            for s in range(S):
                taps[r * S + s, 0, r, s] = 1
        want = F.conv_transpose2d(t.permute(0, 3, 1, 2), taps, padding=(ph, pw), dilation=(dh, dw))[:, 0]
        _close(R.col2im_taps(t, H, W, R_, S, ph, pw, dh, dw), want, "col2im " + name)


def test_glue_restatements():
    g = SC.gen("glue_cpu")
    x, y = torch.randn(50, dtype=torch.float64, generator=g), torch.randn(50, dtype=torch.float64, generator=g)
    _close(R.axpby(x, 0.3, y, -2.0), torch.add(0.3 * x, y, alpha=-2.0))
    _close(R.axpby(x, 0.3), 0.3 * x)
    xs, sc, sh = torch.randn(6, 5, dtype=torch.float64, generator=g), torch.randn(5, dtype=torch.float64, generator=g), torch.randn(5, dtype=torch.float64, generator=g)
    _close(R.channel_affine(xs, sc, sh), torch.addcmul(sh.expand(6, 5), xs, sc.expand(6, 5)))
    _close(R.channel_affine(xs, None, sh), xs + sh)
    _close(R.channel_affine(xs, sc, None), xs * sc)
    for name, ws in SC.WSUM_CASES.items():
        t = SC.wsum_terms(name)
        xl = _leaf(t)
        total = (xl * torch.tensor(ws, dtype=torch.float64)).sum()
        total.backward(torch.tensor(1.7, dtype=torch.float64))
        tot, scaled = R.weighted_sum(list(t.double()), ws)
        # (the planted +-3e7 terms cancel: the 1e-10 is relative to the sum of the magnitudes, against the exactly rounded sum)
        exact = math.fsum(float(v) * w for v, w in zip(t.double(), ws))
        mag = sum(abs(float(v) * w) for v, w in zip(t.double(), ws))
        assert abs(float(tot) - exact) <= TOL * mag and abs(float(total.detach()) - exact) <= TOL * mag, "weighted_sum " + name
        _close(R.weighted_sum_bwd(torch.tensor(1.7, dtype=torch.float64), ws), xl.grad, "weighted_sum bwd")
        t32, s32 = R.weighted_sum_f32(t.numpy(), ws)
        w32 = [float(np.float32(w)) for w in ws]
        tot_r, scaled_r = R.weighted_sum(list(t.double()), w32)
        assert abs(float(t32) - float(tot_r)) <= float(R.sum_bound(2 * len(ws), torch.stack([v.abs() for v in scaled_r]).sum()))
        assert bool(((s32.double() - scaled_r).abs() <= R.U * scaled_r.abs()).all())
        if len(ws) > 2:      # the planted terms make the order matter: the reversed fp32 chain gives other bits
            assert float(R.weighted_sum_f32(t.numpy()[::-1], ws[::-1])[0]) != float(t32), name
    for case in SC.STYLE_MIX_CASES:
        bank, ij, w = SC.style_mix_inputs(case)
        want = bank.double()[ij[0].long()] * w[0].double()[:, None] + bank.double()[ij[1].long()] * w[1].double()[:, None]
        _close(R.style_mix(bank.double(), ij, w.double()), want)
        assert _ratio(R.style_mix_f32(bank, ij, w), want, R.sum_bound(2, R.style_mix(bank.double().abs(), ij, w.double().abs()))) <= 1.0
        assert int(ij[0, 0]) == int(ij[1, 0])


# ---- regime coverage ---------------------------------------------------------------------------------------------------------------------------
def test_tables_reach_every_required_regime():
    reached = SC.all_regimes()
    missing = sorted(SC.REQUIRED_REGIMES - reached)
    assert not missing, "no case reaches: %s" % missing
    assert len(SC.REQUIRED_REGIMES) > 150


def test_grid_cap_and_second_trips():
    """the work-item counts behind the 'second trip' tags, from the shapes, with the grid cap the library uses (hwg_stream_grid: at most
    2048 workgroups; 256 threads)"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "handwriting_line_generation_amd", "csrc", "hwg_common.h")) as f:
        src = f.read()
    assert "hwg_stream_grid" in src
    body = src[src.index("hwg_stream_grid"):][:400]
    assert str(SC.GRID_BLOCKS) in body, "the grid cap in hwg_common.h is not the one the case tables assume"
    assert SC.GRID_CAP == 2048 * 256 == 524288
    for op in SC.NHWC_OPS:
        for direction in ("fwd", "bwd"):
            big = []
            for c in SC.NHWC_CASES:
                if c[1] != op:
                    continue
                name, _, (N, H, W, C), prm = c
                n = int(np.prod(SC.out_shape(c))) if direction == "fwd" else N * H * W * C
                items = n // 4 if C % 4 == 0 else n
                if items > SC.GRID_CAP:
                    assert items % SC.GRID_CAP != 0, "%s: the last trip is full" % c[0]
                    big.append(c[0])
            assert big, "%s %s: no case takes a second trip" % (op, direction)
    assert all(int(np.prod(SC.out_shape(c))) < 2 ** 31 for c in SC.NHWC_CASES)


# ---- copies of the restatements with flaws behind flags (flaw=None: the arithmetic of oracle/resample_ref.py, checked below) -----------------
def avgpool_fwd(x, kh, kw, flaw=None):
    N, H, W, C = x.shape
    P, Q = H // kh, W // kw
    return x[:, :P * kh, :Q * kw].reshape(N, P, kh, Q, kw, C).sum((2, 4)) * (1.0 / (kh if flaw == "avg_divisor_kh" else kh * kw))


def avgpool_bwd(dy, H, W, kh, kw, flaw=None):
    N, P, Q, C = dy.shape
    dx = torch.zeros(N, H, W, C, dtype=dy.dtype)
    g = dy.repeat_interleave(kh, 1).repeat_interleave(kw, 2) * (1.0 / (kh * kw))
    dx[:, :P * kh, :Q * kw] = g
    if flaw == "avg_remainder_row_gets_gradient" and H > P * kh:
        dx[:, P * kh:, :Q * kw] = g[:, -(H - P * kh):]
    return dx


def maxpool_fwd(x, kernel, stride, pad, flaw=None):
    N, H, W, C = x.shape
    (kh, kw), (sh, sw), (ph, pw) = kernel, stride, pad
    P, Q = R.pool_out(H, kh, sh, ph), R.pool_out(W, kw, sw, pw)
    best = torch.full((N, P, Q, C), float("-inf"), dtype=x.dtype)
    idx = torch.full((N, P, Q, C), -1, dtype=torch.int64)
    for a in range(kh):
        h = torch.arange(P) * sh - ph + a
        for b in range(kw):
            w = torch.arange(Q) * sw - pw + b
            ok = ((h >= 0) & (h < H))[:, None] & ((w >= 0) & (w < W))[None, :]
            v = x[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)]
            better = (v >= best) if flaw == "max_last_wins" else (v > best)
            if flaw != "max_nan_dropped":
                better = better | torch.isnan(v)
            take = ok[None, :, :, None] & (better | (idx < 0))
            best = torch.where(take, v, best)
            here = (h[:, None] * (Q if flaw == "max_index_hQ" else W) + w[None, :])[None, :, :, None].expand_as(idx)
            idx = torch.where(take, here, idx)
    return best, idx.to(torch.int32)


def blur3(x, flaw=None):
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    y = torch.zeros_like(x)
    for a in range(3):
        for b in range(3):
            k = (2.0 if a == 1 else 1.0) * (2.0 if b == 1 else 1.0) / 16.0
            if flaw == "blur_corner_weight" and (a, b) == (2, 2):
                k = 2.0 / 16.0
            y = y + k * xp[:, a:a + H, b:b + W]
    return y


def pad2d_fwd(x, pt, pb, pl, pr, mode, value=0.0, flaw=None):
    N, H, W, C = x.shape
    s = -1 if flaw == "crop_offset_sign" else 1
    h, w = torch.arange(H + pt + pb) - s * pt, torch.arange(W + pl + pr) - s * pl
    okh, okw = (h >= 0) & (h < H), (w >= 0) & (w < W)
    h, w = h.clamp(0, H - 1), w.clamp(0, W - 1)
    y = x[:, h][:, :, w]
    if mode == 0:
        y = torch.where((okh[:, None] & okw[None, :])[None, :, :, None], y, torch.full_like(y, value))
    return y


def pad2d_bwd(dy, H, W, pt, pb, pl, pr, mode, flaw=None):
    N, P, Q, C = dy.shape
    h, w = torch.arange(P) - pt, torch.arange(Q) - pl
    okh, okw = (h >= 0) & (h < H), (w >= 0) & (w < W)
    keep = okh[:, None] & okw[None, :] if mode == 0 else torch.ones(P, Q, dtype=torch.bool)
    if flaw == "replicate_adjoint_misses_corner":
        keep = keep & (okh[:, None] | okw[None, :])
    dy = dy * keep[None, :, :, None].to(dy.dtype)
    t = torch.zeros(N, H, Q, C, dtype=dy.dtype).index_add_(1, h.clamp(0, H - 1), dy)
    return torch.zeros(N, H, W, C, dtype=dy.dtype).index_add_(2, w.clamp(0, W - 1), t)


def col2im_taps(t, H, W, R_, S, ph, pw, dh=1, dw=1, flaw=None):
    N, P, Q, RS = t.shape
    dx = torch.zeros(N, H, W, dtype=t.dtype)
    sg = -1 if flaw == "col2im_pad_sign" else 1
    for r in range(R_):
        p = torch.arange(H) + sg * ph - r * dh
        for s in range(S):
            q = torch.arange(W) + sg * pw - s * dw
            ok = ((p >= 0) & (p < P))[:, None] & ((q >= 0) & (q < Q))[None, :]
            tap = (R_ - 1 - r) * S + (S - 1 - s) if flaw == "col2im_taps_mirrored" else r * S + s
            dx = dx + t[:, p.clamp(0, P - 1)][:, :, q.clamp(0, Q - 1)][..., tap] * ok[None].to(t.dtype)
    return dx


def reduce_rows(src, soff, Cn, N, HW, out=None, flaw=None):
    s = src.reshape(N, HW, -1)[:, :256 if flaw == "reduce_drops_rows_from_256" else None, soff:soff + Cn].sum(1)
    return s if out is None else out + s


def copy_channels(src, soff, dst, doff, Cn, HW=1, bcast=0, accumulate=0, flaw=None):
    if flaw == "copy_ignores_doff":
        doff = 0
    out = dst.clone()
    srow = torch.arange(dst.shape[0]) // HW if bcast else torch.arange(dst.shape[0])
    v = src[srow, soff:soff + Cn]
    out[:, doff:doff + Cn] = out[:, doff:doff + Cn] + v if accumulate else v
    return out


def onehot(label, ncls, flaw=None):
    Lr, B = label.shape
    lab = label.reshape(B, Lr) if flaw == "onehot_swaps_L_and_B" else label.t()
    return (lab.long()[:, :, None] == torch.arange(ncls)[None, None, :]).double()


def fused_weight_fwd(w3, mult, flaw=None):
    sh = 1 if flaw == "fused_shift_off_by_one" else 0
    wp = torch.zeros(*w3.shape[:-2], 6, 6, dtype=w3.dtype)
    wp[..., 1:4, 1:4] = w3 * mult
    acc = torch.zeros(*w3.shape[:-2], 4, 4, dtype=w3.dtype)
    for dr in range(2):
        for ds in range(2):
            acc = acc + wp[..., dr + sh:dr + sh + 4, ds:ds + 4]
    return acc / 4


def style_mix_f32(bank, ij, w, flaw=None):
    i, j = (ij[1], ij[0]) if flaw == "style_mix_rows_swapped" else (ij[0], ij[1])
    bk, wn = bank.numpy(), w.numpy()
    return torch.from_numpy(bk[i.numpy()] * wn[0][:, None] + bk[j.numpy()] * wn[1][:, None])


def upsample_fwd(x, fh, fw, flaw=None):
    if flaw == "upsample_factors_swapped":
        fh, fw = fw, fh
    return x.repeat_interleave(fh, 1).repeat_interleave(fw, 2)


def _stale(ref, V):
    """what a kernel whose loop never takes its second trip leaves behind: everything past the first GRID_CAP work items keeps the buffer's
    earlier content (the canary value of the GPU file's buffers)"""
    out = ref.clone().reshape(-1)
    out[SC.GRID_CAP * V:] = CANARY
    return out.reshape(ref.shape)


def _moved(flawed, ent):
    """|flawed - reference| / bound, worst element: what the GPU test would report for a kernel with this flaw"""
    ref, yard, bound = ent
    return _ratio(flawed, ref, bound)


def _flaw_results():
    """flaw -> (how far it moves its case: worst |err| / bound, or inf for an exact comparison that flips; the same measure without the flaw)"""
    d, INF = _d, float("inf")
    flip = lambda bad, good, want: (INF if not G.same(bad, want) else 0.0, INF if not G.same(good, want) else 0.0)
    res = {}
    c = _case("avgpool_k22_c8")
    x, dy, _ = SC.nhwc_inputs(c)
    ent = G.nhwc_reference(c)[1]
    res["avg_divisor_kh"] = (_moved(avgpool_fwd(d(x), 2, 2, "avg_divisor_kh"), ent["y"]), _moved(avgpool_fwd(d(x), 2, 2), ent["y"]))
    c = _case("avgpool_k22_c3_rem")
    x, dy, _ = SC.nhwc_inputs(c)
    ent = G.nhwc_reference(c)[1]
    res["avg_remainder_row_gets_gradient"] = (_moved(avgpool_bwd(d(dy), 7, 11, 2, 2, "avg_remainder_row_gets_gradient"), ent["dx"]), _moved(avgpool_bwd(d(dy), 7, 11, 2, 2), ent["dx"]))
    for flaw, nm, key in (("max_last_wins", "maxpool_g22_c8_ties", 1), ("max_index_hQ", "maxpool_rec_c4_ties", 1), ("max_nan_dropped", "maxpool_g33_c6_special", 0)):
        c = _case(nm)
        x, dy, _ = SC.nhwc_inputs(c)
        want = G.nhwc_reference(c)[0][("y", "idx")[key]]
        res[flaw] = flip(maxpool_fwd(x, *c[3]["geom"], flaw=flaw)[key], maxpool_fwd(x, *c[3]["geom"])[key], want)
    c = _case("upsample_f32_c4")
    x, dy, _ = SC.nhwc_inputs(c)
    res["upsample_factors_swapped"] = flip(upsample_fwd(x, 3, 2, "upsample_factors_swapped"), upsample_fwd(x, 3, 2), G.nhwc_reference(c)[0]["y"])
    c = _case("blur_c8")
    x, dy, _ = SC.nhwc_inputs(c)
    ent = G.nhwc_reference(c)[1]
    res["blur_corner_weight"] = (_moved(blur3(d(x), "blur_corner_weight"), ent["y"]), _moved(blur3(d(x)), ent["y"]))
    c = _case("pad_rep_c4")
    x, dy, _ = SC.nhwc_inputs(c)
    ent = G.nhwc_reference(c)[1]
    a = (3, 4) + c[3]["pad"][:5]
    res["replicate_adjoint_misses_corner"] = (_moved(pad2d_bwd(d(dy), *a, flaw="replicate_adjoint_misses_corner"), ent["dx"]), _moved(pad2d_bwd(d(dy), *a), ent["dx"]))
    c = _case("pad_const_crop_all_c4")
    x, dy, _ = SC.nhwc_inputs(c)
    res["crop_offset_sign"] = flip(pad2d_fwd(x, *c[3]["pad"], flaw="crop_offset_sign"), pad2d_fwd(x, *c[3]["pad"]), G.nhwc_reference(c)[0]["y"])
    for flaw, nm in (("col2im_taps_mirrored", "lds3_tile"), ("col2im_pad_sign", "lds5_disc")):
        c = [k for k in SC.COL2IM_CASES if k[0] == nm][0]
        t = d(SC.col2im_inputs(c))
        ent = G.col2im_reference(c)["dx"]
        res[flaw] = (_moved(col2im_taps(t, *c[2:], flaw=flaw), ent), _moved(col2im_taps(t, *c[2:]), ent))
    c = [k for k in SC.REDUCE_CASES if k[0] == "hw257"][0]
    _, src, prev = G.reduce_values(c, d)
    ent = G.sums_of(lambda cast: G.reduce_values(c, cast)[0], {"out": 257})["out"]
    res["reduce_drops_rows_from_256"] = (_moved(reduce_rows(d(src), c[4], c[5], c[1], c[2], flaw="reduce_drops_rows_from_256"), ent), _moved(reduce_rows(d(src), c[4], c[5], c[1], c[2]), ent))
    c = [k for k in SC.COPY_CASES if k[0] == "soff_doff"][0]
    src, dst = SC.copy_inputs(c)
    a = (src, c[3], dst, c[5], c[6], c[7], c[8], c[9])
    res["copy_ignores_doff"] = flip(copy_channels(*a, flaw="copy_ignores_doff"), copy_channels(*a), G.copy_values(c, _f)["dst"])
    c = SC.ONEHOT_CASES[0]
    lab, _ = SC.onehot_labels(c)
    res["onehot_swaps_L_and_B"] = flip(onehot(lab, c[3], "onehot_swaps_L_and_B"), onehot(lab, c[3]), R.onehot(lab, c[3]))
    AB = SC.FUSED_WEIGHT_CASES[0]
    w3, dw4, prev = G.fused_inputs(AB)
    mult = float(np.float32(SC.FUSED_MULT))
    ent = G.sums_of(lambda cast: {"w4": R.fused_weight_fwd(cast(w3), mult)}, {"w4": 6})["w4"]
    res["fused_shift_off_by_one"] = (_moved(fused_weight_fwd(d(w3), mult, "fused_shift_off_by_one"), ent), _moved(fused_weight_fwd(d(w3), mult), ent))
    c = SC.STYLE_MIX_CASES[0]
    bank, ij, w = SC.style_mix_inputs(c)
    res["style_mix_rows_swapped"] = flip(style_mix_f32(bank, ij, w, "style_mix_rows_swapped"), style_mix_f32(bank, ij, w), R.style_mix_f32(bank, ij, w))
    c = _case("blur_big_v1")
    ent = G.nhwc_reference(c)[1]["y"]
    res["second_trip_never_taken_v1"] = (_moved(_stale(ent[0], 1), ent), _moved(ent[0], ent))
    c = _case("upsample_big_v4")
    want = G.nhwc_reference(c)[0]["y"]
    res["second_trip_never_taken_v4"] = flip(_stale(want, 4), want.clone(), want)
    return res


FLAWS = ("avg_divisor_kh", "avg_remainder_row_gets_gradient", "max_last_wins", "max_index_hQ", "max_nan_dropped", "upsample_factors_swapped",
         "blur_corner_weight", "replicate_adjoint_misses_corner", "crop_offset_sign", "col2im_taps_mirrored", "col2im_pad_sign",
         "reduce_drops_rows_from_256", "copy_ignores_doff", "onehot_swaps_L_and_B", "fused_shift_off_by_one", "style_mix_rows_swapped",
         "second_trip_never_taken_v1", "second_trip_never_taken_v4")


def test_every_seeded_flaw_moves_a_case_past_its_bound():
    res = _flaw_results()
    assert set(res) == set(FLAWS) and len(FLAWS) >= 14
    for flaw in FLAWS:
        with_flaw, without = res[flaw]
        print("%-36s moves its case to %.3g x the bound (without the flaw: %.3g)" % (flaw, with_flaw, without))
        assert without <= 1.0, "%s: the copy without the flaw is off the reference" % flaw
        assert with_flaw >= SENSITIVITY_FACTOR, "%s: moves its case by only %.3g x the bound" % (flaw, with_flaw)
