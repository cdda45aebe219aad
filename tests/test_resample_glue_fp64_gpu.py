"""GPU: the memory-bound kernels of csrc/pool_resample.hip (average / activation + average / max pools, nearest upsample, blur, 2-D padding,
channel copies, pad_channels, reduce_rows, one-hot, permute4, the FusedUpsample weight, col2im_taps) and the glue kernels at the end of
csrc/spectral_loss.hip (axpby, mul, channel_affine, weighted_sum, style_mix) against the restatements of oracle/resample_ref.py, at every
regime of the kernels (case tables and the regimes they cover: oracle/resample_cases.py; the restatements, the tables and their sensitivity
to seeded flaws are checked on the CPU by tests/test_resample_glue_ref_cpu.py; the references and their bounds:
tests/_resample_glue_checks.py; the buffers: tests/_guarded.py). The library's default path only. The entry points are
called through L.call on buffers carved out of one allocation with canaries before, between and after them; the ops.py wrappers that had no
unit test run through autograd.

One line per case is printed: per output the relative L2 error and max|err| / max|ref| against fp64, the yardstick (the same restatement in
fp32 torch on the CPU against the same fp64 value) and the worst |err| / bound over the elements. No bound comes from the kernels:

  family                                           bound                                              measured on an MI355X
  copies, gathers, pad / upsample forward,         torch.equal (NaN positions compared apart,          -
  one-hot, permute, promised zeros, max pool       integer dtype for the indices)
  values and indices, constant-pad adjoint
  act_avgpool fwd / bwd, weighted_sum fwd / bwd,   torch.equal to the fp32 restatement in the          -
  style_mix, fused weight adjoint (both)           kernel's order of rounded operations
  avg pool fwd / bwd                               (K + 2) 2^-24 sum|terms|, K = kh kw + 1 / 1         -
  max pool adjoint, overlapping windows            the same, K = ceil(kh / sh) ceil(kw / sw)           -
  upsample adjoint                                 the same, K = fh fw                                 -
  blur                                             the same, K = 9                                     -
  replicate-pad adjoint                            the same, K = the largest window                    -
  copy_channels accumulate                         the same, K = 2                                     -
  reduce_rows                                      the same, K = HW (+ 1 with accumulate)              -
  col2im_taps                                      the same, K = R S                                   -
  fused weight fwd                                 the same, K = 4 + 2                                 -
  axpby, channel_affine                            2 ulp of |a x| + |b y|: 2 * 2^-23 (|a x| + |b y|)   -
  mul                                              half an ulp: 2^-24 |a b|                            -
(No errors measured on an MI355X stand in the last column yet: every case prints its own on the line it writes.)
Every output that is a sum is also held to YARDSTICK_FACTOR times its yardstick in relative L2 (a yardstick of exactly zero: the derived
bound alone)."""
import numpy as np
import pytest
import torch

from oracle import resample_cases as SC
from oracle import resample_ref as R
from _fp64 import YARDSTICK_FACTOR, _d, _f, _ratio, entry
from _guarded import CANARY, carve, put
from _resample_glue_checks import (_cached, col2im_reference, copy_values, fused_inputs, nhwc_reference, reduce_values, same,
                                    sums_of)

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def _check(label, outs, exact, sums, note=""):
    """outs: {name: kernel output}; exact: {name: tensor} held to torch.equal; sums: {name: entry} held to the derived bound per element
    and to the yardstick; every output must be in one of them; prints one line"""
    txts, bad = [], []
    for name, got in outs.items():
        assert (name in exact) != (name in sums), "%s %s: nothing (or two things) to hold the output to" % (label, name)
        if name in exact:
            ok = same(got, exact[name])
            txts.append("%s %s" % (name, "equal" if ok else "NOT EQUAL"))
            if not ok:
                g = got.detach().cpu()
                n = int((g != exact[name]).sum()) if g.shape == exact[name].shape else -1
                bad.append("%s: differs from the exact value in %d elements" % (name, n))
            continue
        want, yard, bound = sums[name]
        assert tuple(got.shape) == tuple(want.shape), (label, name, tuple(got.shape), tuple(want.shape))
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (label, name)
        d = got.detach().cpu().double() - want
        rel = float(d.norm()) / max(float(want.norm()), 1e-300)
        mx = float(d.abs().max()) / max(float(want.abs().max()), 1e-300) if d.numel() else 0.0
        txt = "%s %.2e/%.2e" % (name, rel, mx)
        if yard is not None:
            txt += " yard %.2e" % yard
            if yard > 0 and rel > YARDSTICK_FACTOR * yard:
                bad.append("%s: rel L2 %.3e is %.1f x the fp32 yardstick %.3e" % (name, rel, rel / yard, yard))
        r = _ratio(got, want, bound)
        txt += " e/b %.2g" % r
        if not r <= 1.0:
            bad.append("%s: |err| is %.3g x the derived bound" % (name, r))
        txts.append(txt)
    print("\n%-34s %s%s" % (label, "  ".join(txts), note))
    assert not bad, "%s: %s" % (label, "; ".join(bad))




def axpby_bound(ax, by=None):
    return 2 * ULP * (ax.double().abs() + (0 if by is None else by.double().abs()))


def _numel(shape):
    return int(np.prod(shape))


# ---- the vectorised NHWC kernels ---------------------------------------------------------------------------------------------------------
def run_nhwc(case, dev):
    from handwriting_line_generation_amd import _lib as L, ops
    name, op, shape, prm = case
    N, H, W, C = shape
    x, dy, mask = SC.nhwc_inputs(case)
    oshape = SC.out_shape(case)
    ni, no = x.numel(), _numel(oshape)
    (xd, dyd, yd, dxd, idxd, md), intact = carve(dev, ni, no, no, ni, no, N * C)
    put(xd, x); put(dyd, dy)
    idx = idxd.view(torch.int32)
    st = ops._stream()
    outs = {"y": yd.view(oshape), "dx": dxd.view(shape)}
    if op == "avgpool":
        kh, kw = prm["k"]
        L.call("hwg_avgpool_fwd", xd, yd, N, H, W, C, kh, kw, st)
        L.call("hwg_avgpool_bwd", dyd, dxd, N, H, W, C, kh, kw, st)
    elif op == "act_avgpool":
        kh, kw = prm["k"]
        m = put(md, mask) if mask is not None else None
        L.call("hwg_act_avgpool_fwd", xd, m, yd, N, H, W, C, kh, kw, prm["act"], SC.SLOPE, st)
        L.call("hwg_act_avgpool_bwd", dyd, xd, m, dxd, N, H, W, C, kh, kw, prm["act"], SC.SLOPE, st)
    elif op in ("maxpool", "maxpool_relu"):
        (kh, kw), (sh, sw), (ph, pw) = prm["geom"]
        P, Q = oshape[1], oshape[2]
        geo = (N, H, W, C, kh, kw, sh, sw, ph, pw, P, Q)
        if op == "maxpool":
            L.call("hwg_maxpool_fwd", xd, yd, idx, *geo, st)
            L.call("hwg_maxpool_bwd", dyd, idx, dxd, *geo, st)
        else:
            L.call("hwg_maxpool_relu_fwd", xd, yd, idx, *geo, st)
            L.call("hwg_maxpool_relu_bwd", dyd, yd, idx, dxd, *geo, st)
        outs["idx"] = idx.view(oshape)
    elif op == "upsample":
        fh, fw = prm["f"]
        L.call("hwg_upsample_nearest_fwd", xd, yd, N, H, W, C, fh, fw, st)
        L.call("hwg_upsample_nearest_bwd", dyd, dxd, N, H, W, C, fh, fw, st)
    elif op == "blur":
        L.call("hwg_blur3", xd, yd, N, H, W, C, st)
        L.call("hwg_blur3", dyd, dxd, N, H, W, C, st)        # its own adjoint, on the output-sized gradient (same shape)
    elif op == "pad":
        pt, pb, pl, pr, mode, value = prm["pad"]
        L.call("hwg_pad2d_fwd", xd, yd, N, H, W, C, pt, pb, pl, pr, mode, value, st)
        L.call("hwg_pad2d_bwd", dyd, dxd, N, H, W, C, pt, pb, pl, pr, mode, st)
    torch.cuda.synchronize()
    return outs, intact


@pytest.mark.parametrize("case", SC.NHWC_CASES, ids=[c[0] for c in SC.NHWC_CASES])
def test_nhwc_kernel_vs_fp64(cuda, case):
    """forward and backward of one case through L.call; canaries around every buffer"""
    exact, sums = nhwc_reference(case)
    outs, intact = run_nhwc(case, cuda)
    _check(case[0], outs, exact, sums)
    assert intact(), "%s: a canary next to a buffer was overwritten" % case[0]


# ---- channel copies, pad_channels, reduce_rows, one-hot, permute ------------------------------------------------------------------------------
def test_copy_channels_vs_fp64(cuda):
    """offsets, broadcast and accumulate; the channels of dst outside [doff, doff + Cn) keep their bits"""
    from handwriting_line_generation_amd import _lib as L, ops
    for case in SC.COPY_CASES:
        name, rows, Cs, soff, Cd, doff, Cn, HW, bcast, acc = case
        src, dst = SC.copy_inputs(case)
        (sd, dd), intact = carve(cuda, src.numel(), dst.numel())
        put(sd, src); put(dd, dst)
        L.call("hwg_copy_channels", sd, Cs, soff, dd, Cd, doff, Cn, rows, HW, bcast, acc, ops._stream())
        got = dd.view(rows, Cd)
        if acc:
            sums = _cached(("copy", name), lambda: sums_of(lambda cast: copy_values(case, cast), {"dst": 2}))
            _check("copy_channels " + name, {"dst": got}, {}, sums)
        else:
            _check("copy_channels " + name, {"dst": got}, copy_values(case, _f), {})
        keep = torch.ones(Cd, dtype=torch.bool)
        keep[doff:doff + Cn] = False
        assert torch.equal(got.cpu()[:, keep], dst[:, keep]), "copy_channels %s: a channel outside the slice changed" % name
        assert intact(), "copy_channels %s: canary overwritten" % name


def test_pad_channels_exact(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    for rows, C, Cpad in SC.PAD_CHANNEL_CASES:
        src = torch.randn(rows, C, generator=SC.gen("padc_%d_%d" % (rows, C)))
        (sd, dd), intact = carve(cuda, src.numel(), rows * Cpad)
        put(sd, src)
        L.call("hwg_pad_channels", sd, C, dd, Cpad, rows, ops._stream())
        _check("pad_channels %dx%d->%d" % (rows, C, Cpad), {"dst": dd.view(rows, Cpad)}, {"dst": R.pad_channels(src, Cpad)}, {})
        assert intact(), "pad_channels: canary overwritten"


def test_reduce_rows_vs_fp64(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    for case in SC.REDUCE_CASES:
        name, N, HW, Cs, soff, Cn, acc = case
        _, src, prev = reduce_values(case, _d)
        (sd, od), intact = carve(cuda, src.numel(), prev.numel())
        put(sd, src); put(od, prev)
        L.call("hwg_reduce_rows", sd, Cs, soff, od, Cn, N, HW, acc, ops._stream())
        sums = _cached(("reduce", name), lambda: sums_of(lambda cast: reduce_values(case, cast)[0], {"out": HW + acc}))
        _check("reduce_rows " + name, {"out": od.view(N, Cn)}, {}, sums)
        assert intact(), "reduce_rows %s: canary overwritten" % name


def test_onehot_exact(cuda):
    """onehot with doff / Cd (the other channels keep their bits), onehot_both, labels outside [0, ncls) -> zero rows"""
    from handwriting_line_generation_amd import _lib as L, ops
    for case in SC.ONEHOT_CASES:
        name, Lr, B, ncls, Cd, doff = case
        lab, prev = SC.onehot_labels(case)
        (ld, od, bd, td), intact = carve(cuda, lab.numel(), prev.numel(), B * Lr * ncls, B * Lr * ncls)
        li = ld.view(torch.int32)
        li.copy_(lab.reshape(-1).to(cuda))
        put(od, prev)
        L.call("hwg_onehot", li, od, Lr, B, ncls, Cd, doff, ops._stream())
        L.call("hwg_onehot_both", li, bd, td, Lr, B, ncls, ops._stream())
        blc, lbc = R.onehot_both(lab, ncls)
        _check("onehot " + name, {"out": od.view(B, Lr, Cd), "blc": bd.view(B, Lr, ncls), "lbc": td.view(Lr, B, ncls)},
               {"out": R.onehot(lab, ncls, Cd, doff, prev.double()).float(), "blc": blc.float(), "lbc": lbc.float()}, {})
        assert intact(), "onehot %s: canary overwritten" % name
    lab, _ = SC.onehot_labels(SC.ONEHOT_CASES[0])
    Lr, B, ncls = SC.ONEHOT_CASES[0][1:4]
    blc, lbc = R.onehot_both(lab, ncls)
    got = ops.onehot_both(lab.to(cuda), ncls)
    assert same(got, lbc.float()) and same(ops.nhwc_of(got), blc.float().view(B, 1, Lr, ncls)) and same(ops.onehot_rows(lab.to(cuda), ncls), blc.float().view(B, 1, Lr, ncls))


def test_permute_exact(cuda):
    """permute4: all 24 permutations of four distinct extents and one tensor past the grid cap; ops.permute at ranks 2 to 4 with its inverse
    as the backward pass; the C == 1 alias branch of to_nchw / to_nhwc"""
    from handwriting_line_generation_amd import _lib as L, ops
    x = torch.randn(SC.PERMUTE_DIMS, generator=SC.gen("permute"))
    xd = x.to(cuda)
    for perm in R.all_perms4():
        dims = [x.shape[p] for p in perm]
        strides = [x.stride(p) for p in perm]
        (od,), intact = carve(cuda, x.numel())
        L.call("hwg_permute4", xd, od, *dims, *strides, ops._stream())
        assert same(od.view(dims), R.permute4(x, dims, strides)) and torch.equal(od.view(dims).cpu(), x.permute(perm)), "permute4 %s" % (perm,)
        assert intact()
        leaf = xd.clone().requires_grad_(True)
        y = ops.permute(leaf, perm)
        g = torch.randn(dims, generator=SC.gen("permute_g")).to(cuda)
        y.backward(g)
        inv = [perm.index(i) for i in range(4)]
        assert torch.equal(y.detach().cpu(), x.permute(perm).contiguous()) and torch.equal(leaf.grad.cpu(), g.cpu().permute(inv).contiguous()), perm
    shape, perm = SC.PERMUTE_BIG
    big = torch.randn(shape, generator=SC.gen("permute_big"))
    assert torch.equal(ops.permute(big.to(cuda), perm).cpu(), big.permute(perm).contiguous()), "permute past the grid cap"
    for shape, perm in SC.PERMUTE_LOW_RANK:
        t = torch.randn(shape, generator=SC.gen("permute_low"))
        leaf = t.to(cuda).requires_grad_(True)
        y = ops.permute(leaf, perm)
        g = torch.randn(tuple(y.shape), generator=SC.gen("permute_low_g"))
        y.backward(g.to(cuda))
        inv = [list(perm).index(i) for i in range(len(perm))]
        assert torch.equal(y.detach().cpu(), t.permute(perm).contiguous()) and torch.equal(leaf.grad.cpu(), g.permute(inv).contiguous()), (shape, perm)
    print("\npermute4: 24 permutations of %s, %s past the grid cap, %d low-rank permutations with their inverses: equal"
          % (SC.PERMUTE_DIMS, SC.PERMUTE_BIG[0], len(SC.PERMUTE_LOW_RANK)))
    t = torch.randn(2, 5, 7, 1, generator=SC.gen("alias"))
    leaf = t.to(cuda).requires_grad_(True)
    y = ops.to_nchw(leaf)
    assert tuple(y.shape) == (2, 1, 5, 7) and y.data_ptr() == leaf.data_ptr() and torch.equal(y.detach().cpu(), t.permute(0, 3, 1, 2))
    z = ops.to_nhwc(y)
    assert tuple(z.shape) == (2, 5, 7, 1) and z.data_ptr() == leaf.data_ptr()
    g = torch.randn(2, 5, 7, 1, generator=SC.gen("alias_g"))
    z.backward(g.to(cuda))
    assert torch.equal(leaf.grad.cpu(), g)


# ---- FusedUpsample weight --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("AB", SC.FUSED_WEIGHT_CASES, ids=["%dx%d" % ab for ab in SC.FUSED_WEIGHT_CASES])
def test_fused_upsample_weight_vs_fp64(cuda, AB):
    """forward to the derived bound; both adjoints to the bits of the fp32 restatement (the accumulating one on a pre-filled buffer)"""
    from handwriting_line_generation_amd import _lib as L, ops
    w3, dw4, prev = fused_inputs(AB)
    n = AB[0] * AB[1]
    (wd, w4d, gd, d3, d3a), intact = carve(cuda, n * 9, n * 16, n * 16, n * 9, n * 9)
    put(wd, w3); put(gd, dw4); put(d3a, prev)
    st = ops._stream()
    L.call("hwg_fused_upsample_weight_fwd", wd, w4d, n, SC.FUSED_MULT, st)
    L.call("hwg_fused_upsample_weight_bwd", gd, d3, n, SC.FUSED_MULT, st)
    L.call("hwg_fused_upsample_weight_bwd_acc", gd, d3a, n, SC.FUSED_MULT, st)
    mult = float(np.float32(SC.FUSED_MULT))
    sums = _cached(("fused", AB), lambda: sums_of(lambda cast: {"w4": R.fused_weight_fwd(cast(w3), mult)}, {"w4": 4 + 2}))
    _check("fused_weight %dx%d" % AB, {"w4": w4d.view(*AB, 4, 4), "dw3": d3.view(*AB, 3, 3), "dw3_acc": d3a.view(*AB, 3, 3)},
           {"dw3": R.fused_weight_bwd_f32(dw4, mult), "dw3_acc": R.fused_weight_bwd_f32(dw4, mult, prev)}, sums)
    assert intact(), "fused_weight: canary overwritten"


def test_fused_upsample_weight_autograd(cuda):
    """ops.fused_upsample_weight: a parameter accumulates into its gradient buffer (two backward passes give the fp32 sum, in order); a
    non-leaf weight gets its gradient from autograd"""
    from handwriting_line_generation_amd import ops
    AB = SC.FUSED_WEIGHT_CASES[0]
    w3, dw4, _ = fused_inputs(AB)
    mult = float(np.float32(SC.FUSED_MULT))
    p = torch.nn.Parameter(w3.to(cuda))
    for _ in range(2):
        ops.fused_upsample_weight(p, SC.FUSED_MULT).backward(dw4.to(cuda))
    once = R.fused_weight_bwd_f32(dw4, mult, torch.zeros_like(w3))
    twice = R.fused_weight_bwd_f32(dw4, mult, once)
    leaf = w3.to(cuda).requires_grad_(True)
    w4 = ops.fused_upsample_weight(leaf.clone(), SC.FUSED_MULT)
    w4.backward(dw4.to(cuda))
    sums = sums_of(lambda cast: {"w4": R.fused_weight_fwd(cast(w3), mult)}, {"w4": 4 + 2})
    _check("fused_weight autograd", {"w4": w4.detach(), "param.grad x2": p.grad, "non-leaf grad": leaf.grad},
           {"param.grad x2": twice, "non-leaf grad": R.fused_weight_bwd_f32(dw4, mult)}, sums)


# ---- col2im_taps -----------------------------------------------------------------------------------------------------------------------------
def _run_col2im(case, dev):
    from handwriting_line_generation_amd import _lib as L, ops
    name, N, H, W, R_, S, ph, pw, dh, dw = case
    t = SC.col2im_inputs(case)
    P, Q = SC.col2im_pq(case)
    (td, dxd), intact = carve(dev, t.numel(), N * H * W)
    put(td, t)
    L.call("hwg_col2im_taps", td, dxd, N, H, W, P, Q, R_, S, ph, pw, dh, dw, ops._stream())
    torch.cuda.synchronize()
    return dxd.view(N, H, W), intact


@pytest.mark.parametrize("case", SC.COL2IM_CASES, ids=[c[0] for c in SC.COL2IM_CASES])
def test_col2im_taps_vs_fp64(cuda, case):
    got, intact = _run_col2im(case, cuda)
    _check("col2im " + case[0], {"dx": got}, {}, col2im_reference(case))
    assert intact(), "col2im %s: canary overwritten" % case[0]


def test_col2im_general_kernel_same_bits(cuda):
    """HWG_COL2IM_LDS=0 sends the 5x5 case to the general kernel: the two promise the same tap order"""
    from handwriting_line_generation_amd import ops
    case = [c for c in SC.COL2IM_CASES if c[0] == SC.COL2IM_NOLDS][0]
    lds, _ = _run_col2im(case, cuda)
    with ops.tuning(HWG_COL2IM_LDS="0"):
        gen, intact = _run_col2im(case, cuda)
        _check("col2im %s, general kernel" % case[0], {"dx": gen}, {}, col2im_reference(case))
    assert intact() and torch.equal(gen, lds), "the general and the LDS col2im kernels differ in bits"


# ---- glue --------------------------------------------------------------------------------------------------------------------------------------
def test_axpby_mul_vs_fp64(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    a, b = 0.7312, -1.377
    af, bf = float(np.float32(a)), float(np.float32(b))
    for n in SC.GLUE_N:
        g = SC.gen("glue_%d" % n)
        x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
        (xd, yd, o1, o2, o3), intact = carve(cuda, n, n, n, n, n)
        put(xd, x); put(yd, y)
        st = ops._stream()
        L.call("hwg_axpby", xd, a, yd, b, o1, n, st)
        L.call("hwg_axpby", xd, a, None, 0.0, o2, n, st)
        L.call("hwg_mul", xd, yd, o3, n, st)
        X, Y = _d(x), _d(y)
        _check("axpby / mul n=%d" % n, {"axpby": o1, "ax": o2, "mul": o3}, {},
               {"axpby": entry(R.axpby(X, af, Y, bf), None, axpby_bound(af * X, bf * Y)), "ax": entry(R.axpby(X, af), None, axpby_bound(af * X)),
                "mul": entry(X * Y, None, 0.5 * ULP * (X * Y).abs())})
        assert intact(), "axpby / mul: canary overwritten"


def test_channel_affine_vs_fp64(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    for rows, C, has_scale, has_shift in SC.AFFINE_CASES:
        g = SC.gen("affine_%d_%d" % (rows, C))
        x, sc, sh = torch.randn(rows, C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
        (xd, sd, hd, od), intact = carve(cuda, rows * C, C, C, rows * C)
        put(xd, x); put(sd, sc); put(hd, sh)
        L.call("hwg_channel_affine", xd, sd if has_scale else None, hd if has_shift else None, od, rows, C, ops._stream())
        ax = _d(x) * _d(sc) if has_scale else _d(x)
        ref = R.channel_affine(_d(x), _d(sc) if has_scale else None, _d(sh) if has_shift else None)
        _check("channel_affine %dx%d scale %d shift %d" % (rows, C, has_scale, has_shift), {"y": od.view(rows, C)}, {},
               {"y": entry(ref, None, axpby_bound(ax, _d(sh).expand(rows, C) if has_shift else None))})
        assert intact(), "channel_affine: canary overwritten"


def test_weighted_sum_same_bits(cuda):
    """forward (the sum and the scaled terms) and backward through ops.weighted_sum, to the bits of the left-to-right fp32 restatement"""
    from handwriting_line_generation_amd import ops
    for name, ws in SC.WSUM_CASES.items():
        x = SC.wsum_terms(name)
        leaves = [x[i].to(cuda).requires_grad_(True) for i in range(len(ws))]
        total, scaled = ops.weighted_sum(leaves, ws)
        gout = torch.tensor(1.7, dtype=torch.float32)
        total.backward(gout.to(cuda))
        want_t, want_s = R.weighted_sum_f32(x.numpy(), ws)
        other, _ = R.weighted_sum_f32(x.numpy()[::-1], ws[::-1])
        _check("weighted_sum " + name, {"sum": total.detach(), "scaled": scaled, "grads": torch.stack([l.grad for l in leaves])},
               {"sum": want_t, "scaled": want_s, "grads": R.weighted_sum_bwd_f32(gout.numpy(), ws)}, {},
               note="  (right-to-left would give %r, not %r)" % (float(other), float(want_t)) if len(ws) > 2 else "")


def test_style_mix_same_bits(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    for case in SC.STYLE_MIX_CASES:
        name, K, B, D = case
        bank, ij, w = SC.style_mix_inputs(case)
        (bd, id_, wd, od), intact = carve(cuda, K * D, 2 * B, 2 * B, B * D)
        put(bd, bank); put(wd, w)
        ii = id_.view(torch.int32)
        ii.copy_(ij.reshape(-1).to(cuda))
        L.call("hwg_style_mix", bd, ii, wd, od, K, B, D, ops._stream())
        _check("style_mix " + name, {"out": od.view(B, D)}, {"out": R.style_mix_f32(bank, ij, w)}, {})
        assert intact(), "style_mix %s: canary overwritten" % name


# ---- the ops.py wrappers that had no unit test, through autograd ----------------------------------------------------------------------------------
def test_glue_wrappers_autograd(cuda):
    from handwriting_line_generation_amd import ops
    g = SC.gen("wrappers")
    dev = cuda
    # split_cols: exact copies both ways
    x = torch.randn(13, 12, generator=g)
    widths = [5, 3, 4]
    leaf = x.to(dev).requires_grad_(True)
    parts = ops.split_cols(leaf, widths)
    gs = [torch.randn(13, w, generator=g) for w in widths]
    torch.autograd.backward(parts, [t.to(dev) for t in gs])
    exact = {"split%d" % i: p for i, p in enumerate(x.split(widths, 1))}
    exact["split dx"] = torch.cat(gs, 1)
    outs = {"split%d" % i: p.detach() for i, p in enumerate(parts)}
    outs["split dx"] = leaf.grad
    _check("split_cols", outs, {k: v.contiguous() for k, v in exact.items()}, {})
    # repeat_rows: exact forward, the sum of k rows backward
    x, k = torch.randn(4, 6, generator=g), 5
    leaf = x.to(dev).requires_grad_(True)
    y = ops.repeat_rows(leaf, k)
    dy = torch.randn(4 * k, 6, generator=g)
    y.backward(dy.to(dev))
    _check("repeat_rows", {"y": y.detach(), "dx": leaf.grad}, {"y": x.repeat_interleave(k, 0)},
           sums_of(lambda cast: {"dx": R.reduce_rows(cast(dy), 0, 6, 4, k)}, {"dx": k}))
    # channel_affine: forward and the data gradient to 2 ulp, the scale / shift gradients (column sums over the rows) to the sum bound
    x, sc, sh = torch.randn(3, 7, 5, generator=g), torch.randn(5, generator=g), torch.randn(5, generator=g)
    lx, ls, lh = (t.to(dev).requires_grad_(True) for t in (x, sc, sh))
    y = ops.channel_affine(lx, ls, lh)
    dy = torch.randn(3, 7, 5, generator=g)
    y.backward(dy.to(dev))
    X, S_, H_, DY = _d(x), _d(sc), _d(sh), _d(dy)
    col = sums_of(lambda cast: {"dscale": (cast(dy) * cast(x)).reshape(21, 5).sum(0), "dshift": cast(dy).reshape(21, 5).sum(0)}, {"dscale": 22, "dshift": 21})
    _check("channel_affine autograd", {"y": y.detach(), "dx": lx.grad, "dscale": ls.grad, "dshift": lh.grad}, {},
           dict(col, y=entry(X * S_ + H_, None, axpby_bound(X * S_, H_.expand_as(X))), dx=entry(DY * S_, None, axpby_bound(DY * S_))))
    # mul_const, scale, add
    x, m, dy = (torch.randn(5, 9, generator=g) for _ in range(3))
    leaf = x.to(dev).requires_grad_(True)
    y = ops.mul_const(leaf, m.to(dev))
    y.backward(dy.to(dev))
    half = lambda v: 0.5 * ULP * v.abs()
    _check("mul_const", {"y": y.detach(), "dx": leaf.grad}, {}, {"y": entry(_d(x) * _d(m), None, half(_d(x) * _d(m))), "dx": entry(_d(dy) * _d(m), None, half(_d(dy) * _d(m)))})
    c = 0.3517
    cf = float(np.float32(c))
    leaf = x.to(dev).requires_grad_(True)
    y = ops.scale(leaf, c)
    y.backward(dy.to(dev))
    assert ops.scale(leaf, 1.0) is leaf
    _check("scale", {"y": y.detach(), "dx": leaf.grad}, {}, {"y": entry(cf * _d(x), None, axpby_bound(cf * _d(x))), "dx": entry(cf * _d(dy), None, axpby_bound(cf * _d(dy)))})
    a, b = 1.0, -0.625
    lx, ly = x.to(dev).requires_grad_(True), m.to(dev).requires_grad_(True)
    z = ops.add(lx, ly, a, b)
    z.backward(dy.to(dev))
    _check("add", {"z": z.detach(), "dx": lx.grad, "dy": ly.grad}, {"dx": dy},
           {"z": entry(_d(x) + b * _d(m), None, axpby_bound(_d(x), b * _d(m))), "dy": entry(b * _d(dy), None, axpby_bound(b * _d(dy)))})
    # zero_rows_from
    leaf = x.to(dev).requires_grad_(True)
    y = ops.zero_rows_from(leaf, 3)
    y.backward(dy.to(dev))
    wy, wg = x.clone(), dy.clone()
    wy[3:] = 0
    wg[3:] = 0
    _check("zero_rows_from", {"y": y.detach(), "dx": leaf.grad}, {"y": wy, "dx": wg}, {})


# ---- host-side refusals: an error before any launch ------------------------------------------------------------------------------------------
def test_host_side_refusals(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    (a, b, c), intact = carve(cuda, 256, 256, 256)
    st = ops._stream()
    ai = a.view(torch.int32)
    big, H31, W31 = 1 << 31, 1 << 16, 1 << 15       # H31 * W31 = 2^31 elements
    ptrs = np.full(17, a.data_ptr(), dtype=np.int64)
    w = np.ones(17, dtype=np.float32)
    refused = [
        ("LAUNCH_V at 2^31 elements", "hwg_avgpool_fwd", (a, b, 1, H31, W31, 1, 1, 1, st)),
        ("LAUNCH_V backward", "hwg_upsample_nearest_bwd", (a, b, 1, H31, W31, 1, 1, 1, st)),
        ("LAUNCH_V2", "hwg_maxpool_fwd", (a, b, ai, 1, H31, W31, 1, 1, 1, 1, 1, 0, 0, H31, W31, st)),
        ("blur", "hwg_blur3", (a, b, 1, H31, W31, 1, st)),
        ("copy_channels at 2^31", "hwg_copy_channels", (a, 1, 0, b, 1, 0, 1, big, 1, 0, 0, st)),
        ("pad_channels at 2^31", "hwg_pad_channels", (a, 1, b, 4, big, st)),
        ("onehot at 2^31", "hwg_onehot", (ai, b, H31, W31, 1, 1, 0, st)),
        ("onehot_both at 2^31", "hwg_onehot_both", (ai, b, c, H31, W31, 1, st)),
        ("permute4 at 2^31", "hwg_permute4", (a, b, H31, W31, 1, 1, 0, 0, 0, 0, st)),
        ("fused weight fwd at 2^31", "hwg_fused_upsample_weight_fwd", (a, b, 1 << 27, 1.0, st)),
        ("fused weight bwd at 2^31", "hwg_fused_upsample_weight_bwd", (a, b, 1 << 28, 1.0, st)),
        ("fused weight bwd_acc at 2^31", "hwg_fused_upsample_weight_bwd_acc", (a, b, 1 << 28, 1.0, st)),
        ("replicate with a negative pad", "hwg_pad2d_fwd", (a, b, 1, 4, 4, 1, -1, 0, 0, 0, 1, 0.0, st)),
        ("pad to an empty output", "hwg_pad2d_fwd", (a, b, 1, 2, 4, 1, -1, -1, 0, 0, 0, 0.0, st)),
        ("pad to an empty width", "hwg_pad2d_fwd", (a, b, 1, 2, 3, 1, 0, 0, -2, -1, 0, 0.0, st)),
        ("weighted_sum n = 0", "hwg_weighted_sum", (ptrs.ctypes.data, w.ctypes.data, 0, b, c, st)),
        ("weighted_sum n = 17", "hwg_weighted_sum", (ptrs.ctypes.data, w.ctypes.data, 17, b, c, st)),
        ("weighted_sum_bwd n = 0", "hwg_weighted_sum_bwd", (a, w.ctypes.data, 0, b, st)),
        ("weighted_sum_bwd n = 17", "hwg_weighted_sum_bwd", (a, w.ctypes.data, 17, b, st)),
        ("pad_channels Cpad % 4 != 0", "hwg_pad_channels", (a, 3, b, 6, 4, st)),
    ]
    for what, fn, args in refused:
        with pytest.raises(L.HwgError):
            L.call(fn, *args)
            pytest.fail("%s was not refused" % what)
    torch.cuda.synchronize()
    assert intact() and bool((a == CANARY).all()) and bool((b == CANARY).all()) and bool((c == CANARY).all()), "a refused call wrote something"
    print("\n%d host-side refusals, nothing launched" % len(refused))
