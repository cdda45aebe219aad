"""GPU: the style-path kernels (csrc/style_ops.hip: window gather / scatter, gather_scores, the confidence-weighted per-line mean, the
AdaIN LinearBank, the MLPChain) and the expert-bank kernels (csrc/expert_bank.hip: the grouped Conv1d forward, data gradient, weight
gradient and its reduce, gather_rows_ptr, segment_accumulate_ptr, and run_experts end to end) against the fp64 CPU restatements of
oracle/style_ref.py, at the step's shapes and at every dispatch regime of the kernels (case tables and the regimes they cover:
oracle/style_cases.py; the restatements, the tables and their sensitivity to seeded flaws are checked on the CPU by
tests/test_style_expert_ref_cpu.py; the references and their bounds: tests/_style_expert_checks.py). The library's default path only.

One line per case is printed: per output the relative L2 error and max|err| / max|ref| against fp64, the yardstick (the same restatement in
fp32 torch on the CPU against the same fp64 value) and the worst |err| / bound over the elements. No bound comes from the kernels:

  family                         bound
  copies, gathers, zeros         torch.equal
  grouped conv fwd / dgrad       per element (K + 2) 2^-24 sum|terms|, K = Cin S + 1 / Cout S
  grouped conv wgrad             the same, K = rows of the run + 1 (the pre-filled value)
  segment_accumulate_ptr         the same, K = windows of the run + 1
  scatter_windows                the same, K = 2 w + 1
  segment mean fwd / bwd         style_ref.segment_mean_bound (K = members of the line)
  gather_scores                  2 ulp of expf, relative: 2 * 2^-23 |ref|
  LinearBank fwd / dx / dW, db   (K + 2) 2^-24 sum|terms|, K = I + 1 / total outputs / B + 1
  MLPChain fwd                   style_ref.chain_fwd_bound: the L2 error of every row, propagated layer by layer
  MLPChain bwd, run_experts      the yardstick alone: a propagated bound is not practical (the sign of an activation decides a factor of
                                 the gradient, GroupNorm divides by a computed deviation); b5's gradient, a plain sum, has the derived one
(No errors measured on an MI355X stand beside the families yet: every case prints its own on the line it writes.)
Every output that is a sum is also held to YARDSTICK_FACTOR times its yardstick in relative L2 (a yardstick of exactly zero: the derived
bound alone)."""
import numpy as np
import pytest
import torch

from oracle import style_cases as SC
from oracle import style_ref as R
from _fp64 import YARDSTICK_FACTOR, _a, _d, _f, _ratio_rows, cpu_threads
from _style_expert_checks import (accumulate_reference, bank_reference, chain_reference, conv_reference, entry, seg_reference,
                                  window_reference)

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def _kind(name):
    return name.rstrip("0123456789").rstrip("._")


def _check(label, outs, refs, note=""):
    """outs: {name: kernel output}; refs: {name: entry}; asserts the derived bound per element and the yardstick; prints one line (of
    the outputs that differ only in a trailing index - experts, layers - the one with the largest error relative to what it is held to)"""
    shown, bad = {}, []
    for name, got in outs.items():
        want, yard, bound = refs[name]
        assert tuple(got.shape) == tuple(want.shape), (label, name, tuple(got.shape), tuple(want.shape))
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (label, name)
        assert bound is not None or (yard is not None and yard > 0), "%s %s: nothing to hold the output to" % (label, name)
        d = got.detach().cpu().double() - want
        rel = float(d.norm()) / max(float(want.norm()), 1e-300)
        mx = float(d.abs().max()) / max(float(want.abs().max()), 1e-300) if d.numel() else 0.0
        txt, score = "%s %.2e/%.2e" % (name, rel, mx), 0.0
        if yard is not None:
            txt += " yard %.2e" % yard
            if yard > 0:
                score = rel / (YARDSTICK_FACTOR * yard)
                if rel > YARDSTICK_FACTOR * yard:
                    bad.append("%s: rel L2 %.3e is %.1f x the fp32 yardstick %.3e" % (name, rel, rel / yard, yard))
        if bound is not None:
            r = _ratio_rows(got, want, bound)
            txt += " e/b %.2g" % r
            score = max(score, r)
            if not r <= 1.0:
                bad.append("%s: |err| is %.3g x the derived bound" % (name, r))
        if _kind(name) not in shown or score > shown[_kind(name)][0]:
            shown[_kind(name)] = (score, txt)
    print("\n%-30s rel L2 / max-max vs fp64: %s%s" % (label, "  ".join(t for _, t in shown.values()), note))
    assert not bad, "%s vs fp64: %s" % (label, "; ".join(bad))




# ---- grouped Conv1d --------------------------------------------------------------------------------------------------------------------
def _tab(ts, dev):
    from handwriting_line_generation_amd import ops
    return ops.h2d(np.array([t.data_ptr() for t in ts], dtype=np.int64), dev)


@pytest.mark.parametrize("case", SC.CONV_CASES, ids=[c[0] for c in SC.CONV_CASES])
def test_grouped_conv_vs_fp64(cuda, case):
    """forward, data gradient and weight gradient through L.call; the gradient buffers are pre-filled (the kernels add), those of absent
    experts must keep their bits"""
    from handwriting_line_generation_amd import _lib as L, ops
    from handwriting_line_generation_amd.model import expert_bank
    name, Cin, Cout, S, R_, plan_name, bias = case
    pad = S // 2
    x, dy, Ws, bs, gW, gb = SC.conv_inputs(case)
    cls = SC.plan_cls(plan_name, R_)
    n = cls.size
    Wd, Bd = [w.to(cuda) for w in Ws], [b.to(cuda) for b in bs]
    gWd, gBd = [t.to(cuda) for t in gW], [t.to(cuda) for t in gb]
    wptr, gwptr = _tab(Wd, cuda), _tab(gWd, cuda)
    bptr, gbptr = (_tab(Bd, cuda), _tab(gBd, cuda)) if bias else (None, None)
    plan = expert_bank.make_plan(cls, cuda)
    tseg, trow, nt, _ = expert_bank.plan_tiles(plan, R_, cuda)
    wrows = expert_bank.WGRAD_TILE_ROWS
    wseg, wrow, wnt, wrun = expert_bank.plan_tiles(plan, R_, cuda, wrows)
    xd, dyd = x.to(cuda), dy.to(cuda)
    y = torch.empty(n, R_, Cout, device=cuda)
    dx = torch.empty(n, R_, Cin, device=cuda)
    st = ops._stream()
    L.call("hwg_grouped_conv1d_fwd", xd, plan["seg_start"], plan["seg_eid"], tseg, trow, nt, wptr, bptr, y, R_, Cin, Cout, S, pad, st)
    L.call("hwg_grouped_conv1d_dgrad", dyd, plan["seg_start"], plan["seg_eid"], tseg, trow, nt, wptr, dx, R_, Cin, Cout, S, pad, st)
    ws = ops.workspace(L.query("hwg_grouped_conv1d_wgrad_workspace", wnt, Cin, Cout, S), cuda)
    L.call("hwg_grouped_conv1d_wgrad", dyd, xd, plan["seg_start"], plan["seg_eid"], plan["G"], wseg, wrow, wrun, wnt, wrows, gwptr, gbptr, R_, Cin, Cout, S,
           pad, ws, ws.numel(), st)
    torch.cuda.synchronize()
    refs = conv_reference(case)
    present = SC.PLANS[plan_name][R_]
    outs = {"y": y, "dx": dx}
    for e in range(SC.E):
        if e in present:
            outs["dW%d" % e] = gWd[e]
            if bias:
                outs["db%d" % e] = gBd[e]
        else:
            assert torch.equal(gWd[e].cpu(), gW[e]), "%s: the weight gradient of absent expert %d was touched" % (name, e)
        if e not in present or not bias:
            assert torch.equal(gBd[e].cpu(), gb[e]), "%s: the bias gradient of expert %d was touched" % (name, e)
    assert set(outs) == set(refs)
    _check("conv " + name, outs, refs)


@pytest.fixture(scope="module")
def expert_modules(cuda):
    """six real CharExtractor modules of the step's size with seeded parameters (GroupNorm affines too), their CPU copies, the bank"""
    from handwriting_line_generation_amd.model import expert_bank
    from handwriting_line_generation_amd.model.char_style import CharExtractor
    Cin, dim, _ = SC.EXPERT_LAYERS[0]
    mods = [CharExtractor(Cin, dim, SC.EXPERT_LAYERS[4][1], 1, True).to(cuda) for _ in range(SC.E)]
    bank = expert_bank.ExpertBank(mods)
    g = SC.gen("expert_modules")
    host = []
    for e in range(SC.E):
        p = {}
        for k in R.EXPERT_KINDS:
            t = bank.params[k][e]
            fan = t[0].numel() if t.dim() > 1 else 1
            v = torch.randn(t.shape, generator=g) * (1.0 / fan ** 0.5 if t.dim() > 1 else 0.2) + (1.0 if k in ("g1", "g2") else 0.0)
            t.data.copy_(v.to(cuda))
            p[k] = v
        host.append(p)
    return mods, bank, host


def _clear_grads(mods):
    for m in mods:
        for p in m.parameters():
            p.grad = None


@pytest.mark.parametrize("layer", SC.AUTOGRAD_LAYERS, ids=[l[0] for l in SC.AUTOGRAD_LAYERS])
def test_grouped_conv_autograd_step_layers_vs_fp64(cuda, expert_modules, layer):
    """the step's layers through model/expert_bank._GroupedConv1d: autograd's data gradient, the parameter gradients in the experts' own
    .grad buffers, absent experts keep grad None"""
    from handwriting_line_generation_amd.model import expert_bank
    mods, bank, host = expert_modules
    wk, R_ = layer
    bk = "b" + wk[1:]
    Cout, Cin = host[0][wk].shape[:2]
    S = host[0][wk].shape[2] if host[0][wk].dim() == 3 else 1
    cls = SC.plan_cls("mixed", R_)
    g = SC.gen("conv_autograd_" + wk)
    x = torch.randn(cls.size, R_, Cin, generator=g)
    dy = torch.randn(cls.size, R_, Cout, generator=g)
    _clear_grads(mods)
    plan = expert_bank.make_plan(cls, cuda, window_rows=(R_,))
    xd = x.view(cls.size, 1, R_, Cin).to(cuda).requires_grad_(True)
    y = expert_bank._GroupedConv1d.apply(xd, bank, wk, bk, plan, S, S // 2)
    y.backward(dy.view(cls.size, 1, R_, Cout).to(cuda))
    torch.cuda.synchronize()
    cpu_threads()
    present = SC.PLANS["mixed"][R_]
    vals = []
    for cast in (_d, _f, _a):
        W = [cast(h[wk]).reshape(Cout, Cin, S) for h in host]
        X, DY = cast(x), cast(dy)
        v = {"y": R.grouped_conv_fwd(X, cls, W, [cast(h[bk]) for h in host], S), "dx": R.grouped_conv_dgrad(DY, cls, W, S)}
        for e, (dW, db) in R.grouped_conv_wgrad(DY, X, cls, S).items():
            v["dW%d" % e], v["db%d" % e] = dW.reshape(host[e][wk].shape), db
        vals.append(v)
    K = lambda k: Cin * S + 1 if k == "y" else Cout * S if k == "dx" else present[int(k[2:])] * R_
    refs = {k: entry(v, vals[1][k], R.sum_bound(K(k), vals[2][k])) for k, v in vals[0].items()}
    outs = {"y": y.detach().view(cls.size, R_, Cout), "dx": xd.grad.view(cls.size, R_, Cin)}
    for e in range(SC.E):
        pw, pb = bank.params[wk][e], bank.params[bk][e]
        if e in present:
            outs["dW%d" % e], outs["db%d" % e] = pw.grad, pb.grad
        else:
            assert pw.grad is None and pb.grad is None, "absent expert %d got a gradient" % e
    _check("conv autograd %s R %d" % (wk, R_), outs, refs)


def test_gather_rows_and_segment_accumulate_vs_fp64(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    from handwriting_line_generation_amd.model import expert_bank
    for C in SC.ACCUMULATE_C:
        cls, rows, pre, refs = accumulate_reference(C)
        plan = expert_bank.make_plan(cls, cuda)
        src = [pre[e].to(cuda) for e in range(SC.E)]
        out = torch.empty(cls.size, C, device=cuda)
        L.call("hwg_gather_rows_ptr", _tab(src, cuda), plan["eid"], out, int(cls.size), C, ops._stream())
        assert torch.equal(out.cpu(), pre[torch.from_numpy(cls)]), "gather_rows_ptr C=%d" % C
        dst = [pre[e].to(cuda) for e in range(SC.E)]
        L.call("hwg_segment_accumulate_ptr", rows.to(cuda), plan["seg_start"], plan["seg_eid"], plan["G"], _tab(dst, cuda), C, ops._stream())
        torch.cuda.synchronize()
        for e in range(SC.E):
            if e not in SC.ACCUMULATE_RUNS:
                assert torch.equal(dst[e].cpu(), pre[e]), "segment_accumulate_ptr touched absent expert %d" % e
        _check("segment_accumulate C=%d" % C, {"g%d" % e: dst[e] for e in SC.ACCUMULATE_RUNS}, refs, "  (gather_rows_ptr: exact)")


def test_run_experts_vs_fp64_per_class_loop(cuda, expert_modules):
    """run_experts end to end against the reference's per-class loop (torch's own ops in fp64, the windows of one class at a time):
    forward, d patches, every expert parameter gradient; the absent expert keeps grad None. Yardstick alone (see the table above)."""
    from handwriting_line_generation_amd.model import expert_bank
    mods, bank, host = expert_modules
    R_, C = SC.EXPERT_R, SC.EXPERT_LAYERS[0][0]
    cls = np.concatenate([np.full(n, e, dtype=np.int64) for e, n in sorted(SC.EXPERTS_RUNS.items())])
    n = int(cls.size)
    g = SC.gen("run_experts")
    x = torch.randn(n, R_, C, generator=g)
    dout = torch.randn(n, SC.EXPERT_LAYERS[4][1], generator=g)
    _clear_grads(mods)
    plan = expert_bank.make_plan(cls, cuda, window_rows=(R_, 1))
    xd = x.view(n, 1, R_, C).to(cuda).requires_grad_(True)
    g1, g2 = mods[0].conv1[2].num_groups, mods[0].conv2[2].num_groups
    assert (g1, g2) == SC.STEP["groups"]
    out = expert_bank.run_experts(bank, xd, plan, g1, g2)
    out.backward(dout.to(cuda))
    torch.cuda.synchronize()
    cpu_threads()
    vals = []
    for dt in (torch.float64, torch.float32):
        xs = x.to(dt).requires_grad_(True)
        ps = [{k: v.to(dt).requires_grad_(True) for k, v in h.items()} for h in host]
        ys = torch.cat([R.char_extractor(ps[e], xs[i0:i1], g1, g2) for e, i0, i1 in R.runs_of(cls)])
        ys.backward(dout.to(dt))
        v = {"out": ys.detach(), "dpatches": xs.grad}
        for e in SC.EXPERTS_RUNS:
            for k in R.EXPERT_KINDS:
                v["%s.%d" % (k, e)] = ps[e][k].grad
        vals.append(v)
    # b5's gradient is the plain sum of the run's d out rows: it has a derived bound (and a yardstick that may be exactly zero)
    ab5 = R.segment_accumulate(dout.double().abs(), cls)
    refs = {k: entry(v, vals[1][k], R.sum_bound(SC.EXPERTS_RUNS[int(k[3:])], ab5[int(k[3:])]) if k.startswith("b5.") else None) for k, v in vals[0].items()}
    outs = {"out": out.detach(), "dpatches": xd.grad.view(n, R_, C)}
    for e in range(SC.E):
        for k in R.EXPERT_KINDS:
            p = bank.params[k][e]
            if e in SC.EXPERTS_RUNS:
                assert p.grad is not None, "%s of expert %d got no gradient" % (k, e)
                outs["%s.%d" % (k, e)] = p.grad
            else:
                assert p.grad is None, "%s of the absent expert %d got a gradient" % (k, e)
    _check("run_experts", outs, refs)


# ---- windows, scores -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.WINDOW_CASES, ids=[c[0] for c in SC.WINDOW_CASES])
def test_windows_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, B, Wx, C, w = case
    x, ib, ip, dp, n_in = SC.window_inputs(case)
    want, refs = window_reference(case)
    xg = x.to(cuda).requires_grad_(True)
    got = ops.gather_windows(xg, ib.to(cuda), ip.to(cuda), w)
    assert tuple(got.shape) == (ib.numel(), 1, 2 * w + 1, C)
    assert torch.equal(got.detach().cpu().view(want.shape), want), "gather_windows %s" % name
    inside = (ib >= 0) & (ib < B) & (ip >= 0) & (ip < Wx)
    assert int(inside.sum()) == n_in and not bool(got.detach().cpu()[~inside].any()), "gather_windows %s: a centre outside the tensor gave a non-zero row" % name
    got.backward(dp.view(got.shape).to(cuda))
    _check("windows " + name, {"dx": xg.grad}, refs, "  (gather: exact, %d centres outside give zero rows)" % int((~inside).sum()))


def test_gather_scores_vs_fp64(cuda):
    from handwriting_line_generation_amd import ops
    x, ib, ip, ic = SC.scores_inputs()
    got = ops.gather_scores(x.to(cuda), ib.to(cuda), ip.to(cuda), ic.to(cuda))
    want = R.gather_scores(x.double(), ib, ip, ic)
    assert float(x.min()) >= -20.0 and float(x.max()) <= 0.0
    _check("gather_scores", {"exp": got}, {"exp": entry(want, None, 2 * ULP * want)})


# ---- segment mean ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.SEG_CASES, ids=[c[0] for c in SC.SEG_CASES])
def test_segment_mean_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, n, B, C, kind = case
    v, wgt, seg, dout = SC.seg_inputs(case)
    vg = v.to(cuda).requires_grad_(True)
    out = ops.segment_weighted_mean(vg, wgt.to(cuda), seg.to(cuda), B)
    out.backward(dout.to(cuda))
    refs = seg_reference(case)
    _check("segment mean " + name, {"out": out.detach(), "dv": vg.grad}, refs)
    if kind == "pad_zero":
        # the member of weight 0 adds exactly 0 to both sums: the walk-all kernel's output must be held to the list kernel case's fp64 value
        base = [c for c in SC.SEG_CASES if c[0] == "n7679"][0]
        assert torch.equal(refs["out"][0], seg_reference(base)["out"][0])
        assert not bool(vg.grad[-1].any())


# ---- LinearBank ------------------------------------------------------------------------------------------------------------------------
def _linears(shapes, Ws, bs, cuda):
    mods = [torch.nn.Linear(i, o).to(cuda) for o, i in shapes]
    for m, W, b in zip(mods, Ws, bs):
        m.weight.data.copy_(W.to(cuda))
        m.bias.data.copy_(b.to(cuda))
    return mods


@pytest.mark.parametrize("case", SC.BANK_CASES, ids=[c[0] for c in SC.BANK_CASES])
def test_linear_bank_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, B, I, O, halves, unused, frozen, xgrad, backward = case
    x, Ws, bs, dys, gW, gb = SC.bank_inputs(case)
    mods = _linears([(o, I) for o in O], Ws, bs, cuda)
    for l, m in enumerate(mods):
        m.weight.requires_grad_(l not in frozen)
        m.bias.requires_grad_(frozen.get(l) != "all")
        if backward:
            m.weight.grad = gW[l].to(cuda) if m.weight.requires_grad else None
            m.bias.grad = gb[l].to(cuda) if m.bias.requires_grad else None
    bank = ops.LinearBank(mods, halves=halves)
    xd = x.to(cuda).requires_grad_(xgrad)
    refs = bank_reference(case)
    if not backward:
        with torch.no_grad():
            parts = bank(xd)
        _check("bank " + name, {"y%d_%d" % (l, h): t for l, pr in enumerate(parts) for h, t in enumerate(pr)}, refs)
        return
    parts = bank(xd)
    outs = {"y%d_%d" % (l, h): t.detach() for l, pr in enumerate(parts) for h, t in enumerate(pr)}
    sum((parts[l][h] * dys[l][h].to(cuda)).sum() for l in range(len(O)) for h in range(halves) if dys[l][h] is not None).backward()
    torch.cuda.synchronize()
    if xgrad:
        outs["dx"] = xd.grad
    else:
        assert xd.grad is None
    for l, m in enumerate(mods):
        if l in frozen:
            assert m.weight.grad is None, "frozen weight %d got a gradient" % l
        else:
            outs["dW%d" % l] = m.weight.grad
        if frozen.get(l) == "all":
            assert m.bias.grad is None, "frozen bias %d got a gradient" % l
        else:
            outs["db%d" % l] = m.bias.grad
    assert set(outs) == set(refs)
    _check("bank " + name, outs, refs)


def test_linear_bank_backward_of_17_rows_is_refused(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    case = [c for c in SC.BANK_CASES if c[0] == "b17_fwd"][0]
    x, Ws, bs, dys, gW, gb = SC.bank_inputs(case)
    mods = _linears([(o, case[2]) for o in case[3]], Ws, bs, cuda)
    parts = ops.LinearBank(mods, halves=2)(x.to(cuda).requires_grad_(True))
    with pytest.raises(L.HwgError):
        sum(t.sum() for pr in parts for t in pr).backward()
    torch.cuda.synchronize()
    assert all(m.weight.grad is None or not bool(m.weight.grad.any()) for m in mods), "a refused backward pass wrote gradients"


# ---- MLPChain --------------------------------------------------------------------------------------------------------------------------
def _run_chain(cuda, case, split):
    """forward, then two backward passes in a row into pre-filled gradients -> outputs by name"""
    from handwriting_line_generation_amd import ops
    name, D, B, L_, frozen, backward = case
    x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
    mods = _linears([(D, D)] * L_, Ws, bs, cuda)
    for l, m in enumerate(mods):
        m.weight.requires_grad_(l != frozen)
        m.bias.requires_grad_(l != frozen)
        if l != frozen:
            m.weight.grad, m.bias.grad = gW[l].to(cuda), gb[l].to(cuda)
    chain = ops.MLPChain(mods, SC.CHAIN_SLOPE)
    xd = x.to(cuda).requires_grad_(True)
    prev = ops.MLP_CHAIN_SPLIT
    ops.MLP_CHAIN_SPLIT = split
    try:
        for _ in range(2):
            h = chain(xd)
            h.backward(dout.to(cuda))
    finally:
        ops.MLP_CHAIN_SPLIT = prev
    torch.cuda.synchronize()
    outs = {"h": h.detach(), "dx": xd.grad}
    for l, m in enumerate(mods):
        if l == frozen:
            assert m.weight.grad is None and m.bias.grad is None, "frozen layer %d got a gradient" % l
        else:
            outs["dW%d" % l], outs["db%d" % l] = m.weight.grad, m.bias.grad
    return outs


@pytest.mark.parametrize("case", SC.CHAIN_CASES, ids=[c[0] for c in SC.CHAIN_CASES])
def test_mlp_chain_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, D, B, L_, frozen, backward = case
    refs = chain_reference(case)
    if not backward:
        x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
        mods = _linears([(D, D)] * L_, Ws, bs, cuda)
        with torch.no_grad():
            h = ops.MLPChain(mods, SC.CHAIN_SLOPE)(x.to(cuda))
        _check("chain " + name, {"h": h}, refs)
        return
    assert ops.MLP_CHAIN_SPLIT, "the two-launch backward pass is the default"
    got = {split: _run_chain(cuda, case, split) for split in (True, False)}
    for split in (True, False):
        assert set(got[split]) == set(refs)
        # the neurons with a pre-activation of exactly 0: h is 0 there, and the derivative the slope
        assert not bool(got[split]["h"][:, list(SC.CHAIN_ZERO_NEURONS)].any())
        _check("chain %s %s" % (name, "split" if split else "single"), got[split], refs)
    diffs = {k: float((got[True][k] - got[False][k]).abs().max()) for k in refs if not torch.equal(got[True][k], got[False][k])}
    assert not diffs, "chain %s: the two-launch backward differs from the single-workgroup kernel: %s" % (name, diffs)


def test_mlp_chain_backward_of_17_rows_is_refused(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    case = [c for c in SC.CHAIN_CASES if c[0] == "d128_b17_fwd"][0]
    name, D, B, L_, frozen, backward = case
    x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
    mods = _linears([(D, D)] * L_, Ws, bs, cuda)
    for split in (True, False):
        prev = ops.MLP_CHAIN_SPLIT
        ops.MLP_CHAIN_SPLIT = split
        try:
            h = ops.MLPChain(mods, SC.CHAIN_SLOPE)(x.to(cuda).requires_grad_(True))
            with pytest.raises(L.HwgError):
                h.backward(dout.to(cuda))
        finally:
            ops.MLP_CHAIN_SPLIT = prev
    torch.cuda.synchronize()
