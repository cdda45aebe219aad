"""CPU: the fp64 restatements of the style-path and expert-bank kernels (oracle/style_ref.py) against torch's own ops and autograd in fp64,
the bookkeeping of the GPU case tables (oracle/style_cases.py: the tables together reach every dispatch regime the kernels have), and the
sensitivity of those tables: thirteen plausible kernel flaws, seeded by flag into copies of the restatements that live in this file only,
each move some case past the bound tests/test_style_expert_fp64_gpu.py holds that case to by SENSITIVITY_FACTOR or more."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import style_cases as SC
from oracle import style_ref as R
import _style_expert_checks as G  # the references and bounds the GPU file holds the device to
from _fp64 import YARDSTICK_FACTOR, _d, _ratio_rows, _rel

SENSITIVITY_FACTOR = 10.0


def _leaf(t):
    return t.double().clone().requires_grad_(True)


def _close(a, b, tol=1e-10):
    torch.testing.assert_close(a, b, rtol=tol, atol=tol)


# ---- copies of the restatements with flaws behind flags (flaw=None: the same arithmetic as oracle/style_ref.py, checked below) -------------
def scatter_windows(dp, idx_b, idx_pos, w, B, Wx, flaw=None):
    """the gradient of gather_windows: dp [n, 2w+1, C] -> dx [B, Wx, C]; windows overlap (at most 2w+1 terms per element), centres outside
    the tensor are ignored"""
    n, WW, C = dp.shape
    b, p = idx_b.long(), idx_pos.long()
    pos = p[:, None] + torch.arange(-w, w + 1)[None, :]
    clipped = ((pos < 0) | (pos >= Wx)).any(1)
    if flaw == "scatter_clipped_shifted":
        pos = pos + clipped[:, None].long()
    ok = (pos >= 0) & (pos < Wx) & ((p >= 0) & (p < Wx) & (b >= 0) & (b < B))[:, None]
    flat = (b[:, None] * Wx + pos)[ok]
    return dp.new_zeros(B * Wx, C).index_add_(0, flat, dp[ok]).reshape(B, Wx, C)


def segment_mean(v, wgt, seg, B, flaw=None):
    """-> out [B, C], wsum [B]: total = sum of wgt_i v_i over the members of a line, out = total / wsum, or total where wsum == 0"""
    n, C = v.shape
    seg = seg.long()
    keep_t = torch.ones(n, dtype=torch.bool)
    keep_w = torch.ones(n, dtype=torch.bool)
    if flaw in ("seg_drop_past_8", "seg_wsum_misses_last"):
        for b in range(B):
            members = (seg == b).nonzero().flatten()
            if flaw == "seg_drop_past_8":
                keep_t[members[members.numel() // 8 * 8:]] = False
            elif members.numel():
                keep_w[members[-1]] = False
    tot = v.new_zeros(B, C).index_add_(0, seg[keep_t], wgt[keep_t, None] * v[keep_t])
    ws = v.new_zeros(B).index_add_(0, seg[keep_w], wgt[keep_w])
    nz = ws != 0
    return torch.where(nz[:, None], tot / torch.where(nz, ws, torch.ones_like(ws))[:, None], tot), ws


def linear_bank_fwd(x, Ws, bs, halves, flaw=None):
    """-> per layer a list of `halves` tensors [B, O_l / halves]"""
    out = []
    for W, b in zip(Ws, bs):
        C = W.shape[0] // halves
        xx = x
        if flaw == "bank_rows_wrap_16":                                                 # FLAW: rows >= 16 read row b - 16
            rows = torch.arange(x.shape[0])
            xx = x[torch.where(rows >= 16, rows - 16, rows)]
        y = xx @ W.t()
        parts = []
        for h in range(halves):
            add = 0 if (flaw == "bank_second_half_bias" and h == 1) else b[h * C:(h + 1) * C]
            parts.append(y[:, h * C:(h + 1) * C] + add)
        out.append(parts)
    return out


def linear_bank_bwd(x, Ws, dys, halves, flaw=None, chunk=SC.LB_OCHUNK):
    """dys: per layer a list of `halves` gradients [B, O_l / halves] or None -> dx [B, I], [dW_l], [db_l]"""
    dy = R._bank_dy(x, Ws, dys, halves)
    first = [0]
    for W in Ws:
        first.append(first[-1] + W.shape[0])
    dWs = [dy[:, first[l]:first[l + 1]].t() @ x for l in range(len(Ws))]
    dbs = [dy[:, first[l]:first[l + 1]].sum(0) for l in range(len(Ws))]
    Wall = torch.cat(list(Ws), 0)
    if flaw == "bank_chunk_first_layer":
        # every chunk of 32 neurons reads the weight rows of the layer its first neuron belongs to (row index = neuron - that layer's start)
        rows = []
        for c0 in range(0, first[-1], chunk):
            l0 = max(l for l in range(len(Ws)) if first[l] <= c0)
            for wv in range(c0, min(c0 + chunk, first[-1])):
                rows.append(Ws[l0][min(wv - first[l0], Ws[l0].shape[0] - 1)])
        Wall = torch.stack(rows)
    return dy @ Wall, dWs, dbs


def mlp_chain_fwd(x, Ws, bs, slope, flaw=None):
    """-> [h_0 = x, h_1, .. h_L]"""
    acts = [x]
    for W, b in zip(Ws, bs):
        a = acts[-1] @ W.t() + b
        h = torch.where(a > 0, a, a * slope)
        if flaw == "chain_rows_from_8" and x.shape[0] > 8:
            h = torch.cat([h[:8], torch.zeros_like(h[8:])])
        acts.append(h)
    return acts


def mlp_chain_bwd(dout, acts, Ws, slope, flaw=None):
    """-> dx, [dW_l], [db_l]; the derivative where h == 0 (a pre-activation of exactly 0) is `slope`"""
    L = len(Ws)
    d = dout
    dWs, dbs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        h = acts[l + 1]
        pos = (h >= 0) if flaw == "chain_derivative_at_zero" else (h > 0)
        d = d * torch.where(pos, torch.ones((), dtype=d.dtype), torch.full((), slope, dtype=d.dtype))
        if flaw == "chain_rows_from_8" and d.shape[0] > 8:
            d = torch.cat([d[:8], torch.zeros_like(d[8:])])
        dWs[l] = d.t() @ acts[l]
        dbs[l] = d.sum(0)
        d = d @ Ws[l]
    return d, dWs, dbs


def _padded(t, pad, flaw_rows=None):
    """[n, R, C] -> [n, R + 2 pad, C], zero rows at both ends of every window (flaw_rows: the neighbouring windows' rows instead)"""
    if pad == 0:
        return t
    n, Rw, C = t.shape
    z = t.new_zeros(n, pad, C)
    if flaw_rows is None:
        return torch.cat([z, t, z], 1)
    before = torch.cat([z[:1], t[:-1, Rw - pad:]], 0)
    after = torch.cat([t[1:, :pad], z[:1]], 0)
    return torch.cat([before, t, after], 1)


def grouped_conv_fwd(x, cls, Ws, bs, S, flaw=None, stage=SC.GT_CK):
    """x [n, R, Cin], Ws[e] [Cout, Cin, S], bs[e] [Cout] or bs None -> y [n, R, Cout]; padding S // 2 inside every window"""
    n, Rw, Cin = x.shape
    pad = S // 2
    xp = _padded(x, pad, True if flaw == "conv_tap_crosses_window" else None)
    ys = []
    for e, i0, i1 in R.runs_of(cls):
        W = Ws[e]
        if flaw == "conv_drop_last_group" and Cin % stage:
            W = torch.cat([W[:, :Cin - 8], torch.zeros_like(W[:, Cin - 8:])], 1)        # the last 8 channels of the last staged step
        if flaw == "conv_upper_k_half" and Cin * S >= SC.SPLIT_K:
            keep = torch.zeros(Cin, dtype=torch.bool)
            for c0 in range(0, Cin, stage):                                             # the lower half of every staged step's 8-channel groups
                groups = min(stage, Cin - c0) // 8
                keep[c0:c0 + (groups + 1) // 2 * 8] = True
            W = W * keep[None, :, None].to(W.dtype)
        y = sum(xp[i0:i1, s:s + Rw] @ W[:, :, s].t() for s in range(S))
        ys.append(y + bs[e] if bs is not None else y)
    return torch.cat(ys, 0)


def grouped_conv_wgrad(dy, x, cls, S, flaw=None, tile_rows=SC.WGRAD_TILE_ROWS):
    """-> {expert: (dW [Cout, Cin, S], db [Cout])} for the experts that have windows"""
    n, Rw, Cin = x.shape
    pad = S // 2
    xp = _padded(x, pad)
    out = {}
    for e, i0, i1 in R.runs_of(cls):
        d = dy[i0:i1]
        rows = (i1 - i0) * Rw
        if flaw == "wgrad_tile_last_row":
            keep = torch.ones(rows, dtype=torch.bool)
            keep[tile_rows - 1::tile_rows] = False
            keep[rows - 1] = False
            d = d * keep.reshape(i1 - i0, Rw, 1).to(d.dtype)
        dW = torch.stack([torch.einsum("nro,nri->oi", d, xp[i0:i1, s:s + Rw]) for s in range(S)], 2)
        db = d.sum((0, 1))
        if flaw == "wgrad_single_tile_twice" and rows <= tile_rows:
            dW, db = 2 * dW, 2 * db
        out[e] = (dW, db)
    return out


# ---- the restatements against torch in fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.WINDOW_CASES, ids=[c[0] for c in SC.WINDOW_CASES])
def test_window_reference_is_zero_padded_slicing(case):
    name, B, Wx, C, w = case
    x, ib, ip, dp, n_in = SC.window_inputs(case)
    xr = _leaf(x)
    got = R.gather_windows(xr, ib, ip, w)
    padded = F.pad(xr, (0, 0, w, w))
    inside = 0
    for k in range(ib.numel()):
        b, p = int(ib[k]), int(ip[k])
        if 0 <= b < B and 0 <= p < Wx:
            assert torch.equal(got[k], padded[b, p:p + 2 * w + 1])
            inside += 1
        else:
            assert not bool(got[k].any())
    assert inside == n_in
    keys = [(int(b), int(p)) for b, p in zip(ib, ip)]
    assert len(set(keys)) == len(keys), "window centres must be unique"
    got.backward(dp.double())
    _close(R.scatter_windows(dp.double(), ib, ip, w, B, Wx), xr.grad, 1e-12)
    # the summation has at most 2 w + 1 terms
    cover = R.scatter_windows(torch.ones(dp.shape, dtype=torch.float64), ib, ip, w, B, Wx)
    assert float(cover.max()) <= 2 * w + 1
    if w > 0 and Wx > 4:
        assert float(cover.max()) >= 2, "no overlapping windows"


def test_scores_reference_and_inputs():
    x, ib, ip, ic = SC.scores_inputs()
    B, Wx, C = x.shape
    assert 0 <= int(ib.min()) and int(ib.max()) < B and 0 <= int(ip.min()) and int(ip.max()) < Wx and 0 <= int(ic.min()) and int(ic.max()) < C
    want = torch.stack([x[int(b), int(p), int(c)].double().exp() for b, p, c in zip(ib, ip, ic)])
    _close(R.gather_scores(x.double(), ib, ip, ic), want, 1e-15)


@pytest.mark.parametrize("case", SC.SEG_CASES[:6], ids=[c[0] for c in SC.SEG_CASES[:6]])
def test_segment_mean_reference_is_the_accumulation_loop(case):
    name, n, B, C, kind = case
    v, wgt, seg, dout = SC.seg_inputs(case)
    vr = _leaf(v)
    tot, ws = [torch.zeros(C, dtype=torch.float64) for _ in range(B)], [torch.zeros((), dtype=torch.float64) for _ in range(B)]
    for i in range(n):
        tot[int(seg[i])] = tot[int(seg[i])] + wgt[i].double() * vr[i]
        ws[int(seg[i])] = ws[int(seg[i])] + wgt[i].double()
    want = torch.stack([tot[b] / ws[b] if float(ws[b]) != 0 else tot[b] for b in range(B)])
    out, wsum = R.segment_mean(v.double(), wgt.double(), seg, B)
    _close(out, want.detach(), 1e-12)
    _close(wsum, torch.stack(ws), 1e-12)
    want.backward(dout.double())
    _close(R.segment_mean_bwd(dout.double(), wgt.double(), seg, wsum), vr.grad, 1e-12)


@pytest.mark.parametrize("case", [c for c in SC.BANK_CASES if c[8]], ids=[c[0] for c in SC.BANK_CASES if c[8]])
def test_linear_bank_reference_is_torch(case):
    name, B, I, O, halves, unused, frozen, xgrad, backward = case
    x, Ws, bs, dys, gW, gb = SC.bank_inputs(case)
    xr, Wr, br = _leaf(x), [_leaf(w) for w in Ws], [_leaf(b) for b in bs]
    got = R.linear_bank_fwd(x.double(), [w.double() for w in Ws], [b.double() for b in bs], halves)
    loss = 0.0
    for l in range(len(O)):
        y = F.linear(xr, Wr[l], br[l])
        C = O[l] // halves
        for h in range(halves):
            _close(got[l][h], y[:, h * C:(h + 1) * C].detach(), 1e-12)
            if dys[l][h] is not None:
                loss = loss + (y[:, h * C:(h + 1) * C] * dys[l][h].double()).sum()
    loss.backward()
    dx, dWs, dbs = R.linear_bank_bwd(x.double(), [w.double() for w in Ws], [[p.double() if p is not None else None for p in parts] for parts in dys], halves)
    _close(dx, xr.grad)
    for l in range(len(O)):
        _close(dWs[l], Wr[l].grad if Wr[l].grad is not None else torch.zeros_like(Wr[l]))
        _close(dbs[l], br[l].grad if br[l].grad is not None else torch.zeros_like(br[l]))


@pytest.mark.parametrize("case", [c for c in SC.CHAIN_CASES if c[5]][::3], ids=[c[0] for c in SC.CHAIN_CASES if c[5]][::3])
def test_mlp_chain_reference_is_torch(case):
    name, D, B, L, frozen, backward = case
    x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
    xr, Wr, br = _leaf(x), [_leaf(w) for w in Ws], [_leaf(b) for b in bs]
    h = xr
    for W, b in zip(Wr, br):
        h = F.leaky_relu(F.linear(h, W, b), SC.CHAIN_SLOPE)
    acts = R.mlp_chain_fwd(x.double(), [w.double() for w in Ws], [b.double() for b in bs], SC.CHAIN_SLOPE)
    _close(acts[-1], h.detach(), 1e-12)
    for a in acts[1:]:          # the planted neurons: a pre-activation of exactly 0 in every layer, in fp32 as in fp64
        assert not bool(a[:, list(SC.CHAIN_ZERO_NEURONS)].any())
    h.backward(dout.double())
    dx, dWs, dbs = R.mlp_chain_bwd(dout.double(), acts, [w.double() for w in Ws], SC.CHAIN_SLOPE)
    _close(dx, xr.grad)
    for l in range(L):
        _close(dWs[l], Wr[l].grad)
        _close(dbs[l], br[l].grad)
        assert bool(dbs[l][list(SC.CHAIN_ZERO_NEURONS)].any()), "the derivative at 0 is the slope, not 0"


_CONV_VS_TORCH = [c for c in SC.CONV_CASES if c[0] in ("step_w1_r5", "step_w4_r1", "k8", "cin264_s3_r8", "k768_at_split", "all_present")]


@pytest.mark.parametrize("case", _CONV_VS_TORCH, ids=[c[0] for c in _CONV_VS_TORCH])
def test_grouped_conv_reference_is_conv1d_expert_by_expert(case):
    name, Cin, Cout, S, R_, plan, bias = case
    x, dy, Ws, bs, gW, gb = SC.conv_inputs(case)
    cls = SC.plan_cls(plan, R_)
    xr, Wr, br = _leaf(x), [_leaf(w) for w in Ws], [_leaf(b) for b in bs]
    y = torch.stack([F.conv1d(xr[i].t().unsqueeze(0), Wr[cls[i]], br[cls[i]] if bias else None, padding=S // 2)[0].t() for i in range(cls.size)])
    (y * dy.double()).sum().backward()
    W64 = [w.double() for w in Ws]
    _close(R.grouped_conv_fwd(x.double(), cls, W64, [b.double() for b in bs] if bias else None, S), y.detach(), 1e-12)
    _close(R.grouped_conv_dgrad(dy.double(), cls, W64, S), xr.grad)
    wg = R.grouped_conv_wgrad(dy.double(), x.double(), cls, S)
    assert set(wg) == set(SC.PLANS[plan][R_])
    for e in range(SC.E):
        if e in wg:
            _close(wg[e][0], Wr[e].grad)
            if bias:
                _close(wg[e][1], br[e].grad)
        else:
            assert Wr[e].grad is None
    acc = R.segment_accumulate(dy.double()[:, 0], cls)
    for e, i0, i1 in R.runs_of(cls):
        _close(acc[e], dy.double()[i0:i1, 0].sum(0), 1e-12)


def test_char_extractor_reference_matches_the_module_layout():
    """the per-class reference network takes the experts' own parameter kinds (model/expert_bank.KINDS) and the module's layer order"""
    from handwriting_line_generation_amd.model import expert_bank
    assert tuple(expert_bank.KINDS) == R.EXPERT_KINDS
    g = SC.gen("char_extractor")
    C, dim, style = 16, 8, 12
    shapes = {"w1": (dim, C, 3), "b1": (dim,), "g1": (dim,), "be1": (dim,), "w2": (C, dim, 3), "b2": (C,), "w3": (2 * dim, C, 1), "b3": (2 * dim,),
              "g2": (2 * dim,), "be2": (2 * dim,), "w4": (2 * dim, 2 * dim), "b4": (2 * dim,), "w5": (style, 2 * dim), "b5": (style,)}
    p = {k: torch.randn(s, generator=g, dtype=torch.float64) * 0.3 for k, s in shapes.items()}
    x = torch.randn(5, 5, C, generator=g, dtype=torch.float64)
    both = R.char_extractor(p, x, 2, 4)
    one_by_one = torch.cat([R.char_extractor(p, x[i:i + 1], 2, 4) for i in range(5)])
    assert both.shape == (5, style)
    _close(both, one_by_one, 1e-12)             # window by window: no statistic is shared between windows


# ---- the tables reach every regime ---------------------------------------------------------------------------------------------------------
def test_constants_are_the_package_ones():
    from handwriting_line_generation_amd.model import expert_bank
    assert (expert_bank.TILE_ROWS, expert_bank.WGRAD_TILE_ROWS) == (SC.GT_ROWS, SC.WGRAD_TILE_ROWS)
    src = open(os.path.join(SC.PKG, "csrc", "expert_bank.hip")).read() + open(os.path.join(SC.PKG, "csrc", "style_ops.hip")).read()
    for text in ("constexpr int MAXR = %d;" % SC.MAXR, "constexpr int GT_ROWS = %d;" % SC.GT_ROWS, "constexpr int GT_CK = %d;" % SC.GT_CK,
                 "Cin * S >= %d ? 512 : 256" % SC.SPLIT_K, "constexpr int LB_MAXB = %d;" % SC.LB_MAXB, "constexpr int LB_OCHUNK = %d;" % SC.LB_OCHUNK,
                 "constexpr int MC_MAXB = %d" % SC.MC_MAXB, "lds <= 60 * 1024"):
        assert text in src, text
    assert SC.SEG_LIST_MAX_N == 7679 and SC.E == 6
    assert (SC.CHAIN_L, SC.CHAIN_D, SC.CHAIN_SLOPE) == (6, 128, 0.2) and SC.EXPERT_R == 5 and (SC.STEP_BATCH, SC.GENERATE_BATCH) == (8, 64)


def _union(cases, fn):
    out = set()
    for c in cases:
        out |= fn(c)
    return out


def test_case_tables_cover_the_required_regimes():
    for required, cases, fn in ((SC.REQUIRED_CONV_REGIMES, SC.CONV_CASES, SC.conv_case_regimes), (SC.REQUIRED_SEG_REGIMES, SC.SEG_CASES, SC.seg_case_regimes),
                                (SC.REQUIRED_BANK_REGIMES, SC.BANK_CASES, SC.bank_case_regimes), (SC.REQUIRED_CHAIN_REGIMES, SC.CHAIN_CASES, SC.chain_case_regimes),
                                (SC.REQUIRED_WINDOW_REGIMES, SC.WINDOW_CASES, SC.window_case_regimes)):
        missing = required - _union(cases, fn)
        assert not missing, missing
    for case in SC.CONV_CASES:
        name, Cin, Cout, S, R_, plan, bias = case
        assert Cin % 8 == 0 and Cout % 4 == 0 and R_ <= SC.MAXR and S in (1, 3)           # what the kernels accept
        assert sorted(SC.PLANS[plan][R_]) == sorted(set(SC.plan_cls(plan, R_).tolist())) and max(SC.PLANS[plan][R_]) < SC.E
    assert set(SC.ACCUMULATE_RUNS.values()) == {1, 7, 8, 9, 17} and SC.ACCUMULATE_C == [256, 300]
    assert len(SC.EXPERTS_RUNS) == 5 and 90 <= sum(SC.EXPERTS_RUNS.values()) <= 110 and max(SC.EXPERTS_RUNS.values()) * SC.EXPERT_R > SC.WGRAD_TILE_ROWS
    # the step's layers through autograd; B = 17 backward passes exist as forward-only cases (the GPU test asserts their refusal)
    assert [l[0] for l in SC.AUTOGRAD_LAYERS] == ["w1", "w2", "w3", "w4", "w5"]
    for case in SC.WINDOW_CASES:
        x, ib, ip, dp, n_in = SC.window_inputs(case)
        assert {0, case[2] - 1} <= set(ip[ib == 0].tolist())                              # centres at 0 and Wx - 1
        assert int((ip < 0).sum()) >= 2 and int((ip >= case[2]).sum()) >= 2 and int((ib < 0).sum()) == 1 and int((ib >= case[1]).sum()) == 1


# ---- sensitivity: seeded flaws -------------------------------------------------------------------------------------------------------------
def _moves(got, refs):
    """over the outputs: the worst |flawed - ref| / bound per element (derived bound), or rel L2 / (YARDSTICK_FACTOR * yardstick) where the
    output is held to the yardstick alone"""
    worst = 0.0
    for k, (want, yard, bound) in refs.items():
        if bound is not None:
            worst = max(worst, _ratio_rows(got[k], want, bound))
        else:
            worst = max(worst, _rel(got[k], want) / (YARDSTICK_FACTOR * yard))
    return worst


def test_flawed_copies_without_flaws_are_the_restatements():
    for case in SC.CONV_CASES[:2] + SC.CONV_CASES[10:12]:
        a, b = G.conv_values(case, _d), G.conv_values(case, _d, fwd=grouped_conv_fwd, wgrad=grouped_conv_wgrad)
        assert all(torch.equal(a[k], b[k]) for k in a)
    for case in SC.BANK_CASES[:3]:
        a, b = G.bank_values(case, _d), G.bank_values(case, _d, fwd=linear_bank_fwd, bwd=linear_bank_bwd)
        assert all(torch.equal(a[k], b[k]) for k in a)
    for case in SC.CHAIN_CASES[:4]:
        a, b = G.chain_values(case, _d)[0], G.chain_values(case, _d, fwd=mlp_chain_fwd, bwd=mlp_chain_bwd)[0]
        assert all(torch.equal(a[k], b[k]) for k in a)
    for case in SC.SEG_CASES[:3]:
        v, wgt, seg, dout = SC.seg_inputs(case)
        assert all(torch.equal(p, q) for p, q in zip(R.segment_mean(v.double(), wgt.double(), seg, case[2]), segment_mean(v.double(), wgt.double(), seg, case[2])))
    case = SC.WINDOW_CASES[0]
    x, ib, ip, dp, n_in = SC.window_inputs(case)
    assert torch.equal(R.scatter_windows(dp.double(), ib, ip, case[4], case[1], case[2]), scatter_windows(dp.double(), ib, ip, case[4], case[1], case[2]))


CONV_FLAWS = {"conv_tap_crosses_window": "fwd", "conv_drop_last_group": "fwd", "conv_upper_k_half": "fwd", "wgrad_tile_last_row": "wgrad",
              "wgrad_single_tile_twice": "wgrad"}


@pytest.mark.parametrize("flaw", sorted(CONV_FLAWS))
def test_conv_cases_notice_a_seeded_flaw(flaw):
    hit = {}
    for case in SC.CONV_CASES:
        if case[0].startswith("step_") and case[0] not in ("step_w1_r5", "step_w3_r5", "step_w5_r1"):
            continue                                    # (the other step layers add nothing here)
        kw = {"fwd": lambda *a: grouped_conv_fwd(*a, flaw=flaw)} if CONV_FLAWS[flaw] == "fwd" else {"wgrad": lambda *a: grouped_conv_wgrad(*a, flaw=flaw)}
        move = _moves(G.conv_values(case, _d, **kw), G.conv_reference(case))
        if move >= SENSITIVITY_FACTOR:
            hit[case[0]] = move
    print("\n%s moves (case, x bound): %s" % (flaw, ", ".join("%s %.1e" % h for h in hit.items())))
    expect = {"conv_tap_crosses_window": "step_w1_r5", "conv_drop_last_group": "cin264_s3", "conv_upper_k_half": "cin264_s3",
              "wgrad_tile_last_row": "step_w3_r5", "wgrad_single_tile_twice": "all_present"}[flaw]
    assert expect in hit, (flaw, hit)


@pytest.mark.parametrize("flaw", ["seg_drop_past_8", "seg_wsum_misses_last"])
def test_segment_mean_cases_notice_a_seeded_flaw(flaw):
    hit = {}
    for case in SC.SEG_CASES[:6]:
        v, wgt, seg, dout = SC.seg_inputs(case)
        out, ws = segment_mean(v.double(), wgt.double(), seg, case[2], flaw=flaw)
        got = {"out": out, "dv": R.segment_mean_bwd(dout.double(), wgt.double(), seg, ws)}
        move = _moves(got, G.seg_reference(case))
        if move >= SENSITIVITY_FACTOR:
            hit[case[0]] = move
    print("\n%s moves: %s" % (flaw, ", ".join("%s %.1e" % h for h in hit.items())))
    assert "counts_c300" in hit and "n255" in hit, (flaw, hit)


def test_window_cases_notice_shifted_clipped_windows():
    hit = {}
    for case in SC.WINDOW_CASES:
        name, B, Wx, C, w = case
        x, ib, ip, dp, n_in = SC.window_inputs(case)
        move = _moves({"dx": scatter_windows(dp.double(), ib, ip, w, B, Wx, flaw="scatter_clipped_shifted")}, G.window_reference(case)[1])
        if move >= SENSITIVITY_FACTOR:
            hit[name] = move
    assert {"step_window", "w6_c1", "w6_c256", "w2_c1"} <= set(hit), hit


@pytest.mark.parametrize("flaw", ["bank_second_half_bias", "bank_chunk_first_layer", "bank_rows_wrap_16"])
def test_bank_cases_notice_a_seeded_flaw(flaw):
    hit = {}
    for case in SC.BANK_CASES:
        got = G.bank_values(case, _d, fwd=lambda *a: linear_bank_fwd(*a, flaw=flaw), bwd=lambda *a: linear_bank_bwd(*a, flaw=flaw))
        move = _moves(got, G.bank_reference(case))
        if move >= SENSITIVITY_FACTOR:
            hit[case[0]] = move
    print("\n%s moves: %s" % (flaw, ", ".join("%s %.1e" % h for h in hit.items())))
    expect = {"bank_second_half_bias": "step", "bank_chunk_first_layer": "b16_i100_odd_total", "bank_rows_wrap_16": "b17_fwd"}[flaw]
    assert expect in hit, (flaw, hit)
    if flaw == "bank_rows_wrap_16":
        assert {"b17_fwd", "b64_fwd", "b17_i100_odd_total_fwd"} == set(hit), hit


@pytest.mark.parametrize("flaw", ["chain_rows_from_8", "chain_derivative_at_zero"])
def test_chain_cases_notice_a_seeded_flaw(flaw):
    hit = {}
    for case in SC.CHAIN_CASES:
        got = G.chain_values(case, _d, fwd=lambda *a: mlp_chain_fwd(*a, flaw=flaw), bwd=lambda *a: mlp_chain_bwd(*a, flaw=flaw))[0]
        move = _moves(got, G.chain_reference(case))
        if move >= SENSITIVITY_FACTOR:
            hit[case[0]] = move
    print("\n%s moves: %s" % (flaw, ", ".join("%s %.1e" % h for h in hit.items())))
    if flaw == "chain_rows_from_8":
        assert {c[0] for c in SC.CHAIN_CASES if c[2] > 8} == set(hit), hit
    else:
        assert {c[0] for c in SC.CHAIN_CASES if c[5]} == set(hit), hit
