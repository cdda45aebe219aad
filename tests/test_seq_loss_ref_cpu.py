"""CPU: the fp64 restatements of the sequence / loss / spectral-norm family (oracle/seq_ref.py) against torch's own functional ops in fp64,
the bookkeeping of the GPU case tables (oracle/seq_cases.py: the tables together reach every loop-trip, length and shape regime of the
kernels, every CTC case but `one_infeasible` is feasible), and the sensitivity of those tables: five plausible kernel flaws, seeded by flag
into copies of the restatements that live in this file only, each move some case by at least 10 x the bound the GPU test holds that case to
(so a bound measured on a kernel with such a flaw could not have blessed it)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import seq_cases as SC
from oracle import seq_ref as R
from _seq_loss_checks import BOUNDS, _leaf

F32_ULP = 2.0 ** -23
# a seeded flaw must move some case by this multiple of the bound tests/test_seq_loss_fp64_gpu.py holds that case to
SENSITIVITY_FACTOR = 10.0


def _close(a, b, tol):
    torch.testing.assert_close(a, b, rtol=tol, atol=tol)


def _rel(got, want):
    d = got.double() - want.double()
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    return float(d.norm()) / max(float(want.double().norm()), 1e-300)


# ---- the restatements against torch in fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.LOG_SOFTMAX_CASES, ids=[c[0] for c in SC.LOG_SOFTMAX_CASES])
def test_log_softmax_reference_is_torch(case):
    name, B, T, C, kind = case
    g = SC.gen("lsm_" + name)
    x = SC.logits(kind, B, T, C, g)
    gy = torch.randn(T, B, C, generator=g).double()
    xa, xb = _leaf(x), _leaf(x)
    ya = R.log_softmax_tbc(xa)
    yb = F.log_softmax(xb[:, 0], dim=2).permute(1, 0, 2)
    assert ya.shape == (T, B, C)
    _close(ya, yb, 1e-12)
    ya.backward(gy); yb.backward(gy)
    _close(xa.grad, xb.grad, 1e-10)


_CTC_REF = {}


def _ctc_reference(case):
    """fp64 loss, per-item nll, d loss / d log-probs (free gradient) and d loss / d logits of one case, computed once"""
    name = case[0]
    if name not in _CTC_REF:
        x, tg = SC.ctc_inputs(case)
        x64 = _leaf(x)
        lp = R.log_softmax_tbc(x64)
        lp.retain_grad()
        loss, nll = R.ctc(lp, tg, case[6], case[5])
        loss.backward()
        _CTC_REF[name] = dict(x=x, tg=tg, lp=lp.detach(), loss=loss.detach(), nll=nll, dlp=lp.grad, dx=x64.grad)
    return _CTC_REF[name]


@pytest.mark.parametrize("case", SC.CTC_CASES, ids=[c[0] for c in SC.CTC_CASES])
def test_ctc_reference_is_torch_and_cases_are_what_they_claim(case):
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = case
    ref = _ctc_reference(case)
    x64 = _leaf(ref["x"])
    lp = F.log_softmax(x64[:, 0], dim=2).permute(1, 0, 2)
    lp.retain_grad()
    il, tl = torch.tensor(in_len), torch.tensor(tg_len)
    nll_t = F.ctc_loss(lp, ref["tg"], il, tl, reduction="none", zero_infinity=False).detach()
    assert bool(torch.isfinite(ref["dlp"]).all()) and bool(torch.isfinite(ref["dx"]).all())
    if name == "one_infeasible":
        assert int(torch.isinf(ref["nll"]).sum()) == 1 and bool(torch.isinf(ref["nll"][2])) and bool(torch.isinf(nll_t[2]))
        _close(ref["nll"][:2], nll_t[:2], 1e-12)
        assert float(ref["loss"]) == 0.0
        assert torch.equal(ref["dlp"], torch.zeros_like(ref["dlp"])) and torch.equal(ref["dx"], torch.zeros_like(ref["dx"]))
        return
    assert bool(torch.isfinite(ref["nll"]).all()), ref["nll"]
    _close(ref["nll"], nll_t, 1e-12)
    loss_t = F.ctc_loss(lp, ref["tg"], il, tl, reduction="mean")
    _close(ref["loss"], loss_t.detach(), 1e-12)
    loss_t.backward()
    _close(ref["dx"], x64.grad, 1e-10)
    # torch reports d loss / d log-probs projected through the log-softmax, as the kernels do
    _close(R.ctc_grad_on_simplex(ref["lp"], ref["dlp"]), lp.grad, 1e-10)
    for b in range(B):
        assert torch.equal(ref["dlp"][in_len[b]:, b], torch.zeros(T - in_len[b], C, dtype=torch.float64))
    if name == "one_path":
        # exactly one alignment per item: nll is minus the sum of that path's log-probs
        for b, row in enumerate(targets):
            path = []
            for k, c in enumerate(row):
                path += ([0] if k and row[k - 1] == c else []) + [c]
            assert len(path) == in_len[b]
            want = -sum(ref["lp"][t, b, c] for t, c in enumerate(path))
            _close(ref["nll"][b], want, 1e-12)


@pytest.mark.parametrize("mode", range(5))
def test_loss_reference_is_torch(mode):
    g = SC.gen("loss_ref_%d" % mode)
    a, b = torch.randn(3, 5, 7, generator=g), torch.randn(3, 5, 7, generator=g)
    theirs = [lambda a, b: F.l1_loss(a, b), lambda a, b: F.mse_loss(a, b), lambda a, b: a.mean(), lambda a, b: F.relu(1.0 - a).mean(),
              lambda a, b: F.relu(1.0 + a).mean()][mode]
    for scale in (1.0, -1.0):
        a1, b1, a2, b2 = _leaf(a), _leaf(b), _leaf(a), _leaf(b)
        la, lb = R.loss(a1, b1 if mode < 2 else None, mode, scale), scale * theirs(a2, b2)
        _close(la, lb, 1e-12)
        (la * 0.5).backward(); (lb * 0.5).backward()
        _close(a1.grad, a2.grad, 1e-10)
        if mode < 2:
            _close(b1.grad, b2.grad, 1e-10)


def test_loss_reference_has_zero_gradient_at_ties():
    for case in SC.LOSS_CASES:
        name, mode, n, scale, wrt, inputs = case
        if inputs != "ties":
            continue
        a, b = SC.loss_inputs(case)
        a64 = _leaf(a)
        R.loss(a64, b.double() if b is not None else None, mode, scale).backward()
        assert torch.equal(a64.grad[::2], torch.zeros(-(-n // 2), dtype=torch.float64)) and bool((a64.grad[1::2] != 0).any())


def _power_iteration_as_the_existing_test(w, u, eps):
    wm = w.view(w.shape[0], -1)
    v2 = torch.mv(wm.t().detach(), u); v2 = v2 / (v2.norm() + eps)
    u2 = torch.mv(wm.detach(), v2); u2 = u2 / (u2.norm() + eps)
    sigma = u2.dot(wm.mv(v2))
    return u2, v2, sigma, w / sigma


@pytest.mark.parametrize("R_,K", [(64, 288), (1, 9), (5, 9), (7, 70)])
def test_spectral_reference_is_the_power_iteration_twice(R_, K):
    w1, w2, u, v, g1, g2 = (t.double() for t in SC.sn_inputs("ref", R_, K))
    ua, ub = u, u
    for w, gw in ((w1, g1), (w2, g2)):
        wa, wb = _leaf(w.view(R_, K, 1, 1)), _leaf(w.view(R_, K, 1, 1))
        ua, va, sa, wsa = R.spectral(wa, ua, v, 1e-12)
        ub, vb, sb, wsb = _power_iteration_as_the_existing_test(wb, ub, 1e-12)
        for x, y in ((ua, ub), (va, vb), (sa, sb), (wsa, wsb)):
            _close(x, y, 1e-12)
        assert not ua.requires_grad and not va.requires_grad
        wsa.backward(gw.view_as(wsa)); wsb.backward(gw.view_as(wsb))
        _close(wa.grad, wb.grad, 1e-10)
        # the closed form the kernels use: G / sigma - <G, W> / sigma^2 u v^T
        want = gw / sa.detach() - (gw * w).sum() / sa.detach() ** 2 * torch.outer(ua, va)
        _close(wa.grad.view(R_, K), want, 1e-10)


def test_pixel_norm_and_argmax_references():
    for case in SC.PIXEL_NORM_CASES:
        x, gy = SC.pixel_norm_inputs(case)
        xa, xb = _leaf(x), _leaf(x)
        ya = R.pixel_norm(xa, 1e-8)
        yb = xb / torch.sqrt(torch.mean(xb ** 2, dim=1, keepdim=True) + 1e-8)
        _close(ya, yb, 1e-12)
        ya.backward(gy.double()); yb.backward(gy.double())
        _close(xa.grad, xb.grad, 1e-10)
        if case[2] == "zero_row":
            assert torch.equal(ya[0].detach(), torch.zeros(case[1], dtype=torch.float64))
            _close(xa.grad[0], gy[0].double() / 1e-4, 1e-10)
    for shape in SC.ARGMAX_SHAPES:
        x, planted = SC.argmax_inputs(shape)
        got = R.argmax_first(x)
        for r in range(shape[0]):
            row = x[r].tolist()
            assert int(got[r]) == row.index(max(row))
        for kind, (r, c) in planted.items():
            assert int(got[r]) == c, kind
    assert {k for s in SC.ARGMAX_SHAPES for k in SC.argmax_inputs(s)[1]} == {"same lane", "different lanes", "all equal"}


# ---- case-table bookkeeping ------------------------------------------------------------------------------------------------------------
def test_step_geometry_is_the_models_own():
    assert SC.NUM_CLASS == 80 and SC.T_MODEL == SC.STEP_WIDTH // 4 - 6           # the recogniser's documented T = W / 4 - 6
    cfg = os.path.join(SC.PKG, os.pardir, "configs", "cf_IAM_hwr_cnnOnly_batchnorm_aug.json")
    with open(cfg) as f:
        assert json.load(f)["model"]["num_class"] == SC.NUM_CLASS
    assert len(SC.SN_MODEL_SHAPES) == 10 and (1, 256) in SC.SN_MODEL_SHAPES and (1, 2304) in SC.SN_MODEL_SHAPES
    assert set(SC.SN_MODEL_SHAPES) <= set(SC.SN_SHAPES)


def test_case_tables_reach_every_regime():
    ctc = set().union(*(SC.ctc_case_regimes(c) for c in SC.CTC_CASES))
    assert SC.REQUIRED_REGIMES["ctc"] <= ctc, SC.REQUIRED_REGIMES["ctc"] - ctc
    loss = set().union(*(SC.loss_case_regimes(c) for c in SC.LOSS_CASES))
    assert SC.REQUIRED_REGIMES["loss"] <= loss, SC.REQUIRED_REGIMES["loss"] - loss
    assert {c[2] for c in SC.LOSS_CASES} == set(SC.LOSS_SIZES)
    sn = set().union(*(SC.sn_shape_regimes(r, k) for r, k in SC.SN_SHAPES))
    assert SC.REQUIRED_REGIMES["sn"] <= sn, SC.REQUIRED_REGIMES["sn"] - sn
    assert not any("R * K past the block cap" in SC.sn_shape_regimes(r, k) for r, k in SC.SN_MODEL_SHAPES)     # hence the extra layer
    for name, shapes in SC.SN_BANKS:          # several layers of different sizes per bank call: early-return blocks in both grids
        assert len(set(shapes)) >= 3 and len({r for r, k in shapes}) >= 3 and len({k for r, k in shapes}) >= 3 and len(shapes) <= 16
    shapes = {(B, T, C) for n, B, T, C, k in SC.LOG_SOFTMAX_CASES}
    assert any(B * T > SC.LOG_SOFTMAX_GRID_WAVES for B, T, C in shapes)                                        # rows > 8192
    assert {C for B, T, C in shapes} >= {1, 5, 64, 65, 200, SC.NUM_CLASS} and (SC.STEP_BATCH, SC.T_MODEL, SC.NUM_CLASS) in shapes
    assert {k for *_, k in SC.LOG_SOFTMAX_CASES} == {"randn", "large", "peaked"}
    x = SC.logits("large", 2, 5, 65, SC.gen("overflow"))
    assert bool(torch.isinf(torch.exp(x)).any())                  # float32 exp of these logits overflows without the max subtraction
    assert {(r, c) for r, c, k in SC.PIXEL_NORM_CASES} == {(8, 128), (5, 1), (3, 65), (6, 200)}
    for case in SC.PIXEL_NORM_CASES:
        x, _ = SC.pixel_norm_inputs(case)
        if case[2] == "tiny":
            assert float((x.double() ** 2).mean(1).max()) < SC.PIXEL_NORM_EPS
        if case[2] == "zero_row":
            assert not bool(x[0].any())
    for T, B, Lr in SC.DTW_CASES:
        assert 2 * Lr + 1 > 256
    assert not bool(SC.dtw_inputs(SC.DTW_CASES[0])[1][-7:, 0].any())


# ---- sensitivity: seeded flaws ---------------------------------------------------------------------------------------------------------
def _ctc_flawed(lp, targets, in_len, tg_len, skip_over_repeats=False, nll_at_last_row=False, no_clamp=False):
    """R.ctc with three flaws behind flags (all off: the same arithmetic as R.ctc, checked below)"""
    T, B, C = lp.shape
    out = []
    for b in range(B):
        S, Tb = int(tg_len[b]), int(in_len[b])
        if nll_at_last_row:
            Tb = T                                                  # FLAW: the recursion runs over, and nll is read at, row T - 1
        ext = torch.zeros(2 * S + 1, dtype=torch.long)
        ext[1::2] = targets[b, :S].long()
        skip = torch.zeros(2 * S + 1, dtype=torch.bool)
        skip[2:] = (ext[2:] != 0) if skip_over_repeats else (ext[2:] != ext[:-2])       # FLAW: s - 2 -> s allowed across a repeat
        minus = lp.new_full((2,), R.NEG)
        alpha = torch.cat((lp[0, b, ext[:2]], lp.new_full((2 * S + 1,), R.NEG)[2:]))
        for t in range(1, Tb):
            a1 = torch.cat((minus[:1], alpha[:-1]))
            a2 = torch.where(skip, torch.cat((minus, alpha[:-2]))[: 2 * S + 1], minus[:1])
            alpha = R._lse_rows(torch.stack((alpha, a1, a2))) + lp[t, b, ext]
        out.append(-R._lse_rows(alpha[-2:].reshape(-1, 1))[0])
    nll = torch.stack(out)
    div = torch.as_tensor(tg_len).to(nll.dtype)
    if not no_clamp:                                                # FLAW: nll / 0 for an empty target
        div = div.clamp(min=1)
    mean = (nll / div).sum() / B
    if bool(torch.isinf(mean)):
        mean = (lp * 0.0).sum()
    return mean


def _loss_flawed(a, b, mode, scale, drop_last_partial_block=False):
    n = a.numel()
    if drop_last_partial_block:                                     # FLAW: the elements behind the last full block of 256 are not summed
        keep = n // 256 * 256
        if keep == 0:
            return a.sum() * 0.0
        return R.loss(a[:keep], b[:keep] if b is not None else None, mode, scale) * keep / n
    return R.loss(a, b, mode, scale)


def _spectral_flawed(w_bar, u, v, eps, sigma_from_old_u=False):
    u1, v1, sigma, wsn = R.spectral(w_bar, u, v, eps)
    if sigma_from_old_u:                                            # FLAW: sigma = u . (W v') with the u of before the iteration
        sigma = u @ (w_bar.reshape(w_bar.shape[0], -1) @ v1)
        wsn = w_bar / sigma
    return u1, v1, sigma, wsn


def _ctc_moves(case, **flaw):
    """relative L2 moves of (loss, d loss / d logits) of one CTC case under a flaw"""
    ref = _ctc_reference(case)
    x64 = _leaf(ref["x"])
    loss = _ctc_flawed(R.log_softmax_tbc(x64), ref["tg"], case[6], case[5], **flaw)
    loss.backward()
    return _rel(loss.detach(), ref["loss"]), _rel(x64.grad, ref["dx"])


def test_flawed_copies_without_flaws_are_the_restatements():
    for case in SC.CTC_CASES[2:7]:
        assert _ctc_moves(case) == (0.0, 0.0), case[0]


FEASIBLE = [c for c in SC.CTC_CASES if c[9] is not None]


@pytest.mark.parametrize("flaw", ["skip_over_repeats", "nll_at_last_row", "no_clamp"])
def test_ctc_cases_notice_a_seeded_flaw(flaw):
    bounds = BOUNDS
    hit = []
    for case in FEASIBLE:
        if case[1] > 300:
            continue                # (the 600-step case adds nothing here and costs a second)
        d_loss, d_grad = _ctc_moves(case, **{flaw: True})
        if d_loss >= SENSITIVITY_FACTOR * bounds[case[9] + "_loss"][0] and d_grad >= SENSITIVITY_FACTOR * bounds[case[9] + "_grad"][0]:
            hit.append((case[0], d_loss, d_grad))
    print("\n%s moves (case, loss, d logits): %s" % (flaw, ", ".join("%s %.1e %.1e" % h for h in hit)))
    assert hit, flaw
    expect = {"skip_over_repeats": "states_gt_256", "nll_at_last_row": "ragged", "no_clamp": "ragged"}[flaw]
    assert expect in [h[0] for h in hit]


def test_loss_cases_notice_a_dropped_partial_block():
    hit = []
    for case in SC.LOSS_CASES:
        name, mode, n, scale, wrt, inputs = case
        a, b = SC.loss_inputs(case)
        a, b = a.double(), b.double() if b is not None else None
        move = _rel(_loss_flawed(a, b, mode, scale, True), R.loss(a, b, mode, scale))
        if move >= SENSITIVITY_FACTOR * (2 * F32_ULP):
            hit.append(name)
        elif n % 256 == 0:
            assert move == 0.0
    assert {"m0_n255", "m1_n255", "m2_n255", "m3_n255", "m4_n255", "m1_n4097"} <= set(hit), hit


def test_spectral_cases_notice_sigma_from_the_old_u():
    bounds = BOUNDS
    hit = []
    for R_, K in SC.SN_SHAPES:
        w1, w2, u, v, g1, g2 = (t.double() for t in SC.sn_inputs("single", R_, K))
        good, bad = R.spectral(w1, u, v, 1e-12), _spectral_flawed(w1, u, v, 1e-12, True)
        if _rel(bad[2], good[2]) >= SENSITIVITY_FACTOR * bounds["sn_sigma"][0] and _rel(bad[3], good[3]) >= SENSITIVITY_FACTOR * bounds["sn_w"][0]:
            hit.append((R_, K))
    assert len(hit) >= len(SC.SN_SHAPES) - 2, hit           # (R = 1: u' = +-1 whatever u was; every other shape notices)
