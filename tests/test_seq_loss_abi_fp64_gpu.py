"""GPU: the entries of csrc/seq_ops.hip and csrc/spectral_loss.hip - hwg_log_softmax_fwd / _bwd, hwg_ctc_fwd / _bwd / _fwd_beta / _bwd_grad,
hwg_dtw_align, hwg_gt_counts, hwg_loss_fwd / _bwd, hwg_masked_l1_fwd / _bwd, hwg_spectral_update / _update_to / _update_multi, hwg_scale_by_ptr,
hwg_spectral_bwd / _bwd_multi, hwg_pixelnorm_fwd / _bwd - called at the C ABI through L.query on guarded buffers, against the fp64 restatements
of oracle/seq_ref.py. The protocol (guarded operands, a workspace of exactly the queried size poisoned with NaN, a second call on a zero-filled
workspace, the under-run by one byte and the null workspace) is that of tests/_guarded.py, with its buffers;
case tables: oracle/abi_cases.py, checked on the CPU by tests/test_abi_cases_cpu.py; the bounds are BOUNDS / DERIVED of
tests/_seq_loss_checks.py, which tests/test_seq_loss_fp64_gpu.py holds the same kernels to: the same arithmetic. The library's default tuning only.

Per entry, what is asserted beyond the protocol, and the worst ratio measured on an MI355X (relative L2 and max|err| / max|ref|, each divided
by its bound, unless a per-element bound is stated; every case prints its own line, kept in profiles/norm_seq_abi_fp64.txt):

  hwg_log_softmax_fwd, _bwd     transpose_bt = 1 against BOUNDS["lsm_fwd"] / ["lsm_grad"] and the bits of ops.log_softmax_tbc; transpose_bt    [y 0.23 / 0.20,
                                = 0 (no Python caller): y and dx are the transpose_bt = 1 outputs with the rows permuted, bit for bit.          dx 0.26 / 0.14]
  hwg_ctc_fwd, _bwd,            the workspace is poisoned before the forward call only (backward reads what forward left). loss and         [loss 0.39 / 0.39,
  hwg_ctc_fwd_beta, _bwd_grad   d log-probs against BOUNDS[family + "_loss" / "_grad"]; the gradient behind an input length is +0 bit       d log-probs 0.08 / 0.07]
                                for bit; an infeasible sample: loss +0 and every gradient +0; the _fwd_beta + _bwd_grad pair gives the
                                bits of the _fwd + _bwd pair (the header's promise); both have the bits of ops.ctc_loss.
  hwg_dtw_align, hwg_gt_counts  the path, its length and the run-length counts equal the oracle's (oracle/seq_oracle.py) exactly; rows       [exact]
                                behind the path are 0.
  hwg_loss_fwd, _bwd            DERIVED["loss_value" / "loss_value_mse" / "loss_grad_const"], BOUNDS["mse_grad"]; bits of ops._Loss.        [value 0.44 / 0.44, gradients 0.50 / 0.50]
  accumulate = 1 of both        (no Python caller) one rounded sum more than the plain call, per element, u = 2^-24:                         [value 0.38, gradients 0.92]
                                  |out - (out0 + v)| <= (k 2u |v| + u |out0 + v|) (1 + 2^-16), v = scale * mean, k = 1 (2 for the squares)
                                  |da - (da0 + d)| <= (k 2u |d| + u |da0 + d|) (1 + 2^-16); db likewise with db0 - d
                                (the first term is DERIVED's bound on the plain call's value, the second the rounding of the new sum)
  hwg_masked_l1_fwd, _bwd       DERIVED["loss_value"] / ["loss_grad_const"] against tests/_fg_mask_ref.masked_l1 (products rounded to       [value 0.14 / 0.14, gradient 0.52 / 0.71]
                                fp32: the definition); the gradient is 0 where the mask is 0 or narrower than the image; bits of
                                ops.masked_l1_loss.
  hwg_spectral_update_to,       u, v against BOUNDS["sn_uv"], sigma and 1 / sigma against BOUNDS["sn_sigma"]. hwg_spectral_update equals       [u, v 0.04 / 0.03,
  hwg_spectral_update           _update_to with null copies; _update_to with one null copy equals the call with both, on u, v, sigma,       sigma, 1 / sigma 0.19 / 0.19]
                                1 / sigma; a copy that is asked for has the bits of the vector; bits of ops.spectral_normalize.
  hwg_scale_by_ptr              BOUNDS["sn_w"]                                                                                               [0.12 / 0.14]
  hwg_spectral_bwd              written and added to a pre-filled dW_bar, BOUNDS["sn_grad"]; bits of the ops backward pass. At (1, 1)         [0.12 / 0.16]
                                W / sigma is +-1 whatever W is: the gradient is the exact cancellation of g / sigma against itself and
                                no fp32 evaluation keeps a digit of it - there the error is measured against the size of g / sigma (as
                                tests/test_seq_loss_fp64_gpu.py does for the one-channel pixel norm).
  hwg_spectral_update_multi     five layers in one call, scratch and snapshot buffers guarded (no size to under-run): per layer the           [u, v 0.06 / 0.05, sigma, 1 / sigma 0.40 / 0.40]
                                bounds of the single call; the snapshot has the bits of u, v.
  hwg_spectral_bwd_multi        the bits of five single hwg_spectral_bwd calls (the header's promise), full protocol                          [exact]
  hwg_pixelnorm_fwd, _bwd       BOUNDS["pixelnorm_fwd" / "pixelnorm_grad" / "pixelnorm_grad_c1"], bits of ops.pixel_norm                     [y 0.26 / 0.25, dx 0.26 / 0.25]
  refusals                      hwg_loss_bwd with a mode outside 0..4 or a pair mode without b, ctc_bwd with a non-positive size:
                                HWG_ERR_ARG before any launch, outputs still NaN."""
import numpy as np
import pytest
import torch

import _fg_mask_ref as FG
from oracle import abi_cases as AC
from oracle import seq_cases as SC
from oracle import seq_ref as R
from _fp64 import SECOND, U, _f32, _ratio, cpu_threads, report
from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)
from _guarded import NAN, Guarded, bits_differ, protocol, refused, same_bits
from _seq_loss_checks import ACC_CASES, BOUNDS, DERIVED, _leaf

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
GOUT = SC.LOSS_GOUT


def _bound(family):
    return DERIVED[family] if family in DERIVED else BOUNDS[family]


def _lib():
    from handwriting_line_generation_amd import _lib as L
    return L


def _worst(got, want, bound):
    """worst |err| / bound over the elements, per-element bounds"""
    return _ratio(got.reshape(want.shape), want, bound)


# ---- log-softmax -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.LOG_SOFTMAX_CASES, ids=[c[0] for c in AC.LOG_SOFTMAX_CASES])
def test_log_softmax_entries_both_row_orders(cuda, case):
    from handwriting_line_generation_amd import ops
    L = _lib()
    name, B, T, C, kind = case
    g = SC.gen("abi_lsm_" + name)
    x = SC.logits(kind, B, T, C, g)
    gy = torch.randn(T, B, C, generator=g)
    rows = B * T
    out = {}
    for tr in (1, 0):
        G = Guarded(cuda, dict(x=x), dict(y=((T, B, C) if tr else (rows, C), F32)))
        f = G.f
        y = protocol(G, "%s hwg_log_softmax_fwd transpose %d" % (name, tr), lambda ws, n: L.query("hwg_log_softmax_fwd", f["x"], f["y"], rows, C, B, T, tr, G.st))["y"]
        dy = gy if tr else gy.permute(1, 0, 2).reshape(rows, C).contiguous()
        G2 = Guarded(cuda, dict(dy=dy, y=y), dict(dx=((B, 1, T, C), F32)))
        h = G2.f
        dx = protocol(G2, "%s hwg_log_softmax_bwd transpose %d" % (name, tr),
                      lambda ws, n: L.query("hwg_log_softmax_bwd", h["dy"], h["y"], h["dx"], rows, C, B, T, tr, G2.st))["dx"]
        out[tr] = (y, dx)
    cpu_threads()
    x64 = _leaf(x)
    yr = R.log_softmax_tbc(x64)
    yr.backward(gy.double())
    shape = "B%d T%d C%d %s" % (B, T, C, kind)
    bad = report("hwg_log_softmax_fwd", shape, 0, [("y", out[1][0], yr.detach(), BOUNDS["lsm_fwd"]),
                                                   ("y rows", out[0][0], R.log_softmax_rows(x.double()), BOUNDS["lsm_fwd"])])
    bad += report("hwg_log_softmax_bwd", shape, 0, [("dx", out[1][1], x64.grad, BOUNDS["lsm_grad"])])
    differ = bits_differ([("y", out[0][0].reshape(B, T, C), out[1][0].permute(1, 0, 2).contiguous()), ("dx", out[0][1], out[1][1])])
    assert not differ, "%s: transpose_bt = 0 is not transpose_bt = 1 with the rows permuted in %s" % (name, differ)
    xg = x.to(cuda).requires_grad_(True)
    yo = ops.log_softmax_tbc(xg)
    yo.backward(gy.to(cuda))
    torch.cuda.synchronize()
    differ = bits_differ([("y", out[1][0], yo.detach()), ("dx", out[1][1], xg.grad)])
    assert not differ, "%s: %s differ from the bits of ops.log_softmax_tbc" % (name, differ)
    assert not bad, "%s vs fp64: %s" % (name, "; ".join(bad))


# ---- CTC -------------------------------------------------------------------------------------------------------------------------------------------
def _ctc_guarded(dev, case):
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = case
    L = _lib()
    x, tg = SC.ctc_inputs(case)
    lp = torch.log_softmax(x[:, 0].permute(1, 0, 2), dim=2).contiguous()             # [T, B, C] fp32: what kernel and reference both read
    need = int(L.query("hwg_ctc_workspace", T, B, Lmax))
    assert need == AC.ctc_workspace_bytes(T, B, Lmax)
    G = Guarded(dev, dict(lp=lp, tg=tg.to(I32), il=torch.tensor(in_len, dtype=I32), tl=torch.tensor(tg_len, dtype=I32), gout=torch.tensor([GOUT])),
                dict(loss=((1,), F32), grad=((T, B, C), F32)), need)
    f = G.f
    fwd = lambda entry: (lambda ws, n, **o: L.query(entry, f["lp"], f["tg"], f["il"], f["tl"], o.get("T", T), o.get("B", B), o.get("C", C), o.get("Lmax", Lmax),        # noqa: E731
                                                    f["loss"], ws, n, G.st))
    bwd = lambda entry: (lambda ws, n, **o: L.query(entry, f["lp"], f["tg"], f["il"], f["tl"], o.get("T", T), o.get("B", B), o.get("C", C), o.get("Lmax", Lmax),        # noqa: E731
                                                    f["gout"], f["grad"], ws, n, G.st))
    return G, lp, tg, fwd, bwd


def _ctc_pair(G, name, fwd, bwd, e_fwd, e_bwd):
    """forward under the full protocol, once more on a poisoned workspace, then backward on the workspace that call left -> (loss, grad)"""
    loss = protocol(G, "%s %s" % (name, e_fwd), fwd(e_fwd), mine=("loss",))["loss"]
    G.reset()
    G.ws_fill(NAN)
    assert fwd(e_fwd)(G.ws, G.need) == 0
    torch.cuda.synchronize()
    assert same_bits(G.get("loss"), loss)
    grad = protocol(G, "%s %s" % (name, e_bwd), bwd(e_bwd), mine=("grad",), poison_ws=False)["grad"]
    return loss, grad


@pytest.mark.parametrize("case", AC.CTC_CASES, ids=[c[0] for c in AC.CTC_CASES])
def test_ctc_entries_on_a_poisoned_workspace(cuda, case):
    from handwriting_line_generation_amd import ops
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = case
    G, lp, tg, fwd, bwd = _ctc_guarded(cuda, case)
    loss, grad = _ctc_pair(G, name, fwd, bwd, "hwg_ctc_fwd", "hwg_ctc_bwd")
    loss_b, grad_b = _ctc_pair(G, name, fwd, bwd, "hwg_ctc_fwd_beta", "hwg_ctc_bwd_grad")
    differ = bits_differ([("loss", loss_b, loss), ("grad", grad_b, grad)])
    assert not differ, "%s: hwg_ctc_fwd_beta + hwg_ctc_bwd_grad differ from hwg_ctc_fwd + hwg_ctc_bwd in %s" % (name, differ)
    for b in range(B):          # behind an item's input length: +0, bit for bit
        assert not grad[in_len[b]:, b].view(I32).any(), "%s: the gradient behind in_len of item %d is not +0" % (name, b)
    cpu_threads()
    lp64 = _leaf(lp)
    lr, nll = R.ctc(lp64, tg, in_len, tg_len)
    (lr * GOUT).backward()
    shape = "T%d B%d C%d Lmax%d NS%d" % (T, B, C, Lmax, 2 * Lmax + 1)
    if family is None:          # one item without an alignment: loss +0, every gradient +0 - of the feasible items too
        assert int(torch.isinf(nll).sum()) == 1 and float(lr.detach()) == 0.0
        assert not loss.view(I32).any() and not grad.view(I32).any(), "%s: loss / gradient of an infeasible batch are not +0" % name
        print("\nabi %-22s %-34s ws %-9d loss +0, gradient +0: exact" % ("hwg_ctc_*", shape, G.need))
        bad = []
    else:
        dlp = R.ctc_grad_on_simplex(lp64, lp64.grad)
        bad = report("hwg_ctc_fwd(_beta)", shape, G.need, [("loss", loss, lr.detach().reshape(1), BOUNDS[family + "_loss"])])
        bad += report("hwg_ctc_bwd(_grad)", shape, G.need, [("dlogp", grad, dlp, BOUNDS[family + "_grad"])])
    lpg = lp.to(cuda).requires_grad_(True)
    lo = ops.ctc_loss(lpg, tg, torch.tensor(in_len), torch.tensor(tg_len))
    (lo * GOUT).backward()
    torch.cuda.synchronize()
    differ = bits_differ([("loss", loss, lo.detach().reshape(1)), ("grad", grad, lpg.grad)])
    assert not differ, "%s: %s differ from the bits of ops.ctc_loss" % (name, differ)
    assert not bad, "%s vs fp64: %s" % (name, "; ".join(bad))


# ---- DTW alignment, run-length counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.DTW_CASES, ids=lambda c: "T%d_B%d_L%d" % c)
def test_dtw_and_gt_counts_entries_exact(cuda, case):
    from oracle import seq_oracle
    L = _lib()
    T, B, Lr = case
    pred, label = SC.dtw_inputs(case)
    C, LL = pred.shape[2], 2 * Lr + 1
    need = int(L.query("hwg_dtw_workspace", T, B, Lr))
    assert need == AC.dtw_workspace_bytes(T, B, Lr)
    G = Guarded(cuda, dict(pred=pred, label=label.to(I32)), dict(out=((T + LL, B), I64), lens=((B,), I32)), need)
    f = G.f
    got = protocol(G, "hwg_dtw_align T%d B%d L%d" % case, lambda ws, n: L.query("hwg_dtw_align", f["pred"], f["label"], T, B, C, Lr, f["out"], f["lens"], ws, n, G.st))
    ref = seq_oracle.correct_pred(pred, label)
    n = ref.shape[0]
    assert int(got["lens"].max()) == n and torch.equal(got["out"][:n], ref) and not got["out"][n:].any(), "dtw T=%d B=%d L=%d" % case
    gt_ref, pos_ref = seq_oracle.gt_counts(ref, label)
    G2 = Guarded(cuda, dict(index=ref.contiguous(), label=label.to(I32)),
                 dict(gt=torch.zeros(Lr, B, 2), minpos=torch.tensor([2 ** 31 - 1], dtype=I32), mismatch=torch.zeros(1, dtype=I32)))
    h = G2.f
    c = protocol(G2, "hwg_gt_counts T%d B%d L%d" % case,
                 lambda ws, n_: L.query("hwg_gt_counts", h["index"], h["label"], n, B, Lr, h["gt"], h["minpos"], h["mismatch"], G2.st))
    assert torch.equal(c["gt"], gt_ref) and int(c["minpos"]) == pos_ref and int(c["mismatch"]) == 0
    print("\nabi %-22s %-34s ws %-9d path of %d steps and its run-length counts exact" % ("hwg_dtw_align/gt_counts", "T%d B%d L%d" % case, need, n))


# ---- losses ------------------------------------------------------------------------------------------------------------------------------------------
def _loss_guarded(dev, case, out0=None, da0=None, db0=None):
    name, mode, n, scale, wrt, inputs = case
    L = _lib()
    a, b = SC.loss_inputs(case)
    need_a, need_b = wrt in ("a", "both"), mode < 2 and wrt in ("b", "both")
    ins = dict(a=a) if b is None else dict(a=a, b=b)
    acc = int(out0 is not None)
    need = int(L.query("hwg_loss_workspace"))
    assert need == AC.LOSS_WORKSPACE_BYTES
    G = Guarded(dev, ins, dict(out=out0 if acc else ((1,), F32)), need)
    f = G.f
    fwd = lambda ws, n_, **o: L.query("hwg_loss_fwd", f["a"], f.get("b"), n, o.get("mode", mode), scale, f["out"], acc, ws, n_, G.st)        # noqa: E731
    outs = {}
    if need_a:
        outs["da"] = da0 if acc else ((n,), F32)
    if need_b:
        outs["db"] = db0 if acc else ((n,), F32)
    G2 = Guarded(dev, dict(ins, gout=torch.tensor([GOUT])), outs)
    h = G2.f
    bwd = lambda ws=None, n_=0, **o: L.query("hwg_loss_bwd", h["a"], None if o.get("no_b") else h.get("b"), n, o.get("mode", mode), scale, h["gout"], h.get("da"),        # noqa: E731
                                             h.get("db"), acc, G2.st)
    return a, b, need_a, need_b, G, fwd, G2, bwd


def _loss_reference(case, a, b, need_a, need_b):
    name, mode, n, scale, wrt, inputs = case
    a64 = a.double().requires_grad_(need_a)
    b64 = b.double().requires_grad_(need_b) if b is not None else None
    lr = R.loss(a64, b64, mode, _f32(scale))
    (lr * GOUT).backward()
    return lr.detach().reshape(1), a64.grad, b64.grad if b64 is not None else None


@pytest.mark.parametrize("case", AC.LOSS_CASES, ids=[c[0] for c in AC.LOSS_CASES])
def test_loss_entries_on_guarded_buffers_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, mode, n, scale, wrt, inputs = case
    a, b, need_a, need_b, G, fwd, G2, bwd = _loss_guarded(cuda, case)
    out = protocol(G, name + " hwg_loss_fwd", fwd)["out"]
    grads = protocol(G2, name + " hwg_loss_bwd", bwd)
    lr, da, db = _loss_reference(case, a, b, need_a, need_b)
    shape = "mode%d n%d scale%+d wrt %s" % (mode, n, scale, wrt)
    bad = report("hwg_loss_fwd", shape, G.need, [("loss", out, lr, DERIVED["loss_value_mse" if mode == 1 else "loss_value"])])
    gb = _bound("mse_grad" if mode == 1 else "loss_grad_const")
    bad += report("hwg_loss_bwd", shape, 0, ([("da", grads["da"], da, gb)] if need_a else []) + ([("db", grads["db"], db, gb)] if need_b else []))
    ag = a.to(cuda).requires_grad_(need_a)
    bg = b.to(cuda).requires_grad_(need_b) if b is not None else None
    lo = ops._Loss.apply(ag, bg, mode, scale)
    (lo * GOUT).backward()
    torch.cuda.synchronize()
    differ = bits_differ([("loss", out, lo.detach().reshape(1))] + ([("da", grads["da"], ag.grad)] if need_a else []) + ([("db", grads["db"], bg.grad)] if need_b else []))
    assert not differ, "%s: %s differ from the bits of ops._Loss" % (name, differ)
    assert not bad, "%s vs fp64: %s" % (name, "; ".join(bad))


@pytest.mark.parametrize("case", ACC_CASES, ids=[c[0] for c in ACC_CASES])
def test_loss_entries_accumulate_into_prefilled_outputs(cuda, case):
    """accumulate = 1: out0 + v and da0 + d, db0 - d, one rounded sum more than the plain call (the bound of the module docstring)"""
    name, mode, n, scale, wrt, inputs = case
    a, b = SC.loss_inputs(case)
    need_a, need_b = wrt in ("a", "both"), mode < 2 and wrt in ("b", "both")
    lr, da, db = _loss_reference(case, a, b, need_a, need_b)
    g = SC.gen("abi_loss_acc_" + name)
    out0 = (lr * 0.75).float()                                                   # of the value's own sign and size
    gmax = float((da if need_a else db).abs().max())
    da0, db0 = torch.randn(n, generator=g) * gmax, torch.randn(n, generator=g) * gmax
    _, _, _, _, G, fwd, G2, bwd = _loss_guarded(cuda, case, out0, da0, db0)
    out = protocol(G, name + " hwg_loss_fwd accumulate", fwd)["out"]
    grads = protocol(G2, name + " hwg_loss_bwd accumulate", bwd)
    k = 2 if mode == 1 else 1
    want = R.loss_accumulate(out0.double(), a.double(), b.double() if b is not None else None, mode, _f32(scale))
    parts = ["out %.2f" % _worst(out, want, (k * 2 * U * lr.abs() + U * want.abs()) * SECOND)]
    for nm, need, g0, d in (("da", need_a, da0, da), ("db", need_b, db0, db)):
        if need:
            w = g0.double() + d
            parts.append("%s %.2f" % (nm, _worst(grads[nm], w, (k * 2 * U * d.abs() + U * w.abs()) * SECOND)))
    print("\nabi %-22s %-34s ws %-9d e/b %s" % ("hwg_loss_* accumulate", "mode%d n%d scale%+d wrt %s" % (mode, n, scale, wrt), G.need, "  ".join(parts)))
    assert all(float(p.split()[1]) <= 1.0 for p in parts), "%s accumulate: |err| over the derived bound: %s" % (name, parts)


def test_loss_bwd_and_ctc_bwd_refusals_write_nothing(cuda):
    """hwg_loss_bwd makes the checks of hwg_loss_fwd (mode in 0..4, a pair mode needs b), ctc_bwd those of ctc_fwd (positive sizes)"""
    case = next(c for c in AC.LOSS_CASES if c[1] == 0 and c[4] == "both")
    _, _, _, _, G, fwd, G2, bwd = _loss_guarded(cuda, case)
    for what, over in (("mode 5", dict(mode=5)), ("mode -1", dict(mode=-1)), ("mode 0 without b", dict(no_b=True)), ("mode 1 without b", dict(mode=1, no_b=True))):
        refused(G2, "hwg_loss_bwd " + what, lambda: bwd(**over))
    for what, over in (("mode 5", dict(mode=5)), ("mode -1", dict(mode=-1))):
        refused(G, "hwg_loss_fwd " + what, lambda: fwd(G.ws, G.need, **over))
    assert bwd() == 0 and fwd(G.ws, G.need) == 0          # (and the same buffers do serve an accepted call)
    Gc, lp, tg, cfwd, cbwd = _ctc_guarded(cuda, AC.CTC_CASES[0])
    for entry in ("hwg_ctc_bwd", "hwg_ctc_bwd_grad"):
        for over in (dict(T=0), dict(B=0), dict(C=0), dict(Lmax=0), dict(T=-1)):
            refused(Gc, "%s %r" % (entry, over), lambda: cbwd(entry)(Gc.ws, Gc.need, **over))
    for over in (dict(T=0), dict(B=0), dict(C=0), dict(Lmax=0)):
        refused(Gc, "hwg_ctc_fwd %r" % over, lambda: cfwd("hwg_ctc_fwd")(Gc.ws, Gc.need, **over))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", AC.MASKED_L1_CASES, ids=lambda c: "%dx%d_w%d" % c)
def test_masked_l1_entries_on_guarded_buffers_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    L = _lib()
    rows, W, Wm = case
    g = SC.gen("abi_masked_l1_%dx%d_%d" % case)
    shape = (1, 1, rows, W)
    r, x = torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1
    x[:, :, ::3, ::2] = r[:, :, ::3, ::2]                                                       # ties r == x
    u = torch.rand((1, 1, rows, Wm), generator=g)
    m = torch.where(u < 0.25, torch.zeros(()), torch.where(u > 0.75, torch.ones(()), (u - 0.25) * 2))
    need = int(L.query("hwg_loss_workspace"))
    G = Guarded(cuda, dict(r=r, x=x, m=m), dict(out=((1,), F32)), need)
    f = G.f
    out = protocol(G, "hwg_masked_l1_fwd %dx%d w%d" % case, lambda ws, n: L.query("hwg_masked_l1_fwd", f["r"], f["x"], f["m"], rows, W, Wm, f["out"], ws, n, G.st))["out"]
    G2 = Guarded(cuda, dict(r=r, x=x, m=m, gout=torch.tensor([GOUT])), dict(dr=(shape, F32)))
    h = G2.f
    dr = protocol(G2, "hwg_masked_l1_bwd %dx%d w%d" % case, lambda ws, n: L.query("hwg_masked_l1_bwd", h["r"], h["x"], h["m"], rows, W, Wm, h["gout"], h["dr"], G2.st))["dr"]
    want_v, want_g = FG.masked_l1(r.numpy(), x.numpy(), m.numpy(), np.float64, gout=GOUT)
    bad = report("hwg_masked_l1_fwd", "rows%d W%d Wm%d" % case, need, [("loss", out, torch.tensor([float(want_v)], dtype=torch.float64), DERIVED["loss_value"])])
    bad += report("hwg_masked_l1_bwd", "rows%d W%d Wm%d" % case, 0, [("dr", dr, torch.from_numpy(want_g), DERIVED["loss_grad_const"])])
    mp = torch.from_numpy(FG.pad_mask(m.numpy(), W))
    assert not dr[mp == 0].any() and not dr[r == x].any(), "d recon where the mask is 0, behind its width, or at a tie"
    rg = r.to(cuda).requires_grad_(True)
    lo = ops.masked_l1_loss(rg, x.to(cuda), m.to(cuda))
    (lo * GOUT).backward()
    torch.cuda.synchronize()
    differ = bits_differ([("loss", out, lo.detach().reshape(1)), ("dr", dr, rg.grad)])
    assert not differ, "masked_l1 %dx%d w%d: %s differ from the bits of ops.masked_l1_loss" % (case + (differ,))
    assert not bad, "masked_l1 %dx%d w%d vs fp64: %s" % (case + ("; ".join(bad),))


# ---- spectral norm -------------------------------------------------------------------------------------------------------------------------------------
def _update(dev, w, u, v, R_, K, variant):
    """one power iteration under the protocol. variant: "both" / "no_u_copy" / "no_v_copy" / "no_copies" (hwg_spectral_update_to) or "plain"
    (hwg_spectral_update) -> (Guarded, outputs)"""
    L = _lib()
    need = int(L.query("hwg_spectral_workspace", R_, K))
    assert need == AC.spectral_workspace_bytes(R_, K)
    G = Guarded(dev, dict(W=w), dict(u=u, v=v, u_copy=((R_,), F32), v_copy=((K,), F32), sigma=((1,), F32), inv_sigma=((1,), F32)), need)
    f = G.f
    eps = SC.SN_EPS
    uc = f["u_copy"] if variant in ("both", "no_v_copy") else None
    vc = f["v_copy"] if variant in ("both", "no_u_copy") else None
    if variant == "plain":
        call = lambda ws, n: L.query("hwg_spectral_update", f["W"], f["u"], f["v"], R_, K, eps, f["sigma"], f["inv_sigma"], ws, n, G.st)        # noqa: E731
    else:
        call = lambda ws, n: L.query("hwg_spectral_update_to", f["W"], f["u"], f["v"], uc, vc, R_, K, eps, f["sigma"], f["inv_sigma"], ws, n, G.st)        # noqa: E731
    mine = ["u", "v", "sigma", "inv_sigma"] + (["u_copy"] if uc is not None else []) + (["v_copy"] if vc is not None else [])
    return G, protocol(G, "spectral %dx%d %s" % (R_, K, variant), call, mine=mine)


def _sn_reference(w, u, v, gw):
    cpu_threads()
    w64 = _leaf(w)
    ref = R.spectral(w64, u.double(), v.double(), _f32(SC.SN_EPS))
    ref[3].backward(gw.double())
    return ref, w64.grad


@pytest.mark.parametrize("shape", AC.SN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_spectral_entries_on_guarded_buffers_vs_fp64(cuda, shape):
    from handwriting_line_generation_amd import ops
    L = _lib()
    R_, K = shape
    w, _, u, v, gw, _ = SC.sn_inputs("abi", R_, K)
    G, both = _update(cuda, w, u, v, R_, K, "both")
    for variant in ("no_u_copy", "no_v_copy", "no_copies", "plain"):
        _, o = _update(cuda, w, u, v, R_, K, variant)
        differ = bits_differ([(k, o[k], both[k]) for k in ("u", "v", "sigma", "inv_sigma")])
        assert not differ, "spectral %dx%d: the %s call differs from the call with both copies in %s" % (R_, K, variant, differ)
    assert not bits_differ([("u_copy", both["u_copy"], both["u"]), ("v_copy", both["v_copy"], both["v"])]), "the snapshot is not the vector"
    ref, dw = _sn_reference(w, u, v, gw)
    label = "R%d K%d" % shape
    bad = report("hwg_spectral_update(_to)", label, G.need,
                 [("u", both["u"], ref[0], BOUNDS["sn_uv"]), ("v", both["v"], ref[1], BOUNDS["sn_uv"]),
                  ("sigma", both["sigma"], ref[2].detach().reshape(1), BOUNDS["sn_sigma"]), ("1/sigma", both["inv_sigma"], 1.0 / ref[2].detach().reshape(1), BOUNDS["sn_sigma"])])
    Gs = Guarded(cuda, dict(W=w, s=both["inv_sigma"]), dict(out=((R_, K), F32)))
    s = Gs.f
    wsn = protocol(Gs, "hwg_scale_by_ptr %dx%d" % shape, lambda ws, n: L.query("hwg_scale_by_ptr", s["W"], s["s"], s["out"], R_ * K, Gs.st))["out"]
    bad += report("hwg_scale_by_ptr", label, 0, [("w_sn", wsn, ref[3].detach(), BOUNDS["sn_w"])])
    need = G.need
    off, parts = AC.spectral_partials(R_, K)
    assert off % 8 == 0 and off + 8 * parts <= need, "the double partials of hwg_spectral_bwd do not fit the queried workspace"
    pre = torch.randn(R_, K, generator=SC.gen("abi_sn_pre_%dx%d" % shape)) * float((gw.double() / ref[2].detach()).abs().max())      # of the terms' size
    size = [(gw.double() / ref[2].detach()).abs()] if shape == (1, 1) else []          # (1, 1): measured against |g / sigma| (+ |pre|), see the module docstring
    written = None
    for acc in (0, 1):
        Gb = Guarded(cuda, dict(dWsn=gw, Wbar=w, u=both["u"], v=both["v"], sigma=both["sigma"]), dict(dWbar=pre if acc else ((R_, K), F32)), need)
        b = Gb.f
        got = protocol(Gb, "hwg_spectral_bwd %dx%d acc %d" % (R_, K, acc), lambda ws, n: L.query(
            "hwg_spectral_bwd", b["dWsn"], b["Wbar"], b["u"], b["v"], b["sigma"], b["dWbar"], R_, K, acc, ws, n, Gb.st))["dWbar"]
        bad += report("hwg_spectral_bwd", label + " acc%d" % acc, need, [("dw_bar", got, dw + (pre.double() if acc else 0.0), BOUNDS["sn_grad"]) + tuple(s_ + acc * pre.double().abs() for s_ in size)])
        written = got if not acc else written
    ug, vg = u.to(cuda), v.to(cuda)
    wg = w.to(cuda).requires_grad_(True)
    wo = ops.spectral_normalize(wg, ug, vg)
    wo.backward(gw.to(cuda))
    torch.cuda.synchronize()
    differ = bits_differ([("u", both["u"], ug), ("v", both["v"], vg), ("w_sn", wsn, wo.detach()), ("dw_bar", written, wg.grad)])
    assert not differ, "spectral %dx%d: %s differ from the bits of ops.spectral_normalize" % (R_, K, differ)
    assert not bad, "spectral %dx%d vs fp64: %s" % (R_, K, "; ".join(bad))


def test_spectral_multi_entries_on_guarded_buffers(cuda):
    """hwg_spectral_update_multi (device table, scratch and snapshot buffers without a size) and hwg_spectral_bwd_multi (host table, sized
    workspace) over AC.SN_BANK"""
    L = _lib()
    shapes = AC.SN_BANK
    n = len(shapes)
    inp = [SC.sn_inputs("abi_bank_%d" % i, R_, K) for i, (R_, K) in enumerate(shapes)]
    spans, off = [], 0
    for R_, K in shapes:
        spans.append(off)
        off += (R_ + K + 3) // 4 * 4
    total = off
    ins = {"W%d" % i: inp[i][0] for i in range(n)}
    ins["table"] = torch.zeros(48 * n, dtype=torch.uint8)
    outs = {}
    for i in range(n):
        outs["u%d" % i], outs["v%d" % i] = inp[i][2], inp[i][3]
    outs.update(copies=((total,), F32), sig=((2 * n,), F32))
    G = Guarded(cuda, ins, outs, total * 4)          # the scratch buffer is the guarded workspace: poisoned, then zero-filled; it has no size to under-run
    f = G.f
    rec = np.zeros(n, dtype=np.dtype([("W", "<u8"), ("u", "<u8"), ("v", "<u8"), ("copy_off", "<i8"), ("ws_off", "<i8"), ("R", "<i4"), ("K", "<i4")]))
    for i, (R_, K) in enumerate(shapes):
        rec[i] = (f["W%d" % i].data_ptr(), f["u%d" % i].data_ptr(), f["v%d" % i].data_ptr(), spans[i], spans[i], R_, K)
    G.set_input("table", torch.from_numpy(rec.view(np.uint8).copy()))
    torch.cuda.synchronize()
    out = protocol(G, "hwg_spectral_update_multi", lambda ws, nb: L.query(
        "hwg_spectral_update_multi", f["table"], n, max(s[0] for s in shapes), max(s[1] for s in shapes), SC.SN_EPS, ws, f["copies"], f["sig"], G.st),
        partly=("copies",), sized=False)
    bad, sigmas = [], []
    for i, (R_, K) in enumerate(shapes):
        ref, _ = _sn_reference(inp[i][0], inp[i][2], inp[i][3], inp[i][4])
        un, vn = out["u%d" % i], out["v%d" % i]
        cu, cv = out["copies"][spans[i]:spans[i] + R_], out["copies"][spans[i] + R_:spans[i] + R_ + K]
        assert not bits_differ([("u", cu, un), ("v", cv, vn)]), "layer %d: the snapshot is not the persisted u, v" % i
        bad += report("hwg_spectral_update_multi", "layer %d R%d K%d" % (i, R_, K), total * 4,
                      [("u", un, ref[0], BOUNDS["sn_uv"]), ("v", vn, ref[1], BOUNDS["sn_uv"]),
                       ("sigma", out["sig"][2 * i:2 * i + 1], ref[2].detach().reshape(1), BOUNDS["sn_sigma"]),
                       ("1/sigma", out["sig"][2 * i + 1:2 * i + 2], 1.0 / ref[2].detach().reshape(1), BOUNDS["sn_sigma"])])
        sigmas.append(out["sig"][2 * i:2 * i + 1].clone())
    pad = out["copies"].clone()
    for i, (R_, K) in enumerate(shapes):
        pad[spans[i]:spans[i] + R_ + K] = NAN
    assert bool(torch.isnan(pad).all()), "hwg_spectral_update_multi wrote between the layers' snapshots"
    assert not bad, "hwg_spectral_update_multi vs fp64: %s" % "; ".join(bad)
    # backward: all layers in two launches, bit-identical to the single calls
    pres = [torch.randn(s, generator=SC.gen("abi_bank_pre_%d" % i)) for i, s in enumerate(shapes)]
    ins, outs = {}, {}
    for i in range(n):
        ins.update({"g%d" % i: inp[i][4], "W%d" % i: inp[i][0], "u%d" % i: out["u%d" % i], "v%d" % i: out["v%d" % i], "s%d" % i: sigmas[i]})
        outs["d%d" % i] = pres[i] if i % 2 else (shapes[i], F32)
    need = int(L.query("hwg_spectral_bwd_multi_workspace", n))
    assert need == n * 512 * 8
    Gm = Guarded(cuda, ins, outs, need)
    m = Gm.f
    host = np.zeros(n, dtype=np.dtype([("dWsn", "<u8"), ("Wbar", "<u8"), ("u", "<u8"), ("v", "<u8"), ("sigma", "<u8"), ("dst", "<u8"), ("R", "<i4"), ("K", "<i4"),
                                       ("acc", "<i4"), ("pad", "<i4")]))
    assert host.dtype.itemsize == 64
    for i, (R_, K) in enumerate(shapes):
        host[i] = tuple(m["%s%d" % (q, i)].data_ptr() for q in "gWuvsd") + (R_, K, i % 2, 0)
    multi = protocol(Gm, "hwg_spectral_bwd_multi", lambda ws, nb: L.query("hwg_spectral_bwd_multi", host.ctypes.data, n, ws, nb, Gm.st))
    for i, (R_, K) in enumerate(shapes):
        one_need = int(L.query("hwg_spectral_workspace", R_, K))
        G1 = Guarded(cuda, {q: ins["%s%d" % (q, i)] for q in "gWuvs"}, dict(d=outs["d%d" % i]), one_need)
        o = G1.f
        G1.ws_fill(NAN)
        assert L.query("hwg_spectral_bwd", o["g"], o["W"], o["u"], o["v"], o["s"], o["d"], R_, K, i % 2, G1.ws, one_need, G1.st) == 0
        torch.cuda.synchronize()
        assert same_bits(G1.get("d"), multi["d%d" % i]) and G1.intact(), "layer %d: hwg_spectral_bwd_multi differs from the single call" % i
    print("\nabi %-22s %-34s ws %-9d the bits of %d single calls" % ("hwg_spectral_bwd_multi", "%d layers" % n, need, n))


# ---- pixel norm ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.PIXEL_NORM_CASES, ids=lambda c: "%dx%d_%s" % c)
def test_pixel_norm_entries_on_guarded_buffers_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    L = _lib()
    rows, C, kind = case
    x, gy = SC.pixel_norm_inputs(case)
    eps = SC.PIXEL_NORM_EPS
    G = Guarded(cuda, dict(x=x), dict(y=((rows, C), F32)))
    f = G.f
    y = protocol(G, "hwg_pixelnorm_fwd %dx%d %s" % case, lambda ws, n: L.query("hwg_pixelnorm_fwd", f["x"], f["y"], rows, C, eps, G.st))["y"]
    G2 = Guarded(cuda, dict(dy=gy, x=x), dict(dx=((rows, C), F32)))
    h = G2.f
    dx = protocol(G2, "hwg_pixelnorm_bwd %dx%d %s" % case, lambda ws, n: L.query("hwg_pixelnorm_bwd", h["dy"], h["x"], h["dx"], rows, C, eps, G2.st))["dx"]
    x64 = _leaf(x)
    yr = R.pixel_norm(x64, _f32(eps))
    yr.backward(gy.double())
    label = "rows%d C%d %s" % case
    bad = report("hwg_pixelnorm_fwd", label, 0, [("y", y, yr.detach(), BOUNDS["pixelnorm_fwd"])])
    if C == 1:
        terms = gy.double() / torch.sqrt(x.double() ** 2 + _f32(eps))
        bad += report("hwg_pixelnorm_bwd", label, 0, [("dx", dx, x64.grad, BOUNDS["pixelnorm_grad_c1"], terms)])
    else:
        bad += report("hwg_pixelnorm_bwd", label, 0, [("dx", dx, x64.grad, BOUNDS["pixelnorm_grad"])])
    xg = x.to(cuda).requires_grad_(True)
    yo = ops.pixel_norm(xg)
    yo.backward(gy.to(cuda))
    torch.cuda.synchronize()
    differ = bits_differ([("y", y, yo.detach()), ("dx", dx, xg.grad)])
    assert not differ, "pixel_norm %dx%d %s: %s differ from the bits of ops.pixel_norm" % (case + (differ,))
    assert not bad, "pixel_norm %dx%d %s vs fp64: %s" % (case + ("; ".join(bad),))
