"""GPU: the sequence, loss and spectral-norm kernels (csrc/seq_ops.hip, csrc/spectral_loss.hip) against the fp64 CPU restatements of
oracle/seq_ref.py, at the training step's shapes and at every loop-trip, length and shape regime of the kernels (case tables and the regimes
they cover: oracle/seq_cases.py; the restatements, the tables and their sensitivity to seeded flaws are checked on the CPU by
tests/test_seq_loss_ref_cpu.py). The bounds (BOUNDS / DERIVED, shared with tests/test_seq_loss_abi_fp64_gpu.py) are those of
tests/_seq_loss_checks.py. The library's default path only.

Every floating-point output is compared by its relative L2 error and by max|err| / max|ref|; one line per case is printed. Integer outputs
(argmax, the DTW alignment and its run-length counts) and the zeros the kernels promise (the CTC gradient behind an input length, loss and
gradient of an infeasible CTC batch, the gradient at an exact tie of L1 / hinge, pixel norm of a zero row) are compared with torch.equal.
The CTC lines also carry the error of torch's own fp32 CPU ctc_loss on the same inputs: the yardstick for what fp32 log-space arithmetic
costs at that shape, never the bound."""
import pytest
import torch
import torch.nn.functional as F

from oracle import seq_cases as SC
from oracle import seq_ref as R
from _fp64 import YARDSTICK_FACTOR, _f32, cpu_threads
from _seq_loss_checks import BOUNDS, DERIVED, ULP, _leaf

pytestmark = pytest.mark.gpu


def _errs(got, want):
    d = got.detach().cpu().double() - want
    return float(d.norm()) / max(float(want.norm()), 1e-300), float(d.abs().max()) / max(float(want.abs().max()), 1e-300)


def _check(label, outs, family, note=""):
    """outs: [(name, got (CPU or GPU), want float64[, the float64 tensor whose size the error is measured against instead of want's])];
    prints one line, asserts the family's bounds"""
    rel_b, max_b = DERIVED[family] if family in DERIVED else BOUNDS[family]
    parts, bad = [], []
    for name, got, want, *scale in outs:
        assert tuple(got.shape) == tuple(want.shape), (label, name, tuple(got.shape), tuple(want.shape))
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (label, name)
        rel, mx = _errs(got, want)
        if scale:
            rel, mx = rel * float(want.norm()) / float(scale[0].norm()), mx * float(want.abs().max()) / float(scale[0].abs().max())
        parts.append("%s %.2e/%.2e" % (name, rel, mx))
        if not (rel <= rel_b and mx <= max_b):
            bad.append("%s: rel L2 %.3e (bound %.1e), max/max %.3e (bound %.1e)" % (name, rel, rel_b, mx, max_b))
    print("\n%-34s [%s] rel L2 / max-max vs fp64: %s%s" % (label, family, "  ".join(parts), note))
    assert not bad, "%s vs fp64: %s" % (label, "; ".join(bad))


def _zeros_like(t):
    return torch.zeros(t.shape, dtype=t.dtype)


@pytest.mark.parametrize("case", SC.LOG_SOFTMAX_CASES, ids=[c[0] for c in SC.LOG_SOFTMAX_CASES])
def test_log_softmax_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, B, T, C, kind = case
    g = SC.gen("lsm_" + name)
    x = SC.logits(kind, B, T, C, g)
    gy = torch.randn(T, B, C, generator=g)
    xg = x.to(cuda).requires_grad_(True)
    y = ops.log_softmax_tbc(xg)
    y.backward(gy.to(cuda))
    cpu_threads()
    x64 = _leaf(x)
    yr = R.log_softmax_tbc(x64)
    yr.backward(gy.double())
    _check("log_softmax " + name + " fwd", [("y", y, yr.detach())], "lsm_fwd")
    _check("log_softmax " + name + " grad", [("dx", xg.grad, x64.grad)], "lsm_grad")


def _ctc_reference(case):
    """fp64: loss, d (0.5 loss) / d log-probs as the kernels report it, d (0.5 loss) / d logits; and what torch's fp32 CPU ctc_loss makes of
    the same logits (None for the infeasible case, where torch's gradient is NaN)"""
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = case
    cpu_threads()
    x, tg = SC.ctc_inputs(case)
    x64 = _leaf(x)
    lp = R.log_softmax_tbc(x64)
    lp.retain_grad()
    loss, nll = R.ctc(lp, tg, in_len, tg_len)
    (loss * 0.5).backward()
    ref = dict(x=x, tg=tg, loss=loss.detach(), nll=nll, dlp=R.ctc_grad_on_simplex(lp, lp.grad), dx=x64.grad, torch32=None)
    if family is not None:
        x32 = x.clone().requires_grad_(True)
        l32 = F.ctc_loss(F.log_softmax(x32[:, 0], dim=2).permute(1, 0, 2), tg, torch.tensor(in_len), torch.tensor(tg_len))
        (l32 * 0.5).backward()
        ref["torch32"] = (_errs(l32, ref["loss"])[0], _errs(x32.grad, ref["dx"])[0])
    return ref


@pytest.mark.parametrize("case", SC.CTC_CASES, ids=[c[0] for c in SC.CTC_CASES])
def test_ctc_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = case
    ref = _ctc_reference(case)
    xg = ref["x"].to(cuda).requires_grad_(True)
    lpg = ops.log_softmax_tbc(xg)
    lpg.retain_grad()
    loss = ops.ctc_loss(lpg, ref["tg"], torch.tensor(in_len), torch.tensor(tg_len))
    (loss * 0.5).backward()
    torch.cuda.synchronize()
    got_loss, dlp, dx = loss.detach().cpu(), lpg.grad.cpu(), xg.grad.cpu()
    for nm, t in (("log-probs", lpg.detach().cpu()), ("loss", got_loss), ("d log-probs", dlp), ("d logits", dx)):
        assert bool(torch.isfinite(t).all()), "ctc %s: non-finite %s" % (name, nm)
    for b in range(B):          # behind an item's input length nothing flows back: exact zeros
        assert torch.equal(dlp[in_len[b]:, b], torch.zeros(T - in_len[b], C)), "ctc %s: d log-probs behind in_len of item %d" % (name, b)
        assert torch.equal(dx[b, 0, in_len[b]:], torch.zeros(T - in_len[b], C)), "ctc %s: d logits behind in_len of item %d" % (name, b)
    if family is None:          # one item without an alignment: loss 0, every gradient 0 - of the feasible items too
        assert int(torch.isinf(ref["nll"]).sum()) == 1 and float(ref["loss"]) == 0.0
        assert torch.equal(got_loss, torch.zeros(())), "ctc %s: loss %r" % (name, float(got_loss))
        assert torch.equal(dlp, _zeros_like(dlp)) and torch.equal(dx, _zeros_like(dx)), "ctc %s: gradient of an infeasible batch" % name
        print("\n%-34s loss 0, gradients 0: exact" % ("ctc " + name))
        return
    y_loss, y_dx = ref["torch32"]
    note = "  (torch fp32 cpu: loss %.2e, dlogits %.2e)" % (y_loss, y_dx)
    _check("ctc " + name + " loss", [("loss", got_loss, ref["loss"])], family + "_loss", note)
    _check("ctc " + name + " grad", [("dlogp", dlp, ref["dlp"]), ("dlogits", dx, ref["dx"])], family + "_grad", note)
    rel_dx = _errs(dx, ref["dx"])[0]
    assert rel_dx <= YARDSTICK_FACTOR * max(y_dx, ULP), "ctc %s: d logits %.2e, %.0f x torch's fp32 %.2e" % (name, rel_dx, rel_dx / y_dx, y_dx)


@pytest.mark.parametrize("case", SC.LOSS_CASES, ids=[c[0] for c in SC.LOSS_CASES])
def test_losses_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, mode, n, scale, wrt, inputs = case
    a, b = SC.loss_inputs(case)
    need_a, need_b = wrt in ("a", "both"), mode < 2 and wrt in ("b", "both")
    ag = a.to(cuda).requires_grad_(need_a)
    bg = b.to(cuda).requires_grad_(need_b) if b is not None else None
    if mode >= 2:
        lg = ops.mean_loss(ag, mode, scale)
    elif scale == 1.0:
        lg = (ops.l1_loss if mode == ops.LOSS_L1 else ops.mse_loss)(ag, bg)
    else:
        lg = ops._Loss.apply(ag, bg, mode, scale)          # the pair losses' public wrappers fix scale = 1
    (lg * SC.LOSS_GOUT).backward()
    a64 = a.double().requires_grad_(need_a)
    b64 = b.double().requires_grad_(need_b) if b is not None else None
    lr = R.loss(a64, b64, mode, _f32(scale))
    (lr * SC.LOSS_GOUT).backward()
    _check("loss " + name + " value", [("loss", lg.detach(), lr.detach())], "loss_value_mse" if mode == 1 else "loss_value")
    outs = ([("da", ag.grad, a64.grad)] if need_a else []) + ([("db", bg.grad, b64.grad)] if need_b else [])
    _check("loss " + name + " grad", outs, "mse_grad" if mode == 1 else "loss_grad_const", "  (scale %+d, wrt %s)" % (scale, wrt))
    if inputs == "ties":
        for nm, t, _ in outs:
            assert torch.equal(t[::2].cpu(), torch.zeros(-(-n // 2))), "loss %s: %s at the ties" % (name, nm)


def _sn_checks(label, got, ref, grad_got, grad_want):
    """got: (u, v, sigma, w_sn) of the kernels; ref: R.spectral's tuple"""
    _check(label + " u v", [("u", got[0], ref[0]), ("v", got[1], ref[1])], "sn_uv")
    _check(label + " sigma", [("sigma", got[2].reshape(()), ref[2].detach())], "sn_sigma")
    _check(label + " w", [("w_sn", got[3], ref[3].detach())], "sn_w")
    _check(label + " grad", [("dw_bar", grad_got, grad_want)], "sn_grad")


def _sn_reference(inputs, eps):
    """two successive fp64 iterations (the second on the moved weight, from the first's u', v') -> [(R.spectral's tuple, d / d w_bar)]"""
    w1, w2, u, v, g1, g2 = inputs
    cpu_threads()
    out, u64, v64 = [], u.double(), v.double()
    for w, gw in ((w1, g1), (w2, g2)):
        w64 = _leaf(w)
        ref = R.spectral(w64, u64, v64, eps)
        ref[3].backward(gw.double())
        out.append((ref, w64.grad))
        u64, v64 = ref[0], ref[1]
    return out


@pytest.mark.parametrize("shape", SC.SN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_spectral_norm_vs_fp64(cuda, shape):
    """ops.spectral_normalize twice on persisted u, v: first on a plain tensor (the gradient is returned to autograd), then on a parameter
    whose .grad is pre-filled (the kernel adds to it)"""
    from handwriting_line_generation_amd import ops
    R_, K = shape
    inputs = SC.sn_inputs("single", R_, K)
    w1, w2, u, v, g1, g2 = inputs
    (ref1, dw1), (ref2, dw2) = _sn_reference(inputs, _f32(SC.SN_EPS))
    ug, vg = u.to(cuda), v.to(cuda)
    wg = w1.to(cuda).requires_grad_(True)
    wsn = ops.spectral_normalize(wg, ug, vg)
    sigma = wsn.grad_fn.saved_tensors[3].clone()
    u1, v1 = ug.clone(), vg.clone()
    wsn.backward(g1.to(cuda))
    _sn_checks("spectral %dx%d it1 tensor" % shape, (u1, v1, sigma, wsn), ref1, wg.grad, dw1)
    pre = torch.randn(R_, K, generator=SC.gen("sn_pre_%dx%d" % shape)) * float(dw2.abs().max())
    p = torch.nn.Parameter(w2.to(cuda))
    p.grad = pre.to(cuda)
    wsn = ops.spectral_normalize(p, ug, vg)
    sigma = wsn.grad_fn.saved_tensors[3].clone()
    wsn.backward(g2.to(cuda))
    _sn_checks("spectral %dx%d it2 param" % shape, (ug, vg, sigma, wsn), ref2, p.grad, dw2 + pre.double())


@pytest.mark.parametrize("bank", SC.SN_BANKS, ids=[b[0] for b in SC.SN_BANKS])
def test_spectral_bank_vs_fp64(cuda, bank):
    """the same through ops.SpectralBank (all layers' power iterations in four launches) and the deferred backward pass (all layers in two
    launches at the join, adding to the pre-filled parameter gradients), two iterations"""
    from handwriting_line_generation_amd import ops
    bname, shapes = bank
    eps = _f32(SC.SN_EPS)
    inputs = [SC.sn_inputs("bank_%s_%d" % (bname, i), R_, K) for i, (R_, K) in enumerate(shapes)]
    refs = [_sn_reference(inp, eps) for inp in inputs]
    params = [torch.nn.Parameter(inp[0].to(cuda)) for inp in inputs]
    us, vs = [inp[2].to(cuda) for inp in inputs], [inp[3].to(cuda) for inp in inputs]
    sb = ops.SpectralBank(list(zip(params, us, vs)))
    for it in (0, 1):
        pres = []
        for i, p in enumerate(params):
            if it:
                p.data.copy_(inputs[i][1].to(cuda))
            dw = refs[i][it][1]
            pres.append(torch.randn(dw.shape, generator=SC.gen("sn_pre_%s_%d_%d" % (bname, i, it))) * float(dw.abs().max()))
            p.grad = pres[i].to(cuda)
        assert sb.valid()
        fresh = sb.update()
        ws = [ops.spectral_scale(p, f) for p, f in zip(params, fresh)]
        before = ops._defer["sn_launches"]
        ops.DEFER_REDUCE = True
        try:
            for i, w in enumerate(ws):
                w.backward(inputs[i][4 + it].to(cuda))
        finally:
            ops.DEFER_REDUCE = False
            ops.join_side_stream()
        torch.cuda.synchronize()
        assert ops._defer["sn_launches"] - before == 1, "deferred spectral backward: %d launches" % (ops._defer["sn_launches"] - before)
        for i, (R_, K) in enumerate(shapes):
            ref, dw = refs[i][it]
            label = "bank %s[%d] %dx%d it%d" % (bname, i, R_, K, it + 1)
            un, vn, sigma, inv_sigma, _ = fresh[i]
            assert torch.equal(un, us[i]) and torch.equal(vn, vs[i]), label + ": the snapshot is not the persisted u, v"
            _sn_checks(label, (us[i], vs[i], sigma, ws[i]), ref, params[i].grad, dw + pres[i].double())
            _check(label + " 1/sigma", [("inv_sigma", inv_sigma.reshape(()), 1.0 / ref[2].detach())], "sn_sigma")


@pytest.mark.parametrize("case", SC.PIXEL_NORM_CASES, ids=lambda c: "%dx%d_%s" % c)
def test_pixel_norm_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    rows, C, kind = case
    x, gy = SC.pixel_norm_inputs(case)
    xg = x.to(cuda).requires_grad_(True)
    y = ops.pixel_norm(xg)
    y.backward(gy.to(cuda))
    x64 = _leaf(x)
    yr = R.pixel_norm(x64, _f32(SC.PIXEL_NORM_EPS))
    yr.backward(gy.double())
    label = "pixel_norm %dx%d %s" % case
    _check(label + " fwd", [("y", y, yr.detach())], "pixelnorm_fwd")
    if C == 1:
        terms = gy.double() / torch.sqrt(x.double() ** 2 + _f32(SC.PIXEL_NORM_EPS))
        _check(label + " grad", [("dx", xg.grad, x64.grad, terms)], "pixelnorm_grad_c1", "  (against the size of dy / d)")
    else:
        _check(label + " grad", [("dx", xg.grad, x64.grad)], "pixelnorm_grad")
    if kind == "zero_row":
        assert torch.equal(y[0].detach().cpu(), torch.zeros(C)), label + ": a zero row"


@pytest.mark.parametrize("shape", SC.ARGMAX_SHAPES, ids=lambda s: "%dx%d" % s)
def test_argmax_first_maximum_exact(cuda, shape):
    from handwriting_line_generation_amd import ops
    x, planted = SC.argmax_inputs(shape)
    got = ops.argmax_rows(x.to(cuda))
    assert got.dtype == torch.int32 and tuple(got.shape) == (shape[0],)
    want = R.argmax_first(x)
    for kind, (r, c) in planted.items():
        assert int(got[r]) == c, "argmax %dx%d: %s tie in row %d: %d, first maximum at %d" % (shape + (kind, r, int(got[r]), c))
    assert torch.equal(got.cpu().long(), want), "argmax %dx%d: rows %s" % (shape + ((got.cpu().long() != want).nonzero().flatten().tolist()[:8],))
    print("\nargmax %dx%d: exact (%d rows with a tied maximum)" % (shape + (int(((x == x.max(1, keepdim=True).values).sum(1) > 1).sum()),)))


@pytest.mark.parametrize("case", SC.DTW_CASES, ids=lambda c: "T%d_B%d_L%d" % c)
def test_dtw_long_labels_exact(cuda, case):
    """more than 256 blank-interleaved label states: the kernel's j loop takes a second trip"""
    from handwriting_line_generation_amd import ops
    from oracle import seq_oracle
    T, B, Lr = case
    pred, label = SC.dtw_inputs(case)
    ref = seq_oracle.correct_pred(pred, label)
    got, lens = ops.dtw_align(pred.to(cuda), label.to(cuda))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref), "dtw T=%d B=%d L=%d" % case
    assert int(lens.max()) == ref.shape[0]
    gt_ref, pos_ref = seq_oracle.gt_counts(ref, label)
    gt, meta = ops.gt_counts(got, label.to(cuda))
    assert torch.equal(gt.cpu(), gt_ref) and int(meta[0].item()) == pos_ref and int(meta[1].item()) == 0
    print("\ndtw T=%d B=%d L=%d: path of %d steps and its run-length counts exact" % (case + (ref.shape[0],)))
