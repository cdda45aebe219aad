"""GPU: the normalisation / activation kernels (csrc/norm_act.hip; the tanh pass of csrc/spectral_loss.hip) against the fp64 CPU restatements
of oracle/norm_ref.py, at the training step's geometries and at every chunk, lane and statistics regime of the kernels (case tables and the
regimes they cover: oracle/norm_cases.py, checked on the CPU by tests/test_norm_act_ref_cpu.py). The library's default path only. The bounds (BOUNDS, shared with
tests/test_norm_abi_fp64_gpu.py) are those of tests/_norm_act_checks.py.

Every output - y, dx, dgamma, dbeta, d(noise weight), running_mean, running_var - is compared by its relative L2 error and by
max|err| / max|ref|; one line per case is printed. relu / leaky relu gates whose fp64 pre-activation lies within 1e-6 of its largest magnitude
take the kernel's own forward output in the fp64 backward (the kernel recomputes the gate in fp32 and may fall on the other side of 0); the
number of those gates that really differ from fp64's sign is asserted to be a handful."""
import pytest
import torch

from oracle import norm_cases as NC
from oracle import norm_ref as R
from _fp64 import _f32, _gen, cpu_threads
from _norm_act_checks import BOUNDS, EPS, MAX_FLIPS, MOMENTUM, _gate_hint, nhwc

pytestmark = pytest.mark.gpu

_REF = {}


def _errs(got, want):
    d = got.detach().cpu().double() - want
    return float(d.norm()) / max(float(want.norm()), 1e-300), float(d.abs().max()) / max(float(want.abs().max()), 1e-300)


def _check(label, outs, family, note=""):
    """outs: [(name, got (CPU or GPU, the reference's layout), want float64)]; prints one line, asserts the family's bounds"""
    rel_b, max_b = BOUNDS[family]
    parts, bad = [], []
    for name, got, want in outs:
        assert tuple(got.shape) == tuple(want.shape), (label, name, tuple(got.shape), tuple(want.shape))
        assert bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (label, name)
        rel, mx = _errs(got, want)
        parts.append("%s %.2e/%.2e" % (name, rel, mx))
        if not (rel <= rel_b and mx <= max_b):
            bad.append("%s: rel L2 %.3e (bound %.1e), max/max %.3e (bound %.1e)" % (name, rel, rel_b, mx, max_b))
    print("\n%-34s [%s] rel L2 / max-max vs fp64: %s%s" % (label, family, "  ".join(parts), note))
    assert not bad, "%s vs fp64: %s" % (label, "; ".join(bad))


def _gates(ref):
    return "  (gates from the kernel: %d, differing: %d)" % (ref["near"], ref["flips"]) if ref["near"] else ""


def _norm_inputs(case):
    name, mode, N, H, W, C, groups, act, slope, mask, inputs, path = case
    g = _gen(name)
    cpg = C // groups if mode == "gn" else 1
    if inputs == "offset16":
        # every statistic group: mean 16 sigma (either sign), sigma in [0.5, 2]
        ng = C // cpg
        sig = (torch.rand(ng, generator=g) * 1.5 + 0.5).repeat_interleave(cpg)
        sgn = torch.where(torch.rand(ng, generator=g) > 0.5, 1.0, -1.0).repeat_interleave(cpg)
        x = (torch.randn(N, C, H, W, generator=g) + 16 * sgn[:, None, None]) * sig[:, None, None]
    elif inputs == "eps-scale":
        x = torch.randn(N, C, H, W, generator=g) * 3e-3
    else:
        x = torch.randn(N, C, H, W, generator=g) * 2 + 0.5
        if inputs == "edges":
            x[:, :cpg] = 0.75                                                    # var 0: rstd = 1 / sqrt(eps)
            x[:, cpg: 2 * cpg] = torch.randn(N, cpg, H, W, generator=g) * 1e-3   # var 1e-6 < eps
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    m = ((torch.rand(N, C, generator=g) > 0.3).float() / 0.7) if mask else None
    gy = torch.randn(N, C, H, W, generator=g)
    rm0 = torch.randn(C, generator=g) * 0.3 + 0.2
    rv0 = torch.rand(C, generator=g) + 0.5
    return x, gamma, beta, m, gy, rm0, rv0


def _bn_warmup_input(x):
    """the input of the first of the two BatchNorm calls whose running-statistics updates are checked"""
    return x * 0.5 + 1.0


def _norm_reference(case, x, gamma, beta, mask, gy, rm0, rv0, y_kernel):
    """fp64 outputs of one case, computed once and shared by every run of it (the kernels are deterministic: same forward bits, same gates)"""
    name, mode, N, H, W, C, groups, act, slope, use_mask, inputs, path = case
    if name in _REF:
        return _REF[name]
    cpu_threads()
    affine = path is not None
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True) if affine else None
    b64 = beta.double().requires_grad_(True) if affine else None
    z = R.norm_pre(x64, mode, groups, g64, b64, mask.double() if mask is not None else None, _f32(EPS))
    hint, near, flips = _gate_hint(z, y_kernel, act)
    y = R.act_ref(z, act, _f32(slope), hint)
    y.backward(gy.double())
    ref = {"y": y.detach(), "dx": x64.grad, "near": near, "flips": flips}
    del y, z
    if affine:
        ref["dgamma"], ref["dbeta"] = g64.grad, b64.grad
    if mode == "bn":
        with torch.no_grad():
            rm1, rv1 = R.running_stats(_bn_warmup_input(x).double(), rm0.double(), rv0.double(), _f32(MOMENTUM))
            ref["running_mean"], ref["running_var"] = R.running_stats(x.double(), rm1, rv1, _f32(MOMENTUM))
    _REF[name] = ref
    return ref


@pytest.mark.parametrize("case", NC.NORM_CASES, ids=[c[0] for c in NC.NORM_CASES])
def test_normalisation_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, mode, N, H, W, C, groups, act, slope, use_mask, inputs, path = case
    x, gamma, beta, mask, gy, rm0, rv0 = _norm_inputs(case)
    xg = nhwc(x).to(cuda).requires_grad_(True)
    mg = mask.to(cuda) if mask is not None else None
    gl = gamma.to(cuda).requires_grad_(True)
    bl = beta.to(cuda).requires_grad_(True)
    gk, bk = (gl, bl) if path == "leaf" else (gl * 1, bl * 1)       # non-leaf: the kernels write a fresh buffer (accumulate = 0)
    rmg, rvg = rm0.to(cuda), rv0.to(cuda)
    if mode == "gn":
        y = ops.group_norm(xg, groups, gk, bk, EPS, mask=mg, act=act, slope=slope)
    elif mode == "bn":
        with torch.no_grad():
            ops.batch_norm_train(nhwc(_bn_warmup_input(x)).to(cuda), gk, bk, rmg, rvg, MOMENTUM, EPS, act=act, slope=slope)
        y = ops.batch_norm_train(xg, gk, bk, rmg, rvg, MOMENTUM, EPS, act=act, slope=slope)
    else:
        assert path is None and act == R.ACT_NONE and mask is None
        y = ops.instance_norm(xg, EPS)
    y_kernel = R.to_nchw(y)
    ref = _norm_reference(case, x, gamma, beta, mask, gy, rm0, rv0, y_kernel)
    pre = {}
    if path == "leaf":          # pre-filled gradients, of the gradients' own magnitude: the kernels must add to them
        g = _gen(name + "/grad")
        pre["dgamma"] = torch.randn(C, generator=g) * float(ref["dgamma"].abs().max())
        pre["dbeta"] = torch.randn(C, generator=g) * float(ref["dbeta"].abs().max())
        gl.grad = pre["dgamma"].to(cuda)
        bl.grad = pre["dbeta"].to(cuda)
    y.backward(nhwc(gy).to(cuda))
    torch.cuda.synchronize()
    assert ref["flips"] <= MAX_FLIPS, "%s: %d gates differ from fp64's (more than a handful)" % (name, ref["flips"])
    offset = inputs == "offset16"
    _check(name + " fwd", [("y", y_kernel, ref["y"])], "offset16" if offset else "norm_fwd", _gates(ref))
    outs = [("dx", R.to_nchw(xg.grad), ref["dx"])]
    if path is not None:
        outs += [("dgamma", gl.grad, ref["dgamma"] + pre.get("dgamma", 0)), ("dbeta", bl.grad, ref["dbeta"] + pre.get("dbeta", 0))]
    _check(name + " grad", outs, "offset16" if offset else "norm_grad")
    if mode == "bn":
        _check(name + " running", [("running_mean", rmg, ref["running_mean"]), ("running_var", rvg, ref["running_var"])], "norm_stats")


def _adain_inputs(case):
    name, N, H, W, C, noise = case
    g = _gen(name)
    x = torch.randn(N, C, H, W, generator=g)
    nz = torch.randn(N, C, H, W, generator=g) if noise == "tensor" else None
    nw = torch.randn(1, C, 1, 1, generator=g) * 0.5
    gamma = torch.randn(N, C, generator=g) + 1
    beta = torch.randn(N, C, generator=g)
    gy = torch.randn(N, C, H, W, generator=g)
    pre = torch.randn(1, C, 1, 1, generator=g)
    return x, nz, nw, gamma, beta, gy, pre


ADAIN_RUNS = [(c, d) for c in NC.ADAIN_CASES for d in ((False, True) if c[5] == "tensor" else (None,))]


@pytest.mark.parametrize("case,defer", ADAIN_RUNS, ids=["%s%s" % (c[0], "" if d is None else "_defer%d" % d) for c, d in ADAIN_RUNS])
def test_generator_epilogue_vs_fp64(cuda, case, defer):
    """noise -> leaky relu -> AdaIN: noise from a tensor, forward and backward with the deferred noise-weight reduction off and on (then
    summed by ops.join_side_stream), and forward-only with the noise drawn inside the kernel (ops.VirtualNoise: the reference takes the values
    materialise() writes)"""
    from handwriting_line_generation_amd import ops
    name, N, H, W, C, noise = case
    x, nz, nw, gamma, beta, gy, pre = _adain_inputs(case)
    scale = (2.0 / C) ** 0.5
    xg = nhwc(x).to(cuda)
    nwg, gg, bg = nw.to(cuda), gamma.to(cuda), beta.to(cuda)
    if noise == "virtual":
        vn = ops.VirtualNoise(1234 + C, 4 * N + 17, (N, H, W, C))
        with torch.no_grad():
            y = ops.adain_epilogue(xg, vn, nwg, gg, bg, scale, 0.2, EPS)
            nz = R.to_nchw(vn.materialise(cuda)).float()
        if name not in _REF:
            cpu_threads()
            _REF[name] = {"y": R.adain(x.double(), nz.double(), nw.double(), gamma.double(), beta.double(), _f32(scale), _f32(0.2), _f32(EPS))}
        _check(name + " fwd", [("y", R.to_nchw(y), _REF[name]["y"])], "adain_fwd")
        return
    xg.requires_grad_(True); nwg.requires_grad_(True); gg.requires_grad_(True); bg.requires_grad_(True)
    y = ops.adain_epilogue(xg, nhwc(nz).to(cuda), nwg, gg, bg, scale, 0.2, EPS)
    u_kernel = R.to_nchw(y.grad_fn.saved_tensors[0])       # the kernel's lrelu output: its backward gates on u > 0
    if name not in _REF:
        cpu_threads()
        x64, nw64, g64, b64 = (t.double().requires_grad_(True) for t in (x, nw, gamma, beta))
        t = R.adain_pre(x64, nz.double(), nw64, _f32(scale))
        hint, near, flips = _gate_hint(t, u_kernel, R.ACT_LRELU)
        u = R.act_ref(t, R.ACT_LRELU, _f32(0.2), hint)
        yr = R.norm_pre(u, "in", 1, g64, b64, None, _f32(EPS))
        yr.backward(gy.double())
        _REF[name] = {"y": yr.detach(), "dx": x64.grad, "dnw": nw64.grad, "dgamma": g64.grad, "dbeta": b64.grad, "near": near, "flips": flips}
        del yr, u, t
    ref = _REF[name]
    pre = pre * float(ref["dnw"].abs().max())
    nwg.grad = pre.to(cuda)          # a leaf noise weight: the kernels add to its gradient
    before = ops._defer["launches"]
    ops.DEFER_REDUCE = defer
    try:
        y.backward(nhwc(gy).to(cuda))
    finally:
        ops.DEFER_REDUCE = False
        ops.join_side_stream()
    torch.cuda.synchronize()
    assert (ops._defer["launches"] - before >= 1) == defer, "deferred reduction %s but %d flush launches" % (defer, ops._defer["launches"] - before)
    assert ref["flips"] <= MAX_FLIPS, "%s: %d gates differ from fp64's" % (name, ref["flips"])
    label = "%s defer=%d" % (name, defer)
    _check(label + " fwd", [("y", R.to_nchw(y), ref["y"])], "adain_fwd", _gates(ref))
    _check(label + " grad", [("dx", R.to_nchw(xg.grad), ref["dx"]), ("dgamma", gg.grad, ref["dgamma"]), ("dbeta", bg.grad, ref["dbeta"]),
                             ("dnoise_w", nwg.grad, ref["dnw"] + pre.double())], "adain_grad")


@pytest.mark.parametrize("case", NC.FROZEN_CASES, ids=[c[0] for c in NC.FROZEN_CASES])
def test_frozen_batchnorm_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import ops
    name, N, H, W, C, act, slope = case
    g = _gen(name)
    x = torch.randn(N, C, H, W, generator=g) * 2 + 0.5
    rm = torch.randn(C, generator=g) * 0.5
    rv = torch.rand(C, generator=g) * 3 + 0.01
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    with torch.no_grad():
        y = ops.norm_apply_frozen(nhwc(x).to(cuda), rm.to(cuda), rv.to(cuda), EPS, gamma.to(cuda), beta.to(cuda), act, slope)
    want = R.frozen_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), act, _f32(slope), _f32(EPS))
    _check(name, [("y", R.to_nchw(y), want)], "frozen")


@pytest.mark.parametrize("case", NC.BIAS_ACT_CASES, ids=[c[0] for c in NC.BIAS_ACT_CASES])
def test_bias_act_vs_fp64(cuda, case):
    """y = act(mask * (x + bias)): vector kernel with and without the index arithmetic, an odd float4 count, more than one grid sweep, the
    scalar kernel; 1/16 of the pre-activations are exactly 0 (relu'(0) = 0, lrelu'(0) = slope, as torch)"""
    from handwriting_line_generation_amd import ops
    name, N, H, W, C, use_bias, use_mask, act, slope = case
    g = _gen(name)
    x = torch.randn(N, C, H, W, generator=g) * 2
    b = torch.randn(C, generator=g) if use_bias else None
    mask = ((torch.rand(N, C, generator=g) > 0.3).float() / 0.7) if use_mask else None
    zero = torch.rand(N, C, H, W, generator=g) < 1 / 16
    x = torch.where(zero, -b[:, None, None] if b is not None else torch.zeros(()), x)
    gy = torch.randn(N, C, H, W, generator=g)
    pre = torch.randn(C, generator=g) if use_bias else None
    xg = nhwc(x).to(cuda).requires_grad_(True)
    bg = b.to(cuda).requires_grad_(True) if b is not None else None
    mg = mask.to(cuda) if mask is not None else None
    if not use_bias and not use_mask and act == R.ACT_RELU:
        y = ops.relu(xg)
    elif not use_bias and not use_mask and act == R.ACT_LRELU:
        y = ops.leaky_relu(xg, slope)
    else:
        y = ops.bias_act(xg, bg, mg, act, slope)
    y_kernel = R.to_nchw(y)
    x64 = x.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if b is not None else None
    z = R.bias_act(x64, b64, mask.double() if mask is not None else None, R.ACT_NONE)
    hint, near, flips = _gate_hint(z, y_kernel, act)
    yr = R.act_ref(z, act, _f32(slope), hint)
    yr.backward(gy.double())
    if bg is not None:
        pre = pre * float(b64.grad.abs().max())
        bg.grad = pre.to(cuda)
    y.backward(nhwc(gy).to(cuda))
    torch.cuda.synchronize()
    assert flips <= MAX_FLIPS, (name, flips)
    _check(name + " fwd", [("y", y_kernel, yr.detach())], "bias_act_fwd", _gates({"near": near, "flips": flips}))
    outs = [("dx", R.to_nchw(xg.grad), x64.grad)]
    if bg is not None:
        outs.append(("dbias", bg.grad, b64.grad + pre.double()))
    _check(name + " grad", outs, "bias_act_grad")


@pytest.mark.parametrize("shape", NC.TANH_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_tanh_vs_fp64(cuda, shape):
    from handwriting_line_generation_amd import ops
    g = _gen("tanh%s" % (shape,))
    x = torch.randn(*shape, generator=g) * 2
    gy = torch.randn(*shape, generator=g)
    xg = x.to(cuda).requires_grad_(True)
    y = ops.tanh(xg)
    y.backward(gy.to(cuda))
    x64 = x.double().requires_grad_(True)
    yr = torch.tanh(x64)
    yr.backward(gy.double())
    _check("tanh %s fwd" % (shape,), [("y", y, yr.detach())], "tanh_fwd")
    _check("tanh %s grad" % (shape,), [("dx", xg.grad, x64.grad)], "tanh_grad")
