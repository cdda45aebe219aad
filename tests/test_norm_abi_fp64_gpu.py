"""GPU: the entries of csrc/norm_act.hip - hwg_norm_fwd / _bwd, hwg_norm_frozen_fwd, hwg_adain_fwd / _fwd_rng / _bwd, hwg_bias_act_fwd / _bwd -
and hwg_colsum, called at the C ABI through L.query (return codes visible, never through ops but for the bit comparisons named below) on
guarded buffers, against the fp64 restatements of oracle/norm_ref.py. Case tables and the regimes they cover: oracle/abi_cases.py, checked on
the CPU by tests/test_abi_cases_cpu.py. The buffers and the protocol are those of tests/_guarded.py; the bounds are the BOUNDS of
tests/_norm_act_checks.py, which tests/test_norm_act_fp64_gpu.py holds the same kernels to: the same arithmetic. The library's default tuning only.

The protocol, for every entry (Guarded and protocol() of tests/_guarded.py): every operand, every output and the workspace are carved out of ONE allocation with
64-float canaries before, between and after them. The workspace has exactly the bytes the entry's query returns (a multiple of 4). Before
the call every output and the workspace are filled with NaN (an output the entry adds to: with its pre-filled value). After the call: return
code 0, canaries intact, every input bit-identical, every output the call does not own unchanged, every documented output finite. A second
call with the workspace filled with ZERO bytes instead of NaN gives the same bits. A call with ws_bytes - 1, and one with ws = NULL, return
HWG_ERR_WORKSPACE and leave outputs and canaries alone. Entries without a workspace get the canary, input and repeatability parts.

Per entry, what is asserted beyond the protocol, and the worst |err| / bound measured on an MI355X (relative L2, max|err| / max|ref|, each
divided by its bound; every case prints its own line, kept in profiles/norm_seq_abi_fp64.txt):

  hwg_norm_fwd, hwg_norm_bwd    31 cases: six geometries x GN / IN / BN x mask off / on, every mode with each activation. y against        [y 0.28 / 0.25,
                                BOUNDS["norm_fwd"]; dx, dgamma, dbeta (written, or added to a pre-filled buffer) against                  dx 0.33 / 0.30, dgamma 0.73 / 0.68, dbeta 0.25 / 0.19,
                                BOUNDS["norm_grad"]; BatchNorm's running statistics after one update against BOUNDS["norm_stats"].         running statistics 0.32 / 0.19]
                                GN (and BN without a mask): y, dx, dgamma, dbeta, running statistics have the bits of ops.group_norm /
                                ops.batch_norm_train on the same inputs.
  affine_per_sample = 1         (no Python caller) IN and GN. Every sample's gamma / beta equal to a shared one: y and dx have the BITS     [sum_n 0.23 / 0.14,
                                of the shared-affine call, the fp64 sum over n of the [N][C] dgamma / dbeta meets BOUNDS["norm_grad"]     distinct y 0.23 / 0.10,
                                against the shared call's reference. Distinct per-sample affines: y, dx, dgamma [N][C], dbeta [N][C]      dx, dgamma, dbeta 0.19 / 0.18]
                                against fp64 under the same two bounds. BatchNorm: batch statistics span the samples and the
                                backward's finalize pass forms c1 / c2 / dgamma / dbeta per channel from gamma[c] - per-sample affine
                                is not defined there, hwg_norm_fwd and hwg_norm_bwd refuse it (HWG_ERR_ARG, nothing written).
  hwg_adain_fwd, _fwd_rng,      y against BOUNDS["adain_fwd"]; dx, dgamma, dbeta, d(noise weight) and dbias (both added to pre-filled      [y 0.25 / 0.17,
  hwg_adain_bwd (not deferred)  buffers) against BOUNDS["adain_grad"]. _fwd_rng gives the BITS of _fwd on the noise hwg_randn writes      gradients 0.22 / 0.14, dbias 0.78 / 0.49]
                                for the same seed and offset (the header's promise). y and dx have the bits of ops.adain_epilogue.
  hwg_norm_frozen_fwd           y against BOUNDS["frozen"], bits of ops.norm_apply_frozen                                                 [0.26 / 0.26]
  hwg_bias_act_fwd, _bwd        y, dx against BOUNDS["bias_act_fwd"] / ["bias_act_grad"], bits of ops.bias_act                            [y 0.27 / 0.25, dx 0.13 / 0.14]
  hwg_colsum                    derived, per element: a sum of `rows` fp32 terms in any order, one more rounded sum when added to a       [0.16]
                                pre-filled out: |err| <= (rows - 1 + accumulate) 2^-24 (sum |x| + |out0|) (1 + 2^-16); one row written,
                                not added: exact. Bits of ops.colsum.
  refusals                      C % 4 != 0 and C > 1024 (every norm entry), groups not dividing C (hwg_norm_fwd, hwg_norm_bwd), BN with
                                affine_per_sample: HWG_ERR_ARG before any launch, outputs still NaN, canaries intact."""
import pytest
import torch

from oracle import abi_cases as AC
from oracle import norm_ref as R
from _fp64 import SECOND, U, _f32, _gen, _ratio, cpu_threads, report
from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)
from _guarded import NAN, Guarded, bits_differ, protocol, refused, same_bits
from _norm_act_checks import BOUNDS, EPS, MAX_FLIPS, MOMENTUM, _gate_hint, nhwc, norm_inputs

pytestmark = pytest.mark.gpu


def nchw(t, N, HW, C):
    """a kernel tensor [N][HW][C] as NCHW float64 [N, C, 1, HW]"""
    return t.detach().cpu().double().reshape(N, 1, HW, C).permute(0, 3, 1, 2).contiguous()


# ---- normalisation ---------------------------------------------------------------------------------------------------------------------------


def norm_forward(dev, c, t, per_sample=0, tag=None, run=protocol):
    """hwg_norm_fwd under the protocol -> (Guarded, {y, mean, rstd[, running_mean, running_var]})"""
    N, HW, C = c["N"], c["HW"], c["C"]
    bn = c["mode"] == "bn"
    ins = dict(x=nhwc(t["x"]), gamma=t["gamma"], beta=t["beta"])
    if t["mask"] is not None:
        ins["mask"] = t["mask"]
    outs = dict(y=((N, HW, C), torch.float32), mean=((N, C), torch.float32), rstd=((N, C), torch.float32))
    if bn:
        outs.update(running_mean=t["rm0"], running_var=t["rv0"])
    from handwriting_line_generation_amd import _lib as L
    need = int(L.query("hwg_norm_workspace", N, HW, C))
    G = Guarded(dev, ins, outs, need)
    f = G.f

    def call(ws, n, **over):
        a = dict(C=C, groups=c["groups"], mode=AC.MODE_ID[c["mode"]], ps=per_sample)
        a.update(over)
        return L.query("hwg_norm_fwd", f["x"], f["y"], N, HW, a["C"], a["mode"], a["groups"], EPS, f["gamma"], f["beta"], a["ps"], f.get("mask"), c["act"],
                       c["slope"], f["mean"], f["rstd"], f["running_mean"] if bn else None, f["running_var"] if bn else None, MOMENTUM, ws, n, G.st)
    G.call = call
    return G, run(G, (tag or c["name"]) + " hwg_norm_fwd", call)


def norm_backward(dev, c, t, fwd, per_sample=0, accumulate=0, tag=None):
    """hwg_norm_bwd under the protocol, from the forward call's y, mean and rstd -> (Guarded, {dx, dgamma, dbeta})"""
    N, HW, C = c["N"], c["HW"], c["C"]
    ins = dict(dy=nhwc(t["gy"]), x=nhwc(t["x"]), y=fwd["y"], gamma=t["gamma"], beta=t["beta"], mean=fwd["mean"], rstd=fwd["rstd"])
    if t["mask"] is not None:
        ins["mask"] = t["mask"]
    ash = tuple(t["gamma"].shape)
    outs = dict(dx=((N, HW, C), torch.float32), dgamma=t["dgamma0"] if accumulate else (ash, torch.float32),
                dbeta=t["dbeta0"] if accumulate else (ash, torch.float32))
    from handwriting_line_generation_amd import _lib as L
    need = int(L.query("hwg_norm_workspace", N, HW, C))
    G = Guarded(dev, ins, outs, need)
    f = G.f

    def call(ws, n, **over):
        a = dict(C=C, groups=c["groups"], mode=AC.MODE_ID[c["mode"]], ps=per_sample)
        a.update(over)
        return L.query("hwg_norm_bwd", f["dy"], f["x"], f["y"], f["dx"], N, HW, a["C"], a["mode"], a["groups"], f["gamma"], f["beta"], a["ps"], f.get("mask"),
                       c["act"], c["slope"], f["mean"], f["rstd"], f["dgamma"], f["dbeta"], accumulate, ws, n, G.st)
    G.call = call
    return G, protocol(G, (tag or c["name"]) + " hwg_norm_bwd", call)


def norm_reference(c, t, y_kernel, per_sample=False):
    """fp64: y, dx, dgamma, dbeta (and the running statistics after one update), gates near 0 taken from the kernel's forward output"""
    cpu_threads()
    x64, g64, b64 = (t[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    m64 = t["mask"].double() if t["mask"] is not None else None
    z = R.norm_pre(x64, c["mode"], c["groups"], g64, b64, m64, _f32(EPS))
    hint, near, flips = _gate_hint(z, y_kernel, c["act"])
    if per_sample:
        y = R.norm_per_sample(x64, c["mode"], c["groups"], g64, b64, m64, c["act"], _f32(c["slope"]), _f32(EPS), hint)
    else:
        y = R.act_ref(z, c["act"], _f32(c["slope"]), hint)
    y.backward(t["gy"].double())
    ref = dict(y=y.detach(), dx=x64.grad, dgamma=g64.grad, dbeta=b64.grad, flips=flips)
    if c["mode"] == "bn":
        with torch.no_grad():
            ref["running_mean"], ref["running_var"] = R.running_stats(t["x"].double(), t["rm0"].double(), t["rv0"].double(), _f32(MOMENTUM))
    return ref


def _shape(c):
    return "%s N%d HW%d C%d g%d act%d%s" % (c["mode"], c["N"], c["HW"], c["C"], c["groups"], c["act"], " mask" if c["mask"] else "")


def _ops_norm(dev, c, t, accumulate):
    """the same case through ops.group_norm / ops.batch_norm_train -> {y, dx, dgamma, dbeta[, running_mean, running_var]} on the device"""
    from handwriting_line_generation_amd import ops
    xg = nhwc(t["x"]).to(dev).requires_grad_(True)
    gl, bl = t["gamma"].to(dev).requires_grad_(True), t["beta"].to(dev).requires_grad_(True)
    gk, bk = (gl, bl) if accumulate else (gl * 1, bl * 1)
    out = {}
    if c["mode"] == "gn":
        y = ops.group_norm(xg, c["groups"], gk, bk, EPS, mask=t["mask"].to(dev) if t["mask"] is not None else None, act=c["act"], slope=c["slope"])
    else:
        out["running_mean"], out["running_var"] = t["rm0"].to(dev), t["rv0"].to(dev)
        y = ops.batch_norm_train(xg, gk, bk, out["running_mean"], out["running_var"], MOMENTUM, EPS, act=c["act"], slope=c["slope"])
    if accumulate:
        gl.grad, bl.grad = t["dgamma0"].to(dev), t["dbeta0"].to(dev)
    y.backward(nhwc(t["gy"]).to(dev))
    torch.cuda.synchronize()
    out.update(y=y.detach(), dx=xg.grad, dgamma=gl.grad, dbeta=bl.grad)
    return out


@pytest.mark.parametrize("c", AC.NORM_CASES, ids=[c["name"] for c in AC.NORM_CASES])
def test_norm_entries_on_guarded_buffers_vs_fp64(cuda, c):
    N, HW, C = c["N"], c["HW"], c["C"]
    t = norm_inputs(c)
    Gf, fwd = norm_forward(cuda, c, t)
    assert Gf.need == AC.norm_workspace_bytes(N, HW, C)
    Gb, bwd = norm_backward(cuda, c, t, fwd, accumulate=c["accumulate"])
    ref = norm_reference(c, t, nchw(fwd["y"], N, HW, C))
    assert ref["flips"] <= MAX_FLIPS, "%s: %d gates differ from fp64's" % (c["name"], ref["flips"])
    pre = (lambda k: t[k + "0"].double()) if c["accumulate"] else (lambda k: 0.0)
    bad = report("hwg_norm_fwd", _shape(c), Gf.need, [("y", nchw(fwd["y"], N, HW, C), ref["y"], BOUNDS["norm_fwd"])])
    bad += report("hwg_norm_bwd", _shape(c) + " acc%d" % c["accumulate"], Gb.need,
                  [("dx", nchw(bwd["dx"], N, HW, C), ref["dx"], BOUNDS["norm_grad"]), ("dgamma", bwd["dgamma"], ref["dgamma"] + pre("dgamma"), BOUNDS["norm_grad"]),
                   ("dbeta", bwd["dbeta"], ref["dbeta"] + pre("dbeta"), BOUNDS["norm_grad"])])
    if c["mode"] == "bn":
        bad += report("hwg_norm_fwd running", _shape(c), Gf.need, [(k, fwd[k], ref[k], BOUNDS["norm_stats"]) for k in ("running_mean", "running_var")])
    if c["mode"] == "gn" or (c["mode"] == "bn" and not c["mask"]):
        o = _ops_norm(cuda, c, t, c["accumulate"])
        mine = dict(fwd, **bwd)
        differ = bits_differ([(k, mine[k], o[k]) for k in o])
        assert not differ, "%s: %s differ from the bits of the ops call" % (c["name"], differ)
    assert not bad, "%s vs fp64: %s" % (c["name"], "; ".join(bad))


@pytest.mark.parametrize("c", AC.PER_SAMPLE_CASES, ids=[c["name"] for c in AC.PER_SAMPLE_CASES])
def test_affine_per_sample_vs_the_shared_call_and_fp64(cuda, c):
    N, HW, C = c["N"], c["HW"], c["C"]
    # every sample's affine equal to a shared one: the bits of the shared call; the [N][C] parameter gradients sum to the shared call's
    t = norm_inputs(c)
    _, fs = norm_forward(cuda, c, t, tag=c["name"] + " shared")
    _, bs = norm_backward(cuda, c, t, fs, tag=c["name"] + " shared")
    te = dict(t, gamma=t["gamma"].expand(N, C).contiguous(), beta=t["beta"].expand(N, C).contiguous())
    Gf, fe = norm_forward(cuda, c, te, per_sample=1, tag=c["name"] + " equal")
    Gb, be = norm_backward(cuda, c, te, fe, per_sample=1, tag=c["name"] + " equal")
    differ = bits_differ([("y", fe["y"], fs["y"]), ("mean", fe["mean"], fs["mean"]), ("rstd", fe["rstd"], fs["rstd"]), ("dx", be["dx"], bs["dx"])])
    assert not differ, "%s: with equal per-sample affines %s differ from the shared-affine call" % (c["name"], differ)
    ref = norm_reference(c, t, nchw(fs["y"], N, HW, C))
    bad = report("hwg_norm_bwd ps=1 sum_n", _shape(c), Gb.need, [(k, be[k].double().sum(0), ref[k], BOUNDS["norm_grad"]) for k in ("dgamma", "dbeta")])
    # distinct per-sample affines against fp64, parameter gradients added to pre-filled [N][C] buffers
    td = norm_inputs(dict(c, name=c["name"] + "/distinct"), per_sample=True)
    Gf, fd = norm_forward(cuda, c, td, per_sample=1, tag=c["name"] + " distinct")
    Gb, bd = norm_backward(cuda, c, td, fd, per_sample=1, accumulate=1, tag=c["name"] + " distinct")
    ref = norm_reference(c, td, nchw(fd["y"], N, HW, C), per_sample=True)
    assert ref["flips"] <= MAX_FLIPS
    bad += report("hwg_norm_fwd ps=1", _shape(c), Gf.need, [("y", nchw(fd["y"], N, HW, C), ref["y"], BOUNDS["norm_fwd"])])
    bad += report("hwg_norm_bwd ps=1 acc1", _shape(c), Gb.need,
                  [("dx", nchw(bd["dx"], N, HW, C), ref["dx"], BOUNDS["norm_grad"]), ("dgamma", bd["dgamma"], ref["dgamma"] + td["dgamma0"].double(), BOUNDS["norm_grad"]),
                   ("dbeta", bd["dbeta"], ref["dbeta"] + td["dbeta0"].double(), BOUNDS["norm_grad"])])
    assert not bad, "%s vs fp64: %s" % (c["name"], "; ".join(bad))


def _plain(G, tag, call):
    """one accepted call outside the protocol -> {name: CPU tensor}"""
    G.reset()
    G.ws_fill(NAN)
    assert call(G.ws, G.need) == 0, tag
    torch.cuda.synchronize()
    return {k: G.get(k) for k in G.outs}


def test_norm_refusals_write_nothing(cuda):
    """what the host code turns down before any launch: C % 4 != 0, C > 1024, groups not dividing C, BatchNorm with a per-sample affine"""
    c = dict(name="refusals", mode="gn", N=2, HW=7, C=8, groups=2, act=AC.ACT_RELU, slope=0.0, mask=True)
    t = norm_inputs(c, per_sample=True)              # [N][C] affines: large enough for either reading
    Gf, fwd = norm_forward(cuda, c, t, per_sample=1, run=_plain)
    Gb, _ = norm_backward(cuda, c, t, fwd, per_sample=1)
    for name, G in (("hwg_norm_fwd", Gf), ("hwg_norm_bwd", Gb)):
        for what, over in (("C 6", dict(C=6)), ("C 1028", dict(C=1028)), ("C 0", dict(C=0)), ("groups 3", dict(groups=3)), ("groups 0", dict(groups=0)),
                           ("mode 3", dict(mode=3)), ("BatchNorm with affine_per_sample", dict(mode=2, ps=1))):
            refused(G, "%s %s" % (name, what), lambda: G.call(G.ws, G.need, **over))
        assert G.call(G.ws, G.need) == 0 and G.intact()          # (and the same buffers do serve an accepted call)
    torch.cuda.synchronize()


# ---- the generator epilogue ----------------------------------------------------------------------------------------------------------------------
def _adain_inputs(case):
    name, N, HW, C = case
    g = _gen(name)
    t = dict(x=torch.randn(N, C, 1, HW, generator=g), nw=torch.randn(C, generator=g) * 0.5, gamma=torch.randn(N, C, generator=g) + 1,
             beta=torch.randn(N, C, generator=g), gy=torch.randn(N, C, 1, HW, generator=g))
    t["dnw0"] = torch.randn(C, generator=g) * (N * HW) ** 0.5
    t["dbias0"] = torch.randn(C, generator=g) * (N * HW) ** 0.5
    return t


@pytest.mark.parametrize("case", AC.ADAIN_CASES, ids=[c[0] for c in AC.ADAIN_CASES])
def test_generator_epilogue_entries_on_guarded_buffers_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import _lib as L, ops
    name, N, HW, C = case
    t = _adain_inputs(case)
    scale, slope = (2.0 / C) ** 0.5, 0.2
    seed, offset = 1234 + C, 4 * N + 17
    noise = ops.VirtualNoise(seed, offset, (N, 1, HW, C)).materialise(cuda).cpu()          # what hwg_randn writes for (seed, offset)
    need = int(L.query("hwg_norm_workspace", N, HW, C))
    outs = dict(u=((N, HW, C), torch.float32), y=((N, HW, C), torch.float32), mean=((N, C), torch.float32), rstd=((N, C), torch.float32))
    G1 = Guarded(cuda, dict(x=nhwc(t["x"]), noise=noise, nw=t["nw"], gamma=t["gamma"], beta=t["beta"]), outs, need)
    f = G1.f
    fwd = protocol(G1, name + " hwg_adain_fwd", lambda ws, n: L.query(
        "hwg_adain_fwd", f["x"], f["noise"], f["nw"], scale, slope, f["gamma"], f["beta"], EPS, f["u"], f["y"], f["mean"], f["rstd"], N, HW, C, ws, n, G1.st))
    G2 = Guarded(cuda, dict(x=nhwc(t["x"]), nw=t["nw"], gamma=t["gamma"], beta=t["beta"]), outs, need)
    h = G2.f
    rng = protocol(G2, name + " hwg_adain_fwd_rng", lambda ws, n: L.query(
        "hwg_adain_fwd_rng", h["x"], seed, offset, h["nw"], scale, slope, h["gamma"], h["beta"], EPS, h["u"], h["y"], h["mean"], h["rstd"], N, HW, C, ws, n, G2.st))
    differ = bits_differ([(k, rng[k], fwd[k]) for k in outs])
    assert not differ, "%s: hwg_adain_fwd_rng differs from hwg_adain_fwd on hwg_randn's noise in %s" % (name, differ)
    G3 = Guarded(cuda, dict(dy=nhwc(t["gy"]), u=fwd["u"], noise=noise, gamma=t["gamma"], mean=fwd["mean"], rstd=fwd["rstd"]),
                 dict(dx=((N, HW, C), torch.float32), dgamma=((N, C), torch.float32), dbeta=((N, C), torch.float32), dnw=t["dnw0"], dbias=t["dbias0"]), need)
    k = G3.f
    bwd = protocol(G3, name + " hwg_adain_bwd", lambda ws, n: L.query(
        "hwg_adain_bwd", k["dy"], k["u"], k["noise"], scale, slope, k["gamma"], k["mean"], k["rstd"], k["dx"], k["dgamma"], k["dbeta"], k["dnw"], k["dbias"], 1,
        N, HW, C, ws, n, G3.st))
    # fp64, the leaky relu's gates near 0 from the kernel's u
    cpu_threads()
    nz = noise.reshape(N, 1, HW, C).permute(0, 3, 1, 2).double()
    x64, nw64, g64, b64 = (t[q].double().requires_grad_(True) for q in ("x", "nw", "gamma", "beta"))
    pre = R.adain_pre(x64, nz, nw64, _f32(scale))
    hint, near, flips = _gate_hint(pre, nchw(fwd["u"], N, HW, C), R.ACT_LRELU)
    yr = R.norm_pre(R.act_ref(pre, R.ACT_LRELU, _f32(slope), hint), "in", 1, g64, b64, None, _f32(EPS))
    yr.backward(t["gy"].double())
    assert flips <= MAX_FLIPS
    shape = "N%d HW%d C%d" % (N, HW, C)
    bad = report("hwg_adain_fwd(_rng)", shape, need, [("y", nchw(fwd["y"], N, HW, C), yr.detach(), BOUNDS["adain_fwd"])])
    bad += report("hwg_adain_bwd", shape, need,
                  [("dx", nchw(bwd["dx"], N, HW, C), x64.grad, BOUNDS["adain_grad"]), ("dgamma", bwd["dgamma"], g64.grad, BOUNDS["adain_grad"]),
                   ("dbeta", bwd["dbeta"], b64.grad, BOUNDS["adain_grad"]), ("dnoise_w", bwd["dnw"], nw64.grad + t["dnw0"].double(), BOUNDS["adain_grad"]),
                   ("dbias", bwd["dbias"], x64.grad.sum((0, 2, 3)) + t["dbias0"].double(), BOUNDS["adain_grad"])])
    # the same through ops
    xg = nhwc(t["x"]).to(cuda).requires_grad_(True)
    y = ops.adain_epilogue(xg, noise.to(cuda), t["nw"].to(cuda), t["gamma"].to(cuda), t["beta"].to(cuda), scale, slope, EPS)
    y.backward(nhwc(t["gy"]).to(cuda))
    torch.cuda.synchronize()
    differ = bits_differ([("y", fwd["y"], y.detach()), ("dx", bwd["dx"], xg.grad)])
    assert not differ, "%s: %s differ from the bits of ops.adain_epilogue" % (name, differ)
    assert not bad, "%s vs fp64: %s" % (name, "; ".join(bad))


def test_generator_epilogue_refusals_write_nothing(cuda):
    from handwriting_line_generation_amd import _lib as L
    N, HW, C = 2, 5, 8
    need = int(L.query("hwg_norm_workspace", N, HW, C))
    g = _gen("adain refusals")
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    big = lambda: ((N, HW, C), torch.float32)            # noqa: E731
    small = lambda: ((N, C), torch.float32)              # noqa: E731
    G = Guarded(cuda, dict(x=r(N, HW, C), noise=r(N, HW, C), nw=r(C), gamma=r(N, C), beta=r(N, C), dy=r(N, HW, C), mean=r(N, C), rstd=r(N, C).abs() + 0.5,
                           rm=r(C), rv=r(C).abs() + 0.5),
                dict(u=big(), y=big(), m=small(), s=small(), dx=big(), dgamma=small(), dbeta=small(), dnw=((C,), torch.float32)), need)
    f = G.f
    for Cb in (6, 1028):
        refused(G, "hwg_adain_fwd C %d" % Cb, lambda: L.query("hwg_adain_fwd", f["x"], f["noise"], f["nw"], 0.5, 0.2, f["gamma"], f["beta"], EPS, f["u"], f["y"],
                                                              f["m"], f["s"], N, HW, Cb, G.ws, G.need, G.st))
        refused(G, "hwg_adain_fwd_rng C %d" % Cb, lambda: L.query("hwg_adain_fwd_rng", f["x"], 1, 2, f["nw"], 0.5, 0.2, f["gamma"], f["beta"], EPS, f["u"], f["y"],
                                                                  f["m"], f["s"], N, HW, Cb, G.ws, G.need, G.st))
        refused(G, "hwg_adain_bwd C %d" % Cb, lambda: L.query("hwg_adain_bwd", f["dy"], f["x"], f["noise"], 0.5, 0.2, f["gamma"], f["mean"], f["rstd"], f["dx"],
                                                              f["dgamma"], f["dbeta"], f["dnw"], None, 0, N, HW, Cb, G.ws, G.need, G.st))
        refused(G, "hwg_norm_frozen_fwd C %d" % Cb, lambda: L.query("hwg_norm_frozen_fwd", f["x"], f["y"], N, HW, Cb, f["rm"], f["rv"], EPS, f["nw"], f["nw"],
                                                                    0, 0.0, f["m"], f["s"], G.st))


# ---- entries without a workspace: frozen BatchNorm, bias_act ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.FROZEN_CASES, ids=[c[0] for c in AC.FROZEN_CASES])
def test_frozen_batchnorm_entry_on_guarded_buffers_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import _lib as L, ops
    name, N, H, W, C, act, slope = case
    HW = H * W
    g = _gen(name)
    x = torch.randn(N, C, 1, HW, generator=g) * 2 + 0.5
    rm, rv = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) * 3 + 0.01
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    G = Guarded(cuda, dict(x=nhwc(x), rm=rm, rv=rv, gamma=gamma, beta=beta),
                dict(y=((N, HW, C), torch.float32), mean=((N, C), torch.float32), rstd=((N, C), torch.float32)))
    f = G.f
    out = protocol(G, name + " hwg_norm_frozen_fwd", lambda ws, n: L.query(
        "hwg_norm_frozen_fwd", f["x"], f["y"], N, HW, C, f["rm"], f["rv"], EPS, f["gamma"], f["beta"], act, slope, f["mean"], f["rstd"], G.st))
    want = R.frozen_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), act, _f32(slope), _f32(EPS))
    bad = report("hwg_norm_frozen_fwd", "N%d HW%d C%d act%d" % (N, HW, C, act), 0, [("y", nchw(out["y"], N, HW, C), want, BOUNDS["frozen"])])
    with torch.no_grad():
        y = ops.norm_apply_frozen(nhwc(x).to(cuda), rm.to(cuda), rv.to(cuda), EPS, gamma.to(cuda), beta.to(cuda), act, slope)
    assert same_bits(out["y"].reshape(-1), y.reshape(-1)), name + ": y differs from the bits of ops.norm_apply_frozen"
    assert not bad, "%s vs fp64: %s" % (name, "; ".join(bad))


@pytest.mark.parametrize("case", AC.BIAS_ACT_CASES, ids=[c[0] for c in AC.BIAS_ACT_CASES])
def test_bias_act_entries_on_guarded_buffers_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import _lib as L, ops
    name, N, H, W, C, use_bias, use_mask, act, slope = case
    HW, rows = H * W, N * H * W
    g = _gen(name)
    x = torch.randn(N, C, 1, HW, generator=g) * 2
    b = torch.randn(C, generator=g) if use_bias else None
    mask = ((torch.rand(N, C, generator=g) > 0.3).float() / 0.7) if use_mask else None
    zero = torch.rand(N, C, 1, HW, generator=g) < 1 / 16                      # pre-activations that are exactly 0
    x = torch.where(zero, -b[:, None, None] if b is not None else torch.zeros(()), x)
    gy = torch.randn(N, C, 1, HW, generator=g)
    ins = dict(x=nhwc(x))
    if use_bias:
        ins["bias"] = b
    if use_mask:
        ins["mask"] = mask
    G = Guarded(cuda, ins, dict(y=((N, HW, C), torch.float32)))
    f = G.f
    fwd = protocol(G, name + " hwg_bias_act_fwd", lambda ws, n: L.query("hwg_bias_act_fwd", f["x"], f.get("bias"), f.get("mask"), f["y"], rows, HW, C, act, slope, G.st))
    ins = dict(dy=nhwc(gy), y=fwd["y"])
    if use_mask:
        ins["mask"] = mask
    G2 = Guarded(cuda, ins, dict(dx=((N, HW, C), torch.float32)))
    h = G2.f
    bwd = protocol(G2, name + " hwg_bias_act_bwd", lambda ws, n: L.query("hwg_bias_act_bwd", h["dy"], h["y"], h.get("mask"), h["dx"], rows, HW, C, act, slope, G2.st))
    x64 = x.double().requires_grad_(True)
    z = R.bias_act(x64, b.double() if use_bias else None, mask.double() if use_mask else None, R.ACT_NONE)
    hint, near, flips = _gate_hint(z, nchw(fwd["y"], N, HW, C), act)
    yr = R.act_ref(z, act, _f32(slope), hint)
    yr.backward(gy.double())
    assert flips <= MAX_FLIPS
    shape = "rows%d HW%d C%d act%d%s%s" % (rows, HW, C, act, " bias" if use_bias else "", " mask" if use_mask else "")
    bad = report("hwg_bias_act_fwd", shape, 0, [("y", nchw(fwd["y"], N, HW, C), yr.detach(), BOUNDS["bias_act_fwd"])])
    bad += report("hwg_bias_act_bwd", shape, 0, [("dx", nchw(bwd["dx"], N, HW, C), x64.grad, BOUNDS["bias_act_grad"])])
    xg = nhwc(x).to(cuda).requires_grad_(True)
    y = ops.bias_act(xg, b.to(cuda) if use_bias else None, mask.to(cuda) if use_mask else None, act, slope)
    y.backward(nhwc(gy).to(cuda))
    torch.cuda.synchronize()
    differ = bits_differ([("y", fwd["y"], y.detach()), ("dx", bwd["dx"], xg.grad)])
    assert not differ, "%s: %s differ from the bits of ops.bias_act" % (name, differ)
    assert not bad, "%s vs fp64: %s" % (name, "; ".join(bad))


# ---- column sums -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", AC.COLSUM_CASES, ids=["%dx%d" % s for s in AC.COLSUM_CASES])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_colsum_on_guarded_buffers_vs_fp64(cuda, rows, C, accumulate):
    from handwriting_line_generation_amd import _lib as L, ops
    g = _gen("colsum %d %d" % (rows, C))
    x = torch.randn(rows, C, generator=g)
    out0 = torch.randn(C, generator=g) * rows ** 0.5
    need = int(L.query("hwg_colsum_workspace", rows, C))
    assert need == -(-rows // 256) * C * 4
    G = Guarded(cuda, dict(x=x), dict(out=out0 if accumulate else ((C,), torch.float32)), need)
    f = G.f
    got = protocol(G, "hwg_colsum %dx%d" % (rows, C), lambda ws, n: L.query("hwg_colsum", f["x"], rows, C, f["out"], accumulate, ws, n, G.st))["out"]
    want = x.double().sum(0) + (out0.double() if accumulate else 0.0)
    bound = (rows - 1 + accumulate) * U * (x.double().abs().sum(0) + (out0.double().abs() if accumulate else 0.0)) * SECOND
    worst = _ratio(got, want, bound)
    print("\nabi %-22s %-34s ws %-9d e/b out %.2f" % ("hwg_colsum", "rows%d C%d acc%d" % (rows, C, accumulate), need, worst))
    o = ops.colsum(x.to(cuda), out=out0.to(cuda) if accumulate else None, accumulate=bool(accumulate))
    assert same_bits(got, o), "hwg_colsum %dx%d: differs from the bits of ops.colsum" % (rows, C)
    assert worst <= 1.0, "hwg_colsum %dx%d acc %d: |err| is %.3g x the derived bound" % (rows, C, accumulate, worst)
