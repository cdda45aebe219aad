"""GPU: the entries of csrc/norm_act.hip - hwg_norm_fwd / _bwd, hwg_norm_frozen_fwd, hwg_adain_fwd / _fwd_rng / _bwd, hwg_bias_act_fwd / _bwd -
and hwg_colsum, called at the C ABI through L.query (return codes visible, never through ops but for the bit comparisons named below) on
guarded buffers, against the fp64 restatements of oracle/norm_ref.py. Case tables and the regimes they cover: oracle/abi_cases.py, checked on
the CPU by tests/test_abi_cases_cpu.py. The buffers are those of tests/test_conv_fp64_gpu.py, loaded from there; the bounds are the BOUNDS of
tests/test_norm_act_fp64_gpu.py, imported: the same kernels and the same arithmetic. The library's default tuning only.

The protocol, for every entry (class Guarded, protocol()): every operand, every output and the workspace are carved out of ONE allocation with
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
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import abi_cases as AC
from oracle import norm_ref as R
from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)

pytestmark = pytest.mark.gpu


def _load(fname):
    """another test file's helpers (importing it needs no GPU)"""
    spec = importlib.util.spec_from_file_location(fname[:-3] + "_shared", os.path.join(os.path.dirname(os.path.abspath(__file__)), fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


F = _load("test_conv_fp64_gpu.py")
NA = _load("test_norm_act_fp64_gpu.py")
carve, put, same_bits, HWG_ERR_ARG, HWG_ERR_WORKSPACE = F.carve, F.put, F.same_bits, F.HWG_ERR_ARG, F.HWG_ERR_WORKSPACE
BOUNDS, EPS, MOMENTUM, MAX_FLIPS, _f32, _gate_hint = NA.BOUNDS, NA.EPS, NA.MOMENTUM, NA.MAX_FLIPS, NA._f32, NA._gate_hint
U = 2.0 ** -24
SECOND = 1 + 2.0 ** -16
NAN = float("nan")


# ---- guarded buffers and the protocol (also loaded by tests/test_seq_loss_abi_fp64_gpu.py) -------------------------------------------------------
class Guarded:
    """inputs {name: CPU tensor}, outputs {name: (shape, dtype) - filled with NaN bits before a call - or a CPU tensor - pre-filled with it}
    and a workspace of exactly `ws_bytes`, all carved out of one allocation. 4- and 8-byte element types (and bytes, in multiples of 4)."""

    def __init__(self, dev, inputs, outputs, ws_bytes=0):
        from handwriting_line_generation_amd import _lib as L, ops
        self.L, self.st, self.dev = L, ops._stream(), dev
        assert ws_bytes % 4 == 0, "workspace of %d bytes: not a multiple of 4" % ws_bytes
        self.need = int(ws_bytes)
        self.ins, self.outs = list(inputs), list(outputs)
        self.shape, self.dtype, self.init = {}, {}, {}
        floats = []
        for k, v in list(inputs.items()) + list(outputs.items()):
            shape, dtype = (tuple(v.shape), v.dtype) if torch.is_tensor(v) else (tuple(v[0]), v[1])
            nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
            assert nbytes % 4 == 0, (k, shape, dtype)
            self.shape[k], self.dtype[k] = shape, dtype
            self.init[k] = v.contiguous() if torch.is_tensor(v) else None
            floats.append(nbytes // 4)
        views, self.intact = carve(dev, *(floats + [self.need // 4]))
        self.f = dict(zip(self.ins + self.outs, views))                 # flat float32 views
        self.ws = views[-1] if self.need else None
        for k in self.ins:
            self.t(k).copy_(self.init[k])
        self.reset()
        torch.cuda.synchronize()
        self.sent = {k: self.f[k].clone() for k in self.ins}

    def t(self, k):
        """the buffer in its own type and shape"""
        return self.f[k].view(self.dtype[k]).view(self.shape[k])

    def set_input(self, k, value):
        self.t(k).copy_(value)
        self.sent[k] = self.f[k].clone()

    def reset(self, names=None):
        for k in self.outs if names is None else names:
            if self.init[k] is None:
                self.f[k].fill_(NAN)
            else:
                self.t(k).copy_(self.init[k])

    def ws_fill(self, value):
        if self.ws is not None:
            self.ws.fill_(value)

    def untouched(self):
        return all(same_bits(self.f[k], self.sent[k]) for k in self.ins)

    def as_reset(self, names=None):
        """the outputs that no longer hold what reset() put there"""
        bad = []
        for k in self.outs if names is None else names:
            ok = bool(torch.isnan(self.f[k]).all()) if self.init[k] is None else same_bits(self.f[k], self.init[k].view(torch.float32).reshape(-1))
            if not ok:
                bad.append(k)
        return bad

    def get(self, k):
        return self.t(k).detach().cpu().clone()


def protocol(G, tag, call, mine=None, partly=(), poison_ws=True, sized=True):
    """the protocol of the module docstring around one entry: call(ws, ws_bytes) -> return code. `mine`: the outputs the entry owns (all of
    them by default), `partly`: those of them it need not fill. poison_ws = False: the workspace carries an earlier call's state (CTC backward)
    -> {name: CPU tensor} of the first call"""
    L = G.L
    mine = list(G.outs) if mine is None else list(mine)
    others = [k for k in G.outs if k not in mine]

    def run(ws, n):
        rc = call(ws, n)
        torch.cuda.synchronize()
        return rc

    kept = {k: G.f[k].clone() for k in others}
    G.reset(mine)
    if poison_ws:
        G.ws_fill(NAN)
    rc = run(G.ws, G.need)
    assert rc == 0, "%s returned %d: %s" % (tag, rc, L.last_error())
    assert G.intact(), "%s: a canary next to a buffer was overwritten" % tag
    assert G.untouched(), "%s: an input changed" % tag
    assert all(same_bits(G.f[k], kept[k]) for k in others), "%s wrote to a buffer it does not own" % tag
    first = {k: G.f[k].clone() for k in mine}
    for k in mine:
        if k not in partly and G.dtype[k] == torch.float32:
            n = int((~torch.isfinite(first[k])).sum())
            assert n == 0, "%s: %d elements of %s are not finite (never written, or written from workspace contents)" % (tag, n, k)
    out = {k: G.get(k) for k in mine}
    G.reset(mine)
    if poison_ws:
        G.ws_fill(0.0)
    assert run(G.ws, G.need) == 0, tag
    differ = [k for k in mine if not same_bits(G.f[k], first[k])]
    assert not differ, "%s: the second call (workspace zero-filled) gives other bits in %s" % (tag, differ)
    assert G.intact() and G.untouched(), "%s: canaries / inputs after the second call" % tag
    if G.need and sized:
        for what, ws, n in (("one byte of workspace too few", G.ws, G.need - 1), ("no workspace", None, G.need)):
            G.reset(mine)
            rc = run(ws, n)
            assert rc == HWG_ERR_WORKSPACE, "%s with %s returned %d" % (tag, what, rc)
            assert not G.as_reset(mine), "%s with %s wrote to %s" % (tag, what, G.as_reset(mine))
            assert G.intact() and G.untouched(), "%s with %s: canaries / inputs" % (tag, what)
    return out


def refused(G, tag, call, code=HWG_ERR_ARG):
    """a call the host code turns down before any launch: its code, nothing written"""
    G.reset()
    rc = call()
    torch.cuda.synchronize()
    assert rc == code, "%s returned %d" % (tag, rc)
    assert not G.as_reset(), "%s wrote to %s" % (tag, G.as_reset())
    assert G.intact() and G.untouched(), tag


def ratios(got, want, bound, size=None):
    """(relative L2 / its bound, max|err| / max|ref| / its bound); inf for a non-finite output. `size`: the float64 tensor whose size the
    error is measured against instead of want's (where want is the small difference of large terms)"""
    got = got.detach().cpu().double().reshape(want.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    d = got - want
    size = want if size is None else size
    return (float(d.norm()) / max(float(size.norm()), 1e-300) / bound[0], float(d.abs().max()) / max(float(size.abs().max()), 1e-300) / bound[1])


def report(entry, shape, ws_bytes, checks):
    """checks: [(name, got, want float64, bound[, size])] -> prints the case's line, returns what is over its bound"""
    parts, bad = [], []
    for name, got, want, bound, *size in checks:
        r = ratios(got, want, bound, *size)
        parts.append("%s %.2f/%.2f" % (name, r[0], r[1]))
        if not (r[0] <= 1.0 and r[1] <= 1.0):
            bad.append("%s: relative L2 %.3g x, max/max %.3g x its bound (%.1e, %.1e)" % (name, r[0], r[1], bound[0], bound[1]))
    print("\nabi %-22s %-34s ws %-9d e/b %s" % (entry, shape, ws_bytes, "  ".join(parts) if parts else "-"))
    return bad


def bits_differ(pairs):
    return [name for name, a, b in pairs if not same_bits(a.reshape(-1), b.reshape(-1))]


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def nchw(t, N, HW, C):
    """a kernel tensor [N][HW][C] as NCHW float64 [N, C, 1, HW]"""
    return t.detach().cpu().double().reshape(N, 1, HW, C).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    """NCHW [N, C, 1, HW] as the kernels' [N, 1, HW, C]"""
    return t.permute(0, 2, 3, 1).contiguous()


# ---- normalisation ---------------------------------------------------------------------------------------------------------------------------
FEW_PIXELS = 16


def norm_inputs(c, per_sample=False):
    """x = 2 randn + 0.5, the inputs of tests/test_norm_act_fp64_gpu.py. With fewer than FEW_PIXELS pixels per channel an InstanceNorm
    statistic is formed from 3 or 5 values, and among 2048 such groups of 2 randn + 0.5 the smallest sample variance is 1e-3 of the group's
    mean square: there the kernels' variance E[x^2] - E[x]^2 from fp32 lane sums keeps four digits (measured at C 1024, HW 3: y 5e-5, dx 2e-3
    of the tensor's maximum - the arithmetic whose cost the "offset16" family of that file measures at mean = 16 sigma), and fp64 itself moves
    by 1e-6 when x moves by an ulp. That is the conditioning of the drawn problem, not the one-chunk regime these shapes are here for: below
    FEW_PIXELS every (n, c) row is standardised to a sample deviation s in [0.5, 2] and a mean of s / 4, whatever the mode pools."""
    N, HW, C = c["N"], c["HW"], c["C"]
    g = _gen(c["name"])
    t = dict(x=torch.randn(N, C, 1, HW, generator=g) * 2 + 0.5)
    if HW < FEW_PIXELS:
        z = t["x"].double()
        s = torch.rand(N, C, 1, 1, generator=g).double() * 1.5 + 0.5
        t["x"] = (((z - z.mean(3, keepdim=True)) / z.std(3, unbiased=False, keepdim=True) + 0.25) * s).float()
    ash = (N, C) if per_sample else (C,)
    t["gamma"] = torch.rand(ash, generator=g) + 0.5
    t["beta"] = torch.randn(ash, generator=g)
    t["mask"] = ((torch.rand(N, C, generator=g) > 0.3).float() / 0.7) if c["mask"] else None
    t["gy"] = torch.randn(N, C, 1, HW, generator=g)
    t["rm0"] = torch.randn(C, generator=g) * 0.3 + 0.2
    t["rv0"] = torch.rand(C, generator=g) + 0.5
    scale = (N * HW) ** 0.5
    t["dgamma0"] = torch.randn(ash, generator=g) * scale
    t["dbeta0"] = torch.randn(ash, generator=g) * scale
    return t


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
    NA._cpu_threads()
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
    NA._cpu_threads()
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
    worst = F._ratio(got, want, bound)
    print("\nabi %-22s %-34s ws %-9d e/b out %.2f" % ("hwg_colsum", "rows%d C%d acc%d" % (rows, C, accumulate), need, worst))
    o = ops.colsum(x.to(cuda), out=out0.to(cuda) if accumulate else None, accumulate=bool(accumulate))
    assert same_bits(got, o), "hwg_colsum %dx%d: differs from the bits of ops.colsum" % (rows, C)
    assert worst <= 1.0, "hwg_colsum %dx%d acc %d: |err| is %.3g x the derived bound" % (rows, C, accumulate, worst)
