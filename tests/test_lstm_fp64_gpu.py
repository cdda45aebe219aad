"""GPU: the LSTM kernels of csrc/lstm.hip - hwg_lstm_fwd (lstm_fwd_step_kernel<1 | 2 | 4 | 8 | 16>), hwg_lstm_bwd (lstm_bwd_step_kernel<...>) and
hwg_lstm_pack_whh - against the numpy fp64 reference tests/_lstm_ref.py, through L.query on the C ABI (never through ops, but for one test
at the end), at every template instance, every kind of partly filled k-slice and every batch tile (case table, the regimes each case covers,
the impulse inputs and the fp32 restatement of the summation order: oracle/lstm_cases.py; the restatement, the table and the sensitivity of
these checks to seeded flaws are checked on the CPU by tests/test_lstm_ref_cpu.py). The buffers are those of tests/test_conv_fp64_gpu.py, loaded
from there.

Every call runs on buffers carved out of one allocation with 64-float canaries before, between and after every operand and every output; y,
gates, c, hseq, dgates, dc_ws, the packed W_hh and the non-training ping-pong are filled with NaN before the call. After the call: return code
0, canaries intact, every input bit-identical, every element the header says is written finite (hseq: all [2][T+1][B][H], the two zero rows
exactly +0), every output the call does not own still NaN, and a second call after re-poisoning gives the same bits.

Per step, at any T. Step t of a direction is recomputed in fp64 from the DEVICE's own h_{t-1} (the neighbouring row of y, which must equal the
hseq row bit for bit) and c_{t-1}, the backward step from the device's own dgates of the step before and its own dc f (dc_ws, while the slot
still holds it): a step's check is independent of every other step and no bound grows with T. u = 2^-24, nj = ceil(H/64); every bound is
multiplied by 1 + 2^-16 for the second-order terms.

  tensor               bound on |device - fp64|                                                                          measured on an MI355X (worst |err| / bound)
  gates[t]             L (n + 2) u A + e_act; n = 4 nj + 4 (the lane's chain of 4 nj fmaf, four butterfly sums), + 2 for      0.62 (H 516, B 63)
                       (xproj + b_hh) + sum; A = |xproj| + |b_hh| + sum_k |W_hh||h|; L = 1/4 (sigmoid) or 1 (tanh), the
                       activation's Lipschitz constant; e_act = 2 u: sigmoid and tanh within 2 ulp of the exact function
                       of their fp32 argument, values <= 1 (the figure of tests/test_lstm_gpu.py; 1 / (1 + expf(-x)) with
                       expf within 1 ulp and a correctly rounded sum and quotient stays within it). First step of a
                       direction: the sum is +0, the pre-activation ONE rounded sum: L u A + e_act.
  c[t]                 3 u (|f c_prev| + |i g|), from the device's gates[t] and c[t-1]: two products and a sum            0.64 (H 768, B 43)
  y[t]                 u |o| (2 + |tanh c| + 2 u), from the device's gates[t] and c[t]: tanhf within 2 ulp, one product   0.71 (H 1024, B 16)
  dgates[t], dc f      with E_dh = e_rec + u (|dy| + |dh_rec|), e_rec = (16 nj + 4) u sum |dgates[t+-1]||W_hh| (the four gate   0.60 (dgates; H 516, B 30), 0.49 (dc_ws; H 64, B 65)
                       blocks in one chain; 0 at the backward's first step, where dh = dy exactly),
                       E_s = 6 u for s = 1 - tanhf(c)^2 (2 u twice through the square, its rounding, the subtraction),
                       E_dc = E_dcn + |o| s E_dh + |dh o| E_s + 2 u |dh o s| + u |dc| (E_dcn = 0 where dc_ws still holds the
                       device's dc f of the step before, else that step's own bound on dc f):
                         i: |g i (1-i)| E_dc + 4 u |.|   (three products and the subtraction 1 - i)
                         f: |c_prev f (1-f)| E_dc + 4 u |.|
                         g: |i (1-g^2)| E_dc + u |dc i| + 2 u |.|   (1 - g g: a product and a subtraction, <= u in all)
                         o: |tanh(c) o (1-o)| E_dh + 2 u |dh o (1-o)| + 4 u |.|
                         dc f: |f| E_dc + u |.|
End to end, T = 6, one case per H, backward from the device's own forward: y and dgates against _lstm_ref with the project's second condition
alone - relative L2 error at most YARDSTICK_FACTOR times that of the fp32 restatement on the same case.               measured: y x0.94 (H 4), dgates x0.90 (every H) of the yardstick
(measured: worst over all cases; every case prints its own line, kept in profiles/lstm_fp64.txt.)"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import lstm_cases as LC
from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)

pytestmark = pytest.mark.gpu


def _conv_module():
    """the convolution file's buffers and comparisons (importing it needs no GPU)"""
    spec = importlib.util.spec_from_file_location("conv_fp64_gpu_shared", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_conv_fp64_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


F = _conv_module()
carve, put, same_bits, YARDSTICK_FACTOR, HWG_ERR_ARG = F.carve, F.put, F.same_bits, F.YARDSTICK_FACTOR, F.HWG_ERR_ARG
U = 2.0 ** -24
E_ACT = 2 * U
SECOND = 1 + 2.0 ** -16
LIP = (0.25, 0.25, 1.0, 0.25)          # gate blocks i, f, g, o


# ---- the conditions, on host arrays (also used, without a GPU, by tests/test_lstm_ref_cpu.py: its seeded flaws are measured against them) ------
def _sig(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def worst(got, want, bound):
    """worst |err| / bound over the elements (an element with a bound of 0 must be exact; a non-finite element is infinitely wrong)"""
    got = np.asarray(got, np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def rel_l2(got, want):
    d = np.asarray(got, np.float64) - want
    if not np.isfinite(d).all():
        return float("inf")
    return float(np.linalg.norm(d)) / max(float(np.linalg.norm(want)), 1e-300)


def walk(d, T):
    """the time rows in the order direction d's forward pass visits them"""
    return list(range(T)) if d == 0 else list(range(T - 1, -1, -1))


def check_forward_steps(x, out):
    """-> ({tensor: worst |err| / bound over all steps and both directions}, [exact properties that do not hold])"""
    T, B, G = x["xp"][0].shape
    H = G // 4
    y, gates, cs, hseq = (np.asarray(out[k], np.float32) for k in ("y", "gates", "c", "hseq"))
    ratios, bad = dict(gates=0.0, c=0.0, y=0.0), []
    terms = 4 * LC.nj(H) + 4 + 2
    lip = np.repeat(np.array(LIP), H)[None, :]
    for d in range(2):
        w64, b64 = x["w"][d].astype(np.float64), x["b"][d].astype(np.float64)
        order = walk(d, T)
        zero_row = hseq[d, 0 if d == 0 else T]
        if not (bits(zero_row) == 0).all():
            bad.append("hseq[%d][%d] is not +0 everywhere" % (d, 0 if d == 0 else T))
        for step, t in enumerate(order):
            xp64 = x["xp"][d][t].astype(np.float64)
            if step == 0:
                pre, bound = xp64 + b64, lip * U * (np.abs(xp64) + np.abs(b64))
                cp = np.zeros((B, H))
            else:
                tp = order[step - 1]
                h = y[tp, :, d * H:(d + 1) * H]
                if not (bits(h) == bits(hseq[d, t if d == 0 else t + 1])).all():
                    bad.append("hseq row of h_%d (direction %d) differs from y" % (tp, d))
                h64 = h.astype(np.float64)
                pre = (xp64 + b64) + h64 @ w64.T
                bound = lip * terms * U * (np.abs(xp64) + np.abs(b64) + np.abs(h64) @ np.abs(w64).T)
                cp = cs[d, tp].astype(np.float64)
            want = np.concatenate([_sig(pre[:, :2 * H]), np.tanh(pre[:, 2 * H:3 * H]), _sig(pre[:, 3 * H:])], axis=1)
            ratios["gates"] = max(ratios["gates"], worst(gates[d, t], want, bound * SECOND + E_ACT))
            i, f, g, o = (gates[d, t][:, q * H:(q + 1) * H].astype(np.float64) for q in range(4))
            ratios["c"] = max(ratios["c"], worst(cs[d, t], f * cp + i * g, 3 * U * (np.abs(f * cp) + np.abs(i * g)) * SECOND))
            tc = np.tanh(cs[d, t].astype(np.float64))
            ratios["y"] = max(ratios["y"], worst(y[t, :, d * H:(d + 1) * H], o * tc, U * np.abs(o) * (2 + np.abs(tc) + 2 * U) * SECOND))
            if not (bits(hseq[d, t + 1 if d == 0 else t]) == bits(y[t, :, d * H:(d + 1) * H])).all():
                bad.append("hseq row of h_%d (direction %d) differs from y" % (t, d))
    return ratios, bad


def check_backward_steps(dy, gates, cs, w, out):
    """gates, cs: what the backward kernel was handed. -> {dgates, dc_ws: worst |err| / bound}"""
    _, T, B, G = gates.shape
    H = G // 4
    dgates, ws = np.asarray(out["dgates"], np.float32), np.asarray(out["dc_ws"], np.float32)
    ratios = dict(dgates=0.0, dc_ws=0.0)
    rec_terms = 16 * LC.nj(H) + 4
    for d in range(2):
        w64 = w[d].astype(np.float64)
        order = walk(d, T)[::-1]
        dcf = E_dcf = None
        for step, t in enumerate(order):
            i, f, g, o = (gates[d, t][:, q * H:(q + 1) * H].astype(np.float64) for q in range(4))
            c = cs[d, t].astype(np.float64)
            cp = cs[d, order[step + 1]].astype(np.float64) if step + 1 < T else np.zeros((B, H))
            dy64 = dy[t][:, d * H:(d + 1) * H].astype(np.float64)
            if step == 0:
                dh, E_dh, dcn, E_dcn = dy64, 0.0, 0.0, 0.0
            else:
                dgp = dgates[d, order[step - 1]].astype(np.float64)
                rec = dgp @ w64
                dh = dy64 + rec
                E_dh = rec_terms * U * (np.abs(dgp) @ np.abs(w64)) + U * (np.abs(dy64) + np.abs(rec))
                if step - 1 >= T - 2:          # the slot still holds the device's dc f of the step before
                    dcn, E_dcn = ws[(step - 1) & 1, d].astype(np.float64), 0.0
                else:
                    dcn, E_dcn = dcf, E_dcf
            tc = np.tanh(c)
            s = 1 - tc * tc
            dc = dcn + dh * o * s
            E_dc = E_dcn + np.abs(o) * s * E_dh + np.abs(dh * o) * 6 * U + 2 * U * np.abs(dh * o * s) + U * np.abs(dc)
            vi, vf, vg, vo = dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)
            want = np.concatenate([vi, vf, vg, vo], axis=1)
            bound = np.concatenate([np.abs(g * i * (1 - i)) * E_dc + 4 * U * np.abs(vi), np.abs(cp * f * (1 - f)) * E_dc + 4 * U * np.abs(vf),
                                    np.abs(i * (1 - g * g)) * E_dc + U * np.abs(dc * i) + 2 * U * np.abs(vg),
                                    np.abs(tc * o * (1 - o)) * E_dh + 2 * U * np.abs(dh * o * (1 - o)) + 4 * U * np.abs(vo)], axis=1)
            ratios["dgates"] = max(ratios["dgates"], worst(dgates[d, t], want, bound * SECOND))
            dcf = dc * f
            E_dcf = (np.abs(f) * E_dc + U * np.abs(dcf)) * SECOND
            if step >= T - 2:
                ratios["dc_ws"] = max(ratios["dc_ws"], worst(ws[step & 1, d], dcf, E_dcf))
    return ratios


_E2E = {}


def e2e_reference(c):
    """(fp64 y, fp64 dgates, relative L2 of the fp32 restatement's y, of its dgates), backward from each one's own forward"""
    if c["name"] not in _E2E:
        x = LC.inputs(c)
        d = lambda a: [v.astype(np.float64) for v in a]
        y, cache = LC.ref().layer_forward(d(x["xp"]), d(x["w"]), d(x["b"]))
        dxp, _, _ = LC.ref().layer_backward(x["dy"].astype(np.float64), cache)
        dg = np.stack(dxp)
        r = LC.restate_forward(x)
        rb = LC.restate_backward(x["dy"], r["gates"], r["c"], x["w"])
        _E2E[c["name"]] = (y, dg, rel_l2(r["y"], y), rel_l2(rb["dgates"], dg), r, rb)
    return _E2E[c["name"]][:4]


def e2e_restatement(c):
    """the fp32 restatement's own forward and backward outputs on the case (computed once, with the reference)"""
    e2e_reference(c)
    return _E2E[c["name"]][4:]


def check_e2e(c, y, dgates):
    """-> {y, dgates: relative L2 / (YARDSTICK_FACTOR * yardstick)} (at most 1 passes), and the line to print"""
    yr, dgr, yard_y, yard_dg = e2e_reference(c)
    ry, rdg = rel_l2(y, yr), rel_l2(dgates, dgr)
    line = "y rel %.3e yard %.3e (x%.2f) dgates rel %.3e yard %.3e (x%.2f)" % (ry, yard_y, ry / yard_y, rdg, yard_dg, rdg / yard_dg)
    return dict(y=ry / (YARDSTICK_FACTOR * yard_y), dgates=rdg / (YARDSTICK_FACTOR * yard_dg)), line


# ---- one case on carved buffers ------------------------------------------------------------------------------------------------------------------
INPUTS = ("xp_f", "xp_r", "w_f", "w_r", "b_f", "b_r", "dy", "gates_in", "c_in")
FWD_OUT, EVAL_OUT, BWD_OUT = ("y", "gates", "c", "hseq"), ("y", "pp"), ("dgates", "dc_ws")
OUTPUTS = ("y", "gates", "c", "hseq", "pp", "whh_t", "dgates", "dc_ws")


class Dev:
    def __init__(self, dev, x, state=None):
        from handwriting_line_generation_amd import _lib as L, ops
        self.L, self.st = L, ops._stream()
        T, B, G = x["xp"][0].shape
        H = G // 4
        self.T, self.B, self.H = T, B, H
        self.shape = dict(xp_f=(T, B, G), xp_r=(T, B, G), w_f=(G, H), w_r=(G, H), b_f=(G,), b_r=(G,), dy=(T, B, 2 * H), gates_in=(2, T, B, G), c_in=(2, T, B, H),
                          y=(T, B, 2 * H), gates=(2, T, B, G), c=(2, T, B, H), hseq=(2, T + 1, B, H), pp=(2, 2, B, H), whh_t=(2, H, G), dgates=(2, T, B, G),
                          dc_ws=(2, 2, B, H))
        views, self.intact = carve(dev, *[int(np.prod(s)) for s in self.shape.values()])
        self.v = dict(zip(self.shape, views))
        gates_in, c_in = state if state is not None else (np.zeros(self.shape["gates_in"], np.float32), np.zeros(self.shape["c_in"], np.float32))
        for k, a in zip(INPUTS, (x["xp"][0], x["xp"][1], x["w"][0], x["w"][1], x["b"][0], x["b"][1], x["dy"], gates_in, c_in)):
            put(self.v[k], torch.from_numpy(np.ascontiguousarray(a)))
        self.poison(OUTPUTS)
        torch.cuda.synchronize()
        self.sent = {k: self.v[k].clone() for k in INPUTS}

    def poison(self, names):
        for k in names:
            self.v[k].fill_(float("nan"))

    def untouched(self):
        return all(same_bits(self.v[k], self.sent[k]) for k in INPUTS)

    def written(self, names):
        """those of `names` that are no longer all NaN"""
        return [k for k in names if not bool(torch.isnan(self.v[k]).all())]

    def get(self, k):
        return self.v[k].detach().cpu().numpy().reshape(self.shape[k]).copy()

    def fwd(self, training=1, **over):
        a = dict(xp_f=self.v["xp_f"], xp_r=self.v["xp_r"], w_f=self.v["w_f"], w_r=self.v["w_r"], b_f=self.v["b_f"], b_r=self.v["b_r"], y=self.v["y"],
                 gates=self.v["gates"] if training else None, c=self.v["c"] if training else self.v["pp"], hseq=self.v["hseq"] if training else None,
                 T=self.T, B=self.B, H=self.H)
        a.update(over)
        rc = self.L.query("hwg_lstm_fwd", a["xp_f"], a["xp_r"], a["w_f"], a["w_r"], a["b_f"], a["b_r"], a["y"], a["gates"], a["c"], a["hseq"], a["T"], a["B"], a["H"],
                          training, self.st)
        torch.cuda.synchronize()
        return rc

    def bwd(self, own_forward=False, **over):
        a = dict(dy=self.v["dy"], gates=self.v["gates" if own_forward else "gates_in"], c=self.v["c" if own_forward else "c_in"], whh_t=self.v["whh_t"],
                 dgates=self.v["dgates"], dc_ws=self.v["dc_ws"], T=self.T, B=self.B, H=self.H)
        a.update(over)
        rc = self.L.query("hwg_lstm_bwd", a["dy"], a["gates"], a["c"], a["whh_t"], a["dgates"], a["dc_ws"], a["T"], a["B"], a["H"], self.st)
        torch.cuda.synchronize()
        return rc

    def pack(self, **over):
        a = dict(w_f=self.v["w_f"], w_r=self.v["w_r"], H=self.H, whh_t=self.v["whh_t"])
        a.update(over)
        rc = self.L.query("hwg_lstm_pack_whh", a["w_f"], a["w_r"], a["H"], a["whh_t"], self.st)
        torch.cuda.synchronize()
        return rc


def _protocol(D, call, mine, tag, partly=()):
    """the protocol of the module docstring around one entry point: `mine` are the outputs the call owns, `partly` those of them it need not fill"""
    others = [k for k in OUTPUTS if k not in mine]
    kept = {k: D.v[k].clone() for k in others}
    D.poison(mine)
    rc = call()
    assert rc == 0, "%s returned %d: %s" % (tag, rc, D.L.last_error())
    assert D.intact(), "%s: a canary next to a buffer was overwritten" % tag
    assert D.untouched(), "%s: an input changed" % tag
    assert all(same_bits(D.v[k], kept[k]) for k in others), "%s wrote to a buffer it does not own" % tag
    first = {k: D.v[k].clone() for k in mine}
    for k in mine:
        if k not in partly:
            n = int((~torch.isfinite(first[k])).sum())
            assert n == 0, "%s: %d elements of %s are not finite (never written, or written wrongly)" % (tag, n, k)
    D.poison(mine)
    assert call() == 0
    assert all(same_bits(D.v[k], first[k]) for k in mine), "%s: the second call gives other bits" % tag
    assert D.intact() and D.untouched(), "%s: canaries / inputs after the second call" % tag
    return {k: D.get(k) for k in mine}


def run_forward(D, tag, training=1):
    return _protocol(D, lambda: D.fwd(training), FWD_OUT if training else EVAL_OUT, tag + " hwg_lstm_fwd")


def run_backward(D, tag, own_forward=False):
    """packs W_hh (checked exactly: whh_t[d][k][r] == w_d[r][k]) and runs hwg_lstm_bwd; at T = 1 only slot 0 of dc_ws is written"""
    wt = _protocol(D, D.pack, ("whh_t",), tag + " hwg_lstm_pack_whh")["whh_t"]
    for d, k in enumerate(("w_f", "w_r")):
        assert (bits(wt[d]) == bits(D.get(k).T)).all(), "%s: the packed W_hh of direction %d is not the transpose" % (tag, d)
    out = _protocol(D, lambda: D.bwd(own_forward), BWD_OUT, tag + " hwg_lstm_bwd", partly=("dc_ws",) if D.T == 1 else ())
    if D.T == 1:
        assert np.isfinite(out["dc_ws"][0]).all() and np.isnan(out["dc_ws"][1]).all(), "%s: at T = 1 exactly slot 0 of dc_ws is written" % tag
    return out


def _report(c, parts):
    H = c["H"]
    print("\nlstm_fp64 %-22s NJ %-2d nj %-2d chunk %-2d tiles %-10s %s" % (c["name"], LC.instance(H), LC.nj(H), LC.chunk(H),
                                                                       "+".join(str(nb) for _, nb in LC.tiles(H, c["B"])), "  ".join(parts)))


@pytest.mark.parametrize("c", LC.STEP_CASES, ids=[c["name"] for c in LC.STEP_CASES])
def test_every_step_against_fp64_from_the_devices_own_state(cuda, c):
    x = LC.inputs(c)
    state = LC.valid_state(x)
    D = Dev(cuda, x, state)
    fr, bad = check_forward_steps(x, run_forward(D, c["name"]))
    br = check_backward_steps(x["dy"], state[0], state[1], x["w"], run_backward(D, c["name"]))
    fr.update(br)
    _report(c, ["e/b %s %.3g" % (k, v) for k, v in fr.items()])
    bad += ["%s: |err| is %.3g x the derived bound" % (k, v) for k, v in fr.items() if not v <= 1.0]
    assert not bad, "%s: %s" % (c["name"], "; ".join(bad))


@pytest.mark.parametrize("c", LC.E2E_CASES, ids=[c["name"] for c in LC.E2E_CASES])
def test_six_steps_end_to_end_against_the_fp32_yardstick(cuda, c):
    x = LC.inputs(c)
    D = Dev(cuda, x)
    f = run_forward(D, c["name"])
    b = run_backward(D, c["name"], own_forward=True)
    ratios, line = check_e2e(c, f["y"], b["dgates"])
    _report(c, [line])
    assert all(v <= 1.0 for v in ratios.values()), "%s: relative L2 over %g x the fp32 yardstick: %s" % (c["name"], YARDSTICK_FACTOR, line)


# ---- impulses: a dropped or doubled k is an exact mismatch ---------------------------------------------------------------------------------------
def check_forward_impulse(H, hot, col, out):
    """-> [what does not hold]. Direction d's first step leaves h = a[b] at unit hot[b] and 0 elsewhere; at its second step gate row r of line
    b must be EXACTLY sig(0) = 1/2 / tanh(0) = 0 where col[r] != hot[b], and the activation of a[b] (within e_act; all such rows of one gate the
    same bits) where it is"""
    bad = []
    B = len(hot)
    for d in range(2):
        first, second = (0, 1) if d == 0 else (1, 0)
        h = out["y"][first, :, d * H:(d + 1) * H]
        a = h[np.arange(B), hot]
        rest = h.copy()
        rest[np.arange(B), hot] = 0
        if not ((rest == 0).all() and (a > 0.5).all()):
            bad.append("direction %d: h of the first step is no multiple of a one-hot vector" % d)
            continue
        g = out["gates"][d, second]
        match = col[None, :] == hot[:, None]                                            # [B, 4H]
        assert match.any(axis=1).all()
        idle = np.tile(np.repeat(np.array([0.5, 0.5, 0.0, 0.5], np.float32), H)[None], (B, 1))
        if not (g[~match] == idle[~match]).all():
            bad.append("direction %d: %d gate elements whose row holds no weight for the hot unit moved" % (d, int((g[~match] != idle[~match]).sum())))
        a64 = a.astype(np.float64)[:, None]
        live = np.concatenate([np.tile(_sig(a64), (1, 2 * H)), np.tile(np.tanh(a64), (1, H)), np.tile(_sig(a64), (1, H))], axis=1)
        if not (np.abs(g.astype(np.float64) - live)[match] <= E_ACT).all():
            bad.append("direction %d: %d gate elements whose row holds the weight 1 for the hot unit are not the activation of h" % (
                d, int((np.abs(g.astype(np.float64) - live)[match] > E_ACT).sum())))
    return bad


def check_backward_impulse(H, hot, blk, w, out):
    """-> [what does not hold]: dgates of the backward's first step is one value v[b] (1; 2 tanhf(1) in block o) at row blk H + hot, and that
    of its second step EXACTLY fl(v W_hh[blk H + hot][u]) / 4 in block g and 0 elsewhere"""
    bad = []
    B = len(hot)
    lines = np.arange(B)
    for d in range(2):
        t0, t1 = (1, 0) if d == 0 else (0, 1)
        g0 = out["dgates"][d, t0]
        v = g0[lines, blk * H + hot]
        rest = g0.copy()
        rest[lines, blk * H + hot] = 0
        want_v = np.where(blk == 3, v, np.float32(1))
        if not ((rest == 0).all() and (v == want_v).all() and (np.abs(v[blk == 3] - 2 * np.tanh(1.0)) <= 4 * E_ACT).all()):
            bad.append("direction %d: dgates of the first step is not the impulse" % d)
            continue
        g1 = out["dgates"][d, t1]
        rec = (w[d][blk * H + hot].astype(np.float64) * v.astype(np.float64)[:, None]).astype(np.float32)        # one rounding, as fmaf from +0
        want = np.zeros_like(g1)
        want[:, 2 * H:3 * H] = rec * np.float32(0.25)
        keep = np.ones(g1.shape, bool)
        for q in range(4):
            keep[lines[blk == 1], q * H + hot[blk == 1]] = False                       # (see backward_impulse: dc f = 2 and c = 1 meet there)
        if not (g1[keep] == want[keep]).all():
            bad.append("direction %d: %d elements of dgates of the second step differ from the one product they are" % (d, int((g1[keep] != want[keep]).sum())))
        if not np.isfinite(g1).all():
            bad.append("direction %d: dgates of the second step is not finite" % d)
    return bad


@pytest.mark.parametrize("H", LC.IMPULSE_H)
def test_impulses(cuda, H):
    x, hot, col = LC.forward_impulse(H)
    D = Dev(cuda, x)
    out = run_forward(D, "impulse H%d" % H)
    bad = check_forward_impulse(H, hot, col, out)
    r, more = check_forward_steps(x, out)
    bad += more + ["%s: |err| is %.3g x the derived bound" % (k, v) for k, v in r.items() if not v <= 1.0]
    for rot in range(4):
        (dy, gates, cs, w), hot, blk = LC.backward_impulse(H, rot)
        xb = dict(xp=x["xp"], w=w, b=x["b"], dy=dy)
        D = Dev(cuda, xb, (gates, cs))
        bad += ["rot %d %s" % (rot, m) for m in check_backward_impulse(H, hot, blk, w, run_backward(D, "impulse H%d rot %d" % (H, rot)))]
    print("\nlstm_fp64 impulse H%d NJ %d: %d lines, %d mismatches" % (H, LC.instance(H), len(hot), len(bad)))
    assert not bad, "H %d: %s" % (H, "; ".join(bad))


# ---- exact properties at the batch tiles below 32 --------------------------------------------------------------------------------------------------
EXACT_H = (68, 768, 1024)


def _both(cuda, x, tag, training=1):
    """forward, then backward from the device's own forward: -> the outputs of both"""
    D = Dev(cuda, x)
    out = run_forward(D, tag, training)
    out.update(run_backward(D, tag, own_forward=True))
    return out


@pytest.mark.parametrize("H", EXACT_H)
def test_a_line_of_a_three_tile_batch_equals_the_line_run_alone(cuda, H):
    c = LC.chunk(H)
    B, T = 2 * c + 1, 3
    x = LC.make_case(T, B, H, seed=60 + H)
    full = _both(cuda, x, "rows H%d" % H)
    for row in sorted({0, 15, 16, c - 1, c, 2 * c}):
        one = dict(xp=[a[:, row:row + 1].copy() for a in x["xp"]], w=x["w"], b=x["b"], dy=x["dy"][:, row:row + 1].copy())
        alone = _both(cuda, one, "row %d alone H%d" % (row, H))
        for k in ("y", "gates", "c", "hseq", "dgates"):
            a, f = (alone[k], full[k][:, row:row + 1]) if k == "y" else (alone[k], full[k][:, :, row:row + 1])
            assert (bits(a) == bits(f)).all(), "H %d row %d: %s differs from the line run alone" % (H, row, k)


@pytest.mark.parametrize("H,T", [(68, 3), (768, 2), (1024, 3)])
def test_the_non_training_call_writes_y_and_the_ping_pong_only(cuda, H, T):
    B = 2 * LC.chunk(H) + 1
    x = LC.make_case(T, B, H, seed=70 + H)
    D = Dev(cuda, x)
    train = run_forward(D, "training H%d" % H)
    D.poison(OUTPUTS)
    ev = run_forward(D, "eval H%d" % H, training=0)          # (the protocol: every other output still NaN, canaries, inputs)
    assert (bits(ev["y"]) == bits(train["y"])).all()
    slot = (T - 1) & 1
    assert (bits(ev["pp"][slot, 0]) == bits(train["c"][0, T - 1])).all() and (bits(ev["pp"][slot, 1]) == bits(train["c"][1, 0])).all()


@pytest.mark.parametrize("H", EXACT_H)
def test_reverse_direction_equals_forward_on_the_flipped_sequence(cuda, H):
    B, T = LC.chunk(H) + 1, 3
    x = LC.make_case(T, B, H, seed=80 + H)
    a = _both(cuda, x, "flip a H%d" % H)
    f = dict(xp=[x["xp"][1][::-1].copy(), x["xp"][0][::-1].copy()], w=x["w"][::-1], b=x["b"][::-1],
             dy=np.concatenate([x["dy"][::-1, :, H:], x["dy"][::-1, :, :H]], axis=2).copy())
    b = _both(cuda, f, "flip b H%d" % H)
    assert (bits(a["y"][:, :, H:]) == bits(b["y"][::-1, :, :H])).all() and (bits(a["y"][:, :, :H]) == bits(b["y"][::-1, :, H:])).all()
    for k in ("gates", "c", "dgates"):
        assert (bits(a[k][1]) == bits(b[k][0][::-1])).all() and (bits(a[k][0]) == bits(b[k][1][::-1])).all(), k


@pytest.mark.parametrize("H", [4, 68, 132, 1024])
def test_pack_whh_is_the_exact_transpose(cuda, H):
    """68 and 132 are no multiples of the kernel's 32 x 32 tile; nothing is written outside [2][H][4H] (canaries) or to any other buffer"""
    x = LC.make_case(1, 1, H, seed=90 + H)
    D = Dev(cuda, x)
    wt = _protocol(D, D.pack, ("whh_t",), "pack H%d" % H)["whh_t"]
    for d in range(2):
        assert (bits(wt[d]) == bits(x["w"][d].T)).all(), d


# ---- refusals and queries ----------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_return_the_argument_error_and_write_nothing(cuda):
    x = LC.make_case(2, 3, 8, seed=1)
    D = Dev(cuda, x)
    v = D.v
    off = lambda k: v[k][1:]                                  # the same buffer, 4 bytes further on
    refused = [("fwd H 6", lambda: D.fwd(H=6)), ("fwd H 1028", lambda: D.fwd(H=1028)), ("fwd T 0", lambda: D.fwd(T=0)), ("fwd B 0", lambda: D.fwd(B=0)),
               ("fwd T B 4H = 2^31", lambda: D.fwd(T=1 << 19, B=1, H=1024)), ("fwd T B 4H > 2^31", lambda: D.fwd(T=3, B=1 << 20, H=512)),
               ("fwd training without gates", lambda: D.fwd(gates=None)), ("fwd training without hseq", lambda: D.fwd(hseq=None)),
               ("fwd y off by 4 bytes", lambda: D.fwd(y=off("y"))), ("fwd W_hh off by 4 bytes", lambda: D.fwd(w_f=off("w_f"))),
               ("fwd W_hh (reverse) off by 4 bytes", lambda: D.fwd(w_r=off("w_r"))),
               ("bwd H 6", lambda: D.bwd(H=6)), ("bwd H 1028", lambda: D.bwd(H=1028)), ("bwd T 0", lambda: D.bwd(T=0)), ("bwd B 0", lambda: D.bwd(B=0)),
               ("bwd T B 4H = 2^31", lambda: D.bwd(T=1 << 19, B=1, H=1024)),
               ("bwd dgates off by 4 bytes", lambda: D.bwd(dgates=off("dgates"))), ("bwd whh_t off by 4 bytes", lambda: D.bwd(whh_t=off("whh_t"))),
               ("pack H 0", lambda: D.pack(H=0)), ("pack H 1028", lambda: D.pack(H=1028)), ("pack without whh_t", lambda: D.pack(whh_t=None))]
    refused += [("fwd without %s" % k, (lambda k=k: D.fwd(**{k: None}))) for k in ("xp_f", "xp_r", "w_f", "w_r", "b_f", "b_r", "y", "c")]
    refused += [("bwd without %s" % k, (lambda k=k: D.bwd(**{k: None}))) for k in ("dy", "gates", "c", "whh_t", "dgates", "dc_ws")]
    refused += [("pack without %s" % k, (lambda k=k: D.pack(**{k: None}))) for k in ("w_f", "w_r")]
    for what, call in refused:
        rc = call()
        assert rc == HWG_ERR_ARG, "%s returned %d" % (what, rc)
        assert not D.written(OUTPUTS), "%s wrote to %s" % (what, D.written(OUTPUTS))
        assert D.intact() and D.untouched(), what
    # (and the same buffers do serve an accepted call)
    assert D.fwd() == 0 and D.pack() == 0 and D.bwd(own_forward=True) == 0 and D.intact()


def test_limit_queries(cuda):
    from handwriting_line_generation_amd import _lib as L
    assert L.query("hwg_lstm_unit_slice") == LC.UNITS == 4
    want = {1: 32, 4: 32, 512: 32, 516: 31, 768: 21, 1024: 16, 1025: 0, 0: 0}
    assert {H: L.query("hwg_lstm_batch_tile", H) for H in want} == want
    assert all(LC.chunk(H) == want[H] for H in want if 1 <= H <= 1024)


# ---- through ops at the new tilings: dW_hh (the convolution weight-gradient path) and db_hh (colsum) at widths they have not seen ------------------
@pytest.mark.parametrize("H,B,T", [(768, 22, 3), (1024, 17, 2)])
def test_ops_lstm_layer_at_the_narrow_batch_tiles(cuda, H, B, T):
    import test_lstm_gpu as G
    c = LC.make_case(T, B, H, seed=H + 10 * B + 1000 * T)
    bad = G.check_against_yardstick("layer H%d B%d T%d" % (H, B, T), G.run_layer(c, cuda), G.ref_layer(c), G.torch_layer(c))
    assert not bad, bad
