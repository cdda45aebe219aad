"""The conditions of the LSTM kernels' fp64 tests, on host arrays (not collected by pytest): tests/test_lstm_fp64_gpu.py holds the device's
outputs to them (its docstring derives the bounds), tests/test_lstm_ref_cpu.py measures its seeded flaws against them."""
import numpy as np

from oracle import lstm_cases as LC
from _fp64 import SECOND, U, YARDSTICK_FACTOR

E_ACT = 2 * U
LIP = (0.25, 0.25, 1.0, 0.25)          # gate blocks i, f, g, o
FWD_OUT = ("y", "gates", "c", "hseq")  # what the training forward call writes


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
