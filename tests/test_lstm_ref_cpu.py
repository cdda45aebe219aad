"""CPU: what tests/test_lstm_fp64_gpu.py rests on. The fp64 reference tests/_lstm_ref.py is pinned to torch.nn.LSTM(...).double() by
tests/test_crnn_cpu.py (not repeated here). This file holds: the fp32 restatement of the summation order (oracle/lstm_cases.py) against fp64
within the per-element bounds of the GPU file - the bounds are sound for the reference alone, headroom printed -; the structure of the
restatement (every k of 0 .. H-1 exactly once, per gate block); the bookkeeping of the case table (every regime of the two step kernels is
reached, the impulse inputs meet every k mod 64 class in every gate block); and the sensitivity of the table: plausible kernel flaws, seeded
into a tile-by-tile copy of the restatement that lives in this file only, each move some case past a condition the GPU file holds it to by
SENSITIVITY_FACTOR or more, or flip an exact comparison (a NaN the call left behind, a canary, a zero row, an impulse)."""
import numpy as np
import pytest

import _lstm_checks as G  # the conditions the GPU file holds the device to
from oracle import lstm_cases as LC
from _fp64 import cpu_threads

SENSITIVITY_FACTOR = 10.0
cpu_threads()


# ---- the restatement against fp64, within the GPU file's bounds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H", LC.H_TABLE)
def test_restatement_stays_within_the_bounds(H):
    """per step (forward from its own h and c, backward from the fp64 state, as the GPU file does it) and end to end: the yardstick is positive"""
    c = next(c for c in LC.E2E_CASES if c["H"] == H)
    x = LC.inputs(c)
    f, fb = G.e2e_restatement(c)
    ratios, bad = G.check_forward_steps(x, f)
    state = LC.valid_state(x)
    ratios.update(G.check_backward_steps(x["dy"], state[0], state[1], x["w"], LC.restate_backward(x["dy"], state[0], state[1], x["w"])))
    _, _, yard_y, yard_dg = G.e2e_reference(c)
    print("\nlstm restatement %-18s %s  yardstick y %.3e dgates %.3e" % (c["name"], "  ".join("e/b %s %.3g" % kv for kv in ratios.items()), yard_y, yard_dg))
    assert not bad, bad
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert 0 < yard_y < 1e-5 and 0 < yard_dg < 1e-5
    e2e, _ = G.check_e2e(c, f["y"], fb["dgates"])
    assert all(abs(v - 1 / G.YARDSTICK_FACTOR) < 1e-12 for v in e2e.values())          # (the restatement is its own yardstick)


@pytest.mark.parametrize("H", LC.H_TABLE)
def test_restatement_touches_every_k_once(H):
    ks = [k for s in range(16) for k in LC.lane_ks(H, s)]
    assert sorted(ks) == list(range(H))
    for s in range(16):
        assert all(k // 4 % 16 == s for k in LC.lane_ks(H, s)) and LC.lane_ks(H, s) == sorted(LC.lane_ks(H, s))
    # and lane_dot walks that schedule: a one-hot x picks every k of every gate block exactly once
    for blocks in (1, 4):
        K = blocks * H
        w = np.arange(1, K + 1, dtype=np.float32)[None, :]
        got = LC.lane_dot(w, np.eye(K, dtype=np.float32), H)
        assert (got[:, 0] == w[0]).all()
    assert len(LC.k_schedule(H)) == 4 * LC.nj(H) and LC.instance(H) >= LC.nj(H)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_regime():
    for r in LC.REGIMES:
        hit = [c["name"] for c in LC.STEP_CASES if r in c["tags"]]
        print("regime %-16s %d cases, e.g. %s" % (r, len(hit), hit[:2]))
        assert hit, r
    assert {LC.instance(H) for H in LC.H_TABLE} == set(LC.INSTANCES) and {LC.chunk(H) for H in LC.H_TABLE} == {32, 31, 21, 16}
    for H in LC.H_TABLE:
        mine = [c for c in LC.STEP_CASES if c["H"] == H]
        assert {c["T"] for c in mine} == {1, 2, 3} and {c["B"] for c in mine} == set(LC.batches(H))
        assert len([c for c in LC.E2E_CASES if c["H"] == H]) == 1
        c = LC.chunk(H)
        # per H: both sides of the k0 / k1 boundary, the full tile, a second tile of one line and a third tile are run with a recurrent product
        later = [x for x in mine if x["T"] > 1]
        for tag in ("nb1to3", "nb16", "nb17" if c >= 17 else "nb16", "nb_chunk", "multi_chunk", "third_tile"):
            assert any(tag in x["tags"] for x in later), (H, tag)
    # dead trailing j and lane-partial last j in every instance that can have them
    assert {LC.instance(c["H"]) for c in LC.STEP_CASES if "dead_j" in c["tags"]} == {4, 8, 16}
    assert {LC.instance(c["H"]) for c in LC.STEP_CASES if "lane_partial" in c["tags"]} == {1, 2, 4, 8, 16}
    assert LC.regimes(68, 1, 1) >= {"NJ2", "lane_partial"} and "dead_j" not in LC.regimes(64, 1, 1) | LC.regimes(1024, 1, 1) and "dead_j" in LC.regimes(132, 1, 1)


def test_impulses_meet_every_class_in_every_block():
    assert {LC.instance(H) for H in LC.IMPULSE_H} == set(LC.INSTANCES)
    for H in LC.IMPULSE_H:
        _, hot, col = LC.forward_impulse(H)
        assert (hot < H).all() and {int(k) % 64 for k in hot} == {k % 64 for k in range(H)}
        if H % 64:
            assert any(k >= H - H % 64 for k in hot)                                   # the partly filled slice
        assert len(LC.tiles(H, len(hot))) >= 2
        for q in range(4):
            assert set(col[q * H:(q + 1) * H]) >= set(hot)
        seen = set()
        for rot in range(4):
            _, hot, blk = LC.backward_impulse(H, rot)
            seen |= {(int(b), int(k) % 64) for b, k in zip(blk, hot)}
        assert seen == {(b, k % 64) for b in range(4) for k in range(H)}


@pytest.mark.parametrize("H", (64, 68, 132))
def test_impulse_checks_pass_the_restatement_and_catch_a_dropped_or_doubled_k(H):
    x, hot, col = LC.forward_impulse(H)
    assert not G.check_forward_impulse(H, hot, col, LC.restate_forward(x))
    (dy, gates, cs, w), hotb, blk = LC.backward_impulse(H, 1)
    assert not G.check_backward_impulse(H, hotb, blk, w, LC.restate_backward(dy, gates, cs, w))
    k = int(hot[0])                                            # line 0's unit: at H = 68 and 132 the k that lane 0 alone holds in the last j
    for factor in (0.0, 2.0):
        def dot(wm, xm, Hh):
            wm = wm.copy()
            wm[:, k::Hh] *= np.float32(factor)
            return LC.lane_dot(wm, xm, Hh)
        assert G.check_forward_impulse(H, hot, col, LC.restate_forward(x, dot=dot)), factor
        assert G.check_backward_impulse(H, hotb, blk, w, LC.restate_backward(dy, gates, cs, w, dot=dot)), factor


# ---- seeded flaws ------------------------------------------------------------------------------------------------------------------------------------
# A copy of the restatement that walks the batch tile by tile and launch by launch as the entry points do, on NaN-filled flat buffers with
# room behind them (the canary), with one flaw switched on.
FLAWS = ("last_j_dropped", "slice_one_float4_too_far", "lines_from_16_given_k0", "clamped_duplicate_stored", "c_prev_from_row_t",
         "c_prev_from_the_wrong_parity", "reverse_reads_row_t_minus_1", "no_hseq_zero_row", "f_gate_uses_c_t", "gate_block_left_out",
         "dcn_from_the_slot_being_written", "second_tile_at_b0_0")


def _dot(w, x, H, flaw):
    """[nb, R]: the lane sums of the tile's lines x [nb, K]"""
    R, K = w.shape
    if flaw == "last_j_dropped" and H % 64:
        Hf = H - H % 64
        if Hf == 0:
            return np.zeros((x.shape[0], R), np.float32)
        cut = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], K // H, H)[:, :, :Hf].reshape(a.shape[0], -1))
        return LC.lane_dot(cut(w), cut(x), Hf)
    out = LC.lane_dot(w, x, H)
    if flaw == "slice_one_float4_too_far" and H % 64 and K == H:
        # the first dead lane of the last j reads k = H .. H+3: the next row's first weights, the next line's first h (nothing behind the last)
        wn = np.concatenate([w[1:, :4], np.zeros((1, 4), np.float32)])
        xn = np.concatenate([x[1:, :4], np.zeros((1, 4), np.float32)])
        out = out + (xn @ wn.T).astype(np.float32)
    return out


def sim_forward(x, flaw=None, training=1):
    T, B, G_ = x["xp"][0].shape
    H = G_ // 4
    BH, room = B * H, 2 * G_
    nan = lambda n: np.full(n + room, np.nan, np.float32)
    y, gates, hseq = nan(T * B * 2 * H), nan(2 * T * B * G_), nan(2 * (T + 1) * BH)
    cbuf = nan(2 * T * BH if training else 4 * BH)
    for tile, (b0, nb) in enumerate(LC.tiles(H, B)):
        if flaw == "second_tile_at_b0_0":
            b0 = 0
        for step in range(T):
            for d in range(2):
                t = T - 1 - step if d else step
                tp = t + 1 if d else t - 1
                lines = b0 + np.arange(nb)
                cw = (d * T + t) * BH if training else ((step & 1) * 2 + d) * BH
                pre = x["xp"][d][t, lines] + x["b"][d]
                cp = np.zeros((nb, H), np.float32)
                if step > 0:
                    cr = (d * T + tp) * BH if training else (((step + 1) & 1) * 2 + d) * BH
                    if flaw == "c_prev_from_row_t" and training:
                        cr = cw
                    if flaw == "c_prev_from_the_wrong_parity" and not training:
                        cr = cw
                    cp = cbuf[cr + b0 * H: cr + (b0 + nb) * H].reshape(nb, H).copy()
                    tr = t - 1 if (flaw == "reverse_reads_row_t_minus_1" and d) else tp
                    h = (y[:T * B * 2 * H].reshape(T, B, 2 * H)[tr, lines, d * H:(d + 1) * H] if 0 <= tr < T else np.full((nb, H), np.nan, np.float32))
                    k = _dot(x["w"][d], np.ascontiguousarray(h), H, flaw)
                    if flaw == "lines_from_16_given_k0" and nb > 16:
                        k[:nb - 16] = k[16:]          # the later pass overwrites k0 of lane s with line s + 16's sum; k1 stays +0
                        k[16:] = 0
                    pre = pre + k
                a = np.concatenate([LC.sigmoid32(pre[:, :2 * H]), np.tanh(pre[:, 2 * H:3 * H]), LC.sigmoid32(pre[:, 3 * H:])], axis=1).astype(np.float32)
                i, f, g, o = (a[:, q * H:(q + 1) * H] for q in range(4))
                c = f * cp + i * g
                h = o * np.tanh(c)
                rows = list(range(nb))
                if flaw == "clamped_duplicate_stored" and nb < LC.MAX_CHUNK:
                    rows.append(nb - 1)               # lane s = nb holds the clamped copy of the last line and stores it to line nb
                for n, r in enumerate(rows):
                    bb = b0 + n
                    if training:
                        p = ((d * T + t) * B + bb) * G_
                        gates[p:p + G_] = a[r]
                        hs = d * (T + 1) * BH
                        p = hs + (t if d else t + 1) * BH + bb * H
                        hseq[p:p + H] = h[r]
                        if step == 0 and flaw != "no_hseq_zero_row":
                            p = hs + (T if d else 0) * BH + bb * H
                            hseq[p:p + H] = 0
                    cbuf[cw + bb * H: cw + bb * H + H] = c[r]
                    p = (t * B + bb) * 2 * H + d * H
                    y[p:p + H] = h[r]
    cut = lambda a, shape: (a[:int(np.prod(shape))].reshape(shape), a[int(np.prod(shape)):])
    out, canaries = {}, []
    for k, a, shape in (("y", y, (T, B, 2 * H)), ("gates", gates, (2, T, B, G_)), ("hseq", hseq, (2, T + 1, B, H)),
                        ("c" if training else "pp", cbuf, (2, T, B, H) if training else (2, 2, B, H))):
        out[k], behind = cut(a, shape)
        canaries.append(behind)
    return out, bool(all(np.isnan(c).all() for c in canaries))


def sim_backward(dy, gates, cs, w, flaw=None):
    _, T, B, G_ = gates.shape
    H = G_ // 4
    dgates = np.full((2, T, B, G_), np.nan, np.float32)
    ws = np.full((2, 2, B, H), np.nan, np.float32)
    one = np.float32(1)
    for b0, nb in LC.tiles(H, B):
        if flaw == "second_tile_at_b0_0":
            b0 = 0
        ln = slice(b0, b0 + nb)
        for step in range(T):
            for d in range(2):
                t = step if d else T - 1 - step
                tn, tp = (t - 1, t + 1) if d else (t + 1, t - 1)
                has_prev = t < T - 1 if d else t > 0
                i, f, g, o = (gates[d, t, ln, q * H:(q + 1) * H] for q in range(4))
                c = cs[d, t, ln]
                cp = cs[d, tp, ln] if has_prev else np.zeros((nb, H), np.float32)
                if flaw == "f_gate_uses_c_t":
                    cp = c
                dh = dy[t, ln, d * H:(d + 1) * H]
                dcn = np.zeros((nb, H), np.float32)
                if step > 0:
                    wt, dg = np.ascontiguousarray(w[d].T), np.ascontiguousarray(dgates[d, tn, ln])
                    if flaw == "gate_block_left_out":
                        wt, dg = wt.copy(), dg.copy()
                        wt[:, 3 * H:], dg[:, 3 * H:] = 0, 0
                    dh = dh + _dot(wt, dg, H, flaw)
                    dcn = ws[(step & 1) if flaw == "dcn_from_the_slot_being_written" else ((step + 1) & 1), d, ln].copy()
                tc = np.tanh(c)
                dc = dcn + dh * o * (one - tc * tc)
                dgates[d, t, ln] = np.concatenate([dc * g * i * (one - i), dc * cp * f * (one - f), dc * i * (one - g * g), dh * tc * o * (one - o)], axis=1)
                ws[step & 1, d, ln] = dc * f
    return dict(dgates=dgates, dc_ws=ws)


def verdict(c, flaw):
    """-> (the worst |err| / bound of the GPU file's per-step conditions, the exact conditions of its protocol that do not hold)"""
    x = LC.inputs(c)
    T = c["T"]
    f, canaries = sim_forward(x, flaw)
    ratios, bad = G.check_forward_steps(x, f)
    bad += ["%s is not finite" % k for k in G.FWD_OUT if not np.isfinite(f[k]).all()]
    if not canaries:
        bad.append("a canary behind a buffer was overwritten")
    ev, canaries = sim_forward(x, flaw, training=0)
    if not (canaries and np.isfinite(ev["y"]).all() and (G.bits(ev["y"]) == G.bits(f["y"])).all()
            and all((G.bits(ev["pp"][(T - 1) & 1, d]) == G.bits(f["c"][d, 0 if d else T - 1])).all() for d in range(2))):
        bad.append("the non-training call gives another y or ping-pong")
    state = LC.valid_state(x)
    b = sim_backward(x["dy"], state[0], state[1], x["w"], flaw)
    ratios.update(G.check_backward_steps(x["dy"], state[0], state[1], x["w"], b))
    if not (np.isfinite(b["dgates"]).all() and np.isfinite(b["dc_ws"][:min(T, 2)]).all()):
        bad.append("dgates or dc_ws is not finite")
    return max(ratios.values()), bad


SMALL = [c for c in LC.STEP_CASES if c["H"] in (4, 68)]          # (the flaws are about tiles, lines and slots: the two smallest H with a partly filled slice)


def test_the_tile_by_tile_copy_without_a_flaw_passes():
    for c in SMALL:
        worst, bad = verdict(c, None)
        assert worst <= 1.0 and not bad, (c["name"], worst, bad)


@pytest.mark.parametrize("flaw", FLAWS)
def test_seeded_flaw_is_caught(flaw):
    caught = []
    for c in SMALL:
        worst, bad = verdict(c, flaw)
        if worst >= SENSITIVITY_FACTOR or bad:
            caught.append((c["name"], worst, bad[:1]))
    print("\nflaw %-34s caught by %d of %d cases, e.g. %s" % (flaw, len(caught), len(SMALL), caught[:2]))
    assert caught, "%s: no case of the table notices it - the table is missing a case" % flaw


def test_end_to_end_condition_notices_a_gate_block_left_out():
    c = next(c for c in LC.E2E_CASES if c["H"] == 68)
    x = LC.inputs(c)
    f, _ = sim_forward(x)
    b = sim_backward(x["dy"], f["gates"], f["c"], x["w"], "gate_block_left_out")
    ratios, line = G.check_e2e(c, f["y"], b["dgates"])
    print("\n" + line)
    assert ratios["dgates"] >= SENSITIVITY_FACTOR and ratios["y"] <= 1.0
