"""CPU: the restatements of the optimizer-tail, Philox and insert-spaces family (oracle/optim_ref.py) against published vectors, torch's own
Adam and the reference trainer's balance loop written out in fp64; the bookkeeping of the GPU case tables (oracle/optim_cases.py: together
they reach every regime they claim); and the sensitivity of those tables: twelve plausible kernel flaws, seeded into copies of the
restatements that live in this file only, each move some case by at least 10 x the bound tests/test_optim_rng_fp64_gpu.py holds that case
to, or flip one of its exact comparisons."""
import os

import numpy as np
import pytest
import torch

from oracle import optim_cases as OC
from oracle import optim_ref as R
import _optim_rng_checks as G  # the bounds the GPU file holds each family to
from _fp64 import _f32

SENSITIVITY_FACTOR = 10.0


# a flaw in the normals has to show against the measured bound; until one is measured, against the derived one the GPU test uses meanwhile
RANDN_BOUND = G.RANDN_ABS if G.RANDN_ABS is not None else G.RANDN_DERIVED


# ---- Philox, u01 -----------------------------------------------------------------------------------------------------------------------------
KAT = [  # Random123's known-answer vectors of philox4x32-10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    assert R.philox4x32(ctr, key) == out


def test_philox_lanes_are_the_integer_restatement():
    for name, seed, offset in OC.RNG_STREAMS:
        blocks = R.philox_blocks(seed, offset, 9)
        for i in range(9):
            assert tuple(int(x) for x in blocks[i]) == R.philox_block(seed, offset + i), (name, i)
    # the kernels' layout: counter (lo, hi, 0, 0), key (lo, hi)
    assert R.philox_block(0, 0) == KAT[0][2]
    assert R.philox_block(0x0000000500000007, 0x0000000b00000003) == R.philox4x32((3, 11, 0, 0), (7, 5))
    # the counter wraps mod 2^64 like the kernels' uint64 sum
    assert tuple(int(x) for x in R.philox_blocks(5, 2 ** 64 - 1, 2)[1]) == R.philox_block(5, 0)


def test_u01_rounding():
    assert R.u01(0xffffffff) == np.float32(1.0)                    # 2^24 - 1 + 0.5 is a tie, the even neighbour is 2^24: the interval is (0, 1]
    assert R.u01(0) == np.float32(2.0 ** -25) and R.u01(255) == R.u01(0)
    assert R.u01(1 << 8) == np.float32(1.5 * 2.0 ** -24)
    top = np.concatenate([np.arange(0, 4096), np.arange(2 ** 23 - 2048, 2 ** 23 + 2048), np.arange(2 ** 24 - 4096, 2 ** 24)]).astype(np.uint32)
    u = R.u01(top << np.uint32(8))
    assert u.dtype == np.float32 and bool((np.diff(u) >= 0).all()) and bool((u > 0).all()) and bool((u <= 1).all())
    assert bool((np.diff(u[:4096 + 2048]) > 0).all())              # strictly increasing below 2^23, where x + 0.5 is exact
    # from 2^23 on the odd values round up onto their even neighbour
    assert R.u01(np.uint32((2 ** 23 + 1) << 8)) == R.u01(np.uint32((2 ** 23 + 2) << 8))
    # the fp64 value of the same formula differs exactly there
    exact = ((top.astype(np.float64)) + 0.5) / 16777216.0
    assert bool((np.abs(u.astype(np.float64) - exact) <= 2.0 ** -25).all())


def test_box_muller_moments_and_order():
    z = R.randn(3, 0, 400000)
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3
    b = R.philox_blocks(3, 0, 4)
    u = R.u01(b).astype(np.float64)
    want = np.sqrt(-2 * np.log(u[:, 0])) * np.cos(2 * np.pi * u[:, 1])
    assert np.allclose(R.box_muller(b)[:, 0], want, rtol=0, atol=1e-15)
    assert np.allclose(R.box_muller(b)[:, 3], np.sqrt(-2 * np.log(u[:, 2])) * np.sin(2 * np.pi * u[:, 3]), rtol=0, atol=1e-15)
    assert R.randn(3, 0, 5).shape == (5,) and np.array_equal(R.randn(3, 0, 5)[:4], R.box_muller(b)[0])
    assert np.array_equal(R.randn(3, 1, 4), R.box_muller(b)[1])     # the next call's counters continue where ceil(n / 4) left off


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------------------
def test_adam_restatement_is_torch_adam():
    g0 = OC.gen("adam_ref_torch")
    for betas in ((0.5, 0.999), (0.9, 0.999)):
        shapes = [(7,), (3, 5), (1,), (64,)]
        params = [torch.nn.Parameter(torch.randn(s, generator=g0, dtype=torch.float64)) for s in shapes]
        mine = [[p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p), 0] for p in params]
        opt = torch.optim.Adam(params, lr=OC.ADAM_LR, betas=betas, eps=OC.ADAM_EPS)
        for it in range(6):
            for k, p in enumerate(params):
                has = (it + k) % 3 != 0 or k == 1                                # some gradients are None on some steps: the counts diverge
                p.grad = torch.randn(p.shape, generator=g0, dtype=torch.float64) * 10.0 ** (k - 2) if has else None
                if has:
                    st = mine[k]
                    st[3] += 1
                    ss, bc = R.adam_scalars(OC.ADAM_LR, betas[0], betas[1], st[3])
                    st[0], _, st[1], st[2] = R.adam_step(st[0], p.grad, st[1], st[2], float(ss), float(bc), betas[0], betas[1], OC.ADAM_EPS)
            opt.step()
        assert sorted({st[3] for st in mine}) != [6]
        for k, p in enumerate(params):
            assert float(opt.state[p]["step"]) == mine[k][3]
            torch.testing.assert_close(mine[k][0], p.detach(), rtol=1e-13, atol=1e-15)
            torch.testing.assert_close(mine[k][1], opt.state[p]["exp_avg"], rtol=1e-13, atol=1e-18)
            torch.testing.assert_close(mine[k][2], opt.state[p]["exp_avg_sq"], rtol=1e-13, atol=1e-20)


def test_fp32_beta_distance_is_the_derived_number():
    """1 - fp32(0.999) against 0.001: the increment of v is 1.3e-5 (relative) short, the update at most half of that off"""
    b2 = float(np.float32(0.999))
    c2 = float(np.float32(1.0) - np.float32(0.999))
    assert c2 == 1.0 - b2                                           # the fp32 difference is exact (Sterbenz): the contract's double 1 - b2 is the kernels'
    rel = (0.001 - c2) / 0.001
    assert 1.28e-5 < rel < 1.30e-5
    g0 = OC.gen("beta_distance")
    g = torch.randn(4096, generator=g0, dtype=torch.float64)
    m, v = torch.randn(4096, generator=g0, dtype=torch.float64) * 0.3, torch.randn(4096, generator=g0, dtype=torch.float64) ** 2 * 1e-3
    p = torch.randn(4096, generator=g0, dtype=torch.float64)
    worst = 0.0
    for step in OC.ADAM_STEPS:
        ss, bc = (float(x) for x in R.adam_scalars(OC.ADAM_LR, 0.5, 0.999, step))
        exact = R.adam_step(p, g, m, v, ss, bc, 0.5, 0.999, OC.ADAM_EPS)
        contract = R.adam_step(p, g, m, v, ss, bc, 0.5, b2, _f32(OC.ADAM_EPS))
        inc = (contract[3] - v * b2) / (exact[3] - v * 0.999) - 1
        assert float(inc.abs().max()) < 1.30e-5 and float(inc.abs().min()) > 1.28e-5
        upd = (exact[0] - p).abs()
        du = ((contract[0] - exact[0]).abs() / upd)[upd > 1e-7]       # (below that the fp64 rounding of p itself shows in the difference)
        worst = max(worst, float(du.max()))
        # and the GPU test's per-element bound on that distance holds it
        dm, dv, bound = G.fp32_beta_distance(g, m, v, ss, bc, 0.5, 0.999, OC.ADAM_EPS, exact)
        assert bool(((contract[0] - exact[0]).abs() <= bound + 2.0 ** -51 * p.abs()).all()) and bool(((contract[3] - exact[3]).abs() <= dv * 1.0001).all())
    assert worst <= 0.5 * rel * 1.01 + 1e-7, worst                  # eps rounded to fp32 adds 6e-9 of eps, visible only where sqrt(v) ~ eps
    print("\nfp32-beta distance: v's increment %.4e short, update off by at most %.3e (bound %.3e)" % (rel, worst, 0.5 * rel))


# ---- balance -------------------------------------------------------------------------------------------------------------------------------------
def _reference_balance_loop(grads, saved, xs):
    """trainer/hw_with_style_trainer.py:341-376 in fp64 torch, tensor by tensor: grads [t] tensor or None, saved [k][t] tensor or None"""
    means, nz_sum, nz_count = [], 0.0, 0
    for gr in grads:
        if gr is None:
            means.append(None)
            continue
        mean = gr.abs().mean()
        means.append(mean)
        if mean != 0:
            nz_sum, nz_count = nz_sum + mean, nz_count + 1
    if nz_count:
        means = [nz_sum / nz_count if (mn is not None and mn == 0) else mn for mn in means]
    out = [None if gr is None else gr.clone() for gr in grads]
    for k, st in enumerate(saved):
        for t, r in enumerate(st):
            if r is not None:
                rm = r.abs().mean()
                if rm != 0:
                    out[t] += xs[k] * r * (means[t] / rm)
    return out


def test_balance_restatement_is_the_reference_loop():
    g0 = OC.gen("balance_loop")
    sizes = [5, 1, 33, 8, 64, 7, 12]
    grads = [torch.randn(n, generator=g0, dtype=torch.float64) * 0.01 for n in sizes]
    grads[2] = torch.zeros(33, dtype=torch.float64)             # zero mean: replaced
    grads[5] = None                                             # no gradient
    saved = [[torch.randn(n, generator=g0, dtype=torch.float64) * 0.1 for n in sizes] for _ in range(3)]
    saved[0][3] = torch.zeros(8, dtype=torch.float64)           # all-zero stashed tensor
    saved[1][4] = None                                          # absent
    for k in range(3):
        saved[k][5] = None
    xs = [0.5, -1.0, 2.0]
    want = _reference_balance_loop(grads, saved, xs)
    coef = R.balance_coef([0.0 if gr is None else R.abs_sum(gr) for gr in grads], [[0.0 if r is None else R.abs_sum(r) for r in st] for st in saved], sizes,
                          [gr is not None for gr in grads], [[r is not None for r in st] for st in saved], xs)
    assert coef[0, 3] == 0 and coef[1, 4] == 0 and (coef[:, 5] == 0).all() and (coef[:, 2] != 0).all()
    for t, gr in enumerate(grads):
        if gr is None:
            continue
        got = R.axpy(gr, [saved[k][t] for k in range(3) if saved[k][t] is not None], [coef[k, t] for k in range(3) if saved[k][t] is not None])
        torch.testing.assert_close(got, want[t], rtol=1e-13, atol=1e-18)
    # no non-zero mean at all: every coefficient is 0
    zero = R.balance_coef([0.0, 0.0], [[1.0, 2.0]], [4, 4], [True, True], [[True, True]], [1.0])
    assert (zero == 0).all()


def test_clamp_keeps_nan_like_clip_grad_value():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0])
    torch.nn.utils.clip_grad_value_([p], 2.0)
    got = R.clamp(torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0]), 2.0)
    assert torch.isnan(got[0]) and torch.isnan(p.grad[0]) and torch.equal(got[1:], p.grad[1:]) and got[1:].tolist() == [2.0, -2.0, 2.0]


# ---- the tables reach what they claim ----------------------------------------------------------------------------------------------------------
def test_chunk_is_the_librarys():
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "handwriting_line_generation_amd", "trainer", "flat_params.py")).read()
    assert int(re.search(r"^CHUNK = (\d+)$", src, re.M).group(1)) == OC.CHUNK


def test_tables_reach_every_regime():
    reached = {
        "lists": set().union(*(OC.list_regimes(e) for e in OC.LISTS)),
        "balance": set().union(*(OC.balance_regimes(c) for c in OC.BALANCE_CASES)),
        "adam": set().union(*(OC.adam_regimes(c, OC.list_layout(OC.LISTS[0])[0]) for c in OC.ADAM_CASES)),
        "rng": set().union(*(OC.rng_regimes(nm, s, o, n) for nm, s, o in OC.RNG_STREAMS for n in OC.RNG_SIZES)),
        "insert": set().union(*(OC.insert_regimes(c) for c in OC.INSERT_CASES)),
    }
    for fam, need in OC.REQUIRED_REGIMES.items():
        assert need <= reached[fam], "%s: not reached: %s" % (fam, sorted(need - reached[fam]))
    assert sum(OC.SIZES) < 1000000
    # every aligned list on its own (a list of scalar-path tensors has no 16-byte loop). A 4096-element chunk is exactly one trip of the
    # four-piece loops: their second trip needs the library's chunk
    for e in OC.LISTS[:2]:
        tags = OC.list_regimes(e)
        assert {"adam trips > 1", "single trips > 1", "unary partial last trip", "adam partial last trip", "scalar tail"} <= tags, e[0]
        assert ("unary trips > 1" in tags) == (e[1] > OC.TRIP["unary"]), e[0]
    # the layout: tensors 16-byte aligned (or one float off), padded to four floats, a sentinel between any two tensors that are not multiples of 4
    for e in OC.LISTS:
        lay, present = OC.list_layout(e)
        assert bool((lay.offsets % 4 == (1 if e[3] else 0)).all()) and lay.offsets[0] >= OC.GUARD and lay.total - lay.offsets[-1] - lay.numel[-1] >= OC.GUARD
        assert int((~lay.mask()).sum()) > 2 * OC.GUARD
        assert lay.nchunks == sum(-(-n // e[1]) for n in OC.SIZES)
        buf = lay.buffer("layout")
        assert bool((buf[torch.from_numpy(~lay.mask())] == OC.SENTINEL).all()) and not bool((buf[torch.from_numpy(lay.mask())] == OC.SENTINEL).any())
        # the chunk tables cover every element exactly once
        seen = np.zeros(lay.total, dtype=np.int64)
        for t, off in zip(lay.chunk_tensor, lay.chunk_off):
            seen[int(lay.offsets[t] + off): int(lay.offsets[t] + min(off + lay.chunk, lay.numel[t]))] += 1
        assert np.array_equal(seen, lay.mask().astype(np.int64))


def test_insert_cases_need_no_element_left_out():
    """the seeds are chosen so that no pre-rounding value of the restatement lies near a half-integer (std 0 apart, where the ties are the
    point), so the GPU test compares every element; the truncated case ends its longest line in a run of two or more"""
    for case in OC.INSERT_CASES:
        name, L, B, lens, cs, ds, dup, kind, seed, offset, cut = case
        counts, label, lens_t = OC.insert_inputs(case)
        assert counts.shape == (L, B, 2) and label.shape == (L, B) and int(label.min()) >= 1 and int(label.max()) < OC.INSERT_CLASSES
        pre = R.insert_spaces_draws(counts.numpy(), lens, cs, ds, seed + 1, offset)
        if cs or ds:
            assert int(OC.insert_near_ties(pre, lens, dup).sum()) == 0, name
        reps = R.insert_spaces_reps(pre, lens, dup)
        starts, lens_max = R.insert_spaces_layout(reps, lens, counts.numpy())
        T = int(lens_max[:B].max() + lens_max[B])
        idx = R.insert_spaces_fill(label.numpy(), lens, reps, starts, T)
        spaced, padded = R.insert_spaces_spaced(label.numpy(), lens, reps, counts.numpy(), OC.INSERT_CLASSES)
        assert torch.equal(torch.nn.functional.one_hot(torch.from_numpy(idx), OC.INSERT_CLASSES).float(), spaced)
        assert padded == [(T - int(n)) / T for n in lens_max[:B]]
        if cut:
            b = int(lens_max[:B].argmax())
            assert reps[b, 2 * lens[b] - 1] >= 2
        if kind == "ties":
            live = reps[0, :2 * lens[0]]
            assert set(live.tolist()) == {0, 2}
        if kind == "negative":
            assert int(reps.sum()) == int(reps[0, 1]) > 0


# ---- seeded flaws --------------------------------------------------------------------------------------------------------------------------------
def _adam_case_setup(case, entry=OC.LISTS[0]):
    lay, present = OC.list_layout(entry)
    p, g, m, v, steps, zero = OC.adam_inputs(case, lay)
    name, betas, gs = case
    ss64, bc64 = R.adam_scalars(OC.ADAM_LR, betas[0], betas[1], steps)
    t = lay.tensor_of()
    per = lambda a: torch.from_numpy(np.where(t >= 0, a.astype(np.float32).astype(np.float64)[np.maximum(t, 0)], 1.0))
    return lay, (p.double(), g.double(), m.double(), v.double()), per(ss64), per(bc64), (_f32(betas[0]), _f32(betas[1]), _f32(OC.ADAM_EPS)), steps


def _flawed_adam(flaw, p, g, m, v, ss, bc, b1, b2, eps, clip):
    if flaw == "bias corrections swapped":
        # step_size from beta2, bc2_sqrt from beta1: lr / (1 - b2^t) and sqrt(1 - b1^t), recovered from the correct scalars' definitions
        return None
    gc = R.clamp(g, clip) if clip > 0 else g
    if flaw == "beta1 for 1 - beta1":
        mm = m + (gc - m) * b1
        vv = v * b2 + (1 - b2) * gc * gc
    elif flaw == "clip after the moments":
        mm = m + (g - m) * (1 - b1)
        vv = v * b2 + (1 - b2) * g * g
    else:
        raise KeyError(flaw)
    return p - ss * (mm / (vv.sqrt() / bc + eps)), gc, mm, vv


@pytest.mark.parametrize("flaw", ["bias corrections swapped", "beta1 for 1 - beta1", "clip after the moments"])
def test_seeded_adam_flaws_move_a_case(flaw):
    best = (0.0, None)
    for case in OC.ADAM_CASES:
        lay, (p, g, m, v), ss, bc, (b1, b2, eps), steps = _adam_case_setup(case)
        act = torch.from_numpy(lay.mask())
        ref = R.adam_step(p, g, m, v, ss, bc, b1, b2, eps, OC.ADAM_CLIP)
        bm, bv, bp = G.adam_bounds(p, ref[1], m, v, ss, bc, b1, b2, eps, ref)
        if flaw == "bias corrections swapped":
            name, betas, gs = case
            t = lay.tensor_of()
            st = np.where(t >= 0, steps[np.maximum(t, 0)], 1).astype(np.float64)
            ss_w = torch.from_numpy(OC.ADAM_LR / (1.0 - betas[1] ** st))
            bc_w = torch.from_numpy(np.sqrt(1.0 - betas[0] ** st))
            bad = R.adam_step(p, g, m, v, ss_w, bc_w, b1, b2, eps, OC.ADAM_CLIP)
        else:
            bad = _flawed_adam(flaw, p, g, m, v, ss, bc, b1, b2, eps, OC.ADAM_CLIP)
        ratio = max(float((((bad[i] - ref[i]).abs() / b.clamp(min=1e-300))[act]).max()) for i, b in ((0, bp), (2, bm), (3, bv)))
        if ratio > best[0]:
            best = (ratio, case[0])
    print("\nseeded flaw %-28s moves adam case %s by %.3g x its bound" % (flaw, best[1], best[0]))
    assert best[0] >= SENSITIVITY_FACTOR


def test_seeded_abs_sum_flaw_dropping_the_scalar_tail():
    lay, present = OC.list_layout(OC.LISTS[0])
    buf = lay.buffer("abssum_chunk65536_0", 0.1)
    best = (0.0, None)
    for k, sl in enumerate(lay.slices()):
        x = buf[sl]
        want = R.abs_sum(x)
        bad = sum(R.abs_sum(x[off:off + (min(lay.chunk, len(x) - off) // 4) * 4]) for off in range(0, len(x), lay.chunk))
        rel = abs(bad - want) / want
        if rel > best[0]:
            best = (rel, lay.sizes[k])
        if lay.sizes[k] == 200003:
            assert rel >= SENSITIVITY_FACTOR * G.DERIVED["abs_sum_rel"], "the largest tensor's three tail elements must show: %.3e" % rel
    print("\nseeded flaw abs-sum without the scalar tail moves the %d-element tensor by %.3g x its bound" % (best[1], best[0] / G.DERIVED["abs_sum_rel"]))
    assert best[0] >= SENSITIVITY_FACTOR * G.DERIVED["abs_sum_rel"]


@pytest.mark.parametrize("flaw", ["zero-mean replacement skipped", "coefficient from the wrong set row"])
def test_seeded_balance_flaws_move_a_case(flaw):
    best = (0.0, None, False)
    for case in OC.BALANCE_CASES:
        sum_d, sum_r, numel, gp, rp, xs = OC.balance_inputs(case)
        want = R.balance_coef(sum_d, sum_r, numel, gp, rp, xs)
        if flaw == "zero-mean replacement skipped":
            d = sum_d / numel
            r = sum_r / numel[None, :]
            live = gp[None, :] & rp & (r != 0)
            bad = np.where(live, xs[:, None].astype(np.float64) * d[None, :] / np.where(live, r, 1.0), 0.0)
        else:
            bad = np.roll(want, 1, axis=0)
        flipped = bool(((want == 0) != (bad == 0)).any())
        nz = want != 0
        rel = float((np.abs(bad - want)[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0
        if rel > best[0] or (flipped and not best[2]):
            best = (max(rel, best[0]), case[0], flipped or best[2])
    print("\nseeded flaw %-36s moves balance case %s by %.3g x its bound%s" % (flaw, best[1], best[0] / G.DERIVED["coef_rel"],
                                                                              ", and flips an exact zero" if best[2] else ""))
    assert best[0] >= SENSITIVITY_FACTOR * G.DERIVED["coef_rel"]


def _randn_with(seed, offset, n, **kw):
    return R.randn(seed, offset, n, **kw)


RNG_FLAWS = {
    "one key increment wrong": lambda s, o, n: R.randn(s, o, n, w=(R.PHILOX_W[0], R.PHILOX_W[1] ^ 0x10)),
    "counter's high word dropped": lambda s, o, n: R.randn(s, o, n, ctr_bits=32),
    "sine and cosine swapped": lambda s, o, n: R.box_muller(R.philox_blocks(s, o, R.stream_blocks(n)), swap=True).reshape(-1)[:n],
    "stream advanced by n // 4": None,
}


@pytest.mark.parametrize("flaw", list(RNG_FLAWS))
def test_seeded_rng_flaws_move_a_case(flaw):
    best = (0.0, None)
    for name, seed, offset in OC.RNG_STREAMS:
        for n in [x for x in OC.RNG_SIZES if x <= 4097]:
            if flaw == "stream advanced by n // 4":
                # the second of two consecutive calls (the GPU test makes both) starts at offset + n // 4
                want, bad = R.randn(seed, offset + R.stream_blocks(n), n), R.randn(seed, offset + n // 4, n)
            else:
                want, bad = R.randn(seed, offset, n), RNG_FLAWS[flaw](seed, offset, n)
            d = float(np.abs(bad - want).max())
            if d > best[0]:
                best = (d, "%s n=%d" % (name, n))
    print("\nseeded flaw %-30s moves randn case %s by %.3g (%.3g x the bound %.1e)" % (flaw, best[1], best[0], best[0] / RANDN_BOUND, RANDN_BOUND))
    assert best[0] >= SENSITIVITY_FACTOR * RANDN_BOUND
    if flaw == "counter's high word dropped":
        # only the streams whose counter passes 2^32 see it: without them the table would be blind to it
        for name, seed, offset in OC.RNG_STREAMS:
            same = np.array_equal(R.randn(seed, offset, 16), R.randn(seed, offset, 16, ctr_bits=32))
            assert same == (name in ("zero", "high_seed")), name
    if flaw == "stream advanced by n // 4":
        assert np.array_equal(R.randn(1, 8, 8), R.randn(1, 0, 40)[32:])      # a multiple of 4 cannot tell: the odd sizes are in the table for this


@pytest.mark.parametrize("flaw", ["round half up", "counter j * B + b"])
def test_seeded_insert_spaces_flaws_flip_a_case(flaw):
    hit = []
    for case in OC.INSERT_CASES:
        name, L, B, lens, cs, ds, dup, kind, seed, offset, cut = case
        counts, label, lens_t = OC.insert_inputs(case)
        pre = R.insert_spaces_draws(counts.numpy(), lens, cs, ds, seed + 1, offset)
        want = R.insert_spaces_reps(pre, lens, dup)
        if flaw == "round half up":
            bad = R.insert_spaces_reps(pre, lens, dup, rounding=R.round_half_up)
        else:
            bad = R.insert_spaces_reps(R.insert_spaces_draws(counts.numpy(), lens, cs, ds, seed + 1, offset, counter=lambda b, j, L_, B_: j * B_ + b), lens, dup)
        n = int((bad != want).sum())
        if n:
            hit.append("%s (%d)" % (name, n))
    print("\nseeded flaw %-20s changes reps in: %s" % (flaw, ", ".join(hit)))
    assert hit
    if flaw == "round half up":
        assert any(h.startswith("ties_std0") for h in hit)
