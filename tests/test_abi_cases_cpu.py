"""CPU: what tests/test_norm_abi_fp64_gpu.py and tests/test_seq_loss_abi_fp64_gpu.py rest on. The tables of oracle/abi_cases.py reach every
regime they name (checked with the make_geo restatement of oracle/norm_cases.py and the byte counts the workspace queries are documented to
return); the fp64 restatements added for the paths no Python caller reaches - per-sample affine (oracle/norm_ref.norm_per_sample), the
accumulating loss (oracle/seq_ref.loss_accumulate), the untransposed log-softmax (oracle/seq_ref.log_softmax_rows) - agree with the
restatements they extend where the two must coincide; and plausible kernel flaws seeded into them (one sample's gamma used for all, out0
dropped, rows left in (t, b) order) each move some case of the tables past the bound the GPU files hold it to by SENSITIVITY_FACTOR or more."""
import pytest
import torch

from oracle import abi_cases as AC
from oracle import norm_cases as NC
from oracle import norm_ref as NR
from oracle import seq_cases as SC
from oracle import seq_ref as SR
from _fp64 import SECOND, U, _f32, cpu_threads
from _norm_act_checks import BOUNDS as NORM_BOUNDS, EPS, norm_inputs
from _seq_loss_checks import ACC_CASES, BOUNDS as SEQ_BOUNDS

SENSITIVITY_FACTOR = 10.0
cpu_threads()


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------------
def test_norm_table_reaches_every_regime():
    shapes = AC.NORM_SHAPES + [AC.HALVED_SHAPE]
    for name, N, HW, C, groups, regime in shapes:
        tags = AC.norm_regimes(N, HW, C)
        g = NC.make_geo(N, HW, C)
        print("norm shape %-16s L %-3d PP %-3d raw %-3d chunks %-2d cs %-4d %s" % (name, g["L"], g["PP"], g["raw"], g["chunks"], g["cs"], sorted(tags)))
        assert regime in tags, (name, regime, tags)
        assert C % groups == 0 and C % 4 == 0 and C <= 1024
        # the byte count hwg_norm_workspace is documented to return, solved for the chunk count
        assert NC.chunks_from_workspace(AC.norm_workspace_bytes(N, HW, C), N, C) == g["chunks"]
    assert {r for s in shapes for r in AC.norm_regimes(*s[1:4])} >= AC.REQUIRED_NORM_REGIMES
    # the geometry the issue's table states, literally
    assert NC.make_geo(3, 5, 4)["PP"] == 256 and NC.make_geo(2, 1025, 4)["chunks"] == 2 and NC.make_geo(3, 85, 48)["PP"] == 21
    g = NC.make_geo(2, 300, 1024)
    assert g["raw"] == 75 and g["chunks"] == 60 and 300 % g["cs"] == 0 and g["cs"] % (NC.NU * g["PP"])      # capped at 64, then re-cut into 60 chunks of 5 pixels
    # the halving regime: one case, and no smaller neighbour reaches it
    _, N, HW, C, _, _ = AC.HALVED_SHAPE
    assert NC.make_geo(N, HW, C)["halved"] and not NC.make_geo(N - 1, HW, C)["halved"] and not NC.make_geo(N, HW - 1, C)["halved"]
    assert sum(NC.make_geo(c["N"], c["HW"], c["C"])["halved"] for c in AC.NORM_CASES) == 1
    # the crossing: every shape with every mode, mask off and on; every mode meets each activation; parameter gradients written and added
    for name, N, HW, C, groups, _ in AC.NORM_SHAPES:
        mine = [c for c in AC.NORM_CASES if (c["N"], c["HW"], c["C"]) == (N, HW, C)]
        assert {(c["mode"], c["mask"]) for c in mine} == {(m, k) for m in AC.MODES for k in (False, True)}, name
    for mode in AC.MODES:
        mine = [c for c in AC.NORM_CASES if c["mode"] == mode]
        assert {c["act"] for c in mine} == {0, 1, 2, 3} and {c["accumulate"] for c in mine} == {0, 1}, mode
        assert all(c["groups"] > 1 for c in mine if mode == "gn" and c["C"] > 4) and all(c["groups"] == 1 for c in mine if mode != "gn")
    assert len({c["name"] for c in AC.NORM_CASES}) == len(AC.NORM_CASES) == 6 * len(AC.NORM_SHAPES) + 1
    assert {c["mode"] for c in AC.PER_SAMPLE_CASES} == {"in", "gn"} and all(c["N"] > 1 for c in AC.PER_SAMPLE_CASES)
    assert any(NC.bias_act_case_regimes(c) & {"more than one grid sweep"} for c in AC.BIAS_ACT_CASES)
    assert {t for c in AC.BIAS_ACT_CASES for t in NC.bias_act_case_regimes(c)} >= NC.REQUIRED_BIAS_ACT_REGIMES
    assert {-(-r // 256) for r, _ in AC.COLSUM_CASES} >= {1, 2, 4} and {c % 4 == 0 for _, c in AC.COLSUM_CASES} == {True, False}


def test_sequence_and_loss_tables_reach_every_regime():
    one, width, sweep = AC.LOG_SOFTMAX_CASES
    assert one[3] == 1 and width[1:4] == (3, 5, SC.num_class())
    over = [s for s in SC.LOG_SOFTMAX_SHAPES if s[1] * s[2] > SC.LOG_SOFTMAX_GRID_WAVES]
    assert sweep[1] * sweep[2] > SC.LOG_SOFTMAX_GRID_WAVES and all(sweep[1] * sweep[2] * sweep[3] <= s[1] * s[2] * s[3] for s in over)
    ragged, infeasible, states = AC.CTC_CASES
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = ragged
    assert (T, B, C, Lmax) == (12, 3, 7, 5) and sum(i < T for i in in_len) == 1 and 0 in tg_len and Lmax in tg_len and any(0 < t < Lmax for t in tg_len)
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = states
    assert (T, B, Lmax) == (265, 2, 130) and 2 * max(tg_len) + 1 == 261 > 256
    for case in AC.CTC_CASES:
        name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = case
        x, tg = SC.ctc_inputs(case)
        nll = SR.ctc_nll(SR.log_softmax_tbc(x.double()), tg, in_len, tg_len)
        assert int(torch.isinf(nll).sum()) == (1 if family is None else 0), (name, nll)
        assert AC.ctc_workspace_bytes(T, B, Lmax) % 4 == 0
    assert sum(c[9] is None for c in AC.CTC_CASES) == 1
    assert all(2 * Lr + 1 > 256 for _, _, Lr in AC.DTW_CASES) and all(AC.dtw_workspace_bytes(*c) % 4 == 0 for c in AC.DTW_CASES)
    assert AC.LOSS_SIZES == [1, 255, 4096, 4097, 131072]
    assert {(c[1], c[2]) for c in AC.LOSS_CASES} == {(m, n) for m in range(5) for n in AC.LOSS_SIZES}
    assert {c[3] for c in AC.LOSS_CASES} == {1.0, -1.0} and {c[4] for c in AC.LOSS_CASES if c[1] < 2} == {"a", "b", "both"}
    assert {c[1] for c in ACC_CASES} == set(range(5)) and {c[4] for c in ACC_CASES if c[1] < 2} >= {"b", "both"}
    assert [r * w for r, w, _ in AC.MASKED_L1_CASES] == [1, 255, 4097] and all(1 <= wm <= w and (wm < w or w == 1) for _, w, wm in AC.MASKED_L1_CASES)
    assert AC.SN_SHAPES[:3] == [(1, 1), (5, 7), (3, 4097)] and AC.SN_SHAPES[3] in SC.SN_MODEL_SHAPES
    assert all(AC.SN_SHAPES[3][0] * AC.SN_SHAPES[3][1] <= r * k for r, k in SC.SN_MODEL_SHAPES)
    assert AC.spectral_partials(3, 4097)[1] == 4 and AC.spectral_partials(5, 7)[1] == 1 and 4097 > SC.SN_DOT_BLOCK      # a row runs into the second dot block
    # the double partials of hwg_spectral_bwd, placed by hand at a rounded-up offset, fit the documented byte count - at the largest count too
    for R_, K in AC.SN_SHAPES + AC.SN_BANK + SC.SN_SHAPES:
        off, parts = AC.spectral_partials(R_, K)
        assert off % 8 == 0 and off >= (R_ + K) * 4 and off + 8 * parts <= AC.spectral_workspace_bytes(R_, K), (R_, K)
    assert AC.spectral_partials(1030, 2037)[1] == 512


# ---- the restatements of the paths no Python caller reaches, and flaws seeded into them ---------------------------------------------------------------
def _errs(got, want):
    d = got - want
    return float(d.norm()) / max(float(want.norm()), 1e-300), float(d.abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("c", AC.PER_SAMPLE_CASES, ids=[c["name"] for c in AC.PER_SAMPLE_CASES])
def test_per_sample_affine_restatement_and_one_gamma_for_all(c):
    N, C = c["N"], c["C"]
    t = norm_inputs(c)
    x, m = t["x"].double(), t["mask"].double() if t["mask"] is not None else None
    shared = NR.norm(x, c["mode"], c["groups"], t["gamma"].double(), t["beta"].double(), m, c["act"], c["slope"], _f32(EPS))
    equal = NR.norm_per_sample(x, c["mode"], c["groups"], t["gamma"].double().expand(N, C), t["beta"].double().expand(N, C), m, c["act"], c["slope"], _f32(EPS))
    assert torch.equal(shared, equal)                         # every sample's affine equal to the shared one: the same function
    td = norm_inputs(dict(c, name=c["name"] + "/distinct"), per_sample=True)
    x, m = td["x"].double(), td["mask"].double() if td["mask"] is not None else None
    g64, b64 = td["gamma"].double().requires_grad_(True), td["beta"].double().requires_grad_(True)
    y = NR.norm_per_sample(x, c["mode"], c["groups"], g64, b64, m, c["act"], c["slope"], _f32(EPS))
    y.backward(td["gy"].double())
    assert g64.grad.shape == (N, C) and b64.grad.shape == (N, C)
    # and sample by sample it is the shared-affine function of that sample alone (IN / GN statistics do not cross samples)
    for n in range(N):
        mn = m[n:n + 1] if m is not None else None
        one = NR.norm(x[n:n + 1], c["mode"], c["groups"], td["gamma"][n].double(), td["beta"][n].double(), mn, c["act"], c["slope"], _f32(EPS))
        assert torch.allclose(one, y[n:n + 1].detach(), rtol=0, atol=1e-12)
    # flaw: the kernel indexes gamma / beta with c instead of n * C + c - sample 0's affine serves every sample
    flawed = NR.norm(x, c["mode"], c["groups"], td["gamma"][0].double(), td["beta"][0].double(), m, c["act"], c["slope"], _f32(EPS))
    rel, mx = _errs(flawed, y.detach())
    print("\nper-sample %-28s one gamma for all: rel L2 %.2e max/max %.2e (bound %.1e, %.1e)" % ((c["name"], rel, mx) + NORM_BOUNDS["norm_fwd"]))
    assert rel >= SENSITIVITY_FACTOR * NORM_BOUNDS["norm_fwd"][0] and mx >= SENSITIVITY_FACTOR * NORM_BOUNDS["norm_fwd"][1]


@pytest.mark.parametrize("case", ACC_CASES, ids=[c[0] for c in ACC_CASES])
def test_accumulating_loss_restatement_and_out0_dropped(case):
    name, mode, n, scale, wrt, inputs = case
    a, b = SC.loss_inputs(case)
    a64, b64 = a.double(), b.double() if b is not None else None
    v = SR.loss(a64, b64, mode, _f32(scale))
    assert SR.loss_accumulate(torch.zeros((), dtype=torch.float64), a64, b64, mode, _f32(scale)) == v
    out0 = (v * 0.75).float().double()
    want = SR.loss_accumulate(out0, a64, b64, mode, _f32(scale))
    k = 2 if mode == 1 else 1
    bound = float((k * 2 * U * v.abs() + U * want.abs()) * SECOND)
    # the bound is sound for an fp32 evaluation in the kernels' order: the mean rounded once, times scale, one rounded sum
    term = {0: (a - b).abs() if b is not None else None, 1: (a - b) * (a - b) if b is not None else None, 2: a, 3: (1 - a).clamp_min(0), 4: (1 + a).clamp_min(0)}[mode]
    v32 = (term.double().sum() / n).float() * torch.tensor(scale)
    got = (out0.float() + v32).double()
    assert abs(float(got - want)) <= bound, (name, float(got - want), bound)
    # flaw: accumulate ignored, out0 dropped
    print("\nloss accumulate %-12s out0 dropped: |err| %.2e, bound %.2e" % (name, abs(float(v - want)), bound))
    assert abs(float(v - want)) >= SENSITIVITY_FACTOR * bound


@pytest.mark.parametrize("case", AC.LOG_SOFTMAX_CASES, ids=[c[0] for c in AC.LOG_SOFTMAX_CASES])
def test_untransposed_log_softmax_restatement_and_rows_left_in_tb_order(case):
    name, B, T, C, kind = case
    x = SC.logits(kind, B, T, C, SC.gen("abi_lsm_" + name)).double()
    tbc = SR.log_softmax_tbc(x)
    rows = SR.log_softmax_rows(x)
    assert rows.shape == (B * T, C) and torch.equal(rows.reshape(B, T, C), tbc.permute(1, 0, 2))
    assert torch.allclose(rows, torch.log_softmax(x.reshape(B * T, C), dim=1), rtol=0, atol=1e-12)
    if B > 1 and T > 1:
        # flaw: transpose_bt = 0 ignored, the rows written in (t, b) order
        rel, mx = _errs(tbc.reshape(T * B, C), rows)
        print("\nlog-softmax %-16s rows left in (t, b) order: rel L2 %.2e max/max %.2e (bound %.1e, %.1e)" % ((name, rel, mx) + SEQ_BOUNDS["lsm_fwd"]))
        assert rel >= SENSITIVITY_FACTOR * SEQ_BOUNDS["lsm_fwd"][0] and mx >= SENSITIVITY_FACTOR * SEQ_BOUNDS["lsm_fwd"][1]


def test_some_table_case_shows_each_flaw():
    assert any(B > 1 and T > 1 for _, B, T, _, _ in AC.LOG_SOFTMAX_CASES) and ACC_CASES and AC.PER_SAMPLE_CASES
