"""GPU: the entries of csrc/style_ops.hip - hwg_gather_windows, hwg_scatter_windows, hwg_gather_scores, hwg_segment_weighted_mean / _bwd,
hwg_linear_bank_fwd / _bwd, hwg_mlp_chain_fwd / _bwd / _bwd_split - and of csrc/expert_bank.hip - hwg_grouped_conv1d_fwd / _dgrad / _wgrad,
hwg_gather_rows_ptr, hwg_segment_accumulate_ptr - called at the C ABI through L.query on guarded buffers, against the fp64 restatements of
oracle/style_ref.py. tests/test_style_expert_fp64_gpu.py holds the same kernels to the same references through ops.*, where the workspace is
never smaller than 1 MiB, no call is ever refused and the tables are whatever ops builds; here:

  protocol     Guarded / protocol() of tests/_guarded.py: every operand, pointer table, weight, gradient buffer and the workspace carved out of
               ONE allocation with canaries between them; outputs and workspace NaN before the call; inputs and tables bit-identical after it;
               a second call on a zero-filled workspace gives the same bits; one byte of workspace too few and a null workspace are refused
               with nothing written. The workspace has exactly the bytes hwg_linear_bank_bwd_workspace / hwg_mlp_chain_bwd_workspace /
               hwg_grouped_conv1d_wgrad_workspace return. The builders (tests/_style_expert_abi.py) run on CPU tensors in
               tests/test_style_expert_abi_cpu.py, which seeds the flaws this file is meant to see.
  cases        the tables of oracle/style_cases.py, references and bounds of tests/_style_expert_checks.py: the derived per-element bound
               and YARDSTICK_FACTOR x the fp32 yardstick, no other tolerance; copies and gathers torch.equal. Buffers an entry adds to are
               pre-filled; those a null table entry freezes, and the absent experts', must keep their bits.
  null tables  bptr == NULL (bank forward, grouped forward), gbptr == NULL (bank, chain, grouped wgrad), one gwptr[l] == 0 with gbptr[l]
               live, one dyptr entry == 0, dx == NULL (bank: no workspace, ws = NULL accepted): what include/hwg.h states.
  chain        hwg_mlp_chain_bwd against hwg_mlp_chain_bwd_split on every backward case: dW, db, dx of the same bits.
  refusals     every HWG_REQUIRE of these entries: HWG_ERR_ARG, nothing written.
  edges        centres one step outside the tensor (hwg_gather_windows / hwg_scatter_windows, hwg_gather_scores): zero rows, nothing added
               to dx, good rows with the bits of the call without the bad rows. x lies inside a slab with a non-zero margin line on both
               sides, so a kernel without its guard reads a non-zero value inside this allocation.

Every case prints one line (kept in profiles/style_expert_abi.txt): per output kind the worst |err| / bound ("e/b") and relative L2 error /
(YARDSTICK_FACTOR x yardstick) ("yard")."""
import pytest
import torch

import _style_expert_abi as A
from oracle import style_cases as SC
from oracle import style_ref as R
from _fp64 import entry
from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)
from _guarded import HWG_ERR_WORKSPACE, bits_differ, protocol, refused
from _style_expert_checks import seg_reference, window_reference

pytestmark = pytest.mark.gpu


def LIB(G):
    from handwriting_line_generation_amd import _lib as L
    return L.query


def _case(table, name):
    return next(c for c in table if c[0] == name)


def _line(entry_name, shape, ws, text):
    print("\nabi %-22s %-34s ws %-9d %s" % (entry_name, shape, ws, text))


def _refuse_all(G, entry_name, call, lists):
    for what, over in lists:
        refused(G, "%s %s" % (entry_name, what), lambda: call(G.ws, G.need, **over))
    assert call(G.ws, G.need) == 0, "%s: the buffers of the refused calls do not serve an accepted one" % entry_name
    G.sync()
    _line(entry_name, "refusals", G.need, "%d calls: HWG_ERR_ARG, nothing written" % len(lists))


# ---- grouped Conv1d ------------------------------------------------------------------------------------------------------------------------
def _conv(cuda, case):
    name, Cin, Cout, S, R_, plan, bias = case
    G = A.conv_setup(cuda, LIB, case)
    refs = A.conv_refs(case)
    y = protocol(G, "conv %s fwd" % name, G.fwd, mine=("y",), sized=False)["y"]
    dx = protocol(G, "conv %s dgrad" % name, G.dgrad, mine=("dx",), sized=False)["dx"]
    grads = protocol(G, "conv %s wgrad" % name, G.wgrad, mine=G.mine_wgrad)          # (the absent experts' buffers, and db without tables: not owned)
    assert set(grads) | {"y", "dx"} == set(refs)
    shape = "%s Cin%d Cout%d S%d R%d%s" % (name, Cin, Cout, S, R_, "" if bias else " no bias")
    bad = A.held("hwg_grouped_conv1d_fwd", shape, 0, {"y": y}, refs)
    bad += A.held("hwg_grouped_conv1d_dgrad", shape, 0, {"dx": dx}, refs)
    bad += A.held("hwg_grouped_conv1d_wgrad", shape, G.need, grads, refs)
    assert not bad, "conv %s vs fp64: %s" % (name, "; ".join(bad))


@pytest.mark.parametrize("case", SC.CONV_CASES, ids=[c[0] for c in SC.CONV_CASES])
def test_grouped_conv_entries_on_guarded_buffers_vs_fp64(cuda, case):
    _conv(cuda, case)


def test_grouped_conv_without_bias_tables(cuda):
    """bptr == NULL: no bias is added; gbptr == NULL: the db buffers keep their bits (the smallest case, its bias tables dropped)"""
    _conv(cuda, _case(SC.CONV_CASES, "k8")[:6] + (False,))


def test_gather_rows_and_segment_accumulate_entries(cuda):
    for C in SC.ACCUMULATE_C:
        G = A.accumulate_setup(cuda, LIB, C)
        rows = protocol(G.Gg, "gather_rows_ptr C=%d" % C, G.Gg.call)["out"]
        assert torch.equal(rows, G.want_rows), "gather_rows_ptr C=%d" % C
        _line("hwg_gather_rows_ptr", "C%d n%d" % (C, rows.shape[0]), 0, "exact")
        got = protocol(G, "segment_accumulate_ptr C=%d" % C, G.call, mine=G.mine)      # (the absent expert's buffer: not owned)
        bad = A.held("hwg_segment_accumulate_ptr", "C%d runs %s" % (C, sorted(SC.ACCUMULATE_RUNS.values())), 0, got, G.refs)
        assert not bad, "segment_accumulate_ptr C=%d vs fp64: %s" % (C, "; ".join(bad))


def test_grouped_conv_refusals(cuda):
    G = A.conv_setup(cuda, LIB, _case(SC.CONV_CASES, "k8"))
    geometry = [("R = 9", dict(R=9))] + [("S = %d pad = %d" % sp, dict(S=sp[0], pad=sp[1])) for sp in ((1, 1), (3, 0), (2, 1), (0, 0), (5, 2), (3, -1))]
    sizes = ("ntiles", "R", "Cin", "Cout", "G", "tile_rows")
    _refuse_all(G, "hwg_grouped_conv1d_fwd", G.fwd, A.refusals(G.fwd, ("bptr",), sizes) + geometry + [("Cin % 8 != 0", dict(Cin=12))])
    _refuse_all(G, "hwg_grouped_conv1d_dgrad", G.dgrad, A.refusals(G.dgrad, (), sizes) + geometry + [("Cout % 4 != 0", dict(Cout=6))])
    _refuse_all(G, "hwg_grouped_conv1d_wgrad", G.wgrad, A.refusals(G.wgrad, ("gbptr",), sizes) + geometry + [("ntiles < G", dict(ntiles=G.wgrad.args["G"] - 1))])
    Ga = A.accumulate_setup(cuda, LIB, SC.ACCUMULATE_C[0])
    _refuse_all(Ga.Gg, "hwg_gather_rows_ptr", Ga.Gg.call, A.refusals(Ga.Gg.call))
    _refuse_all(Ga, "hwg_segment_accumulate_ptr", Ga.call, A.refusals(Ga.call))


# ---- windows, scores -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.WINDOW_CASES, ids=[c[0] for c in SC.WINDOW_CASES])
def test_window_entries_on_guarded_buffers_vs_fp64(cuda, case):
    """the centres of the table that lie inside the tensor (the ones outside: the edge test below, on tensors small enough for them)"""
    name, B, Wx, C, w = case
    x, ib0, ip0, dp0, n_in = SC.window_inputs(case)
    inside = (ib0 >= 0) & (ib0 < B) & (ip0 >= 0) & (ip0 < Wx)
    want, refs = window_reference(case)
    ib, ip, dp, _ = A.window_rows(case)
    G = A.window_setup(cuda, LIB, case, ib, ip, dp)
    patches = protocol(G.Gg, "gather_windows " + name, G.Gg.call)["patches"]
    assert torch.equal(patches, want[inside]), "gather_windows %s" % name
    got = protocol(G, "scatter_windows " + name, G.call)
    assert int(got["win_of"].max()) == n_in - 1 and int((got["win_of"] >= 0).sum()) == n_in and int(got["win_of"].min()) == -1
    shape = "%s B%d Wx%d C%d w%d n%d" % (name, B, Wx, C, w, n_in)
    _line("hwg_gather_windows", shape, 0, "exact")
    bad = A.held("hwg_scatter_windows", shape, 0, {"dx": got["dx"]}, refs)
    assert not bad, "scatter_windows %s vs fp64: %s" % (name, "; ".join(bad))


@pytest.mark.parametrize("name", ["w0_c1", "w6_c1"])
def test_window_centres_one_step_outside_give_zero_rows(cuda, name):
    case = _case(SC.WINDOW_CASES, name)
    _, B, Wx, C, w = case
    assert Wx * C <= A.GUARD
    ib, ip, dp, good = A.window_rows(case, edge=True)
    G = A.window_setup(cuda, LIB, case, ib, ip, dp, margin=True)
    with_bad = dict(protocol(G.Gg, "gather_windows edge " + name, G.Gg.call), dx=protocol(G, "scatter_windows edge " + name, G.call)["dx"])
    G2 = A.window_setup(cuda, LIB, case, ib[good], ip[good], dp[good], margin=True)
    without = dict(protocol(G2.Gg, "gather_windows inside " + name, G2.Gg.call), dx=protocol(G2, "scatter_windows inside " + name, G2.call)["dx"])
    A.edge_rows_hold("windows " + name, with_bad, without, good, sums=("dx",))
    assert torch.equal(without["patches"], R.gather_windows(SC.window_inputs(case)[0], ib[good], ip[good], w))
    _line("hwg_gather/scatter_windows", "%s B%d Wx%d C%d w%d" % case, 0, "%d of %d centres one step outside: zero rows, nothing added" % (int((~good).sum()), good.numel()))


def test_gather_scores_entry_on_guarded_buffers_vs_fp64(cuda):
    x, ib, ip, ic = A.scores_rows(edge=False)
    G = A.scores_setup(cuda, LIB, x, ib, ip, ic)
    got = protocol(G, "gather_scores", G.call)["out"]
    want = R.gather_scores(x.double(), ib, ip, ic)
    bad = A.held("hwg_gather_scores", "B%d Wx%d C%d n%d" % (tuple(x.shape) + (ib.numel(),)), 0, {"exp": got}, {"exp": entry(want, None, 2 * A.ULP * want)})
    # an index one step outside [0, B) x [0, Wx) x [0, C): out = 0 (include/hwg.h)
    x, ib, ip, ic, good = A.scores_rows(edge=True)
    assert x.shape[1] * x.shape[2] <= A.GUARD
    Ge = A.scores_setup(cuda, LIB, x, ib, ip, ic, margin=True)
    Gi = A.scores_setup(cuda, LIB, x, ib[good], ip[good], ic[good], margin=True)
    with_bad, without = protocol(Ge, "gather_scores edge", Ge.call), protocol(Gi, "gather_scores inside", Gi.call)
    A.edge_rows_hold("gather_scores", with_bad, without, good)
    want = R.gather_scores(x.double(), ib[good], ip[good], ic[good])
    bad += A.held("hwg_gather_scores", "B%d Wx%d C%d edge, %d rows outside" % (tuple(x.shape) + (int((~good).sum()),)), 0, {"exp": without["out"]},
                  {"exp": entry(want, None, 2 * A.ULP * want)})
    assert not bad, "gather_scores vs fp64: %s" % "; ".join(bad)


# ---- segment mean ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.SEG_CASES, ids=[c[0] for c in SC.SEG_CASES])
def test_segment_mean_entries_on_guarded_buffers_vs_fp64(cuda, case):
    name, n, B, C, kind = case
    refs = seg_reference(case)
    G = A.seg_setup(cuda, LIB, case)
    fwd = protocol(G, "segment_weighted_mean " + name, G.call)
    Gb = G.backward(fwd["wsum"])
    dv = protocol(Gb, "segment_weighted_mean_bwd " + name, Gb.call)["dv"]
    shape = "%s n%d B%d C%d %s" % case
    bad = A.held("hwg_segment_weighted_mean", shape, 0, {"out": fwd["out"]}, refs) + A.held("hwg_segment_weighted_mean_bwd", shape, 0, {"dv": dv}, refs)
    assert not bad, "segment mean %s vs fp64: %s" % (name, "; ".join(bad))


def test_window_score_and_segment_refusals(cuda):
    case = _case(SC.WINDOW_CASES, "w0_c1")
    ib, ip, dp, _ = A.window_rows(case)
    G = A.window_setup(cuda, LIB, case, ib, ip, dp)
    sizes = ("B", "Wx", "C", "n")
    _refuse_all(G.Gg, "hwg_gather_windows", G.Gg.call, A.refusals(G.Gg.call, (), sizes) + [("window = -1", dict(window=-1))])
    _refuse_all(G, "hwg_scatter_windows", G.call, A.refusals(G.call, (), sizes) + [("window = -1", dict(window=-1))])
    x, jb, jp, jc, good = A.scores_rows(edge=True)
    Gs = A.scores_setup(cuda, LIB, x, jb[good], jp[good], jc[good])
    _refuse_all(Gs, "hwg_gather_scores", Gs.call, A.refusals(Gs.call, (), sizes))
    Gm = A.seg_setup(cuda, LIB, _case(SC.SEG_CASES, "n1"))
    _refuse_all(Gm, "hwg_segment_weighted_mean", Gm.call, A.refusals(Gm.call))
    Gb = Gm.backward(protocol(Gm, "segment_weighted_mean n1", Gm.call)["wsum"])
    _refuse_all(Gb, "hwg_segment_weighted_mean_bwd", Gb.call, A.refusals(Gb.call))


# ---- LinearBank ----------------------------------------------------------------------------------------------------------------------------
def _bank(cuda, case, bias=True, gbias=True, note=""):
    name, B, I, O, halves, unused, frozen, xgrad, backward = case
    refs = A.bank_refs(case, bias, gbias)
    Gf = A.bank_forward(cuda, LIB, case, bias)
    outs = A.bank_parts(protocol(Gf, "bank %s fwd%s" % (name, note), Gf.call)["y"], O, B, halves)
    shape = "%s B%d I%d L%d halves%d%s" % (name, B, I, len(O), halves, note)
    bad = A.held("hwg_linear_bank_fwd", shape, 0, outs, refs)
    if backward:
        Gb = A.bank_backward(cuda, LIB, case, gbias)
        assert (Gb.need == 0 and Gb.ws is None) == (not xgrad)                      # dx == NULL: no workspace, the calls pass ws = NULL
        got = protocol(Gb, "bank %s bwd%s" % (name, note), Gb.call, mine=Gb.mine)     # (frozen buffers: not owned, protocol() asserts them unchanged)
        assert set(got) | set(outs) == set(refs), (sorted(got), sorted(refs))
        bad += A.held("hwg_linear_bank_bwd", shape, Gb.need, got, refs)
        if not xgrad:
            assert Gb.call(None, 12345) == 0, "dx == NULL: any workspace_bytes with a null workspace must be accepted"
            Gb.sync()
    else:
        assert set(outs) == set(refs)
    assert not bad, "bank %s%s vs fp64: %s" % (name, note, "; ".join(bad))


@pytest.mark.parametrize("case", SC.BANK_CASES, ids=[c[0] for c in SC.BANK_CASES])
def test_linear_bank_entries_on_guarded_buffers_vs_fp64(cuda, case):
    _bank(cuda, case)


SMALL_BANK = "b1_i8_halves1"
BANK_VARIANTS = {
    "bptr_null": (dict(), dict(bias=False)),
    "gwptr_entry_null_bias_live": (dict(frozen={0: "weight"}), dict()),
    "dyptr_entry_null": (dict(unused=[(2, 0)], frozen={}), dict()),
    "gbptr_null": (dict(frozen={}), dict(gbias=False)),
    "dx_null": (dict(xgrad=False), dict()),
}


@pytest.mark.parametrize("variant", sorted(BANK_VARIANTS))
def test_linear_bank_null_tables_and_entries(cuda, variant):
    name, B, I, O, halves, unused, frozen, xgrad, backward = _case(SC.BANK_CASES, SMALL_BANK)
    over, kw = BANK_VARIANTS[variant]
    c = dict(unused=unused, frozen=frozen, xgrad=xgrad)
    c.update(over)
    _bank(cuda, (name, B, I, O, halves, c["unused"], c["frozen"], c["xgrad"], True), note=" " + variant, **kw)


def test_linear_bank_refusals(cuda):
    """among them the workspace check of hwg_linear_bank_bwd, which used to come after the launch that adds dW / db: protocol() above refuses a
    workspace one byte short; here the same with the gradient buffers of every layer live"""
    case = _case(SC.BANK_CASES, SMALL_BANK)
    Gf = A.bank_forward(cuda, LIB, case)
    sizes = ("L", "B", "I", "halves", "total_outputs")
    _refuse_all(Gf, "hwg_linear_bank_fwd", Gf.call, A.refusals(Gf.call, ("bptr",), sizes) + [("B = 65535 * 16 + 1", dict(B=65535 * 16 + 1))])
    Gb = A.bank_backward(cuda, LIB, case)
    _refuse_all(Gb, "hwg_linear_bank_bwd", Gb.call, A.refusals(Gb.call, ("gbptr", "dx"), sizes) + [("B = 17", dict(B=17))])
    full = A.bank_backward(cuda, LIB, case[:6] + ({},) + case[7:])
    for what, ws, n in (("one byte of workspace too few", full.ws, full.need - 1), ("no workspace", None, full.need), ("no bytes", full.ws, 0)):
        refused(full, "hwg_linear_bank_bwd with " + what, lambda: full.call(ws, n), code=HWG_ERR_WORKSPACE)


# ---- MLPChain ------------------------------------------------------------------------------------------------------------------------------
def _chain(cuda, case, note="", **kw):
    name, D, B, L_, frozen, backward = case
    refs = A.chain_refs(case, kw.get("gbias", True))
    Gf = A.chain_forward(cuda, LIB, case)
    acts = protocol(Gf, "chain %s fwd" % name, Gf.call)["acts"]
    assert torch.equal(acts[0], SC.chain_inputs(case)[0]), "acts[0] is not x"
    assert not bool(acts[1:, :, list(SC.CHAIN_ZERO_NEURONS)].any()), "a neuron with a pre-activation of exactly 0 is not 0"
    shape = "%s D%d B%d L%d%s" % (name, D, B, L_, note)
    bad = A.held("hwg_mlp_chain_fwd", shape, 0, {"h": acts[L_]}, refs)
    if backward:
        G = A.chain_backward(cuda, LIB, case, acts, **kw)
        one = protocol(G, "chain %s bwd%s" % (name, note), G.single, mine=G.mine, sized=False)
        two = protocol(G, "chain %s bwd_split%s" % (name, note), G.split, mine=G.mine)
        differ = bits_differ([(k, one[k], two[k]) for k in G.mine])
        assert not differ, "chain %s%s: hwg_mlp_chain_bwd_split differs from hwg_mlp_chain_bwd in %s" % (name, note, differ)
        assert set(one) == set(G.mine) <= set(refs) and not set(G.mine) & set(G.frozen), (sorted(one), sorted(refs))
        bad += A.held("hwg_mlp_chain_bwd", shape, 0, one, refs, extra=[("split = single", 0.0)])
        bad += A.held("hwg_mlp_chain_bwd_split", shape, G.need, two, refs)
    assert not bad, "chain %s%s vs fp64: %s" % (name, note, "; ".join(bad))


@pytest.mark.parametrize("case", SC.CHAIN_CASES, ids=[c[0] for c in SC.CHAIN_CASES])
def test_mlp_chain_entries_and_the_two_backward_passes_agree(cuda, case):
    _chain(cuda, case)


SMALL_CHAIN = "d128_b8_l1"
CHAIN_VARIANTS = {"gwptr_entry_null_bias_live": dict(wfrozen=0), "gbptr_null": dict(gbias=False), "dx_null": dict(dx=False)}


@pytest.mark.parametrize("variant", sorted(CHAIN_VARIANTS))
def test_mlp_chain_null_tables_and_entries(cuda, variant):
    _chain(cuda, _case(SC.CHAIN_CASES, SMALL_CHAIN), note=" " + variant, **CHAIN_VARIANTS[variant])


def test_mlp_chain_refusals(cuda):
    case = _case(SC.CHAIN_CASES, SMALL_CHAIN)
    Gf = A.chain_forward(cuda, LIB, case)
    sizes = ("L", "B", "D")
    _refuse_all(Gf, "hwg_mlp_chain_fwd", Gf.call, A.refusals(Gf.call, (), sizes) + [("D = %d" % d, dict(D=d)) for d in (96, 192, 256)])
    acts = protocol(Gf, "chain fwd", Gf.call)["acts"]
    G = A.chain_backward(cuda, LIB, case, acts)
    limits = [("L = 9", dict(L=9)), ("B = 17", dict(B=17)), ("D = 96", dict(D=96)), ("D = 256", dict(D=256))]
    _refuse_all(G, "hwg_mlp_chain_bwd", G.single, A.refusals(G.single, ("gbptr", "dx"), sizes) + limits)
    _refuse_all(G, "hwg_mlp_chain_bwd_split", G.split, A.refusals(G.split, ("gbptr", "dx"), sizes) + limits)
