"""CPU: the builders of tests/_style_expert_abi.py on CPU tensors, with the entries of csrc/style_ops.hip and csrc/expert_bank.hip replaced by
fake ones made from the fp32 restatements of oracle/style_ref.py (Fake: the same signatures, pointer tables resolved to the carved views).

  well-behaved entries   pass protocol() and the references of tests/test_style_expert_abi_fp64_gpu.py on one small case and one case of
                         several tiles / chunks per family: the tables, plans and argument lists the GPU file uses describe the case they claim to.
  seeded flaws           each of these makes protocol() / refused() / the edge check raise, with a message that names the condition:
                         an entry that adds gradients and then returns HWG_ERR_WORKSPACE (the order hwg_linear_bank_bwd had); a store one
                         element behind an expert's weight-gradient buffer; a reduce pass that sums a workspace chunk nobody wrote; a frozen
                         layer whose buffer changes; gathers without the centre clause of their guard, fed centres one step outside.
  footprint              what those bad centres would touch with the guard removed lies inside the slab / the canaries of the allocation.
  table layout           the builders' tables equal the ones ops.LinearBank / ops.MLPChain / model/expert_bank.make_plan build for the same
                         modules; the workspace sizes Fake restates are the ones the library returns."""
import numpy as np
import pytest
import torch

import _style_expert_abi as A
from oracle import style_cases as SC
from oracle import style_ref as R
from _fp64 import entry
from _guarded import GUARD, HWG_ERR_WORKSPACE, bits_differ, protocol, refused
from _style_expert_checks import seg_reference, window_reference

CPU = torch.device("cpu")
GOOD = A.fake_lib()


def _case(table, name):
    return next(c for c in table if c[0] == name)


def _raises(message, fn):
    with pytest.raises(AssertionError) as e:
        fn()
    assert message in str(e.value), str(e.value)


# ---- well-behaved entries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k8", "cin264_s3_r8"])
def test_conv_builders_describe_their_case(name):
    case = _case(SC.CONV_CASES, name)
    G = A.conv_setup(CPU, GOOD, case)
    refs = A.conv_refs(case)
    outs = dict(protocol(G, "fwd", G.fwd, mine=("y",), sized=False), **protocol(G, "dgrad", G.dgrad, mine=("dx",), sized=False))
    outs.update(protocol(G, "wgrad", G.wgrad, mine=G.mine_wgrad))
    assert set(outs) == set(refs) and not A.held("conv", name, G.need, outs, refs)
    assert G.as_reset([k for k in G.outs if k not in outs]) == [], "an absent expert's buffer, or db without tables, changed"


def test_accumulate_builders_describe_their_case():
    G = A.accumulate_setup(CPU, GOOD, SC.ACCUMULATE_C[1])
    assert torch.equal(protocol(G.Gg, "gather_rows", G.Gg.call)["out"], G.want_rows)
    assert not A.held("accumulate", "", 0, protocol(G, "accumulate", G.call, mine=G.mine), G.refs)


@pytest.mark.parametrize("name", ["w0_c1", "w6_c1", "w2_c1"])
def test_window_builders_describe_their_case(name):
    case = _case(SC.WINDOW_CASES, name)
    _, B, Wx, C, w = case
    x, ib0, ip0, dp0, n_in = SC.window_inputs(case)
    inside = (ib0 >= 0) & (ib0 < B) & (ip0 >= 0) & (ip0 < Wx)
    want, refs = window_reference(case)
    ib, ip, dp, _ = A.window_rows(case)
    G = A.window_setup(CPU, GOOD, case, ib, ip, dp)
    assert torch.equal(protocol(G.Gg, "gather", G.Gg.call)["patches"], want[inside])
    got = protocol(G, "scatter", G.call)
    assert int((got["win_of"] >= 0).sum()) == n_in and not A.held("scatter", name, 0, {"dx": got["dx"]}, refs)


def test_scores_and_segment_builders_describe_their_case():
    x, ib, ip, ic, good = A.scores_rows(edge=True)
    G = A.scores_setup(CPU, GOOD, x, ib, ip, ic, margin=True)
    Gi = A.scores_setup(CPU, GOOD, x, ib[good], ip[good], ic[good], margin=True)
    with_bad, without = protocol(G, "scores", G.call), protocol(Gi, "scores", Gi.call)
    A.edge_rows_hold("scores", with_bad, without, good)
    want = R.gather_scores(x.double(), ib[good], ip[good], ic[good])
    assert not A.held("scores", "", 0, {"exp": without["out"]}, {"exp": entry(want, None, 2 * A.ULP * want)})
    for name in ("n1", "counts_c1"):
        case = _case(SC.SEG_CASES, name)
        Gs = A.seg_setup(CPU, GOOD, case)
        fwd = protocol(Gs, "seg", Gs.call)
        Gb = Gs.backward(fwd["wsum"])
        assert not A.held("seg", name, 0, {"out": fwd["out"], "dv": protocol(Gb, "seg bwd", Gb.call)["dv"]}, seg_reference(case))


def _bank(case, lib=GOOD, bias=True, gbias=True):
    name, B, I, O, halves, unused, frozen, xgrad, backward = case
    refs = A.bank_refs(case, bias, gbias)
    Gf = A.bank_forward(CPU, lib, case, bias)
    outs = A.bank_parts(protocol(Gf, "bank fwd", Gf.call)["y"], O, B, halves)
    Gb = A.bank_backward(CPU, lib, case, gbias)
    outs.update(protocol(Gb, "bank bwd", Gb.call, mine=Gb.mine))
    assert set(outs) == set(refs)
    return A.held("bank", name, Gb.need, outs, refs)


@pytest.mark.parametrize("name", ["b1_i8_halves1", "b16_i100_odd_total", "b8_i128_x_const"])
def test_bank_builders_describe_their_case(name):
    assert not _bank(_case(SC.BANK_CASES, name))


def test_bank_variants_have_references_of_their_own():
    name, B, I, O, halves, unused, frozen, xgrad, backward = _case(SC.BANK_CASES, "b1_i8_halves1")
    assert not _bank((name, B, I, O, halves, unused, frozen, xgrad, True), bias=False)
    assert not _bank((name, B, I, O, halves, [(2, 0)], {}, xgrad, True))
    assert not _bank((name, B, I, O, halves, unused, {}, False, True), gbias=False)


def _chain(case, lib=GOOD, **kw):
    name, D, B, L_, frozen, backward = case
    refs = A.chain_refs(case, kw.get("gbias", True))
    Gf = A.chain_forward(CPU, lib, case)
    acts = protocol(Gf, "chain fwd", Gf.call)["acts"]
    G = A.chain_backward(CPU, lib, case, acts, **kw)
    one = protocol(G, "chain bwd", G.single, mine=G.mine, sized=False)
    two = protocol(G, "chain split", G.split, mine=G.mine)
    assert not bits_differ([(k, one[k], two[k]) for k in G.mine]) and set(G.mine) <= set(refs)
    return A.held("chain", name, G.need, dict(one, h=acts[L_]), refs)


def test_chain_builders_describe_their_case():
    assert not _chain(_case(SC.CHAIN_CASES, "d128_b8_l1"))
    assert not _chain(_case(SC.CHAIN_CASES, "d64_b8_l6_frozen2"))
    assert not _chain(_case(SC.CHAIN_CASES, "d128_b8_l1"), wfrozen=0, gbias=False, dx=False)


# ---- seeded flaws ----------------------------------------------------------------------------------------------------------------------------
FULL_BANK = _case(SC.BANK_CASES, "b16_i100_odd_total")


def test_an_entry_that_adds_gradients_and_then_refuses_is_caught():
    G = A.bank_backward(CPU, A.fake_lib("adds_then_refuses"), FULL_BANK)
    _raises("with one byte of workspace too few wrote to ['dW", lambda: protocol(G, "bank bwd", G.call, mine=G.mine))
    _raises("refusal wrote to ['dW", lambda: refused(G, "refusal", lambda: G.call(None, G.need), code=HWG_ERR_WORKSPACE))
    good = A.bank_backward(CPU, GOOD, FULL_BANK)
    refused(good, "refusal", lambda: good.call(good.ws, good.need - 1), code=HWG_ERR_WORKSPACE)


def test_a_store_behind_an_experts_weight_gradient_is_caught():
    for name in ("k8", "cin264_s3_r8"):               # 32 floats (the store lands in the padding of the buffer's last 64) and a multiple of 64 (in the canary)
        G = A.conv_setup(CPU, A.fake_lib("past_end"), _case(SC.CONV_CASES, name))
        _raises("a canary next to a buffer was overwritten", lambda: protocol(G, "wgrad", G.wgrad, mine=G.mine_wgrad))


def test_a_reduce_pass_that_sums_an_unwritten_chunk_is_caught():
    G = A.bank_backward(CPU, A.fake_lib("reduce_reads_unwritten"), FULL_BANK)
    _raises("elements of dx are not finite (never written, or written from workspace contents)", lambda: protocol(G, "bank bwd", G.call, mine=G.mine))


def test_a_frozen_layer_whose_buffer_changes_is_caught():
    G = A.bank_backward(CPU, A.fake_lib("frozen_changes"), FULL_BANK)
    assert "dW0" in G.frozen and "db0" in G.frozen and "dW3" in G.frozen and "db3" in G.mine
    _raises("wrote to a buffer it does not own", lambda: protocol(G, "bank bwd", G.call, mine=G.mine))


@pytest.mark.parametrize("name", ["w0_c1", "w6_c1"])
def test_gathers_without_the_centre_guard_are_caught_inside_the_allocation(name):
    case = _case(SC.WINDOW_CASES, name)
    _, B, Wx, C, w = case
    ib, ip, dp, good = A.window_rows(case, edge=True)
    assert set(ib[~good].tolist()) == {-1, 0, B - 1, B} and set(ip[~good].tolist()) >= {-1, Wx} and int((~good).sum()) == 6
    assert not ((ib[~good] >= 0) & (ib[~good] < B) & (ip[~good] >= 0) & (ip[~good] < Wx)).any()
    # the arithmetic: with the centre clause removed the bad rows read the slab's margin lines and write next to win_of, inside its canaries
    lo, hi, wlo, whi = A.edge_footprint(B, Wx, C, w, ib, ip, good)
    assert Wx * C <= GUARD and -Wx * C <= lo and hi < (B + 1) * Wx * C
    assert -GUARD <= wlo and whi < (B * Wx + 63) // 64 * 64 + GUARD
    lib = A.fake_lib("no_centre_guard")
    G = A.window_setup(CPU, lib, case, ib, ip, dp, margin=True)
    G2 = A.window_setup(CPU, GOOD, case, ib[good], ip[good], dp[good], margin=True)
    with_bad = protocol(G.Gg, "gather", G.Gg.call)
    _raises("a row outside the tensor gave a non-zero patches", lambda: A.edge_rows_hold("windows", with_bad, protocol(G2.Gg, "gather", G2.Gg.call), good))
    _raises("a canary next to a buffer was overwritten", lambda: protocol(G, "scatter", G.call))
    # and the guarded entries pass
    G = A.window_setup(CPU, GOOD, case, ib, ip, dp, margin=True)
    A.edge_rows_hold("windows", dict(protocol(G.Gg, "gather", G.Gg.call), dx=protocol(G, "scatter", G.call)["dx"]),
                     dict(protocol(G2.Gg, "gather", G2.Gg.call), dx=protocol(G2, "scatter", G2.call)["dx"]), good, sums=("dx",))


def test_gather_scores_without_its_guard_is_caught_inside_the_allocation():
    x, ib, ip, ic, good = A.scores_rows(edge=True)
    B, Wx, C = x.shape
    off = (ib.long() * Wx + ip.long()) * C + ic.long()
    assert Wx * C <= GUARD and int(off.min()) >= -Wx * C and int(off.max()) < (B + 1) * Wx * C and int((~good).sum()) == 8
    G = A.scores_setup(CPU, A.fake_lib("no_centre_guard"), x, ib, ip, ic, margin=True)
    Gi = A.scores_setup(CPU, GOOD, x, ib[good], ip[good], ic[good], margin=True)
    _raises("a row outside the tensor gave a non-zero out", lambda: A.edge_rows_hold("scores", protocol(G, "scores", G.call), protocol(Gi, "scores", Gi.call), good))


# ---- table layout ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_tables(monkeypatch):
    from handwriting_line_generation_amd import ops
    monkeypatch.setattr(ops, "h2d", lambda host, device, dtype=None: torch.as_tensor(host).clone())
    return ops


def _linears(G, names, shapes):
    """torch modules whose parameters (and gradients) ARE the carved buffers"""
    mods = []
    for (w, b, gw, gb), (o, i) in zip(names, shapes):
        m = torch.nn.Linear(i, o)
        m.weight.data, m.bias.data = G[0].t(w), G[0].t(b)
        m.weight.requires_grad_(gw is not None)
        m.bias.requires_grad_(gb is not None)
        m.weight.grad = G[1].t(gw) if gw is not None else None
        m.bias.grad = G[1].t(gb) if gb is not None else None
        mods.append(m)
    return mods


def test_bank_tables_have_the_layout_ops_builds(host_tables):
    case = FULL_BANK
    name, B, I, O, halves, unused, frozen, xgrad, backward = case
    Gf, Gb = A.bank_forward(CPU, GOOD, case), A.bank_backward(CPU, GOOD, case)
    names = [("W%d" % l, "b%d" % l, None if l in frozen else "dW%d" % l, None if frozen.get(l) == "all" else "db%d" % l) for l in range(len(O))]
    bank = host_tables.LinearBank(_linears((Gf, Gb), names, [(o, I) for o in O]), halves=halves)
    Ot, first, wptr, bptr, off = bank.tables(CPU, B)
    for k, t in (("O", Ot), ("first", first), ("wptr", wptr), ("bptr", bptr), ("off", off)):
        assert torch.equal(Gf.t(k), t), k
    gw, gb = bank.grad_tables(CPU)
    assert torch.equal(Gb.t("gwptr"), gw) and torch.equal(Gb.t("gbptr"), gb) and int((gw == 0).sum()) == 2 and int((gb == 0).sum()) == 1
    assert bank.total == Gf.call.args["total_outputs"] and Gb.t("dyptr").numel() == len(O) * halves and int((Gb.t("dyptr") == 0).sum()) == len(unused)


def test_chain_tables_have_the_layout_ops_builds(host_tables):
    case = _case(SC.CHAIN_CASES, "d64_b8_l6_frozen2")
    name, D, B, L_, frozen, backward = case
    Gf = A.chain_forward(CPU, GOOD, case)
    Gb = A.chain_backward(CPU, GOOD, case, torch.zeros(L_ + 1, B, D))
    names = [("W%d" % l, "b%d" % l, None if l == frozen else "dW%d" % l, None if l == frozen else "db%d" % l) for l in range(L_)]
    chain = host_tables.MLPChain(_linears((Gf, Gb), names, [(D, D)] * L_), SC.CHAIN_SLOPE)
    wptr, bptr = chain.tables(CPU)
    gw, gb = chain.grad_tables(CPU)
    assert torch.equal(Gf.t("wptr"), wptr) and torch.equal(Gf.t("bptr"), bptr) and torch.equal(Gb.t("gwptr"), gw) and torch.equal(Gb.t("gbptr"), gb)
    assert int(gw[frozen]) == 0 and int(gb[frozen]) == 0 and int((gw == 0).sum()) == 1


def test_conv_plans_are_the_ones_make_plan_builds(host_tables):
    from handwriting_line_generation_amd.model import expert_bank
    for R_ in (1, 5):
        cls = SC.plan_cls("mixed", R_)
        p = A.conv_plan(cls, R_)
        plan = expert_bank.make_plan(cls, CPU, window_rows=(R_,))
        tseg, trow, nt, _ = expert_bank.plan_tiles(plan, R_, CPU)
        wseg, wrow, wnt, wrun = expert_bank.plan_tiles(plan, R_, CPU, expert_bank.WGRAD_TILE_ROWS)
        for k, t in (("seg_start", plan["seg_start"]), ("seg_eid", plan["seg_eid"]), ("tseg", tseg), ("trow", trow), ("wseg", wseg), ("wrow", wrow), ("wrun", wrun)):
            assert p[k].dtype == np.int32 and np.array_equal(p[k], t.numpy()), k
        assert (nt, wnt, plan["G"]) == (p["tseg"].size, p["wseg"].size, p["seg_eid"].size) and (expert_bank.TILE_ROWS, p["tile_rows"]) == (SC.GT_ROWS, SC.WGRAD_TILE_ROWS)


def test_the_restated_workspace_sizes_are_the_librarys():
    from handwriting_line_generation_amd import _lib as L
    for args in ((130, 16, 100), (1, 1, 8), (128, 8, 128), (0, 3, 5), (64, -1, 8)):
        assert A.Fake.hwg_linear_bank_bwd_workspace(*args) == L.query("hwg_linear_bank_bwd_workspace", *args), args
    for args in ((6, 8, 128), (1, 16, 64), (8, 1, 128), (-2, 4, 64)):
        assert A.Fake.hwg_mlp_chain_bwd_workspace(*args) == L.query("hwg_mlp_chain_bwd_workspace", *args), args
    for args in ((11, 248, 132, 3), (1, 8, 4, 1), (-1, 8, 4, 1)):
        assert A.Fake.hwg_grouped_conv1d_wgrad_workspace(*args) == L.query("hwg_grouped_conv1d_wgrad_workspace", *args), args
