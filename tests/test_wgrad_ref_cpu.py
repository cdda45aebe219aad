"""CPU: the weight-gradient restatements (oracle/conv_ref.py: wgrad_direct, colsum, wino_wgrad) in fp64 against torch autograd (conv2d /
conv_transpose2d weight and bias gradients), the Winograd forms against the direct form, the absolute forms against the fp32 restatements' own
error (the bound of tests/test_wgrad_fp64_gpu.py is sound for the reference alone), the bookkeeping of the case table (oracle/wgrad_cases.py:
every regime of the dispatch code and every reduce variant is reached, impulse inputs carry one 1 per channel, the library's planners - which
need no GPU - give the workspace and therefore the split every case claims) and the sensitivity of the table: plausible kernel flaws, seeded into
copies of the restatements that live in this file only, each move some case past a condition the GPU file holds it to by SENSITIVITY_FACTOR or
more, or flip an exact comparison."""
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_ref as R
from oracle import wgrad_cases as WC
import _wgrad_checks as G  # the references and bounds the GPU file holds the device to
from _fp64 import _ratio, cpu_threads

SENSITIVITY_FACTOR = 10.0
TOL = 1e-10


cpu_threads()
ENGINES = ["mfma", "tapn", "narrow", "c1rows", "c1valu", "direct", "wino", "s2"]


def _close(a, b, what=""):
    assert tuple(a.shape) == tuple(b.shape), (what, tuple(a.shape), tuple(b.shape))
    scale = max(float(b.abs().max()), 1.0)
    assert float((a.double() - b.double()).abs().max()) <= TOL * scale, "%s: %.3e" % (what, float((a.double() - b.double()).abs().max()))


def _autograd(c, u, v):
    """torch's own fp64 weight and bias gradient of the layer the descriptor belongs to: -> (dw [R,S,K,C], column sums of u)"""
    N, H, W, C, K, Rr, S = c["shape"]
    nchw = lambda t: t.permute(0, 3, 1, 2)
    if "transposed_layer" in c["tags"]:                  # anchor = the layer input [N,P,Q,K = Cin], gathered = dy [N,H,W,C = Kout]
        w = torch.zeros(K, C, Rr, S, dtype=torch.double, requires_grad=True)
        y = F.conv_transpose2d(nchw(u), w, None, c["stride"], c["pad"], (H - R.out_size(c["P"], c["Q"], Rr, S, c["stride"], c["pad"], (1, 1), 1)[0],
                                                                        W - R.out_size(c["P"], c["Q"], Rr, S, c["stride"], c["pad"], (1, 1), 1)[1]))
        y.backward(nchw(v))
        return w.grad.permute(2, 3, 0, 1), None
    w = torch.zeros(K, C, Rr, S, dtype=torch.double, requires_grad=True)
    b = torch.zeros(K, dtype=torch.double, requires_grad=True)
    F.conv2d(nchw(v), w, b, c["stride"], c["pad"], c["dil"]).backward(nchw(u))
    return w.grad.permute(2, 3, 0, 1), b.grad


# ---- the restatements against torch, and the bound against the fp32 restatement ----------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_restatements_match_autograd_and_bound_their_own_fp32_error(engine):
    d = lambda t: None if t is None else t.double()
    checked = 0
    for c in WC.of_engine(engine):
        u, v, dw0, db0 = WC.inputs(c)
        N, H, W, C, K, Rr, S = c["shape"]
        refs = G.reference(c)
        for s, (ref, yard, bound, rb, yb, bb) in enumerate(refs):
            us, vs = WC.operands(c, u, v, s)
            w0 = None if dw0 is None else dw0[s]
            assert tuple(ref.shape) == (Rr, S, K, C)
            if WC.pixels(c) * K * C * Rr * S <= 6e7 and s == 0:          # torch's fp64 convolution backward is slow: the small cases of every engine
                dw, db = _autograd(c, d(us), d(vs))
                _close(ref - (0 if w0 is None else d(w0)), dw, c["name"] + " direct form")
                if db is not None:
                    _close(R.colsum(d(us)), db, c["name"] + " column sums")
                checked += 1
            if engine in ("wino", "s2"):
                _close(G.restate(c, d(us), d(vs), d(w0)), ref, c["name"] + " Winograd form")
            # A dominates the fp32 restatement's own error: the bound is sound for the reference alone
            r = _ratio(G.restate(c, us, vs, w0), ref, bound)
            assert r <= 1.0, "%s: the fp32 restatement is %.3g x the bound off" % (c["name"], r)
            assert yard > 0
            if rb is not None:
                b0 = None if db0 is None else db0[s]
                assert _ratio(R.colsum(us, b0), rb, bb) <= 1.0 and yb > 0, c["name"]
    assert checked >= 3, engine


def test_transposed_layers_are_held_to_conv_transpose2d():
    cs = [c for c in WC.CASES if "transposed_layer" in c["tags"]]
    assert len(cs) >= 2 and any("output_padding" in c["tags"] for c in cs)
    for c in cs:
        u, v, _, _ = WC.inputs(c)
        dw, _ = _autograd(c, u[0].double(), v[0].double())
        _close(R.wgrad_direct(u[0].double(), v[0].double(), WC.geom(c)), dw, c["name"])


def test_colsum_restatement():
    for rows, C, acc in WC.COLSUM_CASES:
        x, out0 = WC.colsum_input(rows, C, acc)
        want = x.double().sum(0) + (0 if out0 is None else out0.double())
        _close(R.colsum(x.double(), None if out0 is None else out0.double()), want)
        assert bool((R.colsum(x.double(), None if out0 is None else out0.double(), absolute=True) >= want.abs() - 1e-9).all())


# ---- bookkeeping of the table -----------------------------------------------------------------------------------------------------------------
_PX = ["px<step", "px_whole", "px_whole+1", "ranges1", "ranges2", "ranges_many", "ragged_last"]
REQUIRED = {
    "mfma": ["mfma32", "mfma64", "mfma128", "1x1", "3x3p0", "3x3p1", "3x3p2", "1x3d4", "4x4s2p1", "4x4s21", "5x5p2", "d21", "3x3s31_onerow", "transposed_layer",
             "output_padding", "layout_kc", "layout_ck", "layout_pad", "K<tile", "C<tile", "K=tile+4", "C=tile+4", "K_tiles_ragged", "C_tiles_ragged",
             "red_VEC4", "red_LANES4", "rows_off", "ck_256", "sets2", "sets3", "sets8", "set_on_v0", "set_on_v1"] + _PX
            + ["red_ROWS_%s_%d" % (t, sl) for t in ("9", "16", "3", "other") for sl in (1, 4)],
    "tapn": ["tapn", "K<tile", "K=tile+4", "K_tiles_ragged", "k64_below_4096", "k64_rows_off", "64taps", "red_SCALAR", "red_LANES4", "red_LANES32", "layout_ck",
             "sets2", "sets3", "sets8", "set_on_v0", "set_on_v1"] + _PX,
    "narrow": ["narrow<3>", "narrow<4>", "blocks1", "blocks2", "blocks4", "px16384", "px16384+ragged", "pad0", "pad1", "pad2", "3x3s21", "4x4s2", "4x4s21", "mode2",
               "red_LANES32", "sets2", "sets3", "sets8", "set_on_v0", "set_on_v1"],
    "c1rows": ["c1_rows<3>", "c1_rows<5>", "c1_rows<7>", "Q<128", "Q=128", "Q>128", "ragged_segment", "pad0", "pad1", "pad2", "pad3", "segments<512",
               "segments>512", "sets2", "sets3", "sets8", "set_on_v0", "set_on_v1"],
    "c1valu": ["c1<3>", "c1<5>", "c1<7>", "stride2", "dil2", "px%64", "waves>groups"],
    "direct": ["direct<0>", "direct<1>", "K1", "K2", "K8", "K92", "C4", "C12", "C64", "C1024", "px1", "px511", "px512", "px513", "block_cap", "taps_per_thread1",
               "taps_per_thread4", "taps_per_thread8"],
    "wino": ["Qmod4=0", "Qmod4=1", "Qmod4=2", "Qmod4=3", "oddP", "pad0", "pad1", "pad2", "ranges1", "ranges2", "ranges3", "one_round_per_range",
             "padding_workgroups", "layout_ck", "red_ROWS_9_4", "sets2", "sets3"],
    "s2": ["evenHW", "oddHW", "4C_ragged", "ranges1", "ranges2", "ranges3", "sets2", "sets3"]}


def test_table_reaches_every_required_regime():
    for engine, tags in REQUIRED.items():
        have = set().union(*(c["tags"] for c in WC.of_engine(engine)))
        assert not set(tags) - have, "%s: no case reaches %s" % (engine, sorted(set(tags) - have))
    # every tile of the MFMA kernel meets every pixel regime
    for kern in ("mfma32", "mfma64", "mfma128", "tapn"):
        have = set().union(*(c["tags"] for c in WC.CASES if kern in c["tags"]))
        assert not set(_PX) - have, "%s: no case reaches %s" % (kern, sorted(set(_PX) - have))
        geoms = {g[0] for g in WC.GEOMETRIES}
        assert len(geoms) == 10 and not geoms - have, "%s: no case has the taps %s" % (kern, sorted(geoms - have))
    kernel_of = {"mfma": ("mfma32", "mfma64", "mfma128"), "tapn": ("tapn",), "narrow": ("narrow<3>", "narrow<4>"), "c1rows": ("c1_rows<3>", "c1_rows<5>", "c1_rows<7>"),
                 "c1valu": ("c1<3>", "c1<5>", "c1<7>"), "direct": ("direct<0>", "direct<1>"), "wino": ("wino_wgrad",), "s2": ("wino_wgrad",)}
    for c in WC.CASES:
        p = WC.plan(c)
        assert p["kernel"] in kernel_of[c["engine"]], (c["name"], p["kernel"])
        assert (c["engine"] == "s2") == (p["last_plan"] == (7, 36, p["nsplit"])), c["name"]
        assert c["shape"][0] <= 4 and (WC.pixels(c) <= 20000 or "large" in c["tags"]), c["name"]
        assert ("transposed_layer" in c["tags"]) <= (c["stride"] != (1, 1)), c["name"]
        if c["engine"] == "wino":
            assert WC.plan_wino_wgrad(c)[6] == 2, c["name"]
        if "ck_256" in c["tags"] or "rows_off" in c["tags"]:
            assert c["shape"][3] * c["shape"][4] >= 65536 and p["nsplit"] <= 16 and p["reduce"][0] != "ROWS", c["name"]
        if p["ranges"]:                                                            # the pixel ranges tile the anchor pixels
            assert p["ranges"][0][0] == 0 and p["ranges"][-1][1] == WC.pixels(c) and all(a[1] == b[0] for a, b in zip(p["ranges"], p["ranges"][1:])), c["name"]
    assert {c["layout"] for c in WC.CASES} == {"kc", "ck", "pad"}
    assert sum("large" in c["tags"] for c in WC.CASES) == 1
    for e in ("mfma", "tapn", "narrow", "c1rows", "wino", "s2"):                  # every combination of accumulate / bias / bias-accumulate that exists
        assert {(c["acc"], c["bias"]) for c in WC.of_engine(e)} == {(a, b) for a in (False, True) for b in (False, True)}, e
        assert any(c["bias_acc"] for c in WC.of_engine(e)), e
    assert {(c["acc"]) for c in WC.of_engine("direct")} == {False, True} and not any(c["bias"] for c in WC.of_engine("direct"))
    assert WC.plan_wd(WC.BY_NAME["direct1_k92_9x9"]) and not WC.plan_wd(dict(WC.BY_NAME["direct1_k92_9x9"], shape=(1, 9, 57, 1, 96, 9, 9)))   # the widest K


def test_impulse_inputs_carry_one_pixel_per_channel_and_cover_the_sites():
    for name in WC.INDEX_CASES:
        c = WC.BY_NAME[name]
        K, M = c["shape"][4], WC.pixels(c)
        sites = WC.impulse_pixels(c)
        have, p = {m for _, m in sites}, WC.plan(c)
        assert {0, c["Q"] - 1, M - 1} <= have, name
        if p["ranges"]:                                      # the first and the last pixel of the first and of the last range that holds pixels
            rng = [r for r in p["ranges"] if r[1] > r[0]]
            assert {rng[0][0], rng[0][1] - 1, rng[-1][0], rng[-1][1] - 1} <= have, name
        elif c["engine"] in ("wino", "s2"):
            assert {p["first_pixel"](lo) for lo, hi in p["pair_ranges"][:4] if hi > lo} <= have, name
        passes = WC.impulse_passes(c)
        assert sorted(m for ps in passes for _, m in ps) == sorted(m for _, m in sites) and all(0 <= m < M for _, m in sites), name
        for ps in passes:
            u = WC.impulse_u(c, ps)
            assert float(u.sum()) == len(ps) and float(u.reshape(-1, K).sum(0).max()) <= 1.0, name     # the rows of two channels never collide
        assert len(passes) <= 16, name
    kernels = {WC.plan(WC.BY_NAME[n])["kernel"] for n in WC.INDEX_CASES}
    assert kernels >= {"mfma32", "mfma64", "mfma128", "tapn", "narrow<3>", "narrow<4>", "c1_rows<3>", "c1_rows<7>", "c1<5>", "direct<0>", "direct<1>", "wino_wgrad"}
    assert {WC.BY_NAME[n]["engine"] for n in WC.INDEX_CASES} == set(ENGINES)
    assert any(WC.BY_NAME[n]["sets"] > 1 for n in WC.INDEX_CASES)


def test_planner_facts_need_no_launch():
    """the library's own queries (host code, no device needed) give the workspace - and with it the split - every case claims"""
    from handwriting_line_generation_amd import _lib as L, ops
    for c in WC.CASES:
        N, H, W, C, K, Rr, S = c["shape"]
        p = WC.plan(c)
        with ops.tuning(**c["env"]):
            d = ops._desc(N, H, W, C, K, Rr, S, c["stride"], c["pad"], c["dil"], c["P"], c["Q"], 0)
            entry, query = WC.entry(c)
            need = int(L.query(query, d.ptr, c["sets"]) if c["sets"] > 1 else L.query(query, d.ptr))
            assert need == p["ws"], (c["name"], need, p["ws"])
            per_image = (Rr * S * K * C + (0 if c["engine"] == "direct" else K)) * 4
            assert need == c["sets"] * p["nsplit"] * per_image, c["name"]
            if c["engine"] in ("wino", "s2"):
                assert L.query("hwg_wino_wgrad_supported", d.ptr) == 1, c["name"]
                assert int(L.query("hwg_wino_wgrad_sets_workspace", d.ptr, 1)) == int(L.query("hwg_wino_wgrad_workspace", d.ptr)), c["name"]
            else:
                assert L.query("hwg_conv_wgrad_sets_supported", d.ptr) == (0 if c["engine"] == "direct" else 1), c["name"]
                if c["engine"] != "direct":
                    assert int(L.query("hwg_conv_wgrad_sets_workspace", d.ptr, 1)) == int(L.query("hwg_conv_wgrad_workspace", d.ptr)), c["name"]
    for shape, want in WC.SETS_SUPPORTED:
        N, H, W, C, K, Rr, S = shape
        d = ops._desc(N, H, W, C, K, Rr, S, (1, 1), (Rr // 2, S // 2), (1, 1), H, W, 0)
        assert L.query("hwg_conv_wgrad_sets_supported", d.ptr) == want, shape
        if not want:
            assert int(L.query("hwg_conv_wgrad_sets_workspace", d.ptr, 2)) == 0 or not WC.is_direct(C, K, Rr * S), shape
    for name, geo, opt in WC.REFUSALS:
        if opt.get("wino") and "sets" not in opt:
            N, H, W, C, K, Rr, S = geo["shape"]
            d = ops._desc(N, H, W, C, K, Rr, S, (1, 1), geo["pad"], (1, 1), H, W, 0)
            assert L.query("hwg_wino_wgrad_supported", d.ptr) == 0 and int(L.query("hwg_wino_wgrad_workspace", d.ptr)) == 0, name
    for rows, C, acc in WC.COLSUM_CASES:
        assert int(L.query("hwg_colsum_workspace", rows, C)) == WC.colsum_chunks(rows) * C * 4
    assert {WC.colsum_chunks(r) for r, _, _ in WC.COLSUM_CASES} >= {1, 2, 256} and any(r > 256 * 256 for r, _, _ in WC.COLSUM_CASES)
    assert {C for _, C, _ in WC.COLSUM_CASES} >= {1, 2, 3, 4, 5, 64, 68}


# ---- sensitivity: flawed copies of the restatements (this file only) ---------------------------------------------------------------------------
def _direct_copy(c, u, v, dw0=None, ranges=None, offsets=None, clamp_columns=False):
    """wgrad_direct again, by index: offsets(r, s) -> (row offset, column offset) of the tap; clamp_columns reads a padding column from the clamped
    neighbour instead of zero"""
    N, P, Q, K = u.shape
    H, W, C = v.shape[1:]
    (sh, sw), (ph, pw), (dh, dw_), Rr, S = c["stride"], c["pad"], c["dil"], c["shape"][5], c["shape"][6]
    offsets = offsets or (lambda r, s: (r * dh, s * dw_))
    M = N * P * Q
    um = u.reshape(M, K)
    cols = []
    for r in range(Rr):
        for s in range(S):
            oh, ow = offsets(r, s)
            ih, iw = torch.arange(P) * sh - ph + oh, torch.arange(Q) * sw - pw + ow
            okh, okw = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
            if clamp_columns:
                okw = torch.ones_like(okw)
            t = v[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)] * (okh[:, None] & okw[None, :])[None, :, :, None].to(v.dtype)
            cols.append(t.reshape(M, C))
    dw = 0
    for m0, m1 in (ranges or [(0, M)]):
        dw = dw + torch.stack([um[m0:m1].t() @ col[m0:m1] for col in cols]).reshape(Rr, S, K, C)
    return dw if dw0 is None else dw + dw0


def _wino_copy(c, dy, x, flaw):
    """_wino_wgrad_tiles of the 3x3 form again, with one flaw"""
    N, P, Q, K = dy.shape
    H, W, C = x.shape[1:]
    pad, m = c["pad"], 2
    TP, TQ = -(-P // m), -(-Q // m)
    dyp = dy.new_zeros((N, TP * m, TQ * m, K))
    dyp[:, :P, :Q] = dy
    if flaw == "wino_edge_tile_not_masked":                 # the column past the row's end is the next row's first pixel in memory
        flat = torch.cat([dy.reshape(-1, K), dy.new_zeros((TQ * m, K))])
        for q in range(Q, TQ * m):
            idx = (torch.arange(N)[:, None] * P + torch.arange(P)[None, :]) * Q + q
            dyp[:, :P, q] = flat[idx]
    t = dyp.reshape(N, TP, m, TQ, m, K)
    xp = x.new_zeros((N, max(H + 2 * pad[0], m * TP + 2), max(W + 2 * pad[1], m * TQ + 2), C))
    xp[:, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = x
    d = xp.unfold(1, 4, m).unfold(2, 4, m)[:, :TP, :TQ]
    Am, Bm, Gm = torch.tensor(R.AT_23, dtype=dy.dtype).t(), torch.tensor(R.BT_23, dtype=dy.dtype), torch.tensor(R.G_23, dtype=dy.dtype)
    Z = torch.einsum("jb,ntqkib->ntqkij", Am, torch.einsum("ia,ntaqbk->ntqkib", Am, t))
    V = torch.einsum("jb,ntqcib->ntqcij", Bm, torch.einsum("ia,ntqcab->ntqcib", Bm, d))
    dU = torch.einsum("ntqkij,ntqcij->ijkc", Z, V)
    G1 = Gm.clone()
    if flaw == "G_where_G^T_belongs":                       # the square block of the first stage's matrix transposed
        G1[:3] = Gm[:3].t()
    return torch.einsum("js,rjkc->rskc", Gm, torch.einsum("ir,ijkc->rjkc", G1, dU))


def flawed(c, u, v, dw0, flaw, s=0):
    """dw of set s of the case in fp64 with one plausible kernel flaw"""
    us, vs = WC.operands(c, u, v, s)
    w0 = None if dw0 is None else dw0[s]
    rng = WC.plan(c)["ranges"]
    (sh, sw), (dh, dw_) = c["stride"], c["dil"]
    if flaw == "no_flaw":
        return _direct_copy(c, us, vs, w0, ranges=rng)
    if flaw == "last_pixel_of_a_range_dropped":
        return _direct_copy(c, us, vs, w0, ranges=[(rng[0][0], rng[0][1] - 1)] + rng[1:])
    if flaw == "ragged_last_range_counted_twice":
        return _direct_copy(c, us, vs, w0, ranges=rng + rng[-1:])
    if flaw == "padding_column_from_clamped_neighbour":
        return _direct_copy(c, us, vs, w0, clamp_columns=True)
    if flaw == "one_partial_image_left_out":
        return _direct_copy(c, us, vs, w0, ranges=rng[:2] + rng[3:])
    if flaw == "r_and_s_swapped":
        return _direct_copy(c, us, vs, w0, offsets=lambda r, s_: (s_ * dh, r * dw_))
    if flaw == "stride_and_dilation_swapped":
        return _direct_copy(dict(c, stride=c["dil"], dil=c["stride"]), us, vs, w0)
    if flaw == "sa_and_sb_swapped":
        n, sa, sb, sr, ss = WC.dw_strides(c)
        buf = torch.zeros(n, dtype=us.dtype)
        buf[WC.dw_index(dict(c, layout="ck" if c["layout"] == "kc" else "kc")).reshape(-1)] = _direct_copy(c, us, vs, w0).reshape(-1)
        return buf[WC.dw_index(c)]
    if flaw == "dw0_ignored_under_accumulate":
        return _direct_copy(c, us, vs, None)
    if flaw == "set_1_reads_the_anchor_of_set_0":
        return _direct_copy(c, u[0], vs, w0)
    if flaw in ("wino_edge_tile_not_masked", "G_where_G^T_belongs"):
        return _wino_copy(c, us, vs, flaw) + (0 if w0 is None else w0)
    raise KeyError(flaw)


FLAWS = {  # flaw -> (case it is seeded into, set)
    "last_pixel_of_a_range_dropped": ("t32_px129_3x3p0", 0), "ragged_last_range_counted_twice": ("t32_px1155_1x3d4", 0),
    "padding_column_from_clamped_neighbour": ("t32_px128_3x3p1", 0), "one_partial_image_left_out": ("t64_px385_k68_c132", 0),
    "r_and_s_swapped": ("t32_px1155_1x3d4", 0), "stride_and_dilation_swapped": ("t32_dil21", 0), "sa_and_sb_swapped": ("t32_px129_3x3p0", 0),
    "dw0_ignored_under_accumulate": ("t32_px128_3x3p1", 0), "set_1_reads_the_anchor_of_set_0": ("sets2_t32", 1),
    "wino_edge_tile_not_masked": ("wino_q9_k48_c80_split2", 0), "G_where_G^T_belongs": ("wino_q8_k16_c16", 0)}


def test_every_seeded_flaw_moves_a_case_past_its_bound():
    assert len(FLAWS) + 1 >= 12
    for flaw, (name, s) in FLAWS.items():
        c = WC.BY_NAME[name]
        u, v, dw0, _ = (None if t is None else t.double() for t in WC.inputs(c))
        ref, yard, bound = G.reference(c)[s][:3]
        with_flaw = _ratio(flawed(c, u, v, dw0, flaw, s), ref, bound)
        clean = "no_flaw" if c["engine"] not in ("wino", "s2") else None
        without = _ratio(flawed(c, u, v, dw0, clean, s), ref, bound) if clean else _ratio(_wino_copy(c, *WC.operands(c, u, v, s), None) + (0 if dw0 is None else dw0[s]), ref, bound)
        print("%-40s moves %-26s to %.3g x the bound (without the flaw: %.3g)" % (flaw, name, with_flaw, without))
        assert without <= 1.0, "%s: the copy without the flaw is off the reference" % flaw
        assert with_flaw >= SENSITIVITY_FACTOR, "%s: moves its case by only %.3g x the bound" % (flaw, with_flaw)


def test_bias_sum_missing_one_lane_half_is_caught():
    """wgrad_c1_rows_kernel sums the anchor's columns in two 32-lane halves (even and odd pixels of a segment): one of them left out"""
    c = WC.BY_NAME["c1rows_5x5_q128_p1"]
    assert c["bias"]
    u, _, _, db0 = (None if t is None else t.double() for t in WC.inputs(c))
    rb, yb, bb = G.reference(c)[0][3:]
    half = R.colsum(u[0][:, :, 0::2], None if db0 is None else db0[0])
    assert _ratio(R.colsum(u[0], None if db0 is None else db0[0]), rb, bb) <= 1.0
    assert _ratio(half, rb, bb) >= SENSITIVITY_FACTOR


def test_impulse_comparison_flips_under_index_flaws():
    """the exact comparison of the impulse test: a dropped pixel is a row of zeros, a wrong tap another element of v, bit for bit"""
    for name, flaws in (("t32_px129_3x3p0", ("last_pixel_of_a_range_dropped", "sa_and_sb_swapped")), ("t32_px1155_1x3d4", ("r_and_s_swapped",)),
                        ("t32_4x4s2p1", ("stride_and_dilation_swapped", "padding_column_from_clamped_neighbour"))):
        c = dict(WC.BY_NAME[name], acc=False, bias_acc=False)
        _, v, _, _ = WC.inputs(c)
        hit = {f: False for f in flaws}
        for ps in WC.impulse_passes(c):
            u = WC.impulse_u(c, ps)
            want = R.wgrad_direct(u[0].double(), v[0].double(), WC.geom(c)).float()
            assert torch.equal(R.wgrad_direct(u[0], v[0], WC.geom(c)), want) and torch.equal(flawed(c, u.double(), v.double(), None, "no_flaw").float(), want)
            for f in flaws:
                hit[f] |= not torch.equal(flawed(c, u.double(), v.double(), None, f).float(), want)
        assert all(hit.values()), (name, hit)
