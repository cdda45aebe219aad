"""CPU: the restatements of the forward-type convolution products (oracle/conv_ref.py) against torch's own fp64 conv2d / conv_transpose2d and
autograd, the Winograd forms against the direct form, the absolute forms against the fp32 restatements' own error (the bound of
tests/test_conv_fp64_gpu.py is sound for the reference alone), the bookkeeping of the case tables (oracle/conv_cases.py: every regime of the
dispatch code is reached, impulse footprints are disjoint, the library's planners - which need no GPU - give the schedule, split and
workspace every case claims) and the sensitivity of the tables: plausible kernel flaws, seeded into copies of the restatements that live in
this file only, each move some case past the bound the GPU file holds it to by SENSITIVITY_FACTOR or more, or flip an exact comparison."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_cases as CC
from oracle import conv_ref as R
import _conv_checks as G  # the references and bounds the GPU file holds the device to
from _fp64 import _ratio, cpu_threads

SENSITIVITY_FACTOR = 10.0
TOL = 1e-10


cpu_threads()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _close(a, b, what=""):
    assert tuple(a.shape) == tuple(b.shape), (what, tuple(a.shape), tuple(b.shape))
    scale = max(float(b.abs().max()), 1.0)
    assert float((a.double() - b.double()).abs().max()) <= TOL * scale, "%s: %.3e" % (what, float((a.double() - b.double()).abs().max()))


def _torch_value(c, x, w, b, y0):
    """torch's own fp64 convolution of the case"""
    if not c["transposed"]:
        y = F.conv2d(_nchw(x), w.permute(2, 3, 0, 1), b, c["stride"], c["pad"], c["dil"])
    else:
        y = F.conv_transpose2d(_nchw(x), w.permute(3, 2, 0, 1), b, c["stride"], c["pad"], c["opad"])
    y = _nhwc(y)
    return y if y0 is None else y + y0


# ---- the restatements against torch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["mfma", "c1", "to1", "wino", "s2"])
def test_restatements_match_torch_and_bound_their_own_fp32_error(engine):
    for c in CC.of_engine(engine):
        x, w, b, y0 = CC.inputs(c)
        d = lambda t: None if t is None else t.double()
        ref, yard, bound = G.reference(c)
        assert tuple(ref.shape) == (c["shape"][0], c["P"], c["Q"], c["shape"][4])
        _close(ref, _torch_value(c, d(x), d(w), d(b), d(y0)), c["name"] + " direct form")
        if engine in ("wino", "s2"):
            _close(G.restate(c, d(x), d(w), d(b), d(y0)), ref, c["name"] + " Winograd form")
        # A (A_w) dominates the fp32 restatement's own error: the bound is sound for the reference alone
        r = _ratio(G.restate(c, x, w, b, y0), ref, bound)
        assert r <= 1.0, "%s: the fp32 restatement is %.3g x the bound off" % (c["name"], r)
        assert yard > 0


def test_data_gradient_descriptions_match_autograd():
    """the two-tap data gradient and the flipped / transposed-stride weight images describe what autograd computes"""
    g = torch.Generator().manual_seed(3)
    for c in [k for k in CC.of_engine("s2") if k["transposed"]]:
        dy, w, _, _ = (None if t is None else t.double() for t in CC.inputs(c))
        src, Kc, Cc, dgrad = CC.s2_source(c, w)
        xin = torch.zeros(c["shape"][0], Cc, c["P"], c["Q"], dtype=torch.double, requires_grad=True)
        F.conv2d(xin, src.reshape(Kc, Cc, 4, 4), None, 2).backward(_nchw(dy))
        _close(R.wino_s2_conv(dy, w, CC.geom(c)), _nhwc(xin.grad), c["name"])
        _close(R.unlayout(R.wino_s2_image(src, Kc, Cc, Cc * 16, 16, 1, absolute=True), 4 * Cc, Kc), R.filter_transform(R.s2_taps(w, 1), R.G_32, True), c["name"] + " image")
    # 3x3: dx of conv2d(x, wt [K,C,3,3]) is the correlation of dy with the image packed from wt with flip = 1 and the [C,K] strides swapped
    K, C = 6, 5
    wt = torch.randn(K, C, 3, 3, generator=g, dtype=torch.double)
    x = torch.randn(2, C, 7, 9, generator=g, dtype=torch.double, requires_grad=True)
    dy = torch.randn(2, K, 7, 9, generator=g, dtype=torch.double)
    F.conv2d(x, wt, None, 1, 1).backward(dy)
    img = R.pack_image(wt, C, K, K, 3, 3, 9, C * 9, 3, 1, 1)                   # A = C (outputs of THIS product), B = K
    geo = dict(stride=(1, 1), pad=(1, 1), dil=(1, 1), P=7, Q=9, transposed=0)
    _close(R.conv_direct(_nhwc(dy), img.reshape(3, 3, C, K), geo), _nhwc(x.grad), "flipped image = data gradient")
    U = R.unlayout(R.wino_image(wt, C, K, 9, C * 9, 3, 1, 1), C, K)
    _close(R.wino_conv(_nhwc(dy), img.reshape(3, 3, C, K), geo, U=U), _nhwc(x.grad), "flipped Winograd image = data gradient")
    # stride-2 transposed layer = data gradient of the stride-2 convolution
    xs = torch.randn(2, C, 9, 11, generator=g, dtype=torch.double, requires_grad=True)
    ys = F.conv2d(xs, wt[:, :, :, :].repeat(1, 1, 2, 2)[:, :, :4, :4].contiguous(), None, 2, 1)
    dys = torch.randn(ys.shape, generator=g, dtype=torch.double)
    ys.backward(dys)
    w4 = wt.repeat(1, 1, 2, 2)[:, :, :4, :4].permute(2, 3, 1, 0).contiguous()       # logical [4,4,K'=C,C'=K]
    geo = dict(stride=(2, 2), pad=(1, 1), dil=(1, 1), P=9, Q=11, transposed=1)
    _close(R.conv_direct(_nhwc(dys), w4, geo), _nhwc(xs.grad), "fractionally strided product = data gradient (with the output-size slack)")


def test_weight_image_restatements():
    for name, A, B, Bpad, R_, S_, layout, flip in CC.PACK_CASES:
        src, sa, sb, sr, ss = CC.pack_source(name, A, B, R_, S_, layout)
        img = R.pack_image(src, A, B, Bpad, R_, S_, sa, sb, sr, ss, flip)
        t = src.reshape(A, B, R_, S_) if layout == "ab" else src.reshape(B, A, R_, S_).transpose(0, 1)
        if flip:
            t = t.flip(2, 3)
        assert torch.equal(img[:, :, :B], t.permute(2, 3, 0, 1).reshape(R_ * S_, A, B)) and bool((img[:, :, B:] == 0).all())
    for c in CC.of_engine("wino")[:6]:
        _, w, _, _ = CC.inputs(c)
        src, sa, sb, flip = CC.wino_source(c, w)
        K, C = w.shape[2], w.shape[3]
        img = R.wino_image(src.double(), K, C, sa, sb, 3, 1, flip)
        assert img.numel() == 16 * R.ceil16(K) * R.ceil16(C)
        _close(R.unlayout(img, K, C), R.filter_transform(w.double(), R.G_23), c["name"] + " image")


# ---- bookkeeping of the tables ----------------------------------------------------------------------------------------------------------------
REQUIRED = {
    "mfma": ["tile128x128", "tile128x64", "tile128x32", "tile64x64", "M<bm", "M=bm", "M=bm+1", "M>8bm", "K4", "K78", "K80", "K130", "C16", "C32", "C48",
             "C96", "1x1", "1x3d4", "3x3p0", "3x3p1", "3x3p2", "3x3s31", "4x4s2", "4x4s21", "5x5p2", "d21", "split2", "split3", "split4", "split6",
             "split_scalar", "byclass", "merged", "t4x4s2p0", "t4x4s2p1", "ts21", "t6x3s31", "topad", "tonerow", "t3x3s2", "tk24"],
    "c1": ["rows", "q127", "q128", "q129", "pad0", "pad1", "pad2", "pad3", "c1mfma", "6x6", "7x7d12", "7x7s2", "8x8", "tp50", "valu", "k3", "k5", "k80",
           "k256", "k32_4x4s2", "9x9", "second_trip"],
    "to1": ["lpp4", "E<=4", "lpp16", "lanes4", "lanes16", "3x3kernel", "12of16", "lpp64", "c20", "stride2", "dil2", "pad0", "second_trip", "k2"],
    "wino": ["cfg%d_ns%d" % (cfg, ns) for cfg in (0, 1, 2, 5, 6, 7) for ns in (1, 2, 4)] + ["K18", "K34", "K50", "K66", "K78", "M=tm+1", "M<tm", "P1_H3",
                                                                                         "P1_H1", "pad00", "pad11", "pad22", "bal_pieces1", "bal_pieces2",
                                                                                         "bal_pieces3+", "bal_reduce1", "bal_reduce4", "acc_uniform",
                                                                                         "acc_split", "acc_bal"],
    "s2": ["fwd", "dgrad", "K64", "K80", "K96", "ragged3", "split", "bal_cut", "acc_dgrad"]}


def test_tables_reach_every_required_regime():
    for engine, tags in REQUIRED.items():
        have = set().union(*(c["tags"] for c in CC.of_engine(engine)))
        assert not set(tags) - have, "%s: no case reaches %s" % (engine, sorted(set(tags) - have))
    assert all(c["shape"][0] <= 4 for c in CC.CASES)
    assert all(CC.out_numel(c) <= 2.2e6 or "large" in c["tags"] for c in CC.CASES)
    assert sum("large" in c["tags"] for c in CC.CASES) == 3
    # bias / no bias and accumulate / overwrite on every tile and on split, by-class and merged
    for tag in ["tile%dx%d" % t for t in CC.TILES] + ["split", "byclass", "merged"]:
        cs = [c for c in CC.of_engine("mfma") if tag in c["tags"]]
        assert {c["bias"] for c in cs} == {True, False} and {c["acc"] for c in cs} == {True, False}, tag
    # the tags say what the shapes are
    for c in CC.of_engine("mfma"):
        bm = CC._force(c)[0]
        M, t = CC.mfma_M(c), c["tags"]
        assert ("M<bm" in t) <= (M < bm) and ("M=bm" in t) <= (M == bm) and ("M=bm+1" in t) <= (M == bm + 1) and ("M>8bm" in t) <= (M > 8 * bm and M % bm != 0), c["name"]
        assert ("split" in t) == (CC.mfma_plan(c)[0][2] > 1) and ("merged" in t) == (CC.mfma_mode(c) == 2) and ("byclass" in t) == (CC.mfma_mode(c) == 1), c["name"]
        assert ("split_scalar" in t) <= (c["shape"][4] % 4 != 0)
        assert ("topad" in t) <= (c["opad"] != (0, 0)) and ("tonerow" in t) <= (c["shape"][1] == 1)
    for c in CC.of_engine("c1"):
        kern = CC.c1_kernel(c)
        assert {"c1_rows": "rows", "c1_mfma": "c1mfma", "c1": "valu"}[kern] in c["tags"], (c["name"], kern)
        N, H, W, C, K, Rr, S = c["shape"]
        if "second_trip" in c["tags"]:
            assert (kern == "c1_rows" and N * c["P"] * -(-c["Q"] // 128) > 2048) or (kern == "c1_mfma" and -(-N * c["P"] * c["Q"] // 128) > 768), c["name"]
        assert ("tp50" in c["tags"]) <= (Rr * S == 49)
        for q in (127, 128, 129):
            assert ("q%d" % q in c["tags"]) <= (c["Q"] == q), c["name"]
        if kern == "c1":
            assert c["Q"] % (4 * (256 // ((K + 3) // 4))) != 0, c["name"]
    assert CC.c1_kernel(CC.REFUSED) == "refused"
    for c in CC.of_engine("to1"):
        kern, lpp, blocks = CC.to1_kernel(c)
        t = c["tags"]
        assert ("3x3kernel" in t) == (kern == "to1_3x3") and ("lpp4" in t or "lanes4" in t) == (kern == "to1" and lpp == 4), c["name"]
        assert ("lpp64" in t) == (kern == "to1" and lpp == 64) and ("lpp16" in t or "lanes16" in t) <= (lpp == 16), c["name"]
        assert ("second_trip" in t) == (c["shape"][0] * c["P"] * c["Q"] * lpp // 64 // 4 > 4096), c["name"]
    for c in CC.of_engine("wino"):
        desc, plan, ws, per = CC.wino_plan(c)
        t, M = c["tags"], c["shape"][0] * -(-c["P"] // 2) * -(-c["Q"] // 2)
        tm = {0: 64, 1: 32, 2: 128, 5: 64, 6: 64, 7: 32}[desc[0]]
        assert ("M=tm+1" in t) <= (M == tm + 1) and ("M<tm" in t) <= (M < tm), c["name"]
        assert ("P1_H3" in t) <= (c["P"] == 1 and c["shape"][1] == 3) and ("P1_H1" in t) <= (c["P"] == 1 and c["shape"][1] == 1), c["name"]
        if "bal" in t:
            assert ("bal_pieces1" in t) == (max(per) == 1) and ("bal_pieces2" in t) <= (max(per) == 2) and ("bal_pieces3+" in t) <= (max(per) >= 3), (c["name"], per)
            assert ("bal_reduce1" in t) <= (c["shape"][4] % 4 != 0 and max(per) > 1) and ("bal_reduce4" in t) <= (c["shape"][4] % 4 == 0 and max(per) > 1)
            assert ("acc_bal" in t) <= c["acc"]
        elif not ("one_chunk" in t):
            assert "cfg%d_ns%d" % (desc[0], desc[1]) in t, c["name"]
    assert any(c["P"] % 2 and c["Q"] % 2 for c in CC.of_engine("wino")) and {c["pack"] for c in CC.of_engine("wino")} == {"plain", "flip", "strides"}
    for c in CC.of_engine("s2"):
        desc, plan, ws, per = CC.wino_plan(c)
        assert ("split" in c["tags"]) == (desc[1] > 1) and ("bal_cut" in c["tags"]) <= bool(per and max(per) > 1), c["name"]
        assert ("ragged3" in c["tags"]) <= (c["P"] % 3 != 0 or c["Q"] % 3 != 0)


def test_impulse_footprints_are_disjoint_and_cover_the_sites():
    labels = {}
    for name in CC.INDEX_CASES:
        c = CC.BY_NAME[name]
        for sites in CC.impulse_sites(c):
            total = sum(CC.site_footprint(c, s).long() for _, s in sites)
            assert int(total.max()) <= 1, name
            assert all(bool(CC.site_footprint(c, s).any()) for _, s in sites), name
            labels.setdefault(c["engine"], set()).update(lab for lab, _ in sites)
    for engine, have in labels.items():
        assert have >= {"corner00_ch0", "corner0W_chlast", "cornerH0_step2", "cornerHW_lastimage", "lastimage_00", "boundary_lo", "boundary_hi"}, (engine, have)
    assert set(labels) == {"mfma", "c1", "to1", "wino", "s2"}


def test_planner_facts_need_no_launch():
    """the library's own queries (host code, no device needed) give the split, pieces, schedule and workspace every case claims"""
    from handwriting_line_generation_amd import _lib as L, ops
    for c in CC.CASES:
        N, H, W, C, K, Rr, S = c["shape"]
        with ops.tuning(**c["env"]):
            d = ops._desc(N, H, W, C, K, Rr, S, c["stride"], c["pad"], c["dil"], c["P"], c["Q"], c["transposed"])
            need = int(L.query(CC.workspace_entry(c)[1], d.ptr))
            if c["engine"] == "mfma":
                plan, ws = CC.mfma_plan(c)
                assert need == ws, (c["name"], need, ws)
            elif c["engine"] in ("wino", "s2"):
                desc, plan, ws, per = CC.wino_plan(c)
                out = np.full(8, -7, dtype=np.int32)
                L.call("hwg_wino_conv_describe", d.ptr, out.ctypes.data)
                assert [int(v) for v in out] == desc, (c["name"], [int(v) for v in out], desc)
                assert need == ws, (c["name"], need, ws)
                assert L.query("hwg_wino_s2_supported" if c["engine"] == "s2" else "hwg_wino_supported", d.ptr) == 1, c["name"]
            else:
                assert need == 0, c["name"]


# ---- sensitivity: flawed copies of the restatements (this file only) ---------------------------------------------------------------------------
def flawed_direct(c, x, w, b, y0, flaw):
    """the direct form of the case in fp64 with one plausible kernel flaw"""
    g = CC.geom(c)
    N, H, W, C = x.shape
    K = w.shape[2]
    if flaw == "last_tap_dropped_at_right_border":
        y = R.conv_direct(x, w, g, b, y0)
        w2 = w.clone(); w2[:, :-1] = 0
        g1 = dict(g)
        last = R.conv_direct(x, w2, g1)                       # what the last tap column contributes
        y[:, :, -1] -= last[:, :, -1]
        return y
    if flaw == "pad_off_by_one":
        g2 = dict(g, pad=(g["pad"][0], g["pad"][1] - 1))
        xs = torch.zeros(N, H, W + 2, C, dtype=x.dtype); xs[:, :, :W] = x   # the same output size from a shifted window
        return R.conv_direct(xs, w, g2, b, y0)
    if flaw == "filter_flip_ignored":
        return R.conv_direct(x, w.flip(0, 1), g, b, y0)
    if flaw == "bias_once_per_piece":
        return R.conv_direct(x, w, g, b, y0) + (CC.pieces(c) - 1) * b
    if flaw == "y0_ignored":
        return R.conv_direct(x, w, g, b, None)
    if flaw == "last_channel_chunk_dropped":
        bk = 32 if C % 32 == 0 else 16
        return R.conv_direct(x[..., :C - bk], w[..., :C - bk], g, b, y0)
    if flaw == "parity_class_swapped":
        y = R.conv_direct(x, w, g, b, y0)
        P2 = y.shape[1] // 2 * 2
        y[:, :P2] = y[:, :P2].reshape(N, P2 // 2, 2, y.shape[2], K).flip(2).reshape(N, P2, y.shape[2], K)
        return y
    if flaw == "output_padding_row_unwritten":
        y = R.conv_direct(x, w, g, b, y0)
        y[:, -1] = float("nan") if y0 is None else y0[:, -1]
        return y
    if flaw == "stale_piece":
        n = CC.pieces(c)
        ch = [(i * C // n, (i + 1) * C // n) for i in range(n)]
        y = R.conv_direct(x, w, g, b, y0, chunks=ch[:-1])
        other = torch.randn(x.shape, generator=torch.Generator().manual_seed(9), dtype=x.dtype)     # the previous call's piece: another input
        return y + R.conv_direct(other, w, g, chunks=ch[-1:])
    if flaw == "channels_past_K&~3_unwritten":
        y = R.conv_direct(x, w, g, b, y0)
        y[..., K & ~3:] = float("nan") if y0 is None else y0[..., K & ~3:]
        return y
    if flaw == "products_rounded_to_10_bits":
        assert w.shape[:2] == (1, 1)                          # a 1x1 case: every product of the contraction, rounded, then summed
        prod = (x[..., None, :] * w[0, 0]).float()
        prod = (prod.view(torch.int32) + 0x1000 & ~0x1FFF).view(torch.float32).double()
        return R._finish(prod.sum(-1), b, y0, False)
    raise KeyError(flaw)


def flawed_wino(c, x, w, b, y0, flaw):
    g = CC.geom(c)
    y = R.wino_conv(x, w, g, b, y0)
    N, P, Q, K = y.shape
    if flaw == "second_row_of_last_tile_written_for_odd_P":
        # the tile's second output row lands on the next image's first row (or past the tensor: a canary)
        g2 = dict(g, P=P + 1)
        full = R.wino_conv(x, w, g2, b, None)
        for n in range(N - 1):
            y[n + 1, 0] = full[n, P]
        return y
    if flaw == "tile_straddling_two_images_mixes_them":
        # tiles are numbered over N x TP x TQ; a workgroup tile that straddles two images reads every patch from its first tile's image
        TP, TQ = -(-P // 2), -(-Q // 2)
        tm = {0: 64, 1: 32, 2: 128, 5: 64, 6: 64, 7: 32}[CC.wino_plan(c)[0][0]]
        out = y.clone()
        for m in range(N * TP * TQ):
            n, t = divmod(m, TP * TQ)
            n0 = (m // tm * tm) // (TP * TQ)
            if n0 != n:
                tp, tq = divmod(t, TQ)
                out[n, 2 * tp:2 * tp + 2, 2 * tq:2 * tq + 2] = y[n0, 2 * tp:2 * tp + 2, 2 * tq:2 * tq + 2]
        return out
    raise KeyError(flaw)


FLAWS = {  # flaw -> case it is seeded into
    "last_tap_dropped_at_right_border": "tap_3x3_pad0", "pad_off_by_one": "m_plus1_64x64", "filter_flip_ignored": "tap_5x5_pad2",
    "bias_once_per_piece": "split2_128x128", "y0_ignored": "split3_128x64", "last_channel_chunk_dropped": "m_plus1_128x32",
    "parity_class_swapped": "t_4x4s2_p1_class", "output_padding_row_unwritten": "t_opad_k24_merged", "stale_piece": "split4_64x64",
    "channels_past_K&~3_unwritten": "split2_k78_scalar", "products_rounded_to_10_bits": "to1_c4_1x1",
    "second_row_of_last_tile_written_for_odd_P": "w_cfg6_ns1_2x13x37x64x78", "tile_straddling_two_images_mixes_them": "w_cfg0_ns2_3x7x21x64x34"}


def test_every_seeded_flaw_moves_a_case_past_its_bound():
    assert len(FLAWS) >= 13
    for flaw, name in FLAWS.items():
        c = CC.BY_NAME[name]
        x, w, b, y0 = (None if t is None else t.double() for t in CC.inputs(c))
        ref, yard, bound = G.reference(c)
        fn = flawed_wino if c["engine"] == "wino" else flawed_direct
        with_flaw = _ratio(fn(c, x, w, b, y0, flaw), ref, bound)
        without = _ratio(G.restate(c, x, w, b, y0), ref, bound)
        print("%-44s moves %-28s to %.3g x the bound (without the flaw: %.3g)" % (flaw, name, with_flaw, without))
        assert without <= 1.0, "%s: the copy without the flaw is off the reference" % flaw
        assert with_flaw >= SENSITIVITY_FACTOR, "%s: moves its case by only %.3g x the bound" % (flaw, with_flaw)


def test_impulse_comparison_flips_under_index_flaws():
    """the exact comparison of the impulse test: a wrong tap at one corner is another weight, bit for bit"""
    c = dict(CC.BY_NAME["tap_3x3_pad0"], bias=False, acc=False)
    _, w, _, _ = CC.inputs(c)
    sites = CC.impulse_sites(c)[0]
    x = torch.zeros(c["shape"][:4], dtype=torch.double)
    for _, s in sites:
        x[s] = 1.0
    want = R.conv_direct(x, w.double(), CC.geom(c)).float()
    assert torch.equal(R.conv_direct(x.float(), w, CC.geom(c)), want)
    for flaw in ("filter_flip_ignored", "last_tap_dropped_at_right_border", "last_channel_chunk_dropped"):
        assert not torch.equal(flawed_direct(c, x, w.double(), None, None, flaw).float(), want), flaw
