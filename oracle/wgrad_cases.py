"""Case tables of tests/test_wgrad_fp64_gpu.py: the weight-gradient entries (hwg_conv_wgrad with wgrad_mfma_kernel in its 32x32, 64x64, 128x128
and taps-as-N forms, wgrad_narrow_kernel, wgrad_c1_rows_kernel, wgrad_c1_kernel and wgrad_direct_kernel; hwg_wino_wgrad in both forms; the five
reduce families; the *_sets entries; hwg_colsum), every schedule forced through the tuning variables, at the smallest shapes that reach each
regime of the dispatch code. A case is a dict:

  name, engine ("mfma" | "tapn" | "narrow" | "c1rows" | "c1valu" | "direct" | "wino" | "s2"), shape (N, H, W, C, K, R, S) of the DESCRIPTOR
  (gathered tensor v [N,H,W,C], anchor u [N,P,Q,K]), stride, pad, dil, P, Q, env (tuning variables), tags (the regimes it covers; the ones
  that follow from the plan are derived, not written by hand), acc / bias / bias_acc (accumulate into dw, fused bias gradient, accumulate into
  it), layout ("kc" the parameter's own [K][C][R][S], "ck" the transposed parameter's [C][K][R][S], "pad" [K][C+3][R][S] with three channels of
  gap per row, as a channel-padded temporary has), sets and set_on_v (the *_sets entries).

Host-side restatements of the planners (which kernel a case runs, hwg_last_plan's triple, the pixel ranges, the workspace, the reduce
schedule) are here as well; tests/test_wgrad_ref_cpu.py holds them against the library's own queries, which need no GPU.

plan_wgrad sits behind a per-thread HwgPlanCache keyed by the whole descriptor AND the tuning epoch; ops.tuning starts a new epoch on entry and
on exit, so a cached plan cannot outlive the block that forced it and two cases may share a descriptor."""
import zlib

import torch

from oracle import conv_ref as R

CASES = []
_rot = [0]
RED_VEC4, RED_SCALAR, RED_LANES32, RED_LANES4, RED_ROWS = "VEC4", "SCALAR", "LANES32", "LANES4", "ROWS"
HWG_PROF_WGRAD, HWG_PROF_WGRAD_WINO = 1, 7


def cdiv(a, b):
    return -(-a // b)


def _add(engine, name, shape, stride=(1, 1), pad=(0, 0), dil=(1, 1), PQ=None, env=None, tags=(), acc=None, bias=None, bias_acc=None, layout="kc",
         sets=1, set_on_v=0):
    """bias / accumulate / bias-accumulate rotate through their combinations unless given"""
    N, H, W, C, K, Rr, S = shape
    P, Q = PQ or R.out_size(H, W, Rr, S, stride, pad, dil)
    assert P > 0 and Q > 0, name
    assert name not in [c["name"] for c in CASES], name
    k = _rot[0]
    _rot[0] += 1
    acc = bool(k & 1) if acc is None else acc
    bias = bool(k & 2) if bias is None else bias
    if engine == "direct" or set_on_v:
        bias = False
    bias_acc = bias and (bool(k & 4) if bias_acc is None else bias_acc)
    c = dict(name=name, engine=engine, shape=shape, stride=stride, pad=pad, dil=dil, P=P, Q=Q, env=dict(env or {}), tags=set(tags), acc=acc, bias=bias,
             bias_acc=bias_acc, layout=layout, sets=sets, set_on_v=set_on_v)
    c["tags"] |= derived_tags(c)
    CASES.append(c)
    return c


def transposed_layer(N, Hin, Win, Cin, Kout, Rr, S, stride, pad, opad=(0, 0)):
    """shape and PQ of the descriptor ops._make_wgrad_plan builds for a transposed layer: anchor = the layer input x [N,Hin,Win,Cin], gathered =
    dy [N,Hout,Wout,Kout], a strided gather"""
    Hout, Wout = R.out_size(Hin, Win, Rr, S, stride, pad, (1, 1), 1, opad)
    return (N, Hout, Wout, Kout, Cin, Rr, S), (Hin, Win)


def geom(c):
    return dict(stride=c["stride"], pad=c["pad"], dil=c["dil"], R=c["shape"][5], S=c["shape"][6])


def pixels(c):
    return c["shape"][0] * c["P"] * c["Q"]


def inputs(c):
    """u [sets,N,P,Q,K] (set_on_v: [1,...]), v [1,N,H,W,C] (set_on_v: [sets,...]), dw0 [sets,R,S,K,C] or None, db0 [sets,K] or None - fp32, seeded by
    the case's name"""
    N, H, W, C, K, Rr, S = c["shape"]
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()) & 0x7FFFFFFF)
    su, sv = (1, c["sets"]) if c["set_on_v"] else (c["sets"], 1)
    u = torch.randn(su, N, c["P"], c["Q"], K, generator=g)
    v = torch.randn(sv, N, H, W, C, generator=g)
    dw0 = torch.randn(c["sets"], Rr, S, K, C, generator=g) * pixels(c) ** 0.5 if c["acc"] else None
    db0 = torch.randn(c["sets"], K, generator=g) * pixels(c) ** 0.5 if c["bias_acc"] else None
    return u, v, dw0, db0


def operands(c, u, v, s):
    """(u, v) of set s"""
    return (u[0], v[s]) if c["set_on_v"] else (u[s], v[0])


# ---- the dw buffer ----------------------------------------------------------------------------------------------------------------------------
def dw_strides(c):
    """(floats of the buffer, sa, sb, sr, ss): element (k, c, r, s) at k sa + c sb + r sr + s ss"""
    N, H, W, C, K, Rr, S = c["shape"]
    RS = Rr * S
    if c["layout"] == "kc":
        return K * C * RS, C * RS, RS, S, 1
    if c["layout"] == "ck":
        return K * C * RS, RS, K * RS, S, 1
    return K * (C + 3) * RS, (C + 3) * RS, RS, S, 1


def dw_index(c):
    """int64 [R,S,K,C]: where the logical gradient lies in the buffer"""
    N, H, W, C, K, Rr, S = c["shape"]
    _, sa, sb, sr, ss = dw_strides(c)
    r, s = torch.arange(Rr).view(Rr, 1, 1, 1), torch.arange(S).view(1, S, 1, 1)
    k, ch = torch.arange(K).view(1, 1, K, 1), torch.arange(C).view(1, 1, 1, C)
    return k * sa + ch * sb + r * sr + s * ss


# ---- planners, restated -----------------------------------------------------------------------------------------------------------------------
def wg_split(Mtot, ns, bkp=32):
    """(ranges, pixels per range) of conv_mfma.hip: at least four 32-pixel steps per range, ranges of whole steps"""
    ns = max(1, min(ns, (Mtot + 4 * bkp - 1) // (4 * bkp)))
    chunk = cdiv(cdiv(Mtot, ns), bkp) * bkp
    return max(1, cdiv(Mtot, chunk)), chunk


def _tune(c, name, default):
    return int(c["env"].get(name, default))


def is_tapn(C, K, RS):
    return C == 1 and K > 2 and K % 4 == 0 and RS <= 64


def is_direct(C, K, RS):
    return (K <= 2 or C <= 2) and not is_tapn(C, K, RS)


def _c1_square(c):
    N, H, W, C, K, Rr, S = c["shape"]
    return C == 1 and K == 64 and Rr == S and Rr in (3, 5, 7)


def is_c1_rows(c, N):
    return (_tune(c, "HWG_WGRAD_C1", 0) != 1 and _tune(c, "HWG_WGRAD_C1_ROWS", 1) != 0 and _c1_square(c) and c["stride"] == (1, 1) and c["dil"] == (1, 1)
            and N * c["P"] * c["Q"] >= 4096)


def is_c1_valu(c, N):
    return _tune(c, "HWG_WGRAD_C1", 0) != 0 and _c1_square(c) and N * c["P"] * c["Q"] >= 4096


def is_narrow(c):
    N, H, W, C, K, Rr, S = c["shape"]
    mode = _tune(c, "HWG_WGRAD_NARROW", 1)
    nb = cdiv(K, 16) * cdiv(C, 16)
    return (mode != 0 and (Rr, S) in ((3, 3), (4, 4)) and c["dil"] == (1, 1) and C >= 4 and K > 2 and (nb == 1 or (mode == 2 and nb in (2, 4)))
            and pixels(c) >= 16384)


def narrow_blocks(c, N):
    Nn, H, W, C, K, Rr, S = c["shape"]
    streams = 8 // (cdiv(K, 16) * cdiv(C, 16))
    G4 = (N * c["P"] * c["Q"] + 3) // 4
    return max(1, min(512, G4 // (streams * 8)))


def plan_wgrad_model(c, N):
    """(cfg, tile, nsplit, chunk) of the <= 32-channel branch and the forced branch of plan_wgrad_model for a batch of N"""
    Nn, H, W, C, K, Rr, S = c["shape"]
    M = N * c["P"] * c["Q"]
    if K <= 32 and C <= 32:
        cfg, tile = 2, 32
        want = cdiv(1024, Rr * S * cdiv(K, tile) * cdiv(C, tile))
    else:
        cfg, blocks = (int(t) for t in c["env"]["HWG_WGRAD_FORCE"].split(","))     # the model branch is not restated: such cases are forced
        assert cfg == 1 or (cfg == 0 and K >= 128 and C >= 128), c["name"]
        tile = 128 if cfg == 0 else 64
        want = cdiv(blocks, Rr * S * cdiv(K, tile) * cdiv(C, tile))
    return (cfg, tile) + wg_split(M, want)


def plan_wgrad_tapn(c, N):
    Nn, H, W, C, K, Rr, S = c["shape"]
    M = N * c["P"] * c["Q"]
    if is_c1_rows(c, N):
        return (5, 64, min(N * c["P"] * cdiv(c["Q"], 128), 512), 0)
    if is_c1_valu(c, N):
        return (4, 64) + wg_split(M, 768)
    return (3, 64) + wg_split(M, cdiv(1024, cdiv(K, 64)))


def plan_wgrad_sets(c):
    """(cfg, tile, nsplit per set, chunk) of the launch hwg_conv_wgrad / hwg_conv_wgrad_sets makes"""
    N, H, W, C, K, Rr, S = c["shape"]
    sets, tapn, narrow = c["sets"], is_tapn(C, K, Rr * S), is_narrow(c)
    one = plan_wgrad_tapn if tapn else plan_wgrad_model
    cfg, tile, ns, chunk = one(c, N * sets)              # (looked up for the narrow kernel as well: only its nsplit is replaced)
    if narrow:
        return cfg, tile, max(1, narrow_blocks(c, N * sets) // sets), chunk
    if sets > 1:
        ns, chunk = wg_split(N * c["P"] * c["Q"], cdiv(ns, sets))
    return cfg, tile, ns, chunk


def plan_wd(c):
    """wgrad_direct_kernel's plan, None where it refuses: dict(big_on_anchor, G, TSL, PL, MAXT, chunk, nblk)"""
    N, H, W, C, K, Rr, S = c["shape"]
    RS, big = Rr * S, 1 if K > 2 else 0
    bigc = K if big else C
    if bigc % 4 or bigc > 1024 or (big and C != 1):
        return None
    G = bigc // 4
    slots = 256 // G
    if slots < 1:
        return None
    TSL = min(slots, RS)
    PL, MAXT = slots // TSL, cdiv(RS, TSL)
    if MAXT > 8:
        return None
    M = pixels(c)
    nblk = max(1, min(1024, cdiv(M, 512)))
    chunk = cdiv(M, nblk)
    nblk = cdiv(M, chunk)
    if PL * TSL * MAXT * (1 if big else 2) * G * 4 * 4 > 64 * 1024:
        return None
    return dict(big_on_anchor=big, G=G, TSL=TSL, PL=PL, MAXT=MAXT, chunk=chunk, nblk=nblk)


def is_s2(c):
    N, H, W, C, K, Rr, S = c["shape"]
    return (Rr, S) == (4, 4) and c["stride"] == (2, 2) and c["pad"] == (0, 0) and c["dil"] == (1, 1) and H >= 4 and W >= 4


def plan_wino_wgrad(c):
    """(kt, ct, nsplit per set, tile pairs MP, pairs per row TQ2, tile rows TP, tile size mt)"""
    N, H, W, C, K, Rr, S = c["shape"]
    s2 = is_s2(c)
    mt = 3 if s2 else 2
    kt, ct = cdiv(K, 64), cdiv(4 * C if s2 else C, 64)
    TP, TQ2 = cdiv(c["P"], mt), cdiv(cdiv(c["Q"], mt), 2)
    MP = N * TP * TQ2
    rounds_all = cdiv(MP, 4)
    ns = max(1, 256 // (kt * ct * c["sets"]))
    ns = min(ns, max(rounds_all // 4, 1))
    force = _tune(c, "HWG_WINO_WGRAD_SPLIT", 0)
    if force > 0:
        ns = min(force, rounds_all)
    return kt, ct, ns, MP, TQ2, TP, mt


def reduce_schedule(c, nsplit):
    """(variant, ROWS sub-variant (taps class, slices) or None) of the sum of the partial images"""
    N, H, W, C, K, Rr, S = c["shape"]
    RS = Rr * S
    total = RS * K * C + (K if c["bias"] else 0)
    pairs = K * C
    if c["layout"] == "kc" and _tune(c, "HWG_WGRAD_REDUCE_ROWS", 1) and RS <= 49 and pairs >= 65536 and nsplit <= 16:
        return RED_ROWS, ({9: "9", 16: "16", 3: "3"}.get(RS, "other"), 4 if nsplit >= 8 and pairs <= 65536 else 1)
    if nsplit >= 64 and total <= 65536:
        return RED_LANES32, None
    if nsplit >= 8 and total <= 262144:
        return RED_LANES4, None
    return (RED_VEC4 if C % 4 == 0 else RED_SCALAR), None


def plan(c):
    """dict(kernel, last_plan (None: the direct kernel notes none), nsplit (per set), ws (bytes), reduce, ranges ([(begin, end)] anchor-pixel
    ranges of one set's partial images, where the kernel cuts by pixels), extra (c of the bound for dw), bias_extra (for the bias gradient))"""
    N, H, W, C, K, Rr, S = c["shape"]
    RS, M, sets = Rr * S, pixels(c), c["sets"]
    per_image = RS * K * C + K
    if c["engine"] in ("wino", "s2"):
        kt, ct, ns, MP, TQ2, TP, mt = plan_wino_wgrad(c)
        bounds = [MP * i // ns for i in range(ns + 1)]

        def first_pixel(pair):                                                   # the first anchor pixel of a tile pair
            t2, tjp = divmod(pair, TQ2)
            n, ti = divmod(t2, TP)
            return (n * c["P"] + mt * ti) * c["Q"] + 2 * mt * tjp
        return dict(kernel="wino_wgrad", last_plan=(HWG_PROF_WGRAD_WINO, 36 if mt == 3 else 0, ns), nsplit=ns, ws=sets * ns * per_image * 4,
                    reduce=reduce_schedule(c, ns), ranges=None, pair_ranges=list(zip(bounds[:-1], bounds[1:])), first_pixel=first_pixel,
                    extra=(4 + 2 + 4 if mt == 3 else 2 + 2 + 4) + ns - 1 + int(c["acc"]), bias_extra=3 + ns - 1 + int(c["bias_acc"]),
                    launch=(kt * ct * ns * sets, cdiv(kt * ct * ns * sets, 8) * 8))
    if is_direct(C, K, RS):
        p = plan_wd(c)
        if p is None:
            return dict(kernel="refused", last_plan=None, nsplit=0, ws=0, reduce=None, ranges=None, extra=0, bias_extra=0)
        rng = [(i * p["chunk"], min((i + 1) * p["chunk"], M)) for i in range(p["nblk"])]
        return dict(kernel="direct<%d>" % p["big_on_anchor"], last_plan=None, nsplit=p["nblk"], ws=p["nblk"] * RS * K * C * 4, reduce=None, ranges=rng,
                    extra=p["PL"] - 1 + p["nblk"] - 1 + int(c["acc"]), bias_extra=0, wd=p)
    cfg, tile, ns, chunk = plan_wgrad_sets(c)
    tapn = is_tapn(C, K, RS)
    if is_narrow(c):
        streams = 8 // (cdiv(K, 16) * cdiv(C, 16))
        G4, GS = (M + 3) // 4, ns * streams
        rng = [(min(4 * (G4 * i // GS), M), min(4 * (G4 * (i + 1) // GS), M)) for i in range(GS)]
        kernel, code, tree, btree = "narrow<%d>" % Rr, 100 + Rr, streams.bit_length() - 1, 2 + streams.bit_length() - 1
    elif cfg == 5:
        kernel, code, tree, btree, rng = "c1_rows<%d>" % Rr, 15, 3, 1 + 3, None
    elif cfg == 4:
        G, Wt = (M + 63) // 64, ns * 4
        rng = [(min(64 * (G * i // Wt), M), min(64 * (G * (i + 1) // Wt), M)) for i in range(Wt)]
        kernel, code, tree, btree = "c1<%d>" % Rr, 14, 3, 3
    else:
        rng = [(i * chunk, min((i + 1) * chunk, M)) for i in range(ns)]
        kernel = {0: "mfma128", 1: "mfma64", 2: "mfma32", 3: "tapn"}[cfg]
        code, tree, btree = (13 if tapn else cfg), {0: 0, 1: 1, 2: 3, 3: 1}[cfg], 1       # WAVES_K - 1 sums; the bias sum is fp64, rounded once
    return dict(kernel=kernel, last_plan=(HWG_PROF_WGRAD, code, ns), nsplit=ns, ws=sets * ns * per_image * 4, reduce=reduce_schedule(c, ns), ranges=rng,
                extra=tree + ns - 1 + int(c["acc"]), bias_extra=btree + ns - 1 + int(c["bias_acc"]), tile=tile, chunk=chunk)


def entry(c):
    """(entry, its workspace query) the case goes through"""
    wino = c["engine"] in ("wino", "s2")
    if c["sets"] > 1:
        return ("hwg_wino_wgrad_sets", "hwg_wino_wgrad_sets_workspace") if wino else ("hwg_conv_wgrad_sets", "hwg_conv_wgrad_sets_workspace")
    return ("hwg_wino_wgrad", "hwg_wino_wgrad_workspace") if wino else ("hwg_conv_wgrad", "hwg_conv_wgrad_workspace")


def derived_tags(c):
    """the regimes that follow from the shape and the restated plan"""
    N, H, W, C, K, Rr, S = c["shape"]
    p = plan(c)
    t = {p["kernel"]}
    if p["reduce"]:
        t.add("red_" + p["reduce"][0] + ("_%s_%d" % p["reduce"][1] if p["reduce"][1] else ""))
    if c["sets"] > 1:
        t |= {"sets%d" % c["sets"], "set_on_v%d" % c["set_on_v"]}
    t.add("layout_" + c["layout"])
    M, ns = pixels(c), p["nsplit"]
    if p["kernel"] in ("mfma128", "mfma64", "mfma32", "tapn"):
        tile, last = p["tile"], M - (ns - 1) * p["chunk"]
        t |= {"px<step"} if M < 32 else set()
        t |= {"px_whole"} if M % 32 == 0 else set()
        t |= {"px_whole+1"} if M % 32 == 1 and M > 32 else set()
        t.add("ranges1" if ns == 1 else "ranges2" if ns == 2 else "ranges_many" if ns >= 8 else "ranges3-7")
        t |= {"ragged_last"} if ns > 1 and last < 32 else set()
        for nm, n in (("K", K), ("C", C)) if p["kernel"] != "tapn" else (("K", K),):
            t |= {nm + "<tile"} if n < tile else set()
            t |= {nm + "=tile+4"} if n == tile + 4 else set()
            t |= {nm + "_tiles_ragged"} if n > tile and n % tile else set()
    if p["kernel"].startswith("narrow"):
        t.add("blocks%d" % (cdiv(K, 16) * cdiv(C, 16)))
        t.add("px16384" if M == 16384 else "px16384+ragged" if M % 4 else "px>16384")
    if p["kernel"].startswith("c1_rows"):
        nseg = N * c["sets"] * c["P"] * cdiv(c["Q"], 128)
        t.add("Q<128" if c["Q"] < 128 else "Q=128" if c["Q"] == 128 else "Q>128")
        t |= {"ragged_segment"} if c["Q"] % 128 else set()
        t.add("segments>512" if nseg > 512 else "segments<512")
    if p["kernel"].startswith("c1<"):
        t |= {"px%64"} if M % 64 else set()
        t |= {"waves>groups"} if ns * 4 > (M + 63) // 64 else set()
    if p["kernel"].startswith("direct"):
        t |= {"K%d" % K, "C%d" % C, "px%d" % M if M <= 513 else "px_many"}
        t |= {"block_cap"} if M > 1024 * 512 else set()
        t |= {"taps_per_thread%d" % p["wd"]["MAXT"]}
    if p["kernel"] == "wino_wgrad":
        t |= {"Qmod4=%d" % (c["Q"] % 4), "ranges%d" % min(ns, 4)} if c["engine"] == "wino" else {"ranges%d" % min(ns, 4)}
        t |= {"oddP"} if c["P"] % 2 else set()
        t |= {"one_round_per_range"} if ns > 1 and ns == cdiv(p["pair_ranges"][-1][1], 4) else set()
        t |= {"padding_workgroups"} if p["launch"][0] % 8 else set()
    return t


# ---- hwg_conv_wgrad: wgrad_mfma_kernel ---------------------------------------------------------------------------------------------------------
def _mfma(name, shape, force=None, env=None, **kw):
    env = dict(env or {})
    if force:
        env["HWG_WGRAD_FORCE"] = force
    return _add("mfma", name, shape, env=env, **kw)


# 32x32 (K, C <= 32): pixels below one step, whole steps (one range), one more (two ranges, the second of one step and a pixel), many ranges with a
# last one of 3 pixels; K, C in {4, 20, 32}
_mfma("t32_px20_1x1", (1, 4, 5, 4, 20, 1, 1), tags={"1x1"})
_mfma("t32_px128_3x3p1", (1, 8, 16, 20, 4, 3, 3), pad=(1, 1), tags={"3x3p1"})
_mfma("t32_px129_3x3p0", (1, 5, 45, 32, 32, 3, 3), tags={"3x3p0"})
_mfma("t32_px385_3x3p2", (1, 3, 75, 4, 4, 3, 3), pad=(2, 2), tags={"3x3p2"})
_mfma("t32_px1155_1x3d4", (3, 5, 77, 20, 20, 1, 3), pad=(0, 4), dil=(1, 4), tags={"1x3d4"}, bias=True, acc=True, bias_acc=True)
_mfma("t32_4x4s2p1", (2, 10, 14, 20, 32, 4, 4), stride=(2, 2), pad=(1, 1), tags={"4x4s2p1"})
_mfma("t32_4x4s21", (2, 10, 9, 4, 20, 4, 4), stride=(2, 1), pad=(1, 0), tags={"4x4s21"})
_mfma("t32_5x5p2", (1, 7, 9, 20, 4, 5, 5), pad=(2, 2), tags={"5x5p2"})
_mfma("t32_dil21", (2, 9, 9, 32, 20, 3, 3), pad=(2, 1), dil=(2, 1), tags={"d21"})
_mfma("t32_3x3s31_onerow", (2, 3, 40, 20, 32, 3, 3), stride=(3, 1), pad=(0, 1), tags={"3x3s31_onerow"})
_mfma("t32_padded_strides", (2, 6, 11, 20, 12, 3, 3), pad=(1, 1), layout="pad", tags={"3x3p1"}, bias=False, acc=False)
_mfma("t32_ck_acc", (2, 6, 11, 12, 20, 3, 3), pad=(1, 1), layout="ck", bias=True, acc=True)
# 64x64, forced: K, C in {4, 20, 36} below the tile, 68 one block past it, 132 three tiles with a ragged last one
_mfma("t64_px20_k36_c68", (1, 4, 5, 68, 36, 1, 1), force="1,1", tags={"1x1"})
_mfma("t64_px128_k68_c4", (1, 8, 16, 4, 68, 3, 3), force="1,9", pad=(1, 1), tags={"3x3p1"})
_mfma("t64_px129_k132_c20", (1, 3, 43, 20, 132, 1, 1), force="1,6", tags={"1x1"})
_mfma("t64_px385_k68_c132", (1, 5, 77, 132, 68, 1, 3), force="1,72", pad=(0, 4), dil=(1, 4), tags={"1x3d4"})
_mfma("t64_px1155_k36_c36", (3, 5, 77, 36, 36, 3, 3), force="1,90", pad=(1, 1), tags={"3x3p1"}, bias=True, acc=False)
_mfma("t64_4x4s2_k68_ck", (2, 10, 14, 36, 68, 4, 4), force="1,64", stride=(2, 2), pad=(1, 1), layout="ck", tags={"4x4s2p1"})
_mfma("t64_5x5p2_k20_c68", (1, 7, 9, 68, 20, 5, 5), force="1,50", pad=(2, 2), tags={"5x5p2"})
_mfma("t64_3x3p0_k68", (2, 6, 11, 36, 68, 3, 3), force="1,18", tags={"3x3p0"})
# 128x128, forced (K, C >= 128): 132 one block past the tile, 260 three tiles with a ragged last one
_mfma("t128_px20_k132_c132", (1, 4, 5, 132, 132, 1, 1), force="0,4", tags={"1x1"})
_mfma("t128_px128_k260_c132", (1, 8, 16, 132, 260, 1, 1), force="0,6", tags={"1x1"})
_mfma("t128_px129_k132_c260", (1, 3, 43, 260, 132, 1, 1), force="0,12", tags={"1x1"})
_mfma("t128_px385_3x3p1", (1, 5, 77, 132, 132, 3, 3), force="0,144", pad=(1, 1), tags={"3x3p1"})
_mfma("t128_px1155_1x1", (3, 5, 77, 132, 132, 1, 1), force="0,40", tags={"1x1"}, bias=True, acc=True)
_mfma("t128_4x4s21", (2, 10, 9, 132, 132, 4, 4), force="0,64", stride=(2, 1), pad=(1, 0), tags={"4x4s21"})
# transposed layers (anchor = x, gathered = dy, strided gather), one with output_padding
_s, _pq = transposed_layer(2, 5, 7, 20, 12, 4, 4, (2, 2), (1, 1))
_mfma("t32_transposed_4x4s2", _s, stride=(2, 2), pad=(1, 1), PQ=_pq, layout="kc", bias=False, tags={"transposed_layer"})
_s, _pq = transposed_layer(2, 5, 7, 36, 68, 3, 3, (2, 2), (1, 1), (1, 1))
_mfma("t64_transposed_opad", _s, force="1,36", stride=(2, 2), pad=(1, 1), PQ=_pq, bias=False, tags={"transposed_layer", "output_padding"})
# the row-contiguous reduce: 256 x 256 channel pairs (four slices: 8..16 ranges) and one slice (<= 7 ranges, or more pairs), taps 9 / 16 / 3 / other
_mfma("rows_9_sl4", (1, 8, 128, 256, 256, 3, 3), force="1,1152", pad=(1, 1), bias=True, acc=True)
_mfma("rows_16_sl4", (1, 66, 66, 256, 256, 4, 4), force="0,512", stride=(2, 2), pad=(0, 0), bias=False, acc=False)
_mfma("rows_3_sl4", (1, 8, 128, 256, 256, 1, 3), force="1,384", pad=(0, 1), bias=True, acc=False)
_mfma("rows_other_sl4", (2, 16, 32, 256, 256, 1, 1), force="0,32", bias=False, acc=True)
_mfma("rows_9_sl1", (1, 4, 64, 256, 256, 3, 3), force="0,72", pad=(1, 1), bias=False, acc=True)
_mfma("rows_16_sl1", (1, 18, 34, 256, 260, 4, 4), force="1,640", stride=(2, 2), pad=(1, 1), bias=True, acc=True)
_mfma("rows_3_sl1", (1, 4, 64, 260, 256, 1, 3), force="1,40", pad=(0, 1), bias=True, acc=False)
_mfma("rows_other_sl1", (1, 4, 64, 256, 256, 1, 1), force="0,8", bias=False, acc=False)
_mfma("rows_off_9", (1, 8, 128, 256, 256, 3, 3), force="1,1152", pad=(1, 1), env=dict(HWG_WGRAD_REDUCE_ROWS="0"), bias=True, acc=True, tags={"rows_off"})
_mfma("rows_not_for_ck", (1, 8, 128, 256, 256, 3, 3), force="1,1152", pad=(1, 1), layout="ck", bias=True, acc=False, tags={"ck_256"})

# ---- taps-as-N (C == 1) ------------------------------------------------------------------------------------------------------------------------
_add("tapn", "tapn_px20_k4_3x3", (1, 4, 5, 1, 4, 3, 3), pad=(1, 1), tags={"3x3p1"})
_add("tapn", "tapn_px128_k20_5x5", (1, 8, 16, 1, 20, 5, 5), pad=(2, 2), tags={"5x5p2"})
_add("tapn", "tapn_px129_k68_1x3d4", (1, 3, 43, 1, 68, 1, 3), pad=(0, 4), dil=(1, 4), tags={"1x3d4"})
_add("tapn", "tapn_px385_k132_4x4s2", (1, 10, 154, 1, 132, 4, 4), stride=(2, 2), pad=(1, 1), tags={"4x4s2p1"})
_add("tapn", "tapn_px1155_k64_3x3", (3, 5, 77, 1, 64, 3, 3), pad=(1, 1), tags={"k64_below_4096"}, bias=True, acc=True, bias_acc=True)
_add("tapn", "tapn_k64_7x7_rows_off", (1, 64, 70, 1, 64, 7, 7), pad=(3, 3), env=dict(HWG_WGRAD_C1_ROWS="0"), tags={"k64_rows_off"})
_add("tapn", "tapn_8x8_k36", (2, 11, 20, 1, 36, 8, 8), pad=(3, 3), tags={"64taps"})
_add("tapn", "tapn_lanes32_k8_3x3", (2, 64, 66, 1, 8, 3, 3), pad=(1, 1), tags={"3x3p1"})
_add("tapn", "tapn_ck_1x1_s2", (2, 9, 11, 1, 12, 1, 1), stride=(2, 2), layout="ck", tags={"1x1"})

# ---- every tap geometry on every form of wgrad_mfma_kernel --------------------------------------------------------------------------------------
# (tag, R, S, stride, pad, dil, H): two images of H x 14
GEOMETRIES = [("1x1", 1, 1, (1, 1), (0, 0), (1, 1), 10), ("3x3p0", 3, 3, (1, 1), (0, 0), (1, 1), 10), ("3x3p1", 3, 3, (1, 1), (1, 1), (1, 1), 10),
              ("3x3p2", 3, 3, (1, 1), (2, 2), (1, 1), 10), ("1x3d4", 1, 3, (1, 1), (0, 4), (1, 4), 10), ("4x4s2p1", 4, 4, (2, 2), (1, 1), (1, 1), 10),
              ("4x4s21", 4, 4, (2, 1), (1, 0), (1, 1), 10), ("5x5p2", 5, 5, (1, 1), (2, 2), (1, 1), 10), ("d21", 3, 3, (1, 1), (2, 1), (2, 1), 10),
              ("3x3s31_onerow", 3, 3, (3, 1), (0, 1), (1, 1), 3)]
_FORMS = [("t32", [(4, 20), (20, 32), (32, 4), (20, 20)], None), ("t64", [(36, 68), (68, 20), (132, 36), (4, 68)], "1"),
          ("t128", [(132, 132), (260, 132), (132, 260)], "0"), ("tapn", [(4, 1), (20, 1), (68, 1), (132, 1), (64, 1)], None)]
for _f, _chans, _cfg in _FORMS:
    for _i, (_tag, _r, _s, _st, _pd, _dl, _h) in enumerate(GEOMETRIES):
        _k, _c = _chans[_i % len(_chans)]
        _env = {} if _cfg is None else dict(HWG_WGRAD_FORCE="%s,%d" % (_cfg, (1, 40, 200)[_i % 3]))
        _add("tapn" if _f == "tapn" else "mfma", "g_%s_%s" % (_f, _tag), (2, _h, 14, _c, _k, _r, _s), stride=_st, pad=_pd, dil=_dl, env=_env, tags={_tag})

# ---- wgrad_narrow_kernel (>= 16384 pixels) -----------------------------------------------------------------------------------------------------
_add("narrow", "narrow_3x3_16x16_p1", (1, 128, 128, 16, 16, 3, 3), pad=(1, 1), tags={"pad1"})
_add("narrow", "narrow_3x3_4x4_p0", (3, 77, 75, 4, 4, 3, 3), tags={"pad0"})
_add("narrow", "narrow_3x3_k16_c12_p2", (3, 71, 73, 12, 16, 3, 3), pad=(2, 2), tags={"pad2"})
_add("narrow", "narrow_3x3_s21_k4_c12", (1, 257, 128, 12, 4, 3, 3), stride=(2, 1), pad=(1, 1), tags={"3x3s21"})
_add("narrow", "narrow_4x4_s2_16x16", (1, 256, 256, 16, 16, 4, 4), stride=(2, 2), pad=(1, 1), tags={"4x4s2"})
_add("narrow", "narrow_4x4_s21_k12_c4", (1, 150, 222, 4, 12, 4, 4), stride=(2, 1), pad=(1, 0), tags={"4x4s21"})
_add("narrow", "narrow_4x4_s1_p2_k4_c16", (3, 72, 74, 16, 4, 4, 4), pad=(2, 2), tags={"pad2"})
for _k, _c, _r in ((32, 16, 3), (16, 32, 4), (32, 32, 3), (64, 16, 4)):
    _add("narrow", "narrow_%dx%d_k%d_c%d" % (_r, _r, _k, _c), (1, 128 + _r - 3, 128 + _r - 3 + (1 if _k == 64 else 0), _c, _k, _r, _r), pad=(1, 1),
         env=dict(HWG_WGRAD_NARROW="2", **({"HWG_WGRAD_FORCE": "1,64"} if _k > 32 else {})), tags={"mode2"})

# ---- wgrad_c1_rows_kernel (K = 64, C = 1, >= 4096 pixels) ---------------------------------------------------------------------------------------
_add("c1rows", "c1rows_3x3_q127_p0", (1, 35, 129, 1, 64, 3, 3), tags={"pad0"})
_add("c1rows", "c1rows_5x5_q128_p1", (1, 34, 130, 1, 64, 5, 5), pad=(1, 1), tags={"pad1"})
_add("c1rows", "c1rows_7x7_q129_p2", (1, 34, 131, 1, 64, 7, 7), pad=(2, 2), tags={"pad2"})
_add("c1rows", "c1rows_7x7_q300_p3", (2, 7, 300, 1, 64, 7, 7), pad=(3, 3), tags={"pad3"})
_add("c1rows", "c1rows_3x3_tall_thin", (1, 600, 8, 1, 64, 3, 3), pad=(1, 1), tags={"pad1"}, bias=True, acc=True, bias_acc=True)

# ---- wgrad_c1_kernel (HWG_WGRAD_C1=1) ---------------------------------------------------------------------------------------------------------
_V = dict(HWG_WGRAD_C1="1")
_add("c1valu", "c1valu_3x3", (1, 64, 64, 1, 64, 3, 3), pad=(1, 1), env=_V)
_add("c1valu", "c1valu_5x5_s2", (1, 131, 133, 1, 64, 5, 5), stride=(2, 2), pad=(2, 2), env=_V, tags={"stride2"})
_add("c1valu", "c1valu_7x7_d2", (2, 45, 61, 1, 64, 7, 7), pad=(6, 6), dil=(2, 2), env=_V, tags={"dil2"}, bias=True, acc=True)

# ---- wgrad_direct_kernel ---------------------------------------------------------------------------------------------------------------------
_add("direct", "direct0_k1_c4_1x1_px1", (1, 1, 1, 4, 1, 1, 1))
_add("direct", "direct0_k2_c12_3x3_px511", (1, 7, 73, 12, 2, 3, 3), pad=(1, 1))
_add("direct", "direct0_k1_c64_7x7_px512", (2, 16, 16, 64, 1, 7, 7), pad=(3, 3))
_add("direct", "direct0_k2_c1024_1x1_px513", (1, 19, 27, 1024, 2, 1, 1))
_add("direct", "direct0_k2_c64_3x3_s2", (2, 21, 23, 64, 2, 3, 3), stride=(2, 2), pad=(1, 1), layout="ck")
_add("direct", "direct0_k1_c4_block_cap", (1, 725, 725, 4, 1, 1, 1), tags={"large"})
_add("direct", "direct1_k8_9x9", (1, 20, 33, 1, 8, 9, 9), pad=(4, 4))
_add("direct", "direct1_k92_9x9", (1, 9, 57, 1, 92, 9, 9), pad=(4, 4), acc=True)

# ---- hwg_wino_wgrad ----------------------------------------------------------------------------------------------------------------------------
def _wino(name, shape, pad, split=None, **kw):
    N, H, W, C, K = shape
    env = {} if split is None else dict(HWG_WINO_WGRAD_SPLIT=str(split))
    return _add("wino", name, (N, H, W, C, K, 3, 3), pad=pad, env=env, tags={"pad%d" % pad[0]}, **kw)


_wino("wino_q8_k16_c16", (2, 5, 8, 16, 16), (1, 1))
_wino("wino_q9_k48_c80_split2", (2, 7, 9, 80, 48), (1, 1), split=2)
_wino("wino_p1_q10_k64_c64_split3", (3, 3, 12, 64, 64), (0, 0), split=3)
_wino("wino_q11_k80_c144_p2", (1, 2, 9, 144, 80), (2, 2), split=1)
_wino("wino_q1_k144_c48", (2, 9, 3, 48, 144), (0, 0), split=2)
_wino("wino_one_round_per_range", (2, 7, 9, 16, 64), (1, 1), split=99, bias=True, acc=True, bias_acc=True)
_wino("wino_model_split", (4, 16, 33, 48, 80), (1, 1))
_wino("wino_ck_k80_c48", (2, 6, 11, 48, 80), (1, 1), split=2, layout="ck")
_wino("wino_rows_9_sl4", (2, 16, 32, 256, 256), (1, 1), split=8, bias=True, acc=False)


def _s2(name, shape, split=None, **kw):
    N, H, W, C, K = shape
    env = {} if split is None else dict(HWG_WINO_WGRAD_SPLIT=str(split))
    return _add("s2", name, (N, H, W, C, K, 4, 4), stride=(2, 2), env=env, **kw)


_s2("s2_even_c16_k16", (2, 12, 20, 16, 16), tags={"evenHW"}, acc=False, bias=True)
_s2("s2_odd_c20_k48", (2, 13, 23, 20, 48), split=2, tags={"oddHW", "4C_ragged"}, acc=True, bias=False)
_s2("s2_odd_even_c16_k80_split3", (3, 15, 18, 16, 80), split=3, tags={"oddHW"}, bias=True, acc=True, bias_acc=True)

# ---- the *_sets entries -------------------------------------------------------------------------------------------------------------------------
_SETS = [("mfma", "t32", (2, 6, 11, 20, 12, 3, 3), dict(pad=(1, 1))),
         ("mfma", "t64", (1, 5, 45, 36, 68, 3, 3), dict(pad=(1, 1), env=dict(HWG_WGRAD_FORCE="1,72"))),
         ("tapn", "tapn", (2, 9, 30, 1, 20, 5, 5), dict(pad=(2, 2))),
         ("narrow", "narrow", (1, 128, 128, 12, 16, 3, 3), dict(pad=(1, 1))),
         ("c1rows", "c1rows", (1, 33, 130, 1, 64, 3, 3), dict(pad=(1, 1)))]
for _i, (_e, _n, _s, _kw) in enumerate(_SETS):
    for _j, _sets in enumerate((2, 3, 8)):
        _add(_e, "sets%d_%s" % (_sets, _n), _s, sets=_sets, set_on_v=(_i + _j) % 2, **_kw)
_wino("sets2_wino", (2, 7, 9, 48, 64), (1, 1), sets=2)
_wino("sets3_wino_split2", (2, 6, 11, 16, 80), (1, 1), split=2, sets=3)
_s2("sets2_s2", (2, 12, 20, 16, 16), sets=2)
_s2("sets3_s2_split2", (2, 13, 23, 20, 48), split=2, sets=3)

BY_NAME = {c["name"]: c for c in CASES}


def of_engine(e):
    return [c for c in CASES if c["engine"] == e]


# sets = 1 through the sets entry must give the bits of the single-gradient entry
SETS1_CASES = ["t32_px129_3x3p0", "t64_px385_k68_c132", "tapn_px129_k68_1x3d4", "narrow_3x3_k16_c12_p2", "c1rows_3x3_q127_p0", "wino_q9_k48_c80_split2",
               "s2_odd_c20_k48"]

# refusals: (name, shape, geometry, what, expected) - HWG_ERR_ARG with nothing written
REFUSALS = [
    ("refuse_k6", dict(shape=(1, 6, 9, 8, 6, 3, 3), pad=(1, 1)), {}),
    ("refuse_c6", dict(shape=(1, 6, 9, 6, 8, 3, 3), pad=(1, 1)), {}),
    ("refuse_direct_c2_k8", dict(shape=(1, 6, 9, 2, 8, 3, 3), pad=(1, 1)), {}),
    ("refuse_direct_big_side_6", dict(shape=(1, 6, 9, 6, 2, 3, 3), pad=(1, 1)), {}),
    ("refuse_direct_k6_c1_9x9", dict(shape=(1, 12, 13, 1, 6, 9, 9), pad=(4, 4)), {}),
    ("refuse_direct_9_taps_per_thread", dict(shape=(1, 6, 9, 1024, 1, 3, 3), pad=(1, 1)), {}),
    ("refuse_direct_dbias", dict(shape=(1, 6, 9, 12, 2, 3, 3), pad=(1, 1)), dict(bias=True)),
    ("refuse_sets0", dict(shape=(2, 6, 11, 20, 12, 3, 3), pad=(1, 1)), dict(sets=0)),
    ("refuse_sets9", dict(shape=(2, 6, 11, 20, 12, 3, 3), pad=(1, 1)), dict(sets=9)),
    ("refuse_sets_direct", dict(shape=(1, 6, 9, 12, 2, 3, 3), pad=(1, 1)), dict(sets=2)),
    ("refuse_sets_on_v_with_bias", dict(shape=(2, 6, 11, 20, 12, 3, 3), pad=(1, 1)), dict(sets=2, set_on_v=1, bias=True)),
    ("refuse_wino_sets0", dict(shape=(2, 7, 9, 16, 16, 3, 3), pad=(1, 1)), dict(sets=0, wino=True)),
    ("refuse_wino_sets9", dict(shape=(2, 7, 9, 16, 16, 3, 3), pad=(1, 1)), dict(sets=9, wino=True)),
    ("refuse_wino_k12", dict(shape=(2, 7, 9, 16, 12, 3, 3), pad=(1, 1)), dict(wino=True)),
]

# (descriptor, expected hwg_conv_wgrad_sets_supported)
SETS_SUPPORTED = [((2, 6, 11, 20, 12, 3, 3), 1), ((1, 6, 9, 12, 2, 3, 3), 0), ((1, 6, 9, 2, 8, 3, 3), 0), ((1, 6, 9, 1, 8, 3, 3), 1), ((1, 6, 9, 1, 6, 3, 3), 0),
                  ((1, 6, 9, 8, 6, 3, 3), 0), ((1, 6, 9, 6, 8, 3, 3), 0), ((1, 12, 13, 1, 8, 9, 9), 0)]

# ---- index-exact inputs -----------------------------------------------------------------------------------------------------------------------
INDEX_CASES = ["t32_px129_3x3p0", "t32_px1155_1x3d4", "t32_4x4s2p1", "t32_padded_strides", "t64_px385_k68_c132", "t64_3x3p0_k68", "t128_px385_3x3p1",
               "t64_transposed_opad", "tapn_px385_k132_4x4s2", "tapn_8x8_k36", "narrow_3x3_k16_c12_p2", "narrow_4x4_s21_k12_c4", "narrow_3x3_k32_c32",
               "c1rows_7x7_q129_p2", "c1rows_3x3_tall_thin", "c1valu_5x5_s2", "direct0_k2_c12_3x3_px511", "direct0_k2_c1024_1x1_px513", "direct1_k8_9x9",
               "wino_q9_k48_c80_split2", "wino_p1_q10_k64_c64_split3", "s2_odd_c20_k48", "sets3_t32", "sets2_narrow", "sets3_wino_split2"]
MAX_SITES = 16


def impulse_pixels(c):
    """[(label, anchor pixel m)]: the first and the last pixel of split ranges (the first two, a middle one and the last two where there are
    many), the last pixel overall and the four corners of the first and the last image, without repeats"""
    N, P, Q, M = c["shape"][0], c["P"], c["Q"], pixels(c)
    p = plan(c)
    out = [("corner00", 0), ("corner0Q", Q - 1), ("cornerP0", (P - 1) * Q), ("cornerPQ", P * Q - 1), ("last_image_00", (N - 1) * P * Q), ("last", M - 1)]
    if p["ranges"]:
        rng = [r for r in p["ranges"] if r[1] > r[0]]
        pick = sorted({0, 1, len(rng) // 2, len(rng) - 2, len(rng) - 1} & set(range(len(rng))))
        for i in pick:
            out += [("range%d_first" % i, rng[i][0]), ("range%d_last" % i, rng[i][1] - 1)]
    elif c["engine"] in ("wino", "s2"):
        for i, (lo, hi) in enumerate(p["pair_ranges"][:4]):
            if hi > lo:
                out += [("range%d_first" % i, p["first_pixel"](lo)), ("range%d_lastpair" % i, p["first_pixel"](hi - 1))]
    else:                                                                         # c1_rows: 128-pixel segments of a row, dealt out round robin
        qt = cdiv(Q, 128)
        for i, seg in enumerate(sorted({0, 1, p["nsplit"] - 1, p["nsplit"], N * P * qt - 1} & set(range(N * P * qt)))):
            row, t = divmod(seg, qt)
            out += [("seg%d_first" % seg, row * Q + 128 * t), ("seg%d_last" % seg, row * Q + min(128 * t + 127, Q - 1))]
    seen, uniq = set(), []
    for lab, m in out:
        if m not in seen:
            seen.add(m)
            uniq.append((lab, m))
    return uniq[:MAX_SITES]


def impulse_passes(c):
    """[[(k, m), ...], ...]: per pass, the one anchor pixel every channel k carries a 1 at (at most one per channel: the rows dw[:, :, k, :] of two
    channels never collide, and a row has one product per tap)"""
    K = c["shape"][4]
    px = [m for _, m in impulse_pixels(c)]
    return [[(k, m) for k, m in enumerate(px[i:i + K])] for i in range(0, len(px), K)]


def impulse_u(c, sites):
    N, K = c["shape"][0], c["shape"][4]
    u = torch.zeros(N * c["P"] * c["Q"], K)
    for k, m in sites:
        u[m, k] = 1.0
    return u.reshape(1, N, c["P"], c["Q"], K)


def tap_hits(c, site):
    """bool [R,S]: the taps under which some anchor pixel gathers the site (n, h, w) of v"""
    N, H, W, C, K, Rr, S = c["shape"]
    v = torch.zeros(N, H, W, 1, dtype=torch.float64)
    v[site[0], site[1], site[2], 0] = 1.0
    return R.wgrad_direct(torch.ones(N, c["P"], c["Q"], 1, dtype=torch.float64), v, geom(c))[..., 0, 0] != 0


def wino_tap_reach(c, site):
    """bool [R,S]: the taps a NaN at the site may reach in the Winograd forms: every tap (3x3); the taps of the site's parity (two-tap form)"""
    Rr, S = c["shape"][5:]
    out = torch.ones(Rr, S, dtype=torch.bool)
    if c["engine"] == "s2":
        out[:] = False
        out[site[1] % 2::2, site[2] % 2::2] = True
    return out


# ---- hwg_colsum ---------------------------------------------------------------------------------------------------------------------------------
# (rows, C, accumulate): one row, either side of the 256-row chunk, more chunks than the cap of 256; C = 1, 2, 3 (colsum_narrow_kernel), multiples
# of 4 below / at / above the 64 columns of a block column, other widths (the scalar kernel)
COLSUM_CASES = [(1, 1, 0), (255, 2, 1), (256, 3, 0), (257, 1, 1), (70001, 3, 0), (1, 4, 1), (255, 64, 0), (256, 20, 1), (257, 68, 0), (70001, 8, 1),
                (1, 5, 0), (255, 7, 1), (256, 66, 0), (257, 130, 1), (70001, 6, 0), (513, 132, 1)]


def colsum_chunks(rows):
    return max(1, min(256, (rows + 255) // 256))


def colsum_input(rows, C, acc):
    g = torch.Generator().manual_seed(rows * 131 + C)
    return torch.randn(rows, C, generator=g), (torch.randn(C, generator=g) * rows ** 0.5 if acc else None)
