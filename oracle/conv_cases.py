"""Case tables of tests/test_conv_fp64_gpu.py: the forward-type convolution products (hwg_conv_fwd with its MFMA, split-reduce, C == 1 and
K <= 2 kernels, hwg_wino_conv_fwd, hwg_wino_s2_conv) and the weight-image entries, every schedule forced through the tuning variables,
at the smallest shapes that reach each regime of the dispatch code. A case is a dict:

  name, engine ("mfma" | "c1" | "to1" | "wino" | "s2"), shape (N, H, W, C, K, R, S), stride, pad, dil, transposed, P, Q, bias, acc, env
  (tuning variables), tags (the regimes it covers), pack ("plain" | "flip" | "strides": how the Winograd weight image's source is laid out).

Host-side restatements of the planners (which schedule a forced case must run, how large its workspace is) are here as well;
tests/test_conv_ref_cpu.py holds them against the library's own queries, which need no GPU."""
import zlib

import torch

from oracle import conv_ref as R

CASES = []


def _add(engine, name, shape, stride=(1, 1), pad=(0, 0), dil=(1, 1), transposed=0, opad=(0, 0), bias=True, acc=False, env=None, tags=(), pack="plain"):
    N, H, W, C, K, Rr, S = shape
    P, Q = R.out_size(H, W, Rr, S, stride, pad, dil, transposed, opad)
    assert P > 0 and Q > 0, name
    assert name not in [c["name"] for c in CASES], name
    c = dict(name=name, engine=engine, shape=shape, stride=stride, pad=pad, dil=dil, transposed=transposed, opad=opad, P=P, Q=Q, bias=bias, acc=acc,
             env=dict(env or {}), tags=set(tags), pack=pack)
    CASES.append(c)
    return c


def geom(c):
    return dict(stride=c["stride"], pad=c["pad"], dil=c["dil"], P=c["P"], Q=c["Q"], transposed=c["transposed"])


def out_numel(c):
    return c["shape"][0] * c["P"] * c["Q"] * c["shape"][4]


def inputs(c, kind="randn"):
    """x [N,H,W,C], logical weight w [R,S,K,C], bias [K] or None, y0 [N,P,Q,K] or None - fp32, seeded by the case's name"""
    N, H, W, C, K, Rr, S = c["shape"]
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()) & 0x7FFFFFFF)
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(Rr, S, K, C, generator=g) / (Rr * S * C) ** 0.5
    b = torch.randn(K, generator=g) if c["bias"] else None
    y0 = torch.randn(N, c["P"], c["Q"], K, generator=g) if c["acc"] else None
    return x, w, b, y0


# ---- planners, restated -------------------------------------------------------------------------------------------------------------------
def mfma_plan(c):
    """(engine 0, schedule id, split) hwg_last_plan reports for a forced MFMA case, and the workspace bytes (conv_mfma.hip: plan_conv_model)"""
    N, H, W, C, K, Rr, S = c["shape"]
    sh, sw = c["stride"]
    bm, bn, ns = _force(c)
    bk = 32 if C % 32 == 0 else 16
    merged = bool(c["transposed"] and sh * sw > 1 and Rr % sh == 0 and S % sw == 0 and (c["env"].get("HWG_CONV_MERGE") == "2"))
    min_taps = (Rr // sh) * (S // sw) if c["transposed"] else Rr * S
    min_steps = max(min_taps, 1) * (C // bk)
    while ns > 1 and min_steps // ns < 3:
        ns -= 1
    ws = ns * out_numel(c) * 4 if ns > 1 else 0
    return (0, bm * 1000 + bn + (1000000 if merged else 0), ns), ws


def _force(c):
    bm, bn, bk, ns = (int(v) for v in c["env"]["HWG_CONV_FORCE"].split(","))
    return bm, bn, ns


def mfma_mode(c):
    return 0 if not c["transposed"] else (2 if mfma_plan(c)[0][1] >= 1000000 else 1)


def mfma_M(c):
    """rows of the implicit GEMM (per parity class; the merged form: the shared block grid)"""
    N, H, W, C, K, Rr, S = c["shape"]
    (sh, sw), (ph, pw), P, Q = c["stride"], c["pad"], c["P"], c["Q"]
    if not c["transposed"]:
        return N * P * Q
    if mfma_mode(c) == 1:
        return N * -(-P // sh) * -(-Q // sw)
    Pm = max(-(-(P - k) // sh) + (k + ph) // sh for k in range(sh))
    Qm = max(-(-(Q - k) // sw) + (k + pw) // sw for k in range(sw))
    return N * Pm * Qm


def c1_kernel(c):
    """which kernel hwg_conv_c1_fwd_impl launches (conv_direct.hip), "refused" where it returns an error"""
    N, H, W, C, K, Rr, S = c["shape"]
    if (c["env"].get("HWG_C1_ROWS", "1") != "0" and K in (32, 64) and Rr == S and Rr in (3, 5, 7) and c["stride"] == (1, 1) and c["dil"] == (1, 1)):
        return "c1_rows"
    if c["env"].get("HWG_C1_MFMA", "1") != "0" and K in (32, 64) and 36 <= Rr * S <= 64:
        return "c1_mfma"
    KG = (K + 3) // 4
    return "refused" if KG > 256 or Rr * S * KG * 16 > 64 * 1024 else "c1"


def to1_kernel(c):
    """(kernel, lanes per pixel, blocks) of hwg_conv_to1_fwd_impl"""
    N, H, W, C, K, Rr, S = c["shape"]
    lanes = c["env"].get("HWG_TO1_LANES", "1") != "0"
    C4 = C // 4
    E = Rr * S * C4
    lpp = 4 if E <= 4 else 16 if E <= 16 else 64
    if lanes and E > 16 and C4 <= 16:
        lpp = 4 if C4 <= 4 else 16
    blocks = min(max((N * c["P"] * c["Q"] * lpp // 64 + 3) // 4, 1), 4096)
    r3 = lanes and K == 1 and Rr == 3 and S == 3 and c["stride"] == (1, 1) and c["dil"] == (1, 1) and 4 < C4 <= 16
    return ("to1_3x3" if r3 else "to1"), (16 if r3 else lpp), blocks


def _bal_owner(G, U, u):
    return ((u + 1) * G - 1) // U


def wino_plan(c):
    """what hwg_wino_conv_describe reports for a forced Winograd / two-tap case: [cfg, uniform split, balanced workgroups, lead tiles, pieces,
    workgroup tiles, channel chunks, most tiles a tail workgroup touches], the last_plan triple and the workspace bytes (conv_wino.hip)"""
    N, H, W, C, K, Rr, S = c["shape"]
    P, Q = c["P"], c["Q"]
    if c["engine"] == "s2":
        if c["transposed"]:
            Cv, Kv, Pv, Qv = C, 4 * K, H + 1, W + 1
        else:
            Cv, Kv, Pv, Qv = 4 * C, K, P, Q
        cfg, tm, tn, M, sched = 6, 64, 64, N * -(-Pv // 3) * -(-Qv // 3), 36
    else:
        cfg = int(c["env"].get("HWG_WINO_FORCE", "6").split(",")[0])
        tm, tn = {0: (64, 32), 1: (32, 64), 2: (128, 16), 5: (64, 64), 6: (64, 64), 7: (32, 32)}[cfg]
        Cv, Kv, M, sched = C, K, N * -(-P // 2) * -(-Q // 2), cfg
    chunks = Cv // 16
    tiles = -(-M // tm) * -(-Kv // tn)
    bal = c["env"].get("HWG_WINO_BAL", "-1")
    if not bal.startswith("-"):
        f = [int(v) for v in bal.split(",")]
        G, lead = f[0], (f[1] if len(f) > 1 else tiles // 256 * 256)
        rem = tiles - lead
        units = rem * chunks
        G = min(G, units)
        per = [_bal_owner(G, units, t * chunks + chunks - 1) - _bal_owner(G, units, t * chunks) + 1 for t in range(rem)]
        pieces = max(per)
        segs = max((units * (g + 1) // G - 1) // chunks - (units * g // G) // chunks + 1 for g in range(G) if units * (g + 1) // G > units * g // G)
        return [6, 1, G, lead, pieces, tiles, chunks, segs], (6, sched, -G), (pieces * out_numel(c) * 4 if pieces > 1 else 0), per
    ns = min(int(c["env"]["HWG_WINO_FORCE"].split(",")[1]), chunks)
    return [cfg, ns, 0, 0, ns, tiles, chunks, 1], (6, sched, ns), (ns * out_numel(c) * 4 if ns > 1 else 0), []


def pieces(c):
    """partial images summed into an output element at most (1: none)"""
    if c["engine"] == "mfma":
        return mfma_plan(c)[0][2]
    if c["engine"] in ("wino", "s2"):
        return wino_plan(c)[0][4]
    return 1


def contraction(c):
    """T of the bound: products summed into one output element by one workgroup's accumulator chain"""
    N, H, W, C, K, Rr, S = c["shape"]
    if c["engine"] == "wino":
        return C
    if c["engine"] == "s2":
        return C if c["transposed"] else 4 * C
    if c["transposed"]:
        return -(-Rr // c["stride"][0]) * -(-S // c["stride"][1]) * C
    return Rr * S * C


def workspace_entry(c):
    return {"wino": ("hwg_wino_conv_fwd", "hwg_wino_conv_workspace"), "s2": ("hwg_wino_s2_conv", "hwg_wino_s2_workspace")}.get(
        c["engine"], ("hwg_conv_fwd", "hwg_conv_fwd_workspace"))


# ---- hwg_conv_fwd: conv_mfma_kernel + conv_split_reduce_kernel ------------------------------------------------------------------------------
TILES = [(128, 128), (128, 64), (128, 32), (64, 64)]
_rot = [0]


def _mfma(name, shape, tile, ns=1, merge=None, tags=(), **kw):
    """bias / accumulate rotate through their four combinations unless given"""
    k = _rot[0]
    _rot[0] += 1
    kw.setdefault("bias", bool(k & 1))
    kw.setdefault("acc", bool(k & 2))
    C = shape[3]
    env = dict(HWG_CONV_FORCE="%d,%d,%d,%d" % (tile[0], tile[1], 32 if C % 32 == 0 else 16, ns))
    if merge is not None:
        env["HWG_CONV_MERGE"] = merge
    return _add("mfma", name, shape, env=env, tags=set(tags) | {"tile%dx%d" % tile}, **kw)


# M = N P Q against the tile: below one (seven padded, empty workgroup columns), exactly one, one + 1, more than 8 with a ragged last one
_mfma("m_below_128x128", (1, 3, 5, 32, 130, 1, 1), (128, 128), tags={"M<bm", "K130", "C32", "1x1"}, bias=True, acc=False)
_mfma("m_exact_128x64", (1, 8, 16, 16, 78, 1, 1), (128, 64), tags={"M=bm", "K78", "C16"}, bias=False, acc=True)
_mfma("m_plus1_128x32", (1, 3, 43, 48, 4, 1, 1), (128, 32), tags={"M=bm+1", "K4", "C48"}, bias=True, acc=True)
_mfma("m_9tiles_128x128", (3, 5, 77, 96, 80, 1, 1), (128, 128), tags={"M>8bm", "K80", "C96"}, bias=False, acc=False)
_mfma("m_plus1_64x64", (1, 5, 13, 32, 78, 3, 3), (64, 64), pad=(1, 1), tags={"M=bm+1", "3x3p1"}, bias=True, acc=True)
_mfma("m_19tiles_64x64", (3, 5, 77, 16, 130, 1, 1), (64, 64), tags={"M>8bm"}, bias=False, acc=False)
_mfma("m_exact_64x64", (1, 4, 16, 32, 80, 3, 3), (64, 64), pad=(1, 1), tags={"M=bm"}, bias=False, acc=True)
_mfma("m_below_64x64", (1, 2, 9, 48, 4, 1, 1), (64, 64), tags={"M<bm"}, bias=True, acc=False)
_mfma("m_9tiles_128x64", (3, 5, 77, 32, 78, 3, 3), (128, 64), pad=(1, 1), tags={"M>8bm"}, bias=True, acc=False)
_mfma("m_9tiles_128x32", (3, 5, 77, 16, 4, 1, 1), (128, 32), tags={"M>8bm"}, bias=False, acc=False)
_mfma("m_below_128x64", (2, 2, 7, 96, 130, 1, 1), (128, 64), tags={"M<bm"}, bias=True, acc=True)
_mfma("m_exact_128x128", (2, 4, 16, 48, 80, 1, 1), (128, 128), tags={"M=bm"}, bias=True, acc=True)
_mfma("m_plus1_128x128", (1, 3, 43, 16, 78, 1, 1), (128, 128), tags={"M=bm+1"}, bias=False, acc=True)
_mfma("m_below_128x32", (1, 1, 6, 32, 80, 1, 1), (128, 32), tags={"M<bm"}, bias=False, acc=True)
# taps
_mfma("tap_1x3_dil4", (2, 1, 50, 32, 80, 1, 3), (128, 64), pad=(0, 4), dil=(1, 4), tags={"1x3d4"})
_mfma("tap_3x3_pad0", (2, 6, 11, 48, 78, 3, 3), (128, 128), tags={"3x3p0"})
_mfma("tap_3x3_pad2", (1, 4, 9, 16, 80, 3, 3), (64, 64), pad=(2, 2), tags={"3x3p2"})
_mfma("tap_3x3_s31_onerow", (2, 3, 40, 32, 130, 3, 3), (128, 128), stride=(3, 1), pad=(0, 1), tags={"3x3s31"})
_mfma("tap_4x4_s2", (2, 10, 14, 32, 80, 4, 4), (128, 64), stride=(2, 2), pad=(1, 1), tags={"4x4s2"})
_mfma("tap_4x4_s21", (2, 10, 9, 16, 4, 4, 4), (128, 32), stride=(2, 1), pad=(1, 0), tags={"4x4s21"})
_mfma("tap_5x5_pad2", (1, 7, 9, 16, 78, 5, 5), (64, 64), pad=(2, 2), tags={"5x5p2"})
_mfma("tap_dil21", (2, 9, 9, 32, 80, 3, 3), (128, 128), pad=(2, 1), dil=(2, 1), tags={"d21"})
# split: 3x3, C = 64 = 18 steps of 32 channels; 4 pieces is an uneven split; K = 78 takes the scalar body of the reduce kernel
for _ns, _tile, _b, _a in ((2, (128, 128), True, False), (3, (128, 64), False, True), (4, (64, 64), True, True), (6, (128, 32), False, False)):
    _mfma("split%d_%dx%d" % ((_ns,) + _tile), (2, 9, 20, 64, 80, 3, 3), _tile, ns=_ns, pad=(1, 1), tags={"split%d" % _ns, "split"}, bias=_b, acc=_a)
_mfma("split2_k78_scalar", (1, 7, 11, 64, 78, 3, 3), (64, 64), ns=2, pad=(1, 1), tags={"split", "split_scalar"}, bias=True, acc=True)
_mfma("split3_k130_scalar", (1, 7, 11, 64, 130, 3, 3), (128, 128), ns=3, pad=(1, 1), tags={"split", "split_scalar"}, bias=False, acc=False)
# fractionally strided: by class (mode 1) and merged (mode 2)
_T = [("t_4x4s2_p0", (2, 7, 9, 32, 64, 4, 4), (2, 2), (0, 0), (0, 0), {"t4x4s2p0"}),
      ("t_4x4s2_p1", (2, 8, 10, 64, 32, 4, 4), (2, 2), (1, 1), (0, 0), {"t4x4s2p1"}),
      ("t_4x4_s21", (3, 5, 13, 48, 80, 4, 4), (2, 1), (0, 0), (0, 0), {"ts21"}),
      ("t_6x3_s31", (2, 1, 30, 64, 40, 6, 3), (3, 1), (0, 1), (0, 0), {"t6x3s31", "tonerow"}),
      ("t_opad_k24", (2, 5, 11, 32, 24, 4, 4), (2, 2), (1, 1), (1, 1), {"topad", "tk24"}),
      ("t_onerow", (2, 1, 20, 32, 64, 4, 4), (2, 2), (0, 0), (0, 0), {"tonerow"})]
for _i, (_n, _s, _st, _pd, _op, _tg) in enumerate(_T):
    for _j, _m in enumerate(("0", "2")):
        _mfma("%s_%s" % (_n, "class" if _m == "0" else "merged"), _s, TILES[(_i + 2 * _j) % 4], merge=_m, stride=_st, pad=_pd, opad=_op, transposed=1,
              tags=_tg | {"byclass" if _m == "0" else "merged"})
_mfma("t_3x3s2_class_only", (2, 5, 9, 32, 48, 3, 3), (128, 64), merge="2", stride=(2, 2), pad=(1, 1), transposed=1, tags={"t3x3s2", "byclass"})
for _m, _tile, _b, _a in (("0", (64, 64), True, True), ("2", (128, 128), False, True), ("0", (128, 32), False, False), ("2", (128, 64), True, False)):
    _mfma("t_split2_%s_%dx%d" % (("class" if _m == "0" else "merged",) + _tile), (2, 8, 10, 64, 32, 4, 4), _tile, ns=2, merge=_m, stride=(2, 2), pad=(1, 1),
          transposed=1, tags={"split", "byclass" if _m == "0" else "merged"}, bias=_b, acc=_a)

# ---- hwg_conv_fwd, C == 1 ------------------------------------------------------------------------------------------------------------------
def _c1(name, shape, tags=(), **kw):
    k = _rot[0]
    _rot[0] += 1
    kw.setdefault("bias", bool(k & 1))
    kw.setdefault("acc", bool(k & 2))
    return _add("c1", name, shape, tags=tags, **kw)


_c1("rows_3x3_k32_q129", (1, 4, 129, 1, 32, 3, 3), pad=(1, 1), tags={"rows", "q129", "pad1"})
_c1("rows_5x5_k64_q128", (2, 5, 130, 1, 64, 5, 5), pad=(1, 1), tags={"rows", "q128"})
_c1("rows_7x7_k32_q127", (1, 9, 133, 1, 32, 7, 7), tags={"rows", "q127", "pad0"})
_c1("rows_7x7_k64_pad3", (1, 6, 127, 1, 64, 7, 7), pad=(3, 3), tags={"rows", "q127", "pad3"})
_c1("rows_3x3_k64_pad2", (2, 3, 127, 1, 64, 3, 3), pad=(2, 2), tags={"rows", "q129", "pad2"})
_c1("rows_5x5_k32_pad23", (1, 7, 126, 1, 32, 5, 5), pad=(2, 3), tags={"rows", "q128"})
_c1("rows_second_trip", (3, 700, 10, 1, 32, 3, 3), pad=(1, 1), tags={"rows", "second_trip", "large"}, bias=True, acc=True)
_c1("c1mfma_6x6_k32", (2, 12, 15, 1, 32, 6, 6), pad=(2, 2), tags={"c1mfma", "6x6"})
_c1("c1mfma_7x7_dil12_k64", (1, 13, 30, 1, 64, 7, 7), pad=(3, 6), dil=(1, 2), tags={"c1mfma", "7x7d12", "tp50"})
_c1("c1mfma_7x7_s2_k32", (2, 15, 17, 1, 32, 7, 7), stride=(2, 2), pad=(3, 3), tags={"c1mfma", "7x7s2", "tp50"})
_c1("c1mfma_8x8_k64", (1, 11, 20, 1, 64, 8, 8), pad=(3, 3), tags={"c1mfma", "8x8"})
_c1("c1mfma_second_trip", (1, 211, 511, 1, 32, 6, 6), tags={"c1mfma", "second_trip", "large"}, bias=True, acc=True)
_c1("valu_k3", (1, 2, 1030, 1, 3, 3, 3), pad=(1, 1), tags={"valu", "k3"})
_c1("valu_k5", (2, 3, 515, 1, 5, 3, 3), pad=(1, 1), tags={"valu", "k5"})
_c1("valu_k80", (1, 4, 50, 1, 80, 5, 5), pad=(2, 2), tags={"valu", "k80"})
_c1("valu_k256", (1, 3, 19, 1, 256, 3, 3), pad=(1, 1), tags={"valu", "k256"})
_c1("valu_k32_4x4_s2", (2, 10, 22, 1, 32, 4, 4), stride=(2, 2), pad=(1, 1), tags={"valu", "k32_4x4s2"})
_c1("valu_9x9_k32", (1, 12, 21, 1, 32, 9, 9), pad=(4, 4), tags={"valu", "9x9"})
_c1("valu_k32_3x3_rows_off", (1, 5, 37, 1, 32, 3, 3), pad=(1, 1), env=dict(HWG_C1_ROWS="0"), tags={"valu", "rows_off"})
_c1("valu_7x7_k64_mfma_off", (1, 9, 14, 1, 64, 7, 7), pad=(3, 3), dil=(1, 2), env=dict(HWG_C1_MFMA="0"), tags={"valu", "mfma_off"})
REFUSED = _c1("valu_refused_k256_9x9", (1, 9, 12, 1, 256, 9, 9), pad=(4, 4), tags={"refused"}, bias=True, acc=False)

# ---- hwg_conv_fwd, K <= 2 ------------------------------------------------------------------------------------------------------------------
def _to1(name, shape, tags=(), **kw):
    k = _rot[0]
    _rot[0] += 1
    kw.setdefault("bias", bool(k & 1))
    kw.setdefault("acc", bool(k & 2))
    return _add("to1", name, shape, tags=tags, **kw)


_to1("to1_c4_1x1", (2, 5, 13, 4, 1, 1, 1), tags={"lpp4", "E<=4"})
_to1("to1_c16_1x1_k2", (1, 7, 9, 16, 2, 1, 1), tags={"lpp4", "E<=4", "k2"})
_to1("to1_c64_1x1", (2, 3, 11, 64, 1, 1, 1), tags={"lpp16"})
_to1("to1_c16_3x3_lanes", (2, 6, 9, 16, 2, 3, 3), pad=(1, 1), tags={"lanes4"})
_to1("to1_c32_3x3_k2", (1, 7, 10, 32, 2, 3, 3), pad=(1, 1), tags={"lanes16", "k2"})
_to1("to1_c32_3x3_k1", (2, 5, 9, 32, 1, 3, 3), pad=(1, 1), tags={"3x3kernel"})
_to1("to1_c48_3x3_k1", (1, 6, 11, 48, 1, 3, 3), pad=(0, 0), tags={"3x3kernel", "12of16"})
_to1("to1_c256_3x3", (1, 4, 7, 256, 1, 3, 3), pad=(1, 1), tags={"lpp64"})
_to1("to1_c20_1x1", (1, 5, 7, 20, 2, 1, 1), tags={"c20"})
_to1("to1_c20_3x3_s2", (2, 9, 11, 20, 1, 3, 3), stride=(2, 2), pad=(1, 1), tags={"c20", "stride2"})
_to1("to1_c32_3x3_dil2", (1, 9, 12, 32, 1, 3, 3), pad=(0, 0), dil=(2, 2), tags={"dil2", "pad0"})
_to1("to1_c16_3x3_lanes_off", (1, 5, 8, 16, 1, 3, 3), pad=(1, 1), env=dict(HWG_TO1_LANES="0"), tags={"lanes_off", "lpp64"})
_to1("to1_second_trip", (2, 96, 100, 80, 1, 3, 3), pad=(1, 1), tags={"second_trip", "large", "lpp64"}, bias=True, acc=True)

# ---- hwg_wino_conv_fwd --------------------------------------------------------------------------------------------------------------------
def _wino(name, shape, pad, cfg=None, ns=1, bal=None, tags=(), **kw):
    k = _rot[0]
    _rot[0] += 1
    kw.setdefault("bias", bool(k & 1))
    kw.setdefault("acc", bool(k & 2))
    N, H, W, C, K = shape
    env = dict(HWG_WINO="2")
    if bal is None:
        env.update(HWG_WINO_FORCE="%d,%d" % (cfg, ns), HWG_WINO_BAL="-1")
        tags = set(tags) | {"cfg%d" % cfg, "cfg%d_ns%d" % (cfg, ns)}
    else:
        env.update(HWG_WINO_BAL=bal)
        tags = set(tags) | {"bal"}
    return _add("wino", name, (N, H, W, C, K, 3, 3), pad=pad, env=env, tags=tags, **kw)


# shapes of the forced-schedule size: K % 4 != 0 and % 16 != 0, one tile plus two channels; odd P / Q; one output row; pads 0 / 1 / 2
WINO_SHAPES = [((2, 13, 37, 64, 78), (1, 1)), ((1, 9, 33, 64, 66), (0, 1)), ((3, 7, 21, 64, 34), (2, 2)), ((2, 5, 19, 96, 50), (0, 0)),
               ((2, 3, 20, 64, 66), (0, 1)), ((1, 6, 10, 16, 18), (1, 0))]
_k = 0
for _cfg in (0, 1, 2, 5, 6, 7):
    for _ns in (1, 2, 4):
        for _rep in range(2):
            _sh, _pd = WINO_SHAPES[_k % 5]
            _k += 1
            _wino("w_cfg%d_ns%d_%s" % (_cfg, _ns, "x".join(map(str, _sh))), _sh, _pd, cfg=_cfg, ns=_ns,
                  pack=("plain", "flip", "strides")[_k % 3], tags={"K%d" % _sh[4], "pad%d%d" % _pd} | ({"P1_H3"} if _sh[1] == 3 else set()))
_wino("w_cfg2_c16_k18", (1, 6, 10, 16, 18), (1, 0), cfg=2, ns=1, tags={"K18", "M<tm"})
_wino("w_cfg0_c16_k18", (1, 6, 10, 16, 18), (1, 0), cfg=0, ns=2, tags={"K18", "M<tm", "one_chunk"})
# M = N ceil(P/2) ceil(Q/2) one past the tile, on one output row from H = 1 with padding 1
_wino("w_tm64_plus1_cfg6", (1, 1, 129, 64, 78), (1, 1), cfg=6, ns=1, tags={"M=tm+1", "P1_H1"})
_wino("w_tm64_plus1_cfg0", (1, 1, 129, 32, 34), (1, 1), cfg=0, ns=2, tags={"M=tm+1", "P1_H1"})
_wino("w_tm32_plus1_cfg1", (1, 1, 65, 32, 66), (1, 1), cfg=1, ns=1, tags={"M=tm+1", "P1_H1"})
_wino("w_tm32_plus1_cfg7", (1, 1, 65, 64, 50), (1, 1), cfg=7, ns=4, tags={"M=tm+1", "P1_H1"})
_wino("w_tm128_plus1_cfg2", (1, 1, 257, 32, 18), (1, 1), cfg=2, ns=2, tags={"M=tm+1", "P1_H1"})
_wino("w_tm64_plus1_cfg5", (1, 3, 129, 64, 66), (0, 1), cfg=5, ns=1, tags={"M=tm+1", "P1_H3"})
# accumulate on the uniform and the split schedule (every combination also rotates above)
_wino("w_acc_uniform", (2, 13, 37, 64, 78), (1, 1), cfg=6, ns=1, bias=True, acc=True, tags={"acc_uniform"})
_wino("w_acc_split", (2, 13, 37, 64, 78), (1, 1), cfg=6, ns=4, bias=True, acc=True, tags={"acc_split"})
# balanced schedule of the 64 x 64 kernel: 10 tiles x 4 chunks; tiles in one piece (G = 10), two (3, 7) and four (40); with a lead region
_wino("w_bal10_one_piece", (2, 13, 37, 64, 78), (1, 1), bal="10", tags={"bal_pieces1"}, bias=True, acc=True)
_wino("w_bal3_k78", (2, 13, 37, 64, 78), (1, 1), bal="3", tags={"bal_pieces2", "bal_reduce1"}, bias=True, acc=False)
_wino("w_bal7_k78_acc", (2, 13, 37, 64, 78), (1, 1), bal="7", tags={"bal_pieces2", "bal_reduce1", "acc_bal"}, bias=True, acc=True)
_wino("w_bal40_k78", (2, 13, 37, 64, 78), (1, 1), bal="40", tags={"bal_pieces3+", "bal_reduce1"}, bias=False, acc=True)
_wino("w_bal7_k80", (2, 13, 37, 64, 80), (1, 1), bal="7", tags={"bal_pieces2", "bal_reduce4", "acc_bal"}, bias=False, acc=True, pack="flip")
_wino("w_bal40_k96_c96", (2, 5, 19, 96, 96), (0, 0), bal="11", tags={"bal_pieces3+", "bal_reduce4"}, bias=True, acc=False, pack="strides")
_wino("w_bal5_k66", (1, 9, 33, 64, 66), (0, 1), bal="5", tags={"bal_reduce1"}, bias=True, acc=True)

# ---- hwg_wino_s2_conv ---------------------------------------------------------------------------------------------------------------------
def _s2(name, shape, dgrad=0, ns=None, bal=None, tags=(), **kw):
    N, H, W, C, K = shape
    env = dict(HWG_WINO_S2="2", HWG_WINO_BAL="-1" if bal is None else bal)
    env["HWG_WINO_FORCE"] = "6,%d" % (ns or 1)
    if bal is not None:
        env.pop("HWG_WINO_FORCE")
    kw.setdefault("bias", not dgrad)
    return _add("s2", name, (N, H, W, C, K, 4, 4), stride=(2, 2), transposed=dgrad, env=env,
                tags=set(tags) | {"dgrad" if dgrad else "fwd"}, **kw)


_s2("s2_fwd_k64", (2, 12, 20, 16, 64), tags={"K64", "ragged3"}, acc=False)
_s2("s2_fwd_k80", (1, 10, 38, 32, 80), tags={"K80", "ragged3"}, acc=True)
_s2("s2_fwd_k96_odd", (2, 15, 23, 16, 96), tags={"K96", "ragged3"}, acc=False, bias=False)
_s2("s2_fwd_two_tiles", (3, 26, 50, 16, 64), tags={"K64", "M>tm"}, acc=True)
_s2("s2_fwd_split2", (3, 8, 26, 16, 64), ns=2, tags={"split"}, acc=True)
_s2("s2_fwd_split4_k80", (2, 6, 34, 32, 80), ns=4, tags={"split"}, acc=False)
_s2("s2_fwd_bal3", (2, 14, 22, 16, 96), bal="3", tags={"bal", "bal_cut"}, acc=True)
_s2("s2_fwd_bal7", (2, 14, 44, 48, 64), bal="7", tags={"bal", "bal_cut"}, acc=False)
_s2("s2_dgrad_k16", (2, 5, 9, 64, 16), dgrad=1, tags={"acc_dgrad"}, acc=True)
_s2("s2_dgrad_k32", (1, 4, 18, 80, 32), dgrad=1, acc=False)
_s2("s2_dgrad_split2", (2, 3, 10, 64, 16), dgrad=1, ns=2, tags={"split"}, acc=True)
_s2("s2_dgrad_bal5", (2, 5, 9, 64, 32), dgrad=1, bal="5", tags={"bal", "bal_cut"}, acc=True)

BY_NAME = {c["name"]: c for c in CASES}
RUN_CASES = [c for c in CASES if "refused" not in c["tags"]]


def of_engine(e):
    return [c for c in RUN_CASES if c["engine"] == e]


# the smallest cases of each engine: impulses and the single NaN
INDEX_CASES = ["m_plus1_64x64", "m_9tiles_128x64", "tap_3x3_pad0", "tap_4x4_s2", "split2_k78_scalar", "t_4x4s2_p1_class", "t_4x4s2_p1_merged", "t_opad_k24_merged",
               "t_split2_class_64x64", "rows_3x3_k32_q129", "c1mfma_6x6_k32", "valu_k5", "to1_c16_3x3_lanes", "to1_c32_3x3_k1", "to1_c20_3x3_s2",
               "w_cfg0_ns2_3x7x21x64x34", "w_cfg6_ns1_2x13x37x64x78", "w_cfg5_ns2_2x13x37x64x78", "w_bal7_k78_acc", "s2_fwd_k64", "s2_fwd_two_tiles", "s2_dgrad_k16"]


def impulse_sites(c):
    """[[(label, (n, h, w, ch)), ...], ...]: the ones of the impulse inputs - the four corners, the pixels on either side of the first tile
    boundary of the implicit GEMM's rows, the first and last channel, the first channel of the second contraction step, the last image -
    shared out over as few inputs as it takes to keep the output footprints within one input disjoint (neighbouring pixels overlap under any
    filter wider than one tap; tests/test_conv_ref_cpu.py asserts the disjointness for the table)"""
    N, H, W, C, K, Rr, S = c["shape"]
    bk = 16 if c["engine"] in ("wino", "s2") else (32 if C % 32 == 0 else 16)
    c2 = min(bk, C - 1)
    cand = [("corner00_ch0", (0, 0, 0, 0)), ("corner0W_chlast", (0, 0, W - 1, C - 1)), ("cornerH0_step2", (0, H - 1, 0, c2)),
            ("cornerHW_lastimage", (N - 1, H - 1, W - 1, C - 1)), ("lastimage_00", (N - 1, 0, 0, c2))]
    # either side of the first tile boundary: the input pixels under the centre tap of rows bm - 1 and bm of the implicit GEMM (Winograd: of
    # the first output pixel of tiles tm - 1 and tm)
    bm = {"mfma": _force(c)[0] if c["engine"] == "mfma" else 0, "c1": 128, "to1": 16}.get(c["engine"], 64)
    unit = {"wino": 2, "s2": 3}.get(c["engine"], 1)
    if c["transposed"]:
        gp, gq = (H, W) if c["engine"] == "mfma" else (-(-(H + 1) // 3), -(-(W + 1) // 3))
    else:
        gp, gq = -(-c["P"] // unit), -(-c["Q"] // unit)
    for lab, m in (("boundary_lo", bm - 1), ("boundary_hi", bm)):
        n, t = divmod(m, gp * gq)
        tp, tq = divmod(t, gq)
        if n >= N:
            continue
        if c["transposed"]:
            h, w_ = tp * unit, tq * unit
        else:
            h = tp * unit * c["stride"][0] - c["pad"][0] + (Rr // 2) * c["dil"][0]
            w_ = tq * unit * c["stride"][1] - c["pad"][1] + (S // 2) * c["dil"][1]
        cand.append((lab, (n, min(max(h, 0), H - 1), min(max(w_, 0), W - 1), (m * 7) % C)))
    sets = []
    for lab, s in cand:
        fp = site_footprint(c, s)
        for st in sets:
            if not bool((st[1] & fp).any()):
                st[0].append((lab, s))
                st[1] |= fp
                break
        else:
            sets.append([[(lab, s)], fp.clone()])
    return [st[0] for st in sets]


def site_footprint(c, site):
    """bool [N,P,Q]: the output pixels an input pixel reaches"""
    N, H, W, C, K, Rr, S = c["shape"]
    x = torch.zeros(N, H, W, 1, dtype=torch.float64)
    x[site[0], site[1], site[2], 0] = 1.0
    return R.conv_direct(x, torch.ones(Rr, S, 1, 1, dtype=torch.float64), geom(c))[..., 0] != 0


def wino_tile_footprint(c, site):
    """bool [N,P,Q]: the outputs of the Winograd tiles whose 4x4 input patch holds the pixel (what a NaN there may reach): tile t of m outputs
    reads rows m t .. m t + 3 of the padded image"""
    N, H, W, C, K, Rr, S = c["shape"]
    n, h, w_ = site[:3]
    if c["engine"] == "wino":
        m, hp, wp, Pv, Qv, rep = 2, h + c["pad"][0], w_ + c["pad"][1], c["P"], c["Q"], 1
    elif not c["transposed"]:
        m, hp, wp, Pv, Qv, rep = 3, h // 2, w_ // 2, c["P"], c["Q"], 1           # the pixel of the space-to-depth image
    else:
        m, hp, wp, Pv, Qv, rep = 3, h + 1, w_ + 1, H + 1, W + 1, 2              # outputs: the 2x2 blocks of dx
    out = torch.zeros(N, Pv, Qv, dtype=torch.bool)
    for tp in range(-(-Pv // m)):
        for tq in range(-(-Qv // m)):
            if m * tp <= hp <= m * tp + 3 and m * tq <= wp <= m * tq + 3:
                out[n, m * tp:m * tp + m, m * tq:m * tq + m] = True
    if rep == 2:
        out = out[:, :, None, :, None].expand(N, Pv, 2, Qv, 2).reshape(N, 2 * Pv, 2 * Qv)
    return out


# ---- the pack entries -----------------------------------------------------------------------------------------------------------------------
# (name, A, B, Bpad, R, S, layout "ab" = [A,B,R,S] source / "ba" = [B,A,R,S] source (the [C,K,R,S] strides of a transposed layer), flip)
PACK_CASES = [("plain_16x16_3x3", 16, 16, 16, 3, 3, "ab", 0), ("ragged_13x7_pad16", 13, 7, 16, 3, 3, "ab", 0), ("flip_5x9_pad12_4x4", 5, 9, 12, 4, 4, "ab", 1),
              ("ckrs_18x20_pad32_flip", 18, 20, 32, 3, 3, "ba", 1), ("ckrs_3x1_7x7", 33, 1, 1, 7, 7, "ba", 0), ("taps_1x1_49x24", 49, 24, 24, 1, 1, "ba", 0),
              ("rect_6x3_40x17_pad32", 40, 17, 32, 6, 3, "ab", 0)]
WINO_PACK_CASES = [("w_16x16", 16, 16, "ab", 0), ("w_18x20_flip", 18, 20, "ab", 1), ("w_78x48_ckrs", 78, 48, "ba", 0), ("w_33x17_ckrs_flip", 33, 17, "ba", 1)]
S2_PACK_CASES = [("s2_64x16_fwd", 64, 16, 0), ("s2_80x12_fwd", 80, 12, 0), ("s2_64x16_dgrad", 64, 16, 1), ("s2_20x7_dgrad", 20, 7, 1)]


def pack_source(name, A, B, R_, S_, layout):
    """-> (flat fp32 source, sa, sb, sr, ss)"""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    if layout == "ab":
        return torch.randn(A * B * R_ * S_, generator=g), B * R_ * S_, R_ * S_, S_, 1
    return torch.randn(A * B * R_ * S_, generator=g), R_ * S_, A * R_ * S_, S_, 1


def wino_source(c, w):
    """the source tensor hwg_wino_pack_weight reads for a Winograd case, from the logical weight w [3,3,K,C]: -> (flat src, sa, sb, flip)"""
    K, C = w.shape[2], w.shape[3]
    if c["pack"] == "plain":
        return w.permute(2, 3, 0, 1).contiguous().reshape(-1), C * 9, 9, 0
    if c["pack"] == "flip":
        return w.flip(0, 1).permute(2, 3, 0, 1).contiguous().reshape(-1), C * 9, 9, 1
    return w.permute(3, 2, 0, 1).contiguous().reshape(-1), 9, K * 9, 0


def s2_source(c, w):
    """the convolution's weight [Kc,Cc,4,4] whose image hwg_wino_s2_pack_weight makes for a two-tap case, from the descriptor's logical weight
    w [4,4,K,C]: -> (flat src, Kc, Cc, dgrad)"""
    if not c["transposed"]:
        return w.permute(2, 3, 0, 1).contiguous().reshape(-1), w.shape[2], w.shape[3], 0
    return w.permute(3, 2, 0, 1).contiguous().reshape(-1), w.shape[3], w.shape[2], 1
