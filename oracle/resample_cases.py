"""Case tables of tests/test_resample_glue_fp64_gpu.py (csrc/pool_resample.hip and the glue kernels at the end of csrc/spectral_loss.hip
against the restatements of oracle/resample_ref.py), their seeded inputs, and the regime bookkeeping tests/test_resample_glue_ref_cpu.py
checks them with. The shapes are the smallest that reach each regime of the kernels, not the workload's; one case per kernel and direction
is large enough for a second, ragged trip of the grid-stride loop (the launch grid is capped at GRID_CAP work items)."""
import zlib

import torch

GRID_BLOCKS, GRID_THREADS = 2048, 256              # hwg_stream_grid's cap, the kernels' workgroup
GRID_CAP = GRID_BLOCKS * GRID_THREADS


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def work_items(elements, C=1):
    """work items of a vectorised kernel: 4 channels each where C % 4 == 0"""
    return elements // 4 if C % 4 == 0 else elements


def trip_tags(prefix, items):
    """a second trip needs more than GRID_CAP items; ragged: the last trip is not full"""
    return {prefix + " second trip, ragged"} if items > GRID_CAP and items % GRID_CAP else set()


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


# ---- the vectorised NHWC kernels: name, op, (N, H, W, C), parameters ----------------------------------------------------------------------
BIG4, BIG1 = (2, 1030, 16, 64), (2, 1400, 64, 3)       # 2 109 440 elements in vectors of 4 / 537 600 single: both just past GRID_CAP items
NONE, RELU, LRELU = 0, 1, 2
SLOPE = 0.2
G22, GREC, G12, G33 = ((2, 2), (2, 2), (0, 0)), ((2, 2), (2, 1), (0, 1)), ((1, 2), (1, 2), (0, 0)), ((3, 3), (1, 1), (1, 1))

_AVG = [("k22_c8", (2, 6, 10, 8), (2, 2)), ("k22_c3_rem", (1, 7, 11, 3), (2, 2)), ("k12_c1_row", (2, 1, 9, 1), (1, 2)),
        ("k21_c6_col", (1, 9, 1, 6), (2, 1)), ("k12_c4", (1, 4, 8, 4), (1, 2)), ("k21_c4_rem", (2, 9, 5, 4), (2, 1)),
        ("big_v4", (2, 1030, 33, 64), (1, 2)),           # outputs 2 x 1030 x 16 x 64: the forward pass's second trip; inputs: three trips backward
        ("big_v1", (2, 1400, 256, 3), (2, 2))]           # outputs 2 x 700 x 128 x 3
_ACTS = [(RELU, True), (LRELU, False), (NONE, True), (LRELU, True), (RELU, False), (NONE, False), (LRELU, True), (RELU, False)]
_MAX = [("g22_c8_ties", (2, 6, 10, 8), G22, "quant"), ("rec_c4_ties", (2, 8, 9, 4), GREC, "quant"), ("g12_c1_row", (1, 1, 9, 1), G12, "quant"),
        ("g33_c3_ties", (1, 5, 7, 3), G33, "quant"), ("g33_c6_special", (2, 4, 6, 6), G33, "special"), ("g33_c4_col", (1, 7, 1, 4), G33, "quant"),
        ("g22_c1_rem", (2, 7, 5, 1), G22, "randn"), ("rec_c6", (1, 4, 5, 6), GREC, "randn"),
        ("big_v4", BIG4, G33, "quant"), ("big_v1", BIG1, G33, "randn")]
_UP = [("f21_c8", (2, 3, 5, 8), (2, 1)), ("f12_c3", (1, 4, 3, 3), (1, 2)), ("f22_c1_row", (2, 1, 7, 1), (2, 2)), ("f32_c6_col", (1, 5, 1, 6), (3, 2)),
       ("f22_c4", (1, 3, 4, 4), (2, 2)), ("f32_c4", (2, 2, 3, 4), (3, 2)), ("big_v4", BIG4, (2, 1)), ("big_v1", BIG1, (1, 2))]
_BLUR = [("c8", (2, 5, 7, 8)), ("c3", (1, 4, 6, 3)), ("h1_c1", (2, 1, 9, 1)), ("w1_c6", (1, 6, 1, 6)), ("h2_c4", (1, 2, 5, 4)), ("w2_c4", (2, 5, 2, 4)),
         ("big_v4", BIG4), ("big_v1", BIG1)]
# (pt, pb, pl, pr, mode, value)
_PAD = [("const_pos_c8", (2, 4, 6, 8), (1, 2, 3, 0, 0, 0.5)), ("const_crop_c3", (1, 6, 7, 3), (-1, 2, 0, -2, 0, -1.25)),
        ("const_crop_all_c4", (2, 5, 6, 4), (-1, -1, -2, -1, 0, 0.0)), ("const_h1_c4", (1, 1, 5, 4), (1, 1, 0, 2, 0, 0.0)),
        ("rep_c4", (2, 3, 4, 4), (1, 2, 2, 1, 1, 0.0)), ("rep_larger_c1", (1, 2, 3, 1), (3, 4, 5, 4, 1, 0.0)), ("rep_h1_c6", (2, 1, 5, 6), (2, 1, 1, 2, 1, 0.0)),
        ("rep_w1_c3", (1, 4, 1, 3), (0, 1, 2, 2, 1, 0.0)), ("big_v4", BIG4, (1, 0, 0, 1, 0, 2.0)), ("big_v1", BIG1, (1, 1, 1, 1, 1, 0.0))]

NHWC_CASES = ([("avgpool_" + n, "avgpool", s, dict(k=k)) for n, s, k in _AVG]
              + [("act_avgpool_" + n, "act_avgpool", s, dict(k=k, act=a, mask=m)) for (n, s, k), (a, m) in zip(_AVG, _ACTS)]
              + [("maxpool_" + n, "maxpool", s, dict(geom=g, fill=f)) for n, s, g, f in _MAX]
              + [("maxpool_relu_" + n, "maxpool_relu", s, dict(geom=g, fill=f)) for n, s, g, f in _MAX if f != "special"]
              + [("upsample_" + n, "upsample", s, dict(f=f)) for n, s, f in _UP]
              + [("blur_" + n, "blur", s, {}) for n, s in _BLUR]
              + [("pad_" + n, "pad", s, dict(pad=p)) for n, s, p in _PAD])
NHWC_OPS = ("avgpool", "act_avgpool", "maxpool", "maxpool_relu", "upsample", "blur", "pad")

# ---- the step's geometries: read off the model the shipped IAM config builds (on the meta device: no weights are allocated), walking the
# networks' module lists with the convolution arithmetic between the resampling ops; one line of STEP_H x STEP_W pixels (the batch cut to 1)
STEP_H, STEP_W, STEP_N = 64, 512, 1
_POOL_MARKERS = {"avgpool 2": (2, 2), "avgpool (1,2)": (1, 2), "maxpool 2x2": G22, "maxpool (2,2)/(2,1)/(0,1)": GREC}


def _conv_out(H, W, conv, pad=None):
    (kh, kw), (sh, sw), (dh, dw) = conv.kernel_size, conv.stride, conv.dilation
    ph, pw = conv.padding if pad is None else pad
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def _step_cases():
    from .style_cases import _step_model
    net = _step_model()
    cases, fused, N = [], [], STEP_N

    def add(op, shape, prm):
        if not any(c[1] == op and c[2] == tuple(shape) and c[3] == prm for c in NHWC_CASES + cases):
            cases.append(("step_%s_%d" % (op, len(cases)), op, tuple(int(v) for v in shape), prm))
    # generator: nearest upsample before the 3x3 conv of the 'up' blocks, the blur behind every upsampling block, the fused 4x4 weight
    H, W = 1, STEP_W // 4
    for blk in net.generator.conv:
        if blk.kind == "up":
            add("upsample", (N, H, W, blk.conv1[1].weight.shape[1]), dict(f=tuple(blk.up_scale)))
        if blk.kind == "fused":
            fused.append((int(blk.conv1[0].weight.shape[0]), int(blk.conv1[0].weight.shape[1])))
        H, W, C = blk.out_shape(N, H, W)
        if blk.kind in ("up", "fused"):
            add("blur", (N, H, W, C), {})
    assert (H, W) == (STEP_H, STEP_W)
    # discriminator: LeakyReLU + average pool in one pass behind the spectral-norm convs (a Dropout2d mask where the Sequential has one), the
    # plain average pool behind the GroupNorm layer
    d = net.discriminator
    H, W, C, spectral, drop = STEP_H, STEP_W, 1, False, False
    for seq in [d.in_conv, d.convs1, d.convs2, d.convs3] + ([d.convs4] if d.use_low else []):
        for m in seq:
            inner = getattr(m, "module", None)
            if inner is not None and hasattr(inner, "weight_bar"):
                w, (ph, pw) = inner.weight_bar, m.padding
                H, W, C, spectral, drop = H + 2 * ph - w.shape[2] + 1, W + 2 * pw - w.shape[3] + 1, int(w.shape[0]), True, False
            elif isinstance(m, torch.nn.Conv2d):
                (H, W), C, spectral, drop = _conv_out(H, W, m), m.out_channels, False, False
            elif type(m).__name__ == "Dropout2d":
                drop = True
            elif getattr(m, "what", "").startswith("avgpool"):
                k = _POOL_MARKERS[m.what]
                add("act_avgpool", (N, H, W, C), dict(k=k, act=LRELU, mask=drop)) if spectral else add("avgpool", (N, H, W, C), dict(k=k))
                H, W = H // k[0], W // k[1]
    # recogniser: every pool sits behind a conv without a norm, so all four are the ReLU variant
    r = net.hwr
    H, W, C = STEP_H, STEP_W + 2 * r.pad_cols, 1
    if r.pad_cols:
        add("pad", (N, STEP_H, STEP_W, 1), dict(pad=(0, 0, r.pad_cols, r.pad_cols, 0, 0.0)))
    for m in r.cnn:
        if isinstance(m, torch.nn.Conv2d):
            (H, W), C = _conv_out(H, W, m), m.out_channels
        elif getattr(m, "what", "").startswith("maxpool"):
            g = _POOL_MARKERS[m.what]
            add("maxpool_relu", (N, H, W, C), dict(geom=g, fill="randn"))
            H, W = (H + 2 * g[2][0] - g[0][0]) // g[1][0] + 1, (W + 2 * g[2][1] - g[0][1]) // g[1][1] + 1
    assert H == 1
    # style extractor: replicate padding in front of every trunk conv, the (1,2) ReLU max pool and the full-width average pool of the head
    s = net.style_extractor
    H, W, C = STEP_H, STEP_W, 1
    for blk in s.down:
        left, right, top, bottom = blk.padding
        if any(blk.padding):
            add("pad", (N, H, W, C), dict(pad=(top, bottom, left, right, 1 if blk.pad_mode == "replicate" else 0, 0.0)))
        (H, W), C = _conv_out(H + top + bottom, W + left + right, blk.conv, (0, 0)), blk.conv.out_channels
    assert H == 1
    add("maxpool_relu", (N, 1, W, C), dict(geom=G12, fill="randn"))
    add("avgpool", (N, 1, W // 2, C), dict(k=(1, W // 2)))
    return cases, fused


STEP_CASES, STEP_FUSED = _step_cases()
NHWC_CASES = NHWC_CASES + STEP_CASES


def out_shape(case):
    name, op, (N, H, W, C), prm = case
    if op in ("avgpool", "act_avgpool"):
        return (N, H // prm["k"][0], W // prm["k"][1], C)
    if op in ("maxpool", "maxpool_relu"):
        (kh, kw), (sh, sw), (ph, pw) = prm["geom"]
        return (N, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1, C)
    if op == "upsample":
        return (N, H * prm["f"][0], W * prm["f"][1], C)
    if op == "pad":
        pt, pb, pl, pr = prm["pad"][:4]
        return (N, H + pt + pb, W + pl + pr, C)
    return (N, H, W, C)


def nhwc_inputs(case):
    """-> x, dy (and for act_avgpool the per-(n, c) mask or None). Pools with ties: a few integer levels; the ReLU variant: the left half of
    every row non-positive (whole windows at or below zero); 'special': NaN, +inf and -inf planted; act_avgpool: exact zeros and negative
    zeros among the pre-activations, zeros in the mask."""
    name, op, shape, prm = case
    g = gen(name)
    N, H, W, C = shape
    fill = prm.get("fill", "randn")
    if fill == "randn":
        x = torch.randn(shape, generator=g)
    else:
        x = torch.randint(-2, 3, shape, generator=g).float()
    if fill == "special":
        flat = x.view(-1)
        pos = torch.randperm(flat.numel(), generator=g)[:18]
        flat[pos[:6]] = float("nan")
        flat[pos[6:12]] = float("inf")
        flat[pos[12:]] = float("-inf")
        x[1, :2, :2, 0] = float("-inf")                 # a whole corner window of -inf: the first tap's index must come out
    if op == "maxpool_relu":
        x[:, :, :max(W // 2, 1)] = -x[:, :, :max(W // 2, 1)].abs()
    extra = None
    if op == "act_avgpool":
        flat = x.view(-1)
        pos = torch.randperm(flat.numel(), generator=g)[:max(flat.numel() // 8, 2)]
        flat[pos[0::2]] = 0.0
        flat[pos[1::2]] = -0.0
        if prm["mask"]:
            extra = torch.where(torch.rand(N, C, generator=g) < 0.3, torch.zeros(N, C), torch.rand(N, C, generator=g) * 2 - 0.5)
            extra[0, 0] = 0.0
    dy = torch.randn(out_shape(case), generator=g)
    return x, dy, extra


def nhwc_regimes(case):
    name, op, (N, H, W, C), prm = case
    out = out_shape(case)
    t = {"V = 4" if C % 4 == 0 else "V = 1, C = %d" % C, "N == 1" if N == 1 else "N > 1"}
    if H == 1:
        t.add("H == 1")
    if W == 1:
        t.add("W == 1")
    t |= trip_tags("fwd", work_items(_numel(out), C)) | trip_tags("bwd", work_items(N * H * W * C, C))
    if op in ("avgpool", "act_avgpool"):
        kh, kw = prm["k"]
        t.add("kernel %dx%d" % (kh, kw))
        for nm, ext, k in (("H", H, kh), ("W", W, kw)):
            if k > 1:
                t.add("%s %s by the kernel" % (nm, "divisible" if ext % k == 0 else "not divisible"))
    if op == "act_avgpool":
        t.add("act %d" % prm["act"])
        t.add("mask with zeros" if prm["mask"] else "no mask")
        t.add("exact and negative zeros")
    if op in ("maxpool", "maxpool_relu"):
        t.add("geometry k%s s%s p%s" % prm["geom"])
        t.add({"quant": "ties", "special": "NaN, +inf, -inf", "randn": "no ties"}[prm["fill"]])
        if op == "maxpool_relu":
            t.add("non-positive windows")
    if op == "upsample":
        t.add("factors %dx%d" % prm["f"])
    if op == "blur":
        for nm, ext in (("H", H), ("W", W)):
            if ext <= 2:
                t.add("%s == %d" % (nm, ext))
    if op == "pad":
        pt, pb, pl, pr, mode, value = prm["pad"]
        pads = (pt, pb, pl, pr)
        if mode == 0:
            t.add("constant")
            if min(pads) < 0 < max(pads) and 0 in pads:
                t.add("constant: positive, zero and negative pads")
            if max(pads) < 0:
                t.add("constant: crop on every side")
        else:
            t.add("replicate")
            if max(pt, pb) > H or max(pl, pr) > W:
                t.add("replicate: pad larger than the side")
            if max(pt, pb) > 0 and max(pl, pr) > 0:
                t.add("replicate: corner accumulation")
    return {"%s: %s" % (op, x) for x in t}


# ---- copy_channels: name, rows, Cs, soff, Cd, doff, Cn, HW, bcast, accumulate (src rows = rows / HW under bcast) -----------------------------
COPY_CASES = [("slice", 37, 7, 0, 4, 0, 4, 1, 0, 0), ("soff_doff", 37, 7, 2, 9, 3, 4, 1, 0, 0), ("soff_doff_acc", 21, 6, 1, 8, 2, 5, 1, 0, 1),
              ("bcast_hw1", 13, 5, 1, 7, 2, 3, 1, 1, 0), ("bcast_k", 35, 4, 0, 6, 1, 4, 5, 1, 0), ("bcast_hw_acc", 24, 3, 0, 5, 2, 3, 12, 1, 1),
              ("big", 75000, 8, 1, 9, 1, 7, 1, 0, 0), ("big_bcast_acc", 75000, 8, 0, 9, 2, 7, 250, 1, 1)]


def copy_inputs(case):
    name, rows, Cs, soff, Cd, doff, Cn, HW, bcast, acc = case
    g = gen("copy_" + name)
    return torch.randn(rows // HW if bcast else rows, Cs, generator=g), torch.randn(rows, Cd, generator=g)


def copy_regimes(case):
    name, rows, Cs, soff, Cd, doff, Cn, HW, bcast, acc = case
    t = {"accumulate %d" % acc} | trip_tags("items", rows * Cn)
    if soff > 0:
        t.add("soff > 0")
    if doff > 0:
        t.add("doff > 0")
    if Cd > Cn:
        t.add("Cd > Cn")
    if bcast:
        t.add("bcast HW == 1" if HW == 1 else "bcast HW == H W" if rows // HW <= 2 else "bcast HW == k")
    return {"copy_channels: " + x for x in t}


# rows, C, Cpad
PAD_CHANNEL_CASES = [(33, 3, 4), (17, 5, 8), (9, 8, 8), (1, 1, 4), (11, 6, 12), (262200, 5, 8)]
# name, N, HW, Cs, soff, Cn, accumulate
REDUCE_CASES = [("hw1", 3, 1, 5, 0, 5, 0), ("hw255", 2, 255, 4, 1, 3, 0), ("hw256", 2, 256, 3, 0, 3, 1), ("hw257", 1, 257, 6, 2, 4, 0),
                ("hw1000", 2, 1000, 5, 1, 3, 1)]


def reduce_regimes(case):
    name, N, HW, Cs, soff, Cn, acc = case
    t = {"HW == %d" % HW, "accumulate %d" % acc}
    if soff > 0:
        t.add("soff > 0")
    return {"reduce_rows: " + x for x in t}


# name, L, B, ncls, Cd, doff
ONEHOT_CASES = [("plain", 5, 3, 7, 7, 0), ("doff_cd", 4, 2, 6, 11, 3), ("one_class", 3, 1, 1, 4, 2), ("big", 100, 70, 80, 80, 0), ("big_cd", 100, 70, 80, 83, 2)]


def onehot_labels(case):
    """labels in [0, ncls) with some outside on both sides (zero rows)"""
    name, Lr, B, ncls, Cd, doff = case
    g = gen("onehot_" + name)
    lab = torch.randint(0, ncls, (Lr, B), generator=g, dtype=torch.int32)
    lab.view(-1)[0] = -1
    lab.view(-1)[-1] = ncls
    if lab.numel() > 4:
        lab.view(-1)[2] = ncls + 5
    return lab, torch.randn(B, Lr, Cd, generator=g)


PERMUTE_DIMS = (2, 3, 5, 7)                        # four distinct extents: all 24 permutations
PERMUTE_BIG = ((2, 64, 1400, 3), (0, 3, 1, 2))    # NHWC -> NCHW, 537 600 elements
PERMUTE_LOW_RANK = [((6, 11), (1, 0)), ((6, 11), (0, 1))] + [((3, 5, 4), p) for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))]

# FusedUpsample weights [A, B, 3, 3]; the last: 58 300 filters = 932 800 outputs forward, 524 700 backward (both past GRID_CAP, ragged)
FUSED_WEIGHT_CASES = [(3, 5), (1, 1), (16, 8), (220, 265)] + [ab for ab in STEP_FUSED if ab not in ((3, 5), (1, 1), (16, 8), (220, 265))]
FUSED_MULT = 0.0589                                # sqrt(2 / fan_in), the kind of constant EqualLR passes

# ---- col2im_taps: name, N, H, W, R, S, ph, pw, dh, dw; stride 1: P = H + 2 ph - dh (R - 1) -------------------------------------------------
LDS_TILES = {3: (8, 32), 5: (8, 32), 7: (8, 16)}
COL2IM_CASES = [("lds3_tile", 2, 8, 32, 3, 3, 1, 1, 1, 1), ("lds3_off_asym", 1, 11, 45, 3, 3, 0, 1, 1, 1), ("lds3_small", 1, 3, 5, 3, 3, 2, 1, 1, 1),
                ("lds3_p0", 1, 9, 33, 3, 3, 0, 0, 1, 1),
                ("lds5_disc", 2, 9, 40, 5, 5, 0, 2, 1, 1), ("lds5_tile", 1, 16, 64, 5, 5, 2, 2, 1, 1), ("lds5_small", 1, 5, 7, 5, 5, 4, 3, 1, 1),
                ("lds5_p0", 1, 12, 37, 5, 5, 0, 0, 1, 1), ("lds5_p1", 1, 6, 9, 5, 5, 1, 1, 1, 1), ("lds5_p3", 1, 6, 9, 5, 5, 3, 3, 1, 1),
                ("lds7_tile", 1, 8, 16, 7, 7, 3, 3, 1, 1), ("lds7_off_asym", 2, 13, 21, 7, 7, 0, 3, 1, 1), ("lds7_small", 1, 7, 9, 7, 7, 6, 5, 1, 1),
                ("lds7_p0", 1, 10, 20, 7, 7, 0, 0, 1, 1), ("lds7_p12", 1, 9, 17, 7, 7, 1, 2, 1, 1), ("lds7_p45", 1, 5, 18, 7, 7, 4, 5, 1, 1),
                ("gen_d12", 2, 9, 13, 3, 3, 1, 2, 1, 2), ("gen_d21", 1, 10, 9, 3, 3, 2, 1, 2, 1), ("gen_r23", 1, 7, 9, 2, 3, 0, 1, 1, 1),
                ("gen_r4", 2, 9, 70, 4, 4, 1, 2, 1, 1)]
COL2IM_NOLDS = "lds5_disc"                       # run once more with HWG_COL2IM_LDS=0: bit-identical to the LDS kernel


def col2im_pq(case):
    name, N, H, W, R, S, ph, pw, dh, dw = case
    return H + 2 * ph - dh * (R - 1), W + 2 * pw - dw * (S - 1)


def col2im_inputs(case):
    name, N, H, W, R, S, ph, pw, dh, dw = case
    P, Q = col2im_pq(case)
    assert P > 0 and Q > 0, name
    return torch.randn(N, P, Q, R * S, generator=gen("col2im_" + name))


def col2im_regimes(case):
    name, N, H, W, R, S, ph, pw, dh, dw = case
    lds = dh == 1 and dw == 1 and R == S and R in LDS_TILES
    t = {"N == 1" if N == 1 else "N > 1"}
    if lds:
        th, tw = LDS_TILES[R]
        k = "lds %dx%d" % (R, S)
        t |= {k, k + (": H on the tile" if H % th == 0 else ": H smaller than a tile" if H < th else ": H off the tile"),
              k + (": W on the tile" if W % tw == 0 else ": W smaller than a tile" if W < tw else ": W off the tile"),
              k + ": pads %d" % ph, k + ": pads %d" % pw}
        if (ph, pw) == (0, R // 2):
            t.add(k + ": pad (0, R/2)")
        t = {x if x.startswith("lds") else k + ": " + x for x in t}
    else:
        t = {"general: " + x for x in t}
        t.add("general: dilation (%d,%d)" % (dh, dw) if (dh, dw) != (1, 1) else "general: non-square taps" if R != S else "general: R = %d" % R)
    return {"col2im: " + x for x in t}


# ---- glue ------------------------------------------------------------------------------------------------------------------------------------
GLUE_N = [1, 777, 1000, GRID_CAP + 777]            # axpby / mul element counts (the last: second trip, ragged)
AFFINE_CASES = [(37, 5, True, True), (16, 8, False, True), (9, 3, True, False), (4, 1, False, False), (104900, 5, True, True)]   # rows, C, scale, shift
# weights (exactly 1.0 among them); the terms are built so that the left-to-right fp32 order matters
WSUM_CASES = {"n1_w1": [1.0], "n1": [0.3], "n2": [1.0, 0.7], "n16": [1.0, 0.1, 1.0, 0.5, 3.0, 1.0, 0.01, 2.5, 1.0, 0.75, 1e-3, 7.0, 1.0, 0.2, 0.9, 1.0]}


def wsum_terms(name):
    n = len(WSUM_CASES[name])
    x = torch.randn(n, generator=gen("wsum_" + name)) * 3
    if n >= 3:
        x[0], x[2] = 3.0e7, -3.0e7           # (a + b) + c != a + (b + c) in fp32 for the terms between them
    return x


# K, B, D
STYLE_MIX_CASES = [("small", 5, 3, 7), ("off256", 4, 8, 33), ("at256", 6, 2, 128), ("two_blocks", 3, 5, 103)]


def style_mix_inputs(case):
    name, K, B, D = case
    g = gen("mix_" + name)
    ij = torch.randint(0, K, (2, B), generator=g, dtype=torch.int32)
    ij[1, 0] = ij[0, 0]                     # an equal pair
    if B > 2:
        ij[:, 2] = ij[:, 1]                 # a repeated pair
    w = torch.rand(2, B, generator=g)
    return torch.randn(K, D, generator=g), ij, w


def style_mix_regimes(case):
    name, K, B, D = case
    return {"style_mix: equal and repeated pairs", "style_mix: B D %s a multiple of 256" % ("on" if (B * D) % 256 == 0 else "off")}


def _glue_regimes():
    t = set()
    for n in GLUE_N:
        t |= {"glue: " + x for x in trip_tags("items", n)} | {"glue: n = 1"} if n == 1 else {"glue: " + x for x in trip_tags("items", n)}
    for rows, C, sc, sh in AFFINE_CASES:
        t.add("channel_affine: scale %s shift %s" % ("set" if sc else "null", "set" if sh else "null"))
        t |= {"channel_affine: " + x for x in trip_tags("items", rows * C)}
    for name, ws in WSUM_CASES.items():
        t.add("weighted_sum: n = %d" % len(ws))
        if 1.0 in ws and len(ws) > 1:
            t.add("weighted_sum: a weight of exactly 1")
    return t


def all_regimes():
    t = set()
    for c in NHWC_CASES:
        t |= nhwc_regimes(c)
    for c in COPY_CASES:
        t |= copy_regimes(c)
    for rows, C, Cpad in PAD_CHANNEL_CASES:
        t |= {"pad_channels: " + x for x in trip_tags("items", rows * (Cpad // 4))}
        t.add("pad_channels: %s" % ("Cpad == C" if Cpad == C else "last vector partly zero" if C % 4 else "whole zero vectors"))
        if Cpad - C >= 4 and C % 4:
            t.add("pad_channels: whole zero vectors")
    for c in REDUCE_CASES:
        t |= reduce_regimes(c)
    for name, Lr, B, ncls, Cd, doff in ONEHOT_CASES:
        t |= {"onehot: " + x for x in trip_tags("items", Lr * B * ncls)}
        t.add("onehot: doff > 0, Cd > ncls" if doff > 0 and Cd > ncls else "onehot: plain")
    t |= {"permute4: " + x for x in trip_tags("items", _numel(PERMUTE_BIG[0]))}
    t |= {"permute: rank %d" % len(s) for s, p in PERMUTE_LOW_RANK}
    for A, B in FUSED_WEIGHT_CASES:
        t |= {"fused_weight: " + x for x in trip_tags("fwd", A * B * 16) | trip_tags("bwd", A * B * 9)}
    for c in COL2IM_CASES:
        t |= col2im_regimes(c)
    for c in STYLE_MIX_CASES:
        t |= style_mix_regimes(c)
    return t | _glue_regimes()


def _required():
    t = set()
    for op in NHWC_OPS:
        t |= {"%s: %s" % (op, x) for x in ("V = 4", "V = 1, C = 1", "V = 1, C = 3", "V = 1, C = 6", "N == 1", "N > 1", "H == 1", "W == 1",
                                           "fwd second trip, ragged", "bwd second trip, ragged")}
    for op in ("avgpool", "act_avgpool"):
        t |= {"%s: %s" % (op, x) for x in ("kernel 2x2", "kernel 1x2", "kernel 2x1", "H divisible by the kernel", "H not divisible by the kernel",
                                           "W divisible by the kernel", "W not divisible by the kernel")}
    t |= {"act_avgpool: " + x for x in ("act 0", "act 1", "act 2", "mask with zeros", "no mask", "exact and negative zeros")}
    for op in ("maxpool", "maxpool_relu"):
        t |= {"%s: geometry k%s s%s p%s" % ((op,) + g) for g in (G22, GREC, G12, G33)} | {op + ": ties"}
    t |= {"maxpool: NaN, +inf, -inf", "maxpool_relu: non-positive windows"}
    t |= {"upsample: factors %dx%d" % f for f in ((2, 1), (1, 2), (2, 2), (3, 2))}
    t |= {"blur: %s == %d" % (a, n) for a in "HW" for n in (1, 2)}
    t |= {"pad: " + x for x in ("constant", "replicate", "constant: positive, zero and negative pads", "constant: crop on every side",
                                "replicate: pad larger than the side", "replicate: corner accumulation")}
    t |= {"copy_channels: " + x for x in ("soff > 0", "doff > 0", "Cd > Cn", "bcast HW == 1", "bcast HW == k", "bcast HW == H W", "accumulate 0",
                                          "accumulate 1", "items second trip, ragged")}
    t |= {"pad_channels: " + x for x in ("items second trip, ragged", "Cpad == C", "last vector partly zero", "whole zero vectors")}
    t |= {"reduce_rows: HW == %d" % n for n in (1, 255, 256, 257, 1000)} | {"reduce_rows: soff > 0", "reduce_rows: accumulate 0", "reduce_rows: accumulate 1"}
    t |= {"onehot: items second trip, ragged", "onehot: doff > 0, Cd > ncls", "onehot: plain", "permute4: items second trip, ragged", "permute: rank 2",
          "permute: rank 3", "fused_weight: fwd second trip, ragged", "fused_weight: bwd second trip, ragged"}
    for R, (th, tw) in LDS_TILES.items():
        k = "col2im: lds %dx%d" % (R, R)
        t |= {k, k + ": N > 1", k + ": pad (0, R/2)"} | {k + ": pads %d" % p for p in range(R)}
        t |= {k + ": %s %s" % (a, w) for a in "HW" for w in ("on the tile", "off the tile", "smaller than a tile")}
    t |= {"col2im: general: " + x for x in ("dilation (1,2)", "dilation (2,1)", "non-square taps", "R = 4", "N > 1", "N == 1")}
    t |= {"weighted_sum: n = %d" % n for n in (1, 2, 16)} | {"weighted_sum: a weight of exactly 1"}
    t |= {"style_mix: equal and repeated pairs", "style_mix: B D off a multiple of 256", "style_mix: B D on a multiple of 256"}
    t |= {"glue: items second trip, ragged", "glue: n = 1", "channel_affine: items second trip, ragged"}
    t |= {"channel_affine: scale %s shift %s" % (a, b) for a in ("set", "null") for b in ("set", "null")}
    return t


REQUIRED_REGIMES = _required()
