"""Case tables of tests/test_style_expert_fp64_gpu.py (the style-path kernels of csrc/style_ops.hip and the expert-bank kernels of
csrc/expert_bank.hip against the fp64 restatements of oracle/style_ref.py), their seeded inputs, and the regime bookkeeping
tests/test_style_expert_ref_cpu.py checks them with.

The step shapes are read off the model the shipped IAM config builds (on the meta device: no weights are allocated): the five layers and
the window of a character expert, the style chain, the AdaIN bank's widths; the batch sizes are the trainer's 8 lines per generator pass
and generate.py's lines per call. The constants restated from the kernels (tile rows, staging width, thread counts) are named at the top
of each section; the CPU test checks the ones Python can see against the package."""
import inspect
import json
import os
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "handwriting_line_generation_amd")
IAM_CONFIG = os.path.join(ROOT, "configs", "cf_IAMslant_noMask_charSpecSingleAppend_GANMedMT_autoAEMoPrcp2tightNewCTCUseGen_balB_hCF0.75_sMG.json")
STEP_BATCH = 8               # lines per generator / style pass of a iam_gan_b4a2_w512 step (oracle/seq_cases.py, oracle/norm_cases.py)
E = 6                        # experts per weight table (the model has one per class; six keep the tables small)


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _step_model():
    from handwriting_line_generation_amd.model.hw_with_style import HWWithStyle
    with open(IAM_CONFIG) as f:
        cfg = dict(json.load(f)["model"])
    cfg.pop("pretrained_hwr", None)
    with torch.device("meta"):
        return HWWithStyle(cfg)


def _step_shapes():
    from handwriting_line_generation_amd import generate
    from handwriting_line_generation_amd.model.layers import Linear, Marker
    net = _step_model()
    ex = net.style_extractor.char_extractor[0]
    layers = []
    for m in (ex.conv1[1], ex.conv1[4], ex.conv2[1], ex.fc[0], ex.fc[2]):
        w = m.weight
        layers.append((int(w.shape[1]), int(w.shape[0]), int(w.shape[2]) if w.dim() == 3 else 1))
    emb = list(net.generator.style_emb)
    lin = [m for m in emb if isinstance(m, Linear)]
    slopes = {float(m.what.split()[-1]) for m in emb if isinstance(m, Marker) and m.what.startswith("leaky relu")}
    assert len(slopes) == 1 and len({tuple(m.weight.shape) for m in lin}) == 1
    bank = [int(m.weight.shape[0]) for blk in net.generator.conv for m in (blk.adain1.style, blk.adain2.style)]
    return dict(expert_layers=layers, window=int(net.style_extractor.window), groups=(ex.conv1[2].num_groups, ex.conv2[2].num_groups),
                chain=(len(lin), int(lin[0].weight.shape[0]), slopes.pop()), bank_I=int(net.generator.conv[0].adain1.style.weight.shape[1]), bank_O=bank,
                generate_batch=int(inspect.signature(generate.bucket_by_length).parameters["batch_lines"].default))


STEP = _step_shapes()
EXPERT_LAYERS = STEP["expert_layers"]            # (Cin, Cout, S) of w1 .. w5
EXPERT_R = 2 * STEP["window"] + 1                # positions per window before the pool (1 after it)
CHAIN_L, CHAIN_D, CHAIN_SLOPE = STEP["chain"]
BANK_I, BANK_O = STEP["bank_I"], STEP["bank_O"]
GENERATE_BATCH = STEP["generate_batch"]


# ---- grouped Conv1d ----------------------------------------------------------------------------------------------------------------------
GT_ROWS, GT_CK, MAXR, WGRAD_TILE_ROWS, SPLIT_K = 32, 256, 8, 64, 768      # csrc/expert_bank.hip, model/expert_bank.py
# windows per expert. "mixed": experts 0 and 5 (the first and the last id) absent; per R a run of one window, runs that fill a forward tile
# exactly / by one row more where R divides 32 / 33, and a run of at least three weight-gradient tiles whose last tile holds one row where
# R allows an odd row count. "single": one run (two weight-gradient tiles). "all": every expert present, every run a single tile.
PLANS = {
    "mixed": {1: {1: 1, 2: 32, 3: 33, 4: 129}, 2: {1: 1, 2: 16, 3: 17, 4: 40}, 5: {1: 1, 2: 7, 3: 13, 4: 77}, 8: {1: 1, 2: 4, 3: 5, 4: 17}},
    "single": {R: {2: 14} for R in (1, 2, 5, 8)},
    "all": {R: {0: 2, 1: 1, 2: 3, 3: 1, 4: 2, 5: 4} for R in (1, 2, 5, 8)},
}
# name, Cin, Cout, S, R, plan, bias tables present
_NAMES = ("w1", "w2", "w3", "w4", "w5")
CONV_CASES = [("step_%s_r%d" % (nm, R), ci, co, s, R, "mixed", True) for R in (EXPERT_R, 1) for nm, (ci, co, s) in zip(_NAMES, EXPERT_LAYERS)] + [
    ("k8", 8, 4, 1, 1, "mixed", True),                     # one 8-channel group; a 4-wide Cout: ragged everywhere, dgrad cn = 4
    ("k744_below_split", 248, 132, 3, 5, "mixed", True),   # Cin * S = 744: the last contraction without the K split (256 threads)
    ("k768_at_split", 256, 260, 3, 2, "mixed", True),      # Cin * S = 768: the first with it; Cout 260: a second dgrad step of cn = 4
    ("cin264_s3", 264, 132, 3, 5, "mixed", True),          # a second staged step of ONE group: the upper half-wave's range is empty
    ("cin264_s3_r8", 264, 4, 3, 8, "mixed", False),        # the same at MAXR, without bias tables
    ("cin264_s1", 264, 260, 1, 2, "mixed", True),          # no split (264 < 768), two staged steps; wgrad z block 1 holds 8 channels
    ("cin512_s1", 512, 260, 1, 1, "mixed", False),         # two full staged steps without the split
    ("cin768_s1", 768, 132, 1, 8, "single", True),         # three staged steps with the split, S = 1
    ("single_run", EXPERT_LAYERS[0][0], EXPERT_LAYERS[0][1], 3, 5, "single", True),
    ("all_present", EXPERT_LAYERS[1][0], EXPERT_LAYERS[1][1], 3, 5, "all", False),
]
# the step's layers through model/expert_bank._GroupedConv1d (autograd, a bank of real CharExtractor modules): kind, R
AUTOGRAD_LAYERS = [("w1", EXPERT_R), ("w2", EXPERT_R), ("w3", EXPERT_R), ("w4", 1), ("w5", 1)]


def plan_cls(plan, R):
    """-> the expert id of every window, ascending (int64 numpy)"""
    import numpy as np
    return np.concatenate([np.full(n, e, dtype=np.int64) for e, n in sorted(PLANS[plan][R].items())])


def conv_inputs(case):
    """-> x [n, R, Cin], dy [n, R, Cout], [W_e], [b_e], [pre-filled dW_e], [pre-filled db_e]; nothing is zero: every row next to a window
    boundary would change the result if a tap reached across"""
    name, Cin, Cout, S, R, plan, bias = case
    g = gen("conv_" + name)
    n = int(plan_cls(plan, R).size)
    x = torch.randn(n, R, Cin, generator=g)
    dy = torch.randn(n, R, Cout, generator=g)
    Ws = [torch.randn(Cout, Cin, S, generator=g) * 0.05 for _ in range(E)]
    bs = [torch.randn(Cout, generator=g) * 0.1 for _ in range(E)]
    gW = [torch.randn(Cout, Cin, S, generator=g) * 3 for _ in range(E)]
    gb = [torch.randn(Cout, generator=g) * 3 for _ in range(E)]
    return x, dy, Ws, bs, gW, gb


def conv_case_regimes(case):
    name, Cin, Cout, S, R, plan, bias = case
    runs = PLANS[plan][R]
    tags = {"R = %d" % R, "S = %d" % S}
    tags.add("fwd K split (512 threads)" if Cin * S >= SPLIT_K else "fwd no K split (256 threads)")
    if Cin * S in (SPLIT_K - 24, SPLIT_K):
        tags.add("Cin * S = %d" % (Cin * S))
    if Cin > GT_CK:
        tags.add("fwd several staged steps")
        if Cin % GT_CK == 8 and Cin * S >= SPLIT_K:
            tags.add("fwd last step of one group under the K split")
    if Cout % 128:
        tags.add("fwd ragged 128 block of Cout")
    if Cout % 32:
        tags.add("wgrad ragged 32 block of Cout")
    if Cout % GT_CK == 4:
        tags.add("dgrad last step cn = 4")
    if Cin % 128:
        tags.add("dgrad ragged 128 block of Cin")
    if 0 < Cin % 256 <= 32:
        tags.add("wgrad z block mostly outside")
    if name.startswith("step_w"):                       # (w3 and w4 have the same shape: the name tells them apart)
        layer = _NAMES.index(name.split("_")[1])
        assert (Cin, Cout, S) == EXPERT_LAYERS[layer] and R in (EXPERT_R, 1) and plan == "mixed"
        tags.add("step layer %d R %d" % (layer, R))
    for e, n in runs.items():
        rows = n * R
        if n == 1:
            tags.add("run of one window")
        if rows == GT_ROWS:
            tags.add("run of exactly 32 rows")
        if rows == GT_ROWS + 1:
            tags.add("run of 33 rows")
        if rows > 2 * WGRAD_TILE_ROWS and rows % WGRAD_TILE_ROWS == 1:
            tags.add("wgrad three tiles or more, the last of one row")
        tags.add("wgrad single tile: direct add" if rows <= WGRAD_TILE_ROWS else "wgrad several tiles: partial images reduced")
        if rows > GT_ROWS and GT_ROWS % R:
            tags.add("windows straddle the 32-row tiles")
    if len(runs) == 1:
        tags.add("single run")
    if 0 not in runs and E - 1 not in runs and len(runs) > 1:
        tags.add("first and last expert absent")
    if len(runs) == E:
        tags.add("every expert present")
    tags.add("bias tables" if bias else "no bias tables")
    return tags


# runs of 1, 7, 8, 9 and 17 windows (expert 4 absent): below, at and past the eight-row batches of segment_accumulate_ptr, two batches and one
ACCUMULATE_RUNS = {0: 1, 1: 7, 2: 8, 3: 9, 5: 17}
ACCUMULATE_C = [256, 300]          # one trip of the 256 threads; a second, partial trip


# ---- windows -----------------------------------------------------------------------------------------------------------------------------
# name, B, Wx, C, window
WINDOW_CASES = [
    ("step_window", STEP_BATCH, 122, EXPERT_LAYERS[0][0], STEP["window"]),
    ("w0_c1", 2, 9, 1, 0),
    ("w6_c1", 2, 9, 1, 6),           # 13 positions over 9 columns: windows clipped at both ends at once
    ("w6_c256", 3, 40, 256, 6),
    ("w2_c1", 3, 40, 1, 2),
]


def window_inputs(case):
    """-> x [B, Wx, C], idx_b, idx_pos (int32; unique centres: first, second, third column - overlapping windows -, the last two columns,
    some in between, then centres outside the tensor), d patches, and how many of the centres are inside"""
    name, B, Wx, C, w = case
    g = gen("win_" + name)
    x = torch.randn(B, Wx, C, generator=g)
    inside = []
    for b in range(B):
        cols = {0, 1, 2, Wx - 1, Wx - 2, Wx // 2} | set(torch.randint(0, Wx, (4,), generator=g).tolist())
        inside += [(b, p) for p in sorted(cols)]
    r = max(w, 1)              # the last two: centres outside whose windows reach back inside the tensor
    outside = [(0, -1), (0, Wx), (-1, 3), (B, 3), (1, -100), (1, Wx + w + 5), (B - 1, -r), (B - 1, Wx - 1 + r)]
    perm = torch.randperm(len(inside) + len(outside), generator=g).tolist()
    both = inside + outside
    idx = torch.tensor([both[k] for k in perm], dtype=torch.int32)
    dp = torch.randn(len(both), 2 * w + 1, C, generator=g)
    return x, idx[:, 0].contiguous(), idx[:, 1].contiguous(), dp, len(inside)


def scores_inputs():
    """log-probs in [-20, 0] at the recogniser's step geometry, in-range indices only -> x [B, Wx, C], idx_b, idx_pos, idx_cls"""
    B, Wx, C, n = STEP_BATCH, 122, 80, 500
    g = gen("scores")
    x = -20.0 * torch.rand(B, Wx, C, generator=g)
    x[0, 0, 0], x[B - 1, Wx - 1, C - 1] = 0.0, -20.0
    ib = torch.randint(0, B, (n,), generator=g, dtype=torch.int32)
    ip = torch.randint(0, Wx, (n,), generator=g, dtype=torch.int32)
    ic = torch.randint(0, C, (n,), generator=g, dtype=torch.int32)
    ib[:2], ip[:2], ic[:2] = torch.tensor([0, B - 1]), torch.tensor([0, Wx - 1]), torch.tensor([0, C - 1])
    return x, ib, ip, ic


# ---- segment mean -----------------------------------------------------------------------------------------------------------------------
SEG_LIST_LDS = 60 * 1024           # hwg_segment_weighted_mean: the list kernel while (2 n + 1) * 4 bytes fit
SEG_LIST_MAX_N = (SEG_LIST_LDS // 4 - 1) // 2
# name, n, B, C, kind. kinds: "uniform" weights in (0, 1); "counts": lines of 0, 1, 7, 8, 9, 0 and 16 members; "wide": weights 1e-6 .. 1;
# "zero_line": the weights of line 1 are all 0 and those of line 2 are +-0.5 in pairs (wsum == 0 exactly with a total that is not 0);
# "pad_zero": the inputs of the case named n7679 plus one member of weight 0 - the same sums to the bit, through the other kernel
SEG_CASES = [
    ("n1", 1, 3, 128, "uniform"),
    ("counts_c300", 41, 7, 300, "counts"),
    ("counts_c1", 41, 7, 1, "counts"),
    ("n255", 255, STEP_BATCH, 128, "uniform"),
    ("n256", 256, STEP_BATCH, 1, "wide"),
    ("n257", 257, STEP_BATCH, 300, "zero_line"),
    ("n7679", SEG_LIST_MAX_N, STEP_BATCH, 128, "wide"),
    ("n7680", SEG_LIST_MAX_N + 1, STEP_BATCH, 128, "pad_zero"),
    ("n7680_c300", SEG_LIST_MAX_N + 1, 5, 300, "zero_line"),
]
SEG_COUNTS = [0, 1, 7, 8, 9, 0, 16]


def seg_inputs(case):
    """-> v [n, C], wgt [n], seg [n] int32 (inside [0, B)), dout [B, C]"""
    name, n, B, C, kind = case
    if kind == "pad_zero":
        base = [c for c in SEG_CASES if c[0] == "n7679"][0]
        v, wgt, seg, dout = seg_inputs(base)
        g = gen("seg_pad")
        return (torch.cat([v, torch.randn(1, C, generator=g)]), torch.cat([wgt, torch.zeros(1)]), torch.cat([seg, torch.tensor([3], dtype=torch.int32)]), dout)
    g = gen("seg_" + name)
    v = torch.randn(n, C, generator=g)
    dout = torch.randn(B, C, generator=g)
    if kind == "counts":
        assert sum(SEG_COUNTS) == n and len(SEG_COUNTS) == B
        seg = torch.cat([torch.full((c,), b, dtype=torch.int32) for b, c in enumerate(SEG_COUNTS)])[torch.randperm(n, generator=g)]
    else:
        seg = torch.randint(0, B, (n,), generator=g, dtype=torch.int32)
    wgt = torch.rand(n, generator=g) * 0.999 + 0.001
    if kind == "wide":
        wgt = 10.0 ** (-6.0 * torch.rand(n, generator=g))
        wgt[0], wgt[n - 1] = 1e-6, 1.0
    if kind == "zero_line":
        wgt[seg == 1] = 0.0
        m2 = (seg == 2).nonzero().flatten()
        if m2.numel() % 2:
            seg[m2[-1]] = 0                                           # an odd member out goes to line 0
            m2 = m2[:-1]
        wgt[m2[0::2]], wgt[m2[1::2]] = 0.5, -0.5
    return v, wgt, seg, dout


def seg_case_regimes(case):
    name, n, B, C, kind = case
    v, wgt, seg, dout = seg_inputs(case)
    counts = torch.bincount(seg.long(), minlength=B).tolist()
    tags = {"n = %d" % n} if n in (1, 255, 256, 257, SEG_LIST_MAX_N, SEG_LIST_MAX_N + 1) else set()
    tags.add("list kernel" if (2 * n + 1) * 4 <= SEG_LIST_LDS else "walk-all kernel")
    tags |= {"line of %d" % c for c in counts if c in (0, 1, 7, 8, 9)}
    tags.add("C = %d" % C)
    ws = torch.zeros(B, dtype=torch.float64).index_add_(0, seg.long(), wgt.double())
    tot = torch.zeros(B, dtype=torch.float64).index_add_(0, seg.long(), wgt.double().abs())
    if any(c > 0 and float(ws[b]) == 0.0 and float(tot[b]) == 0.0 for b, c in enumerate(counts)):
        tags.add("line with all weights zero")
    if any(float(ws[b]) == 0.0 and float(tot[b]) > 0.0 for b in range(B)):
        tags.add("wsum == 0 with a non-zero total")
    if float(wgt[wgt > 0].min()) <= 1e-6 and float(wgt.max()) >= 1.0:
        tags.add("weights 1e-6 .. 1")
    if kind == "pad_zero":
        tags.add("both kernels on the same sums")
    assert int(seg.min()) >= 0 and int(seg.max()) < B
    return tags


# ---- LinearBank ------------------------------------------------------------------------------------------------------------------------
LB_MAXB, LB_OCHUNK = 16, 32
_ODD_O = [6, 58, 64, 2]            # first neurons 0, 6, 64, 128: the 32-neuron chunk 0 holds layers 0 and 1; 130 outputs in all
# name, B, I, O, halves, unused outputs [(layer, half)], frozen {layer: "all" | "weight"}, x requires grad, backward
BANK_CASES = [
    ("step", STEP_BATCH, BANK_I, BANK_O, 2, [(3, 1)], {}, True, True),
    ("b1_i8_halves1", 1, 8, [6, 58, 64], 1, [], {1: "weight"}, True, True),
    # halves = 2: (1, 1) = neurons 35 .. 63, unused from the middle of chunk 1 on; (2, 0) = neurons 64 .. 95 = the whole of chunk 2
    ("b16_i100_odd_total", 16, 100, _ODD_O, 2, [(1, 1), (2, 0)], {0: "all", 3: "weight"}, True, True),
    ("b8_i128_x_const", STEP_BATCH, 128, _ODD_O, 2, [(2, 0)], {2: "weight"}, False, True),
    ("b17_fwd", 17, BANK_I, BANK_O, 2, [], {}, False, False),
    ("b64_fwd", GENERATE_BATCH, BANK_I, BANK_O, 2, [], {}, False, False),
    ("b17_i100_odd_total_fwd", 17, 100, _ODD_O, 2, [], {}, False, False),
]


def bank_inputs(case):
    """-> x, [W_l], [b_l], dys (per layer a list of `halves` gradients or None), [pre-filled dW_l], [pre-filled db_l]"""
    name, B, I, O, halves, unused, frozen, xgrad, bwd = case
    g = gen("bank_" + name)
    x = torch.randn(B, I, generator=g)
    Ws = [torch.randn(o, I, generator=g) * 0.1 for o in O]
    bs = [torch.randn(o, generator=g) for o in O]
    dys = [[None if (l, h) in unused else torch.randn(B, o // halves, generator=g) for h in range(halves)] for l, o in enumerate(O)]
    gW = [torch.randn(o, I, generator=g) * 2 for o in O]
    gb = [torch.randn(o, generator=g) * 2 for o in O]
    return x, Ws, bs, dys, gW, gb


def bank_case_regimes(case):
    name, B, I, O, halves, unused, frozen, xgrad, bwd = case
    first = [sum(O[:l]) for l in range(len(O) + 1)]
    tags = {"B = %d" % B, "I = %d" % I, "halves = %d" % halves, "backward" if bwd else "forward only"}
    if I % 64:
        tags.add("I % 64 != 0")
    if first[-1] % 4:
        tags.add("total outputs % 4 != 0")
    if any(f % LB_OCHUNK for f in first[1:-1]):
        tags.add("dgrad chunk across a layer boundary")
    if B > LB_MAXB:
        tags.add("several row blocks")
        if B % LB_MAXB:
            tags.add("ragged last row block")
    if (O, B) == (BANK_O, STEP_BATCH) and I == BANK_I:
        tags.add("step geometry")
    if bwd:
        used = [True] * first[-1]
        for l, h in unused:
            C = O[l] // halves
            used[first[l] + h * C:first[l] + (h + 1) * C] = [False] * C
        for c0 in range(0, first[-1], LB_OCHUNK):
            chunk = used[c0:c0 + LB_OCHUNK]
            if not any(chunk):
                tags.add("chunk of unused outputs only")
            elif not all(chunk):
                tags.add("unused outputs inside a chunk")
        tags |= {"frozen layer" if v == "all" else "weight frozen, bias trained" for v in frozen.values()}
        tags.add("x requires grad" if xgrad else "x constant (dx null)")
    return tags


# ---- MLPChain --------------------------------------------------------------------------------------------------------------------------
MC_MAXB = 16
# name, D, B, L, frozen layer or None, backward. Every (D, B <= 8 | B > 8) pair is one template instance of each backward kernel.
CHAIN_CASES = [("d%d_b%d_l%d" % (D, B, CHAIN_L), D, B, CHAIN_L, None, True) for D in (64, 128) for B in (1, 8, 9, 16)] + [
    ("d128_b8_l1", 128, 8, 1, None, True),
    ("d64_b9_l8", 64, 9, 8, None, True),
    ("d128_b16_l8_frozen3", 128, 16, 8, 3, True),       # the 152 KB instance at its largest L
    ("d64_b8_l6_frozen2", 64, 8, CHAIN_L, 2, True),
    ("d128_b17_fwd", 128, 17, CHAIN_L, None, False),
    ("d128_b40_fwd", 128, 40, CHAIN_L, None, False),
    ("d128_b64_fwd", 128, GENERATE_BATCH, CHAIN_L, None, False),
    ("d64_b17_fwd", 64, 17, CHAIN_L, None, False),
]
CHAIN_ZERO_NEURONS = (5, 40)       # in every layer these neurons have a zero weight row and a zero bias: their pre-activation is exactly 0


def chain_inputs(case):
    """-> x [B, D], [W_l], [b_l], dout [B, D], [pre-filled dW_l], [pre-filled db_l]"""
    name, D, B, L, frozen, bwd = case
    g = gen("chain_" + name)
    x = torch.randn(B, D, generator=g)
    Ws = [torch.randn(D, D, generator=g) * (0.5 / D ** 0.5) for _ in range(L)]          # 2-norm about 1: errors are not amplified from layer to layer
    bs = [torch.randn(D, generator=g) * 0.3 for _ in range(L)]
    for W, b in zip(Ws, bs):
        for o in CHAIN_ZERO_NEURONS:
            W[o], b[o] = 0.0, 0.0
    dout = torch.randn(B, D, generator=g)
    gW = [torch.randn(D, D, generator=g) for _ in range(L)]
    gb = [torch.randn(D, generator=g) for _ in range(L)]
    return x, Ws, bs, dout, gW, gb


def chain_case_regimes(case):
    name, D, B, L, frozen, bwd = case
    tags = {"L = %d" % L}
    if bwd:
        tags.add("backward instance <%d, %d>" % (D, 8 if B <= 8 else 16))
        tags.add("backward B = %d" % B)
        if frozen is not None and 0 < frozen < L - 1:
            tags.add("frozen layer in the middle")
    else:
        tags.add("forward only D = %d B = %d" % (D, B))
    tags.add("forward instance <%d, %d>" % (D, 8 if (D == 128 and B <= 8) else 16))
    if (D, L) == (CHAIN_D, CHAIN_L) and B == STEP_BATCH:
        tags.add("step geometry")
    return tags


# ---- run_experts end to end ----------------------------------------------------------------------------------------------------------------
# windows per expert (expert 3 absent): about 100 windows over 5 of 6 experts, one run of several tiles
EXPERTS_RUNS = {0: 3, 1: 41, 2: 1, 4: 14, 5: 40}


REQUIRED_CONV_REGIMES = (
    {"step layer %d R %d" % (l, R) for l in range(5) for R in (EXPERT_R, 1)}
    | {"Cin * S = 744", "Cin * S = 768", "fwd K split (512 threads)", "fwd no K split (256 threads)", "fwd several staged steps",
       "fwd last step of one group under the K split", "fwd ragged 128 block of Cout", "wgrad ragged 32 block of Cout", "dgrad last step cn = 4",
       "dgrad ragged 128 block of Cin", "wgrad z block mostly outside", "R = 1", "R = 2", "R = 5", "R = 8", "S = 1", "S = 3",
       "run of one window", "run of exactly 32 rows", "run of 33 rows", "wgrad three tiles or more, the last of one row",
       "wgrad single tile: direct add", "wgrad several tiles: partial images reduced", "windows straddle the 32-row tiles", "single run",
       "first and last expert absent", "every expert present", "bias tables", "no bias tables"})
REQUIRED_SEG_REGIMES = (
    {"n = %d" % n for n in (1, 255, 256, 257, SEG_LIST_MAX_N, SEG_LIST_MAX_N + 1)} | {"line of %d" % c for c in (0, 1, 7, 8, 9)}
    | {"C = 1", "C = 128", "C = 300", "list kernel", "walk-all kernel", "line with all weights zero", "wsum == 0 with a non-zero total",
       "weights 1e-6 .. 1", "both kernels on the same sums"})
REQUIRED_BANK_REGIMES = (
    {"B = %d" % b for b in (1, 8, 16, 17, GENERATE_BATCH)} | {"I = %d" % i for i in (8, 100, 128)}
    | {"I % 64 != 0", "total outputs % 4 != 0", "dgrad chunk across a layer boundary", "halves = 1", "halves = 2", "several row blocks",
       "ragged last row block", "step geometry", "chunk of unused outputs only", "unused outputs inside a chunk", "frozen layer",
       "weight frozen, bias trained", "x requires grad", "x constant (dx null)", "backward", "forward only"})
REQUIRED_CHAIN_REGIMES = (
    {"backward instance <%d, %d>" % (D, BM) for D in (64, 128) for BM in (8, 16)} | {"backward B = %d" % b for b in (1, 8, 9, 16)}
    | {"forward instance <128, 8>", "forward instance <128, 16>", "forward instance <64, 16>", "L = 1", "L = 6", "L = 8",
       "frozen layer in the middle", "step geometry", "forward only D = 128 B = 17", "forward only D = 128 B = 40",
       "forward only D = 128 B = %d" % GENERATE_BATCH, "forward only D = 64 B = 17"})
REQUIRED_WINDOW_REGIMES = {"window = 0", "window = 2", "window = 6", "C = 1", "C = 256", "clipped at both ends at once"}


def window_case_regimes(case):
    name, B, Wx, C, w = case
    tags = {"window = %d" % w, "C = %d" % C}
    if 2 * w + 1 > Wx:
        tags.add("clipped at both ends at once")
    return tags
