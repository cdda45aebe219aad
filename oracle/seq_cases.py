"""Case tables of tests/test_seq_loss_fp64_gpu.py (log-softmax, CTC, the loss reductions, spectral norm, pixel norm, argmax and the DTW
alignment against fp64 / exact restatements), their seeded inputs, and the regime bookkeeping tests/test_seq_loss_ref_cpu.py checks them with.

The recogniser's output geometry and the discriminator's spectral-norm layer shapes are read off the models themselves (built on the meta
device: no weights are allocated), the class count off the shipped IAM character set (its characters plus the CTC blank)."""
import json
import os
import zlib

import torch
from torch import nn

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "handwriting_line_generation_amd")
STEP_BATCH, STEP_WIDTH = 8, 512          # lines per recogniser pass and their width in a iam_gan_b4a2_w512 step


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def num_class():
    with open(os.path.join(PKG, "data", "IAM_char_set.json")) as f:
        return len(json.load(f)["idx_to_char"]) + 1


def hwr_time_steps(width):
    """columns the recogniser (model/cnn_only_hwr.py) emits for a line `width` pixels wide: every layer's width arithmetic, in order"""
    from handwriting_line_generation_amd.model.cnn_only_hwr import CNNOnlyHWR
    from handwriting_line_generation_amd.model.layers import Marker
    with torch.device("meta"):
        net = CNNOnlyHWR(num_class(), norm="batch")
    W = width
    for m in list(net.cnn) + list(net.cnn1d):
        if isinstance(m, (nn.Conv2d, nn.Conv1d)):
            k, p, d, s = m.kernel_size[-1], m.padding[-1], m.dilation[-1], m.stride[-1]
            W = (W + 2 * p - d * (k - 1) - 1) // s + 1
        elif isinstance(m, Marker) and m.what == "maxpool 2x2":
            W = W // 2
        elif isinstance(m, Marker) and m.what == "maxpool (2,2)/(2,1)/(0,1)":       # width: kernel 2, stride 1, padding 1
            W = W + 2 - 2 + 1
        else:
            assert isinstance(m, Marker) and m.what in ("relu", "log softmax") or isinstance(m, nn.modules.batchnorm._BatchNorm), m
    return W


def discriminator_sn_shapes():
    """(R, K) = (C_out, C_in * kh * kw) of every spectral-norm layer model/discriminator_ap.py builds (both heads), in module order"""
    from handwriting_line_generation_amd.model.discriminator_ap import DiscriminatorAP, SpectralConv2d
    with torch.device("meta"):
        net = DiscriminatorAP(use_low=True, use_med=True)
    out = []
    for m in net.modules():
        if isinstance(m, SpectralConv2d):
            w = m.module.weight_bar
            out.append((w.shape[0], w.numel() // w.shape[0]))
    return out


T_MODEL, NUM_CLASS = hwr_time_steps(STEP_WIDTH), num_class()


# ---- logits ----------------------------------------------------------------------------------------------------------------------------
def peaked_offset(B, T, C, g, blank_frac=0.7, gain=10.0):
    """bench.py's "peaked recogniser" pattern, restated: per column one class (the blank with probability 0.7) gets +10; the pattern of
    line b is the shared one rolled by 7 columns per line index -> [B, T, C]"""
    cls = torch.randint(1, C, (4096,), generator=g)
    cls[torch.rand(4096, generator=g) < blank_frac] = 0
    off = torch.zeros(B, T, C)
    for b in range(B):
        off[b, torch.arange(T), cls[(torch.arange(T) + 7 * b) % 4096]] = gain
    return off


def logits(kind, B, T, C, g):
    """[B, 1, T, C] float32. kind: "randn"; "large" = randn * 30 + 60 (exp overflows without the max subtraction); "peaked" = randn + the
    peaked pattern; "x3" / "x4" / "x6" = that multiple of randn"""
    x = torch.randn(B, 1, T, C, generator=g)
    if kind == "large":
        x = x * 30 + 60
    elif kind == "peaked":
        x = x + peaked_offset(B, T, C, g)[:, None]
    elif kind != "randn":
        x = x * float(kind[1:])
    return x


# name, B, T, C: through ops.log_softmax_tbc forward and backward, with every input kind ("peaked" needs a non-blank class)
LOG_SOFTMAX_SHAPES = [
    ("step", STEP_BATCH, T_MODEL, NUM_CLASS),      # the recogniser's own output for 512-wide lines
    ("c5", 3, 7, 5),                               # C < 64: idle lanes
    ("c64", 2, 9, 64),                             # exactly one wave of classes
    ("c65", 2, 5, 65),                             # one class into the second trip of the lane loop
    ("c200", 2, 4, 200),                           # four trips, the last partial
    ("rows9100", 70, 130, 80),                     # more rows than the 8192 waves of the capped grid: the grid-stride trip runs
    ("one", 1, 1, 1),                              # a single class: log-prob 0, gradient 0
]
LOG_SOFTMAX_CASES = [(n + "_" + k, B, T, C, k) for n, B, T, C in LOG_SOFTMAX_SHAPES for k in ("randn", "large", "peaked") if C > 1 or k != "peaked"]
LOG_SOFTMAX_GRID_WAVES = 2048 * 4


# ---- CTC -------------------------------------------------------------------------------------------------------------------------------
# name, T, B, C, Lmax, tg_len, in_len, logits kind, targets, family. targets: "random" (characters 1 .. C-1), "pairs" (every odd position
# repeats its predecessor: the s-2 skip is forbidden at every second character), "ones" (one character: every skip forbidden) or a literal
# list of rows (zero-padded to Lmax). Families differ in the fp32 log-space error the problem itself carries (torch's own fp32 ctc_loss:
# 2e-5 for unit logits, 4e-4 .. 6e-4 for peaked ones, 3e-3 for 600 steps of 4 x randn).
_ONE_PATH = [[1, 1, 2, 2, 3, 3, 4], [5, 6, 7, 8, 1, 2, 3, 4], [2, 2, 2, 2, 2, 2]]
CTC_CASES = [
    ("step_randn", T_MODEL, STEP_BATCH, NUM_CLASS, 30, [30] * 8, [T_MODEL] * 8, "randn", "random", "ctc_plain"),     # the step's own shape
    ("step_peaked", T_MODEL, STEP_BATCH, NUM_CLASS, 30, [30] * 8, [T_MODEL] * 8, "peaked", "random", "ctc_peaked"),  # and bench.py's logits
    # an empty target (S = 0, one state, divisor max(0, 1)), in_len < T (zero gradient tail, nll read at row in_len - 1), in_len = 2
    ("ragged", 130, 4, 80, 60, [60, 33, 0, 1], [130, 121, 130, 2], "randn", "random", "ctc_plain"),
    # 281 states: the 256-wide alpha / beta loops and the 128-wide grad loop take a second (third) trip; the skip rule is live everywhere
    ("states_gt_256", 300, 3, 80, 140, [140, 129, 5], [300, 281, 300], "x3", "pairs", "ctc_peaked"),
    # in_len = length + repeats: exactly one alignment per item, every alpha off that path is -inf
    ("one_path", 12, 3, 9, 8, [7, 8, 6], [10, 8, 11], "randn", _ONE_PATH, "ctc_plain"),
    # item 2 one step short: its nll is infinite, so the loss is 0 and every gradient exactly 0 (for the two feasible items too)
    ("one_infeasible", 12, 3, 9, 8, [7, 8, 6], [10, 8, 10], "randn", _ONE_PATH, None),
    ("t1", 1, 2, 80, 3, [1, 0], [1, 1], "randn", "random", "ctc_plain"),                                           # one time step
    ("c2", 40, 2, 2, 12, [12, 5], [40, 30], "randn", "ones", "ctc_plain"),                                          # blank plus one character
    ("c200", 20, 2, 200, 6, [6, 4], [20, 17], "randn", "random", "ctc_plain"),          # the grad kernel's class loop takes a second trip
    ("long_peaked", 600, 2, 96, 40, [40, 3], [600, 600], "x4", "random", "ctc_long"),   # fp32 log-space error at its largest
]


def ctc_inputs(case):
    """-> logits [B, 1, T, C] float32, targets [B, Lmax] int64 (zero beyond each length)"""
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = case
    g = gen("ctc_" + name.replace("one_infeasible", "one_path"))          # one_infeasible: one_path's inputs, one length changed
    x = logits(kind, B, T, C, g)
    if isinstance(targets, list):
        tg = torch.zeros(B, Lmax, dtype=torch.int64)
        for b, row in enumerate(targets):
            tg[b, :len(row)] = torch.tensor(row)
    elif targets == "ones":
        tg = torch.ones(B, Lmax, dtype=torch.int64)
    else:
        tg = torch.randint(1, C, (B, Lmax), generator=g)
        if targets == "pairs":
            tg[:, 1::2] = tg[:, 0:Lmax - 1:2]
    for b in range(B):
        tg[b, tg_len[b]:] = 0
    return x, tg


def ctc_case_regimes(case):
    name, T, B, C, Lmax, tg_len, in_len, kind, targets, family = case
    x, tg = ctc_inputs(case)
    tags = set()
    if 2 * max(tg_len) + 1 > 256:
        tags.add("states > 256")
    if any(i < T for i in in_len):
        tags.add("in_len < T")
    if 0 in tg_len:
        tags.add("empty target")
    if C > 128:
        tags.add("C > 128")
    if T == 1:
        tags.add("T = 1")
    if C == 2:
        tags.add("C = 2")
    if any(tg_len[b] > 1 and bool((tg[b, 1:tg_len[b]] == tg[b, :tg_len[b] - 1]).any()) for b in range(B)):
        tags.add("repeated characters")
    if (T, B, C) == (T_MODEL, STEP_BATCH, NUM_CLASS):
        tags.add("step geometry")
    return tags


# ---- losses ----------------------------------------------------------------------------------------------------------------------------
LOSS_SIZES = [1, 255, 4096, 4097, 131072, 2101265]        # one thread; one partial block; one full block of 4096; one element into the second;
LOSS_BLOCK, LOSS_MAX_BLOCKS = 4096, 512                   # 32 blocks; 513 blocks' worth: past the 512-block cap, every block strides twice
LOSS_GOUT = 0.5
_WRT = ("a", "b", "both")


def _loss_cases():
    """name, mode, n, scale, which inputs require a gradient, inputs. Scale and gradient destinations rotate over the sizes so that every
    mode meets scale +1 and -1 (the trainer's sign) and every pair loss meets "a", "b" and "both"."""
    out = []
    for mode in range(5):
        for i, n in enumerate(LOSS_SIZES):
            scale = 1.0 if (i + mode) % 2 == 0 else -1.0
            wrt = _WRT[(i + mode) % 3] if mode < 2 else "a"
            out.append(("m%d_n%d" % (mode, n), mode, n, scale, wrt, "randn"))
    # exact ties at every second element: a == b (L1), a == 1 and a == -1 (the hinges): the gradient there is 0
    out += [("m0_ties", 0, 4097, 1.0, "both", "ties"), ("m3_ties", 3, 4097, -1.0, "a", "ties"), ("m4_ties", 4, 4097, 1.0, "a", "ties")]
    # 1000 + randn: an fp32 running sum over 131072 terms would keep 3 digits of the part that varies; the double partials keep all of it
    out += [("m2_offset1000", 2, 131072, 1.0, "a", "offset1000"), ("m1_offset1000", 1, 131072, 1.0, "both", "offset1000")]
    return out


LOSS_CASES = _loss_cases()


def loss_inputs(case):
    name, mode, n, scale, wrt, inputs = case
    g = gen("loss_" + name)
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g) if mode < 2 else None
    if inputs == "offset1000":
        a = a + 1000
        if b is not None:
            b = b + 1000
    if inputs == "ties":
        if mode == 0:
            b[::2] = a[::2]
        else:
            a[::2] = 1.0 if mode == 3 else -1.0
    return a, b


def loss_case_regimes(case):
    name, mode, n, scale, wrt, inputs = case
    tags = {"mode %d scale %+d" % (mode, scale), "inputs " + inputs}
    if mode < 2:
        tags.add("mode %d wrt %s" % (mode, wrt))
    if -(-n // LOSS_BLOCK) > LOSS_MAX_BLOCKS:
        tags.add("n past the block cap")
    if n % 256:
        tags.add("partial last block")
    return tags


# ---- spectral norm -----------------------------------------------------------------------------------------------------------------------
SN_EPS = 1e-12
SN_MODEL_SHAPES = discriminator_sn_shapes()
SN_EXTRA_SHAPES = [
    (64, 49),         # the C_in = 1 first layer's geometry (7 x 7 taps, K < 64: idle lanes in the row kernel, one partial column block)
    (5, 9),           # R not a multiple of 4 and below it per block, K < 64
    (7, 70),          # R % 4 = 3, K one wave and a bit
    (64, 1025),       # K one past the 1024 threads of the normalise kernel: its loop takes a second trip for one element
    (130, 3000),      # R % 4 = 2, K three trips
    (1030, 2037),     # R * K = 2,098,110 > 2,097,152: the backward pass's dot product runs past its 512-block cap; R > 1024 too
]
SN_SHAPES = sorted(set(SN_MODEL_SHAPES)) + SN_EXTRA_SHAPES
# the layers one SpectralBank runs together (four launches forward, two backward): the discriminator's own ten, and the odd shapes - the
# blocks of the max_R / max_K grids beyond a smaller layer's own extent return early
SN_BANKS = [("discriminator", SN_MODEL_SHAPES), ("odd", SN_EXTRA_SHAPES)]
SN_DOT_BLOCK, SN_DOT_MAX_BLOCKS = 4096, 512


def sn_inputs(name, R, K):
    """weight (two of them: the second iteration runs on a moved weight, as after an optimizer step), u, v, two upstream gradients"""
    g = gen("sn_%s_%dx%d" % (name, R, K))
    w1 = torch.randn(R, K, generator=g) * 0.05
    w2 = w1 + torch.randn(R, K, generator=g) * 0.005
    u = torch.randn(R, generator=g)
    v = torch.randn(K, generator=g)
    return w1, w2, u / u.norm(), v / v.norm(), torch.randn(R, K, generator=g), torch.randn(R, K, generator=g)


def sn_shape_regimes(R, K):
    tags = set()
    if K > 1024:
        tags.add("K > 1024")
    if R % 4:
        tags.add("R % 4 != 0")
    if K < 64:
        tags.add("K < 64")
    if R == 1:
        tags.add("R = 1")
    if -(-R * K // SN_DOT_BLOCK) > SN_DOT_MAX_BLOCKS:
        tags.add("R * K past the block cap")
    return tags


# ---- pixel norm, argmax, DTW -------------------------------------------------------------------------------------------------------------
PIXEL_NORM_EPS = 1e-8
PIXEL_NORM_SHAPES = [(8, 128), (5, 1), (3, 65), (6, 200)]      # the generator's style width; one class; one lane into the second trip; four trips
PIXEL_NORM_INPUTS = ("randn", "tiny", "zero_row")              # tiny = 1e-5 * randn: mean(x^2) = 1e-10 < eps; zero_row: row 0 all zero
PIXEL_NORM_CASES = [(r, c, k) for r, c in PIXEL_NORM_SHAPES for k in PIXEL_NORM_INPUTS]


def pixel_norm_inputs(case):
    rows, C, kind = case
    g = gen("pixelnorm_%dx%d_%s" % case)
    x = torch.randn(rows, C, generator=g)
    if kind == "tiny":
        x = x * 1e-5
    if kind == "zero_row":
        x[0] = 0.0
    return x, torch.randn(rows, C, generator=g)


ARGMAX_SHAPES = [(60, 16), (T_MODEL * STEP_BATCH, NUM_CLASS), (7, 1), (9, 200)]


def argmax_inputs(shape):
    """values on a grid of 0.5 (ties between lanes in most rows) and three planted rows: the maximum twice in one lane (c and c + 64, where
    C allows), in two different lanes with the later lane holding the smaller index, and an all-equal row"""
    rows, C = shape
    g = gen("argmax_%dx%d" % shape)
    x = (torch.randn(rows, C, generator=g) * 2).round() / 2
    planted = {}
    if C > 64:
        x[0, 3] = x[0, 67] = 50.0
        planted["same lane"] = (0, 3)
        x[1, 70] = x[1, 9] = 50.0                # lane 6 holds index 70, lane 9 index 9: the smaller index sits in the later lane
        planted["different lanes"] = (1, 9)
    elif C > 1:
        x[1, C - 1] = x[1, 2] = 50.0
        planted["different lanes"] = (1, 2)
    x[2] = -3.5
    planted["all equal"] = (2, 0)
    return x, planted


DTW_CASES = [(150, 2, 130), (300, 1, 128)]      # (T, B, Lr): LL = 2 Lr + 1 = 261 and 257 > 256, the j loop takes a second trip
DTW_CLASSES = 20


def dtw_inputs(case):
    T, B, Lr = case
    g = gen("dtw_%dx%dx%d" % case)
    pred = torch.log_softmax(torch.randn(T, B, DTW_CLASSES, generator=g) * 3, dim=2)
    label = torch.randint(1, DTW_CLASSES, (Lr, B), generator=g)
    label[Lr - 7:, 0] = 0            # a zero-padded label tail on line 0
    return pred, label


REQUIRED_REGIMES = {
    "ctc": {"states > 256", "in_len < T", "empty target", "C > 128", "T = 1", "C = 2", "repeated characters", "step geometry"},
    "loss": {"n past the block cap", "partial last block", "inputs ties", "inputs offset1000"}
            | {"mode %d scale %+d" % (m, s) for m in range(5) for s in (1, -1)} | {"mode %d wrt %s" % (m, w) for m in (0, 1) for w in _WRT},
    "sn": {"K > 1024", "R % 4 != 0", "K < 64", "R = 1", "R * K past the block cap"},
}
