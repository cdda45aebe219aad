"""Case tables of tests/test_norm_abi_fp64_gpu.py and tests/test_seq_loss_abi_fp64_gpu.py: the entries of csrc/norm_act.hip, csrc/seq_ops.hip and
csrc/spectral_loss.hip (and hwg_colsum) called at the C ABI on guarded buffers, with a workspace of exactly the queried size. Small shapes, one
per regime of the kernels - not the training step's shapes, which tests/test_norm_act_fp64_gpu.py and tests/test_seq_loss_fp64_gpu.py run
through ops. Where oracle/norm_cases.py or oracle/seq_cases.py already hold a small case of a regime it is taken from there, with its input
generator; only what is missing is added. tests/test_abi_cases_cpu.py checks that every regime named here is reached, and restates the byte
counts the workspace queries are documented to return."""
from oracle import norm_cases as NC
from oracle import seq_cases as SC

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = NC.ACT_NONE, NC.ACT_RELU, NC.ACT_LRELU, NC.ACT_TANH
MODES = ("gn", "in", "bn")
MODE_ID = {"in": 0, "gn": 1, "bn": 2}

# ---- normalisation ---------------------------------------------------------------------------------------------------------------------------
# geometry (NC.make_geo: L = C / 4 lanes per pixel, PP = 256 / L pixels per pass, chunks = ceil(HW / (4 PP)), capped at 64, halved while
# chunks * N > 4096): name, N, HW, C, groups of the GroupNorm runs, the regime the shape is there for
NORM_SHAPES = [
    ("c4_hw5", 3, 5, 4, 2, "all lanes on pixels, one partial pass"),
    ("c4_hw1025", 2, 1025, 4, 1, "two ragged chunks"),
    ("c48_hw85", 3, 85, 48, 4, "PP 21, four idle lanes, two chunks"),
    ("c1024_hw3", 2, 3, 1024, 8, "PP 1, one chunk"),
    ("c1024_hw300", 2, 300, 1024, 4, "chunk cap reached, ragged"),
]
HALVED_SHAPE = ("c1024_hw253_n65", 65, 253, 1024, 8, "chunks halved")       # the smallest tensor that reaches the halving: one case only
_ACTS = ((ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LRELU, 0.2), (ACT_TANH, 0.0))


def _norm_cases():
    """the shapes x (gn, in, bn) x (mask off, on); the activation and the parameter-gradient mode (written / added to a pre-filled buffer)
    rotate over the cases, so that every mode meets each activation"""
    out, k = [], 0
    for name, N, HW, C, groups, _ in NORM_SHAPES:
        for mode in MODES:
            for mask in (False, True):
                act, slope = _ACTS[k % 4]
                out.append(dict(name="%s_%s%s_act%d" % (name, mode, "_mask" if mask else "", act), mode=mode, N=N, HW=HW, C=C,
                                groups=groups if mode == "gn" else 1, act=act, slope=slope, mask=mask, accumulate=(k // 4) % 2))
                k += 1
            k += 1          # (three modes x two masks = six cases per shape: one more step and the next shape starts at another activation)
    name, N, HW, C, groups, _ = HALVED_SHAPE
    out.append(dict(name=name + "_gn_act1", mode="gn", N=N, HW=HW, C=C, groups=groups, act=ACT_RELU, slope=0.0, mask=False, accumulate=0))
    return out


NORM_CASES = _norm_cases()
# affine_per_sample = 1 (gamma, beta, dgamma, dbeta are [N][C]): InstanceNorm and GroupNorm; no Python caller reaches it
PER_SAMPLE_CASES = [
    dict(name="ps_c48_hw85_in_lrelu", mode="in", N=3, HW=85, C=48, groups=1, act=ACT_LRELU, slope=0.2, mask=False),
    dict(name="ps_c48_hw85_gn_mask", mode="gn", N=3, HW=85, C=48, groups=4, act=ACT_NONE, slope=0.0, mask=True),
    dict(name="ps_c4_hw1025_gn_tanh", mode="gn", N=2, HW=1025, C=4, groups=2, act=ACT_TANH, slope=0.0, mask=False),
    dict(name="ps_c1024_hw300_in_relu_mask", mode="in", N=2, HW=300, C=1024, groups=1, act=ACT_RELU, slope=0.0, mask=True),
]
# name, N, HW, C: the generator epilogue (hwg_adain_fwd, _fwd_rng, _bwd)
ADAIN_CASES = [("adain_c4_hw1025", 2, 1025, 4), ("adain_c48_hw85", 3, 85, 48), ("adain_c1024_hw300", 2, 300, 1024)]
# the eval-mode BatchNorm cases of NC small enough, and C = 1024
FROZEN_CASES = [c for c in NC.FROZEN_CASES if c[1] * c[2] * c[3] * c[4] <= 1 << 16] + [("frozen_c1024_none", 2, 1, 3, 1024, ACT_NONE, 0.0)]
# bias_act: every case of NC but the step's own (the vector kernel with and without index arithmetic, odd float4 count, two sweeps, scalar kernel)
BIAS_ACT_CASES = [c for c in NC.BIAS_ACT_CASES if not c[0].startswith("step_")]
# rows, C of hwg_colsum: one chunk written directly (rows <= 256), two chunks, C = 1 / 3 (narrow kernel), C % 4 == 0 and not
COLSUM_CASES = [(1, 1), (300, 3), (256, 12), (257, 12), (1000, 70)]


def norm_workspace_bytes(N, HW, C):
    """what hwg_norm_workspace is documented to return: two partial buffers of N * chunks * C double pairs, c1 / c2 [N][C] floats, 256"""
    g = NC.make_geo(N, HW, C)
    return 2 * (N * g["chunks"] * C * 2 * 8) + 2 * N * C * 4 + 256


def norm_regimes(N, HW, C):
    g = NC.make_geo(N, HW, C)
    tags = set()
    if g["PP"] == 256 and HW < 256:
        tags.add("all lanes on pixels, one partial pass")
    if g["chunks"] == 2 and HW % g["cs"]:
        tags.add("two ragged chunks")
    if g["PP"] == 21 and 256 - g["PP"] * g["L"] == 4 and g["chunks"] == 2:
        tags.add("PP 21, four idle lanes, two chunks")
    if g["PP"] == 1 and g["chunks"] == 1:
        tags.add("PP 1, one chunk")
    if g["raw"] > 64 and not g["halved"] and g["cs"] % (NC.NU * g["PP"]):          # ragged: a chunk is no whole number of NU-deep trips
        tags.add("chunk cap reached, ragged")
    if g["halved"]:
        tags.add("chunks halved")
    return tags


REQUIRED_NORM_REGIMES = {s[5] for s in NORM_SHAPES} | {HALVED_SHAPE[5]}

# ---- log-softmax, CTC, DTW ---------------------------------------------------------------------------------------------------------------------
_SWEEP = min((s for s in SC.LOG_SOFTMAX_SHAPES if s[1] * s[2] > SC.LOG_SOFTMAX_GRID_WAVES), key=lambda s: s[1] * s[2] * s[3])
# name, B, T, C, logits kind (SC.logits)
LOG_SOFTMAX_CASES = [("one_lane", 1, 1, 1, "randn"), ("model_width", 3, 5, SC.NUM_CLASS, "large"), ("sweep_" + _SWEEP[0],) + _SWEEP[1:] + ("peaked",)]

# SC.CTC_CASES' format (name, T, B, C, Lmax, tg_len, in_len, logits kind, targets, family), inputs by SC.ctc_inputs
CTC_CASES = [
    # ragged: one input length below T (padding rows: the gradient behind it is +0), target lengths 0, Lmax and one in between
    ("abi_ragged", 12, 3, 7, 5, [0, 5, 3], [12, 12, 9], "randn", "random", "ctc_plain"),
    next(c for c in SC.CTC_CASES if c[0] == "one_infeasible"),
    # NS = 2 * 130 + 1 = 261 states: the 256-thread loops of the alpha / beta kernels take a second trip, the 128-thread gradient loop a third
    ("abi_states_261", 265, 2, 9, 130, [130, 64], [265, 200], "x3", "pairs", "ctc_peaked"),
]
DTW_CASES = SC.DTW_CASES


def ctc_workspace_bytes(T, B, Lmax):
    """hwg_ctc_workspace: log_alpha and log_beta [B][T][2 Lmax + 1], nll [B], the flag word and three floats of padding"""
    return (2 * B * T * (2 * Lmax + 1) + B + 4) * 4


def dtw_workspace_bytes(T, B, L):
    LL = 2 * L + 1
    return (B * T * LL + 15) // 16 * 16 + B * (T + LL) * 4


# ---- losses, spectral norm -----------------------------------------------------------------------------------------------------------------------
LOSS_SIZES = [n for n in SC.LOSS_SIZES if n <= 131072]          # without the 2.1 M entry
LOSS_CASES = [c for c in SC.LOSS_CASES if c[2] in LOSS_SIZES and c[5] == "randn"]
LOSS_WORKSPACE_BYTES = 512 * 8
# rows, W, Wm: rows * W of 1, 255 and 4097; the mask is narrower than the image wherever W allows one (1 <= Wm)
MASKED_L1_CASES = [(1, 1, 1), (5, 51, 37), (17, 241, 200)]
SN_SHAPES = [(1, 1), (5, 7), (3, 4097), min(SC.SN_MODEL_SHAPES, key=lambda s: s[0] * s[1])]
SN_BANK = [(5, 7), (1, 1), (3, 4097), SN_SHAPES[3], (7, 70)]       # one hwg_spectral_update_multi / hwg_spectral_bwd_multi call over all of them


def spectral_workspace_bytes(R, K):
    return (R + K + 8) * 4 + 512 * 8 + 16


def spectral_partials(R, K):
    """(byte offset of hwg_spectral_bwd's double partials inside the workspace, how many it writes)"""
    return ((R + K + 8) * 4 + 7) // 8 * 8, max(1, min(512, -(-R * K // SC.SN_DOT_BLOCK)))
