"""Case tables of tests/test_norm_act_fp64_gpu.py (the normalisation / activation kernels against fp64) and the geometry bookkeeping that
tests/test_norm_act_ref_cpu.py checks them with: a restatement of make_geo (csrc/norm_act.hip) and the regimes each case exercises.

The step geometries are those of one iam_gan_b4a2_w512 curriculum cycle (N, H*W, C, groups, activation, mask as the trainer calls them):
  discriminator GroupNorm 16 x 29696 x 64 / 8 groups / leaky relu 0.1; its masked GroupNorms 16 x 2048 x 64 and 16 x 8192 x 32 / relu
  style extractor GroupNorm 4 x 16384 x 128, 4 x 3328 x 256, 4 x 65536 x 64 / relu
  recogniser BatchNorm 8 x 1032 x 512 and 8 x 126 x 512 / relu
  generator epilogue 8 x 31232 x 16, 8 x 7808 x 32, 8 x 976 x 128, 8 x 488 x 256; generation calls (in-kernel noise) 64 x 5824 x 32
  discriminator bias_act 16 x 6656 x 128 / mask / leaky relu 0.1"""

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
NU, NORM_PASSES = 4, 4        # pixels in flight per thread, sweeps per workgroup (csrc/norm_act.hip)

# name, mode, N, H, W, C, groups, act, slope, mask, inputs, parameter-gradient path
#   inputs: "randn" = 2 * randn + 0.5; "offset16" = per-channel mean 16 sigma; "edges" = first statistic group constant (var 0), second group
#   sigma 1e-3 (var 1e-6, below eps); "eps-scale" = 3e-3 * randn. With a count of 2, BatchNorm's output is +-1 / sqrt(1 + eps / var) for any x,
#   so its data gradient is the eps / (var + eps) remainder of the terms it is formed from: at var ~ 4 that is 2.5e-6 of them and every fp32
#   evaluation keeps about 1e-3 of it; at var ~ eps the gradient is of the terms' size and the comparison well-conditioned.
#   path: "leaf" = leaf gamma / beta whose .grad is pre-filled (kernels accumulate), "fresh" = gamma * 1 / beta * 1 (kernels write), None = no affine
NORM_CASES = [
    ("step_D_gn_lrelu", "gn", 16, 58, 512, 64, 8, ACT_LRELU, 0.1, False, "randn", "leaf"),
    ("step_D_gn_mask", "gn", 16, 16, 128, 64, 8, ACT_RELU, 0.0, True, "randn", "fresh"),
    ("step_D_gn_mask_c32", "gn", 16, 32, 256, 32, 8, ACT_RELU, 0.0, True, "randn", "leaf"),
    ("step_style_gn", "gn", 4, 32, 512, 128, 8, ACT_RELU, 0.0, False, "randn", "leaf"),
    ("step_style_gn_c256", "gn", 4, 13, 256, 256, 8, ACT_RELU, 0.0, False, "edges", "fresh"),
    ("step_style_gn_offset16", "gn", 4, 64, 1024, 64, 8, ACT_RELU, 0.0, False, "offset16", "leaf"),
    ("step_hwr_bn", "bn", 8, 8, 129, 512, 1, ACT_RELU, 0.0, False, "randn", "leaf"),
    ("step_hwr_bn1d", "bn", 8, 1, 126, 512, 1, ACT_RELU, 0.0, False, "edges", "fresh"),
    ("halved_gn1_c1024_tanh", "gn", 65, 16, 16, 1024, 1, ACT_TANH, 0.0, False, "randn", "fresh"),
    ("chunk1_in_c32", "in", 2, 3, 5, 32, 1, ACT_NONE, 0.0, False, "edges", None),
    ("in_c48_ragged", "in", 3, 7, 131, 48, 1, ACT_NONE, 0.0, False, "offset16", None),
    ("bn_c4_ragged_lrelu", "bn", 2, 1, 5003, 4, 1, ACT_LRELU, 0.2, False, "edges", "leaf"),
    ("gn_c8_cpg2_tanh_mask", "gn", 3, 20, 33, 8, 4, ACT_TANH, 0.0, True, "edges", "leaf"),
    ("gn_c80_cpg16_lrelu_mask", "gn", 5, 9, 77, 80, 5, ACT_LRELU, 0.2, True, "randn", "fresh"),
    ("gn_c512_cpg64_relu", "gn", 2, 1, 300, 512, 8, ACT_RELU, 0.0, False, "edges", "leaf"),
    ("gn_c1024_chunk1_none", "gn", 3, 1, 3, 1024, 4, ACT_NONE, 0.0, False, "randn", "fresh"),
    ("bn_n1_tanh", "bn", 1, 16, 100, 64, 1, ACT_TANH, 0.0, False, "edges", "leaf"),
    ("bn_hw1_lrelu", "bn", 12, 1, 1, 256, 1, ACT_LRELU, 0.1, False, "randn", "fresh"),
    ("bn_count2_none", "bn", 2, 1, 1, 128, 1, ACT_NONE, 0.0, False, "eps-scale", "leaf"),
]

# name, N, H, W, C, noise ("tensor": noise from a tensor, forward + backward with the deferred reduction off and on; "virtual": ops.VirtualNoise,
# forward only, drawn inside the kernel)
ADAIN_CASES = [
    ("step_gen_c16", 8, 64, 488, 16, "tensor"),
    ("step_gen_c32", 8, 32, 244, 32, "tensor"),
    ("step_gen_c128", 8, 8, 122, 128, "tensor"),
    ("step_gen_c256", 8, 4, 122, 256, "tensor"),
    ("gen_c48_ragged", 3, 5, 67, 48, "tensor"),
    ("step_generate_c32", 64, 32, 182, 32, "virtual"),
    ("generate_c80_ragged", 5, 7, 91, 80, "virtual"),
]

# name, N, H, W, C, act, slope (eval-mode BatchNorm, no statistics pass)
FROZEN_CASES = [
    ("frozen_hwr_relu", 8, 8, 129, 512, ACT_RELU, 0.0),
    ("frozen_c4_tanh", 2, 3, 50, 4, ACT_TANH, 0.0),
    ("frozen_c80_lrelu", 3, 5, 31, 80, ACT_LRELU, 0.2),
]

# name, N, H, W, C, bias, mask, act, slope; every case has elements whose pre-activation is exactly 0
BIAS_ACT_CASES = [
    ("step_D_lrelu_mask", 16, 52, 128, 128, False, True, ACT_LRELU, 0.1),
    ("vec_bias_mask_odd4_2sweeps", 3, 1, 116509, 12, True, True, ACT_LRELU, 0.2),
    ("vec_relu_plain", 4, 2, 127, 256, False, False, ACT_RELU, 0.0),
    ("vec_relu_plain_odd4", 5, 1, 3, 12, False, False, ACT_RELU, 0.0),
    ("vec_bias_tanh", 2, 3, 9, 16, True, False, ACT_TANH, 0.0),
    ("vec_bias_none", 3, 2, 5, 8, True, False, ACT_NONE, 0.0),
    ("scalar_c1_bias_mask_relu", 3, 5, 7, 1, True, True, ACT_RELU, 0.0),
    ("scalar_c3_mask_lrelu", 2, 4, 11, 3, False, True, ACT_LRELU, 0.2),
    ("scalar_c78_bias_mask_lrelu", 4, 3, 5, 78, True, True, ACT_LRELU, 0.1),
]

TANH_SIZES = [(3, 50), (7, 100003)]       # the second spans more than one grid sweep (2048 x 256 threads)


def make_geo(N, HW, C):
    """csrc/norm_act.hip make_geo, restated: lanes per pixel, pixels per pass, raw and final chunk count, chunk length"""
    L = C // 4
    PP = 256 // L
    raw = -(-HW // (PP * NORM_PASSES))
    chunks = min(raw, 64)
    halved = False
    while chunks > 1 and chunks * N > 4096:
        chunks >>= 1
        halved = True
    chunks = max(chunks, 1)
    cs = -(-HW // chunks)
    chunks = -(-HW // cs)
    return dict(L=L, PP=PP, raw=raw, chunks=chunks, cs=cs, halved=halved)


def chunks_from_workspace(nbytes, N, C):
    """hwg_norm_workspace = 2 * N * chunks * C * 16 + 8 * N * C + 256 bytes, solved for chunks"""
    rest = nbytes - 256 - 8 * N * C
    assert rest > 0 and rest % (32 * N * C) == 0, (nbytes, N, C)
    return rest // (32 * N * C)


def geometry_regimes(N, HW, C):
    g = make_geo(N, HW, C)
    tags = set()
    if g["chunks"] == 1:
        tags.add("chunks=1")
    if g["raw"] > 64 and g["chunks"] == 64:
        tags.add("chunks capped at 64")
    if g["halved"]:
        tags.add("chunks halved (N*chunks > 4096)")
    if HW % g["cs"]:
        tags.add("ragged last chunk")
    if g["cs"] % (NU * g["PP"]):
        tags.add("chunk not a multiple of NU*PP")
    if C in (4, 48, 80, 1024):
        tags.add("C=%d" % C)
    if 256 % g["L"]:
        tags.add("idle threads")
    return tags


def norm_case_regimes(case):
    name, mode, N, H, W, C, groups, act, slope, mask, inputs, path = case
    tags = geometry_regimes(N, H * W, C) | {"mode " + mode, "act %d" % act, "inputs " + inputs}
    if name.startswith("step_"):
        tags.add("step geometry")
    if mask:
        tags.add("mask")
    if path:
        tags.add("param grads " + path)
    if mode == "gn":
        cpg = C // groups
        tags.add("gn one group" if groups == 1 else "gn cpg %d" % cpg)
    if mode == "bn":
        if N == 1:
            tags.add("bn N=1")
        if H * W == 1:
            tags.add("bn HW=1")
        if N * H * W == 2:
            tags.add("bn count 2")
    return tags


def bias_act_case_regimes(case):
    name, N, H, W, C, bias, mask, act, slope = case
    tags = {"act %d" % act}
    if C % 4:
        tags.add("scalar C=%d" % C)
        return tags
    total4 = N * H * W * C // 4
    tags.add("vector with bias and mask" if (bias and mask) else "vector without bias or mask" if not (bias or mask) else "vector")
    if total4 % 2:
        tags.add("odd float4 count")
    if total4 > 2 * 2048 * 256:
        tags.add("more than one grid sweep")
    return tags


REQUIRED_NORM_REGIMES = {
    "step geometry", "chunks=1", "chunks capped at 64", "chunks halved (N*chunks > 4096)", "ragged last chunk", "chunk not a multiple of NU*PP",
    "C=4", "C=1024", "C=48", "C=80", "idle threads", "gn cpg 2", "gn cpg 64", "gn one group", "bn N=1", "bn HW=1", "bn count 2",
    "inputs offset16", "inputs edges", "act 0", "act 1", "act 2", "act 3", "mask", "param grads leaf", "param grads fresh", "mode in", "mode gn", "mode bn",
}
REQUIRED_BIAS_ACT_REGIMES = {
    "vector with bias and mask", "vector without bias or mask", "odd float4 count", "more than one grid sweep", "scalar C=1", "scalar C=3",
    "scalar C=78", "act 0", "act 1", "act 2", "act 3",
}
