"""The convolution geometries of tests/test_ops_gpu.py that tools/gen_golden_conv_dispatch.py records the dispatch of as well (not collected
by pytest): the named layer cases, the seeded random ones and the 4x4 stride-2 pad-0 layers of the two-tap Winograd entries."""
import os as _os

CONV_CASES = [
    # name, N,H,W,C,K,R,S, stride, pad, dil, transposed
    ("mfma128x128_bk32", 4, 32, 260, 32, 128, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("mfma128x64_bk16", 4, 32, 260, 16, 64, 3, 3, (1, 1), (0, 1), (1, 1), False),
    ("mfma128x32", 2, 20, 70, 32, 16, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("mfma64x64_smallM", 2, 4, 50, 128, 128, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("mfma_k80_edge", 2, 1, 61, 64, 80, 1, 3, (1, 1), (0, 0), (1, 1), False),
    ("mfma_c208", 2, 1, 40, 208, 128, 1, 3, (1, 1), (0, 1), (1, 1), False),
    ("dil4_conv1d", 2, 1, 60, 64, 64, 1, 3, (1, 1), (0, 4), (1, 4), False),
    ("stride2_4x4", 2, 16, 40, 32, 64, 4, 4, (2, 2), (1, 1), (1, 1), False),
    ("stride21_4x4", 2, 8, 30, 32, 32, 4, 4, (2, 1), (0, 1), (1, 1), False),
    ("k63_5x5", 1, 9, 20, 16, 48, 5, 5, (1, 1), (2, 2), (1, 1), False),
    ("c1_7x7", 2, 20, 50, 1, 64, 7, 7, (1, 1), (0, 3), (1, 1), False),
    ("c1_5x5", 2, 16, 40, 1, 32, 5, 5, (1, 1), (2, 2), (1, 1), False),
    ("c1_7x7_many_chunks", 4, 64, 256, 1, 64, 7, 7, (1, 1), (0, 3), (1, 1), False),
    ("c1_4x4_s2_k80", 2, 33, 70, 1, 80, 4, 4, (2, 2), (1, 1), (1, 1), False),
    ("c1_3x3", 2, 16, 41, 1, 64, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("to1_3x3", 3, 3, 20, 256, 1, 3, 3, (1, 1), (0, 1), (1, 1), False),
    ("to1_1x1", 3, 1, 20, 256, 1, 1, 1, (1, 1), (0, 0), (1, 1), False),
    ("to2_1x1", 3, 1, 20, 32, 2, 1, 1, (1, 1), (0, 0), (1, 1), False),
    ("to1_16", 2, 16, 40, 16, 1, 1, 1, (1, 1), (0, 0), (1, 1), False),
    ("to1_3x3_c64", 2, 20, 50, 64, 1, 3, 3, (1, 1), (1, 1), (1, 1), False),          # the nine-loads-in-flight 3x3 head kernel (decoder image head)
    ("to1_3x3_c32_pad01", 3, 9, 31, 32, 1, 3, 3, (1, 1), (0, 1), (1, 1), False),
    ("to1_3x3_c48", 2, 7, 23, 48, 1, 3, 3, (1, 1), (1, 1), (1, 1), False),           # (12 of the 16 lanes of a pixel hold channels)
    ("convT_lift_4x3", 2, 1, 30, 208, 256, 4, 3, (1, 1), (0, 1), (1, 1), True),
    ("convT_s2_4x4", 2, 8, 20, 64, 32, 4, 4, (2, 2), (1, 1), (1, 1), True),
    ("convT_s1_3x3", 2, 6, 20, 32, 32, 3, 3, (1, 1), (1, 1), (1, 1), True),
    ("convT_6x3", 2, 1, 12, 32, 64, 6, 3, (1, 1), (0, 0), (1, 1), True),
    ("convT_to1", 2, 8, 20, 32, 1, 3, 3, (1, 1), (1, 1), (1, 1), True),
    # one row on the narrow side: the data gradient of a pad-0 layer whose output has ONE row, and the forward of a transposed layer with
    # one input row, both run as their stride-(R, 1) twins (row classes with 1 x S taps each)
    ("onerow_out_3x3_c64", 2, 3, 40, 64, 48, 3, 3, (1, 1), (0, 1), (1, 1), False),
    ("onerow_out_6x3_c32", 3, 6, 25, 32, 64, 6, 3, (1, 1), (0, 0), (1, 1), False),
    ("onerow_out_3x3_c512", 2, 3, 30, 512, 512, 3, 3, (1, 1), (0, 0), (1, 1), False),
    ("onerow_out_4x4_s21", 2, 4, 41, 64, 64, 4, 4, (2, 1), (0, 0), (1, 1), False),
    ("onerow_out_4x4_s21_h5", 2, 5, 41, 64, 64, 4, 4, (2, 1), (0, 0), (1, 1), False),      # a dead fifth input row (the style extractor's last block)
    ("onerow_out_4x4_s22", 2, 4, 40, 32, 48, 4, 4, (2, 2), (0, 1), (1, 1), False),
    # Winograd F(2x2,3x3) path (3x3 / stride 1 / dilation 1, >= 16 output channels): odd sizes, every padding the networks use
    # (0/1 forward, 2 = data gradient of pad 0), channel counts off the tile sizes, the split-channel schedule, 16-wide layers
    ("wino_odd_pad1", 3, 9, 13, 16, 16, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("wino_pad0_k48", 2, 7, 30, 32, 48, 3, 3, (1, 1), (0, 0), (1, 1), False),
    ("wino_pad01_c48_k80", 2, 6, 21, 48, 80, 3, 3, (1, 1), (0, 1), (1, 1), False),
    ("wino_split_c256", 1, 4, 30, 256, 64, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("wino_k16_wide", 2, 32, 120, 16, 16, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("wino_c24_padded", 2, 5, 11, 24, 32, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("wino_big_tiles", 4, 20, 130, 64, 128, 3, 3, (1, 1), (0, 1), (1, 1), False),
    ("wino_1row", 2, 3, 40, 128, 256, 3, 3, (1, 1), (0, 1), (1, 1), False),
    # narrow layers (K, C <= 32, >= 16 k output pixels): the all-taps 16x16x4 weight-gradient kernel, 1 / 2 / 4 channel blocks, ragged blocks
    ("narrow_16x16_3x3", 2, 64, 160, 16, 16, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("narrow_16to32_4x4s2", 3, 128, 200, 16, 32, 4, 4, (2, 2), (1, 1), (1, 1), False),
    ("narrow_32x32_3x3_pad0", 2, 42, 258, 32, 32, 3, 3, (1, 1), (0, 0), (1, 1), False),
    ("narrow_c20_k24", 2, 64, 161, 20, 24, 3, 3, (1, 1), (1, 1), (1, 1), False),
    # single-channel first layers with 64 filters and >= 4096 output pixels: weight gradient with the input rows staged in LDS (c1rows_*, the
    # default) - ragged last segment, pads 0 / 1 / 2 / 3 - and on the VALU weight-gradient kernel (wgrad_c1_kernel, HWG_WGRAD_C1=1;
    # off by default: measured slower than the taps-as-N MFMA kernel) - ragged last 64-pixel group, pad 0 / 1 / 3, dilation, few and many ranges
    ("c1rows_3x3", 3, 40, 67, 1, 64, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("c1rows_5x5_pad0", 2, 36, 131, 1, 64, 5, 5, (1, 1), (0, 0), (1, 1), False),
    ("c1rows_7x7", 2, 70, 150, 1, 64, 7, 7, (1, 1), (0, 3), (1, 1), False),
    ("c1rows_7x7_pad2", 5, 33, 129, 1, 64, 7, 7, (1, 1), (2, 2), (1, 1), False),
    ("c1valu_3x3", 3, 40, 67, 1, 64, 3, 3, (1, 1), (1, 1), (1, 1), False),
    ("c1valu_5x5_pad0", 2, 36, 131, 1, 64, 5, 5, (1, 1), (0, 0), (1, 1), False),
    ("c1valu_7x7_dil2", 2, 70, 150, 1, 64, 7, 7, (1, 1), (3, 6), (1, 2), False),
    ("c1valu_3x3_big", 8, 64, 256, 1, 64, 3, 3, (1, 1), (1, 1), (1, 1), False),
    # RIMES (78 classes): channel counts that are not multiples of 4
    ("rimes_convT_lift_206", 2, 1, 20, 206, 64, 4, 3, (1, 1), (0, 1), (1, 1), True),
    ("rimes_conv1d_to78", 2, 1, 30, 64, 78, 1, 3, (1, 1), (0, 0), (1, 1), False),
    ("rimes_conv1d_334", 2, 1, 30, 334, 32, 1, 5, (1, 1), (0, 2), (1, 1), False),
]


WINO_S2_CASES = [(2, 12, 20, 16, 64, ""), (1, 10, 38, 32, 80, ""), (3, 8, 26, 64, 128, "HWG_WINO_FORCE=6,2"), (2, 14, 44, 48, 64, "HWG_WINO_BAL=7"),
                 (2, 6, 130, 128, 96, "HWG_WINO_FORCE=6,4"), (1, 16, 64, 32, 256, "HWG_WINO_BAL=40,0"), (4, 66, 130, 64, 128, "")]



def _random_conv_cases(n=36, seed=2026):
    import random
    rnd = random.Random(seed)
    cases = []
    while len(cases) < n:
        transposed = rnd.random() < 0.25
        C = rnd.choice([1, 3, 16, 16, 32, 48, 64, 80, 128, 208, 256])
        K = rnd.choice([1, 2, 16, 32, 64, 78, 80, 128, 256])
        R = rnd.choice([1, 1, 3, 3, 4, 5, 7]); S = rnd.choice([1, 3, 3, 4, 5, 7])
        if transposed:
            st = rnd.choice([(1, 1), (2, 2), (2, 1)]); dil = (1, 1)
            R = max(R, st[0]); S = max(S, st[1])
            pad = (rnd.randint(0, min(1, R - 1)), rnd.randint(0, min(1, S - 1)))
        else:
            st = rnd.choice([(1, 1), (1, 1), (2, 2), (2, 1)])
            dil = rnd.choice([(1, 1), (1, 1), (1, 2), (2, 1)]) if st == (1, 1) else (1, 1)
            pad = (rnd.randint(0, R // 2 + 1), rnd.randint(0, S // 2 + 1))
        N = rnd.randint(1, 5); H = rnd.randint(1, 19); W = rnd.randint(1, 75)
        if not transposed:
            if H + 2 * pad[0] < dil[0] * (R - 1) + 1 or W + 2 * pad[1] < dil[1] * (S - 1) + 1:
                continue
        if transposed and ((H - 1) * st[0] - 2 * pad[0] + R < 1 or (W - 1) * st[1] - 2 * pad[1] + S < 1):
            continue      # empty output
        if (C == 1 and K <= 2) or N * H * W * max(C, K) > 3_000_000:
            continue
        cases.append(("rnd%d_C%dK%d_%dx%d_s%s_p%s_d%s%s" % (len(cases), C, K, R, S, st, pad, dil, "_T" if transposed else ""), N, H, W, C, K, R, S, st, pad, dil,
                      transposed))
    return cases


RANDOM_CONV_CASES = _random_conv_cases(int(_os.environ.get("HWG_TEST_RANDOM_CONVS", "36")), int(_os.environ.get("HWG_TEST_RANDOM_SEED", "2026")))
