"""Plain restatements of the optimizer-tail, Philox and insert-spaces family (csrc/optim_rng.hip, csrc/philox.h), for the tests that hold the
HIP kernels against them. No kernel is needed to run anything here: float64 torch / numpy and Python integers, written from the definitions.

  abs_sum:          sum |g| of one tensor
  balance_coef:     the balanced add of trainer/hw_with_style_trainer.py:341-376: D_t = mean|grad_t|, zero means are replaced by the mean of
                    the non-zero ones; coef[k][t] = x_k * D_t / R_kt with R_kt = mean|stash_k,t|, 0 where the stashed tensor is absent or
                    all zero (and where the tensor has no gradient)
  axpy:             dst + sum_k coef_k * src_k
  clamp:            torch.clamp: a NaN stays NaN, an infinity becomes the bound
  adam_step:        the kernels' arithmetic contract, in float64 on the values the kernels receive (betas and eps rounded to fp32, the fp32
                    step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) that HipAdam.step uploads):
                      g = clamp(g, -clip, clip) if clip > 0;  m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g^2;  p -= ss * m / (sqrt(v) / bc2 + eps)
                    With the exact double betas this is torch.optim.Adam (no weight decay, no amsgrad).
  philox4x32:       Philox4x32-10 (Salmon et al., Random123) in Python integers; the kernels' block of (seed, ctr) has counter
                    (lo32(ctr), hi32(ctr), 0, 0) and key (lo32(seed), hi32(seed)). philox_blocks is the same in numpy uint64 lanes.
  u01:              ((float)(x >> 8) + 0.5f) * 2^-24 in numpy float32, bit for bit hwg_u01 - including the tie that rounds to even from
                    x >> 8 = 2^23 on, so that the interval is (0, 1]
  randn:            Box-Muller in float64 from those fp32 uniforms; the four normals of a block are (ra cos a, ra sin a, rb cos b, rb sin b),
                    ra = sqrt(-2 ln u0), a = 2 pi u1, rb = sqrt(-2 ln u2), b = 2 pi u3
  dropmask:         keep where u01 >= float32(p), kept value 1 / (1 - float32(p))
  insert_spaces_*:  model/hw_with_style.py:302-328 with the device generator: one block per (line b, character j) at counter
                    offset + b * L + j; blanks = max(rint(c0 + count_std z0), 0), repeats = max(rint(c1 + dup_std z1), 0) (1 without
                    count_duplicates), z0 / z1 the two cosine normals of the block, rint = round half to even (Python's round)"""
import math

import numpy as np
import torch

M32 = 0xFFFFFFFF
PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)


# ---- multi-tensor operations ---------------------------------------------------------------------------------------------------------------
def abs_sum(g):
    return float(g.double().abs().sum())


def balance_coef(sum_d, sum_r, numel, grad_present, r_present, xs):
    """sum_d [nt], sum_r [nsets][nt] float64 sums of |.|, numel [nt], grad_present [nt] / r_present [nsets][nt] bool, xs [nsets]
    -> coef [nsets][nt] float64"""
    sum_d, sum_r = np.asarray(sum_d, dtype=np.float64), np.asarray(sum_r, dtype=np.float64)
    numel = np.asarray(numel, dtype=np.float64)
    grad_present, r_present = np.asarray(grad_present, dtype=bool), np.asarray(r_present, dtype=bool)
    d = sum_d / numel
    nonzero = grad_present & (d != 0)
    if nonzero.any():
        d = np.where(grad_present & (d == 0), d[nonzero].sum() / nonzero.sum(), d)
    r = sum_r / numel[None, :]
    live = grad_present[None, :] & r_present & (r != 0)
    xs = np.asarray(xs, dtype=np.float64)[:, None]
    return np.where(live, xs * d[None, :] / np.where(live, r, 1.0), 0.0)


def axpy(dst, srcs, coefs):
    out = dst.double().clone()
    for s, c in zip(srcs, coefs):
        out += float(c) * s.double()
    return out


def clamp(g, c):
    return torch.clamp(g, -c, c)


def adam_step(p, g, m, v, step_size, bc2_sqrt, beta1, beta2, eps, clip=0.0):
    """float64 tensors (or anything broadcastable for step_size / bc2_sqrt) -> (p, g, m, v) after the step; the inputs are not modified"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if clip > 0:
        g = clamp(g, clip)
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    p = p - step_size * (m / (v.sqrt() / bc2_sqrt + eps))
    return p, g, m, v


def adam_scalars(lr, beta1, beta2, steps):
    """(step_size, bc2_sqrt) in float64 for per-tensor step counts (numpy int array), from the exact betas"""
    t = np.asarray(steps, dtype=np.float64)
    return lr / (1.0 - beta1 ** t), np.sqrt(1.0 - beta2 ** t)


# ---- Philox --------------------------------------------------------------------------------------------------------------------------------
def philox4x32(counter, key, rounds=10, m=PHILOX_M, w=PHILOX_W):
    """counter: four 32-bit ints, key: two -> four 32-bit ints"""
    c, k = [int(x) & M32 for x in counter], [int(x) & M32 for x in key]
    for _ in range(rounds):
        p0, p1 = m[0] * c[0], m[1] * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + w[0]) & M32, (k[1] + w[1]) & M32]
    return tuple(c)


def philox_block(seed, ctr, **kw):
    """the block the kernels draw for (seed, ctr), both 64-bit"""
    seed, ctr = int(seed) & (2 ** 64 - 1), int(ctr) & (2 ** 64 - 1)
    return philox4x32((ctr & M32, ctr >> 32, 0, 0), (seed & M32, seed >> 32), **kw)


def philox_blocks(seed, ctr0, nblocks, m=PHILOX_M, w=PHILOX_W, ctr_bits=64):
    """blocks of the counters ctr0 .. ctr0 + nblocks - 1 (mod 2^64) -> uint32 [nblocks][4]; philox_block in numpy lanes"""
    seed = int(seed) & (2 ** 64 - 1)
    ctr = (np.uint64(int(ctr0) & (2 ** 64 - 1)) + np.arange(nblocks, dtype=np.uint64)) & np.uint64(2 ** ctr_bits - 1)     # wraps mod 2^64
    m32 = np.uint64(M32)
    c = [ctr & m32, ctr >> np.uint64(32), np.zeros(nblocks, dtype=np.uint64), np.zeros(nblocks, dtype=np.uint64)]
    k = [seed & M32, seed >> 32]
    for _ in range(10):
        p0, p1 = np.uint64(m[0]) * c[0], np.uint64(m[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & m32]
        k = [(k[0] + w[0]) & M32, (k[1] + w[1]) & M32]
    return np.stack(c, axis=1).astype(np.uint32)


def u01(x):
    """uint32 (array) -> float32 in (0, 1]"""
    x = np.asarray(x, dtype=np.uint32)
    return ((x >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def stream_blocks(n):
    """counters a call that writes n elements consumes"""
    return (n + 3) // 4


def box_muller(blocks, swap=False):
    """uint32 [nb][4] -> float64 [nb][4] = (ra cos a, ra sin a, rb cos b, rb sin b)"""
    u = u01(blocks).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a, b = 2.0 * math.pi * u[:, 1], 2.0 * math.pi * u[:, 3]
    first, second = (np.sin, np.cos) if swap else (np.cos, np.sin)
    return np.stack([ra * first(a), ra * second(a), rb * first(b), rb * second(b)], axis=1)


def randn(seed, offset, n, **kw):
    """-> float64 [n]: what hwg_randn(seed, offset) writes into n elements"""
    return box_muller(philox_blocks(seed, offset, stream_blocks(n), **kw)).reshape(-1)[:n]


def dropmask(seed, offset, n, p):
    """-> (keep bool [n], kept value float64)"""
    p32 = np.float32(p)
    u = u01(philox_blocks(seed, offset, stream_blocks(n))).reshape(-1)[:n]
    return u >= p32, 1.0 / (1.0 - float(p32))


# ---- insert_spaces -------------------------------------------------------------------------------------------------------------------------
def insert_spaces_draws(counts, lens, count_std, dup_std, seed, offset, counter=None):
    """counts float32 [L][B][2], lens [B] -> float64 [B][L][2]: c0 + count_std z0 and c1 + dup_std z1 before rounding (NaN beyond a line's
    length). count_std / dup_std as the kernel receives them (fp32). counter(b, j, L, B): position in the stream, b * L + j by default."""
    counts = np.asarray(counts, dtype=np.float32)
    L, B = counts.shape[:2]
    cs, ds = float(np.float32(count_std)), float(np.float32(dup_std))
    pre = np.full((B, L, 2), np.nan)
    for b in range(B):
        for j in range(int(lens[b])):
            i = b * L + j if counter is None else counter(b, j, L, B)
            z = box_muller(philox_blocks(seed, int(offset) + i, 1))[0]
            pre[b, j, 0] = float(counts[j, b, 0]) + cs * z[0]
            pre[b, j, 1] = float(counts[j, b, 1]) + ds * z[2]
    return pre


def round_half_even(x):
    return np.rint(x)


def round_half_up(x):
    return np.floor(x + 0.5)


def insert_spaces_reps(pre, lens, count_duplicates, rounding=round_half_even):
    """-> int [B][2L]: (blanks, repeats) per character, zeros beyond a line's length"""
    B, L = pre.shape[:2]
    reps = np.zeros((B, 2 * L), dtype=np.int64)
    for b in range(B):
        n = int(lens[b])
        reps[b, 0:2 * n:2] = np.maximum(rounding(pre[b, :n, 0]), 0)
        reps[b, 1:2 * n:2] = np.maximum(rounding(pre[b, :n, 1]), 0) if count_duplicates else 1
    return reps


def insert_spaces_layout(reps, lens, counts):
    """-> (starts [B][L] (defined below each length), lens_max [B + 1]): a character's run starts behind its blanks; lens_max[b] the expanded
    length of line b, lens_max[B] = max(ceil(max counts), 3)"""
    B, L = reps.shape[0], reps.shape[1] // 2
    starts, lens_max = np.zeros((B, L), dtype=np.int64), np.zeros(B + 1, dtype=np.int64)
    for b in range(B):
        pos = 0
        for j in range(int(lens[b])):
            pos += reps[b, 2 * j]
            starts[b, j] = pos
            pos += reps[b, 2 * j + 1]
        lens_max[b] = pos
    lens_max[B] = max(math.ceil(float(np.asarray(counts, dtype=np.float32).max())), 3)
    return starts, lens_max


def insert_spaces_fill(label, lens, reps, starts, T):
    """label int [L][B] -> idx int [T][B], 0 = blank; a run that passes T is cut there"""
    L, B = label.shape
    idx = np.zeros((T, B), dtype=np.int64)
    for b in range(B):
        for j in range(int(lens[b])):
            s, n = int(starts[b, j]), int(reps[b, 2 * j + 1])
            idx[s:min(s + n, T), b] = label[j, b]
    return idx


def insert_spaces_spaced(label, lens, reps, counts, num_class):
    """the reference's own construction for given draws: every line as the list [0] * blanks + [character] * repeats ..., a one-hot tensor
    [longest line + max_count][B][num_class] with the blank class behind each line's end, and the padded fraction of every line"""
    L, B = label.shape
    max_count = max(math.ceil(float(np.asarray(counts, dtype=np.float32).max())), 3)
    lines = []
    for b in range(B):
        line = []
        for j in range(int(lens[b])):
            line += [0] * int(reps[b, 2 * j]) + [int(label[j, b])] * int(reps[b, 2 * j + 1])
        lines.append(line)
    T = max(len(line) for line in lines) + max_count
    spaced = torch.zeros(T, B, num_class)
    for b, line in enumerate(lines):
        for t, cls in enumerate(line):
            spaced[t, b, cls] = 1
        spaced[len(line):, b, 0] = 1
    return spaced, [(T - len(line)) / T for line in lines]
