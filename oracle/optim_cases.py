"""Case tables of tests/test_optim_rng_fp64_gpu.py (the multi-tensor optimizer kernels, the Philox kernels and insert_spaces of
csrc/optim_rng.hip against the restatements of oracle/optim_ref.py), their seeded inputs, and the regime bookkeeping
tests/test_optim_rng_ref_cpu.py checks them with. numpy and torch only: nothing here needs the library or a GPU."""
import zlib

import numpy as np
import torch

CHUNK = 65536                 # trainer/flat_params.py's chunk (tests/test_optim_rng_ref_cpu.py asserts they are the same)
SMALL_CHUNK = 4096            # the kernels take the chunk as an argument: multi-chunk tensors stay small with this one
GUARD = 64                    # sentinel floats before and behind every buffer
SENTINEL = -7250.0            # also in the padding of every tensor to a multiple of 4 floats (the FlatParams layout)
THREADS = 256
# elements one workgroup moves per trip of its 16-byte loop: MT_U = 4 pieces per thread (unary, axpy, the clip-only branch), AU = 2 (the two
# Adam kernels), one piece (abs-sum, axpy-sets)
TRIP = {"unary": 4 * THREADS * 4, "adam": 2 * THREADS * 4, "single": THREADS * 4}


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ---- tensor-list geometry --------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 5, 7,                                        # under one 16-byte piece, or one piece and a tail
         1023, 1024, 1025,                                        # around the 1024-element trip of abs-sum / axpy-sets
         1200, 1201, 1202, 1203, 2047, 2048, 2052, 4100, 6147,    # partial last trips: the clamped duplicate load, which must not store
         65535, 65536, 65537, 65540, 131075,                      # chunk edges
         200003]                                                  # one large tensor: 4 chunks of 65536 (49 of 4096), odd tail
NT = len(SIZES)
# name, chunk, absent tensors (pointer entry 0), misaligned (every tensor starts one float behind a 16-byte boundary: the al == false
# scalar path, which FlatParams never produces)
LISTS = [
    ("chunk65536", CHUNK, (), False),
    ("chunk4096_absent", SMALL_CHUNK, (0, 11, NT - 1), False),
    ("chunk4096_misaligned", SMALL_CHUNK, (), True),
]


class Layout:
    """where the tensors of a list live in one flat float buffer: [guard | t0 pad | t1 pad | ... | guard], and the kernels' chunk tables"""

    def __init__(self, sizes, chunk, misaligned=False):
        self.sizes, self.chunk, self.misaligned = list(sizes), chunk, misaligned
        self.nt = len(self.sizes)
        pos, offs = GUARD, []
        for n in self.sizes:
            offs.append(pos + (1 if misaligned else 0))
            pos += (n + 3) // 4 * 4 + (4 if misaligned else 0)
        self.offsets = np.array(offs, dtype=np.int64)
        self.numel = np.array(self.sizes, dtype=np.int64)
        self.total = pos + GUARD
        ct, co = [], []
        for k, n in enumerate(self.sizes):
            for off in range(0, n, chunk):
                ct.append(k); co.append(off)
        self.chunk_tensor, self.chunk_off = np.array(ct, dtype=np.int32), np.array(co, dtype=np.int64)
        self.nchunks = len(ct)

    def slices(self):
        return [slice(int(o), int(o + n)) for o, n in zip(self.offsets, self.numel)]

    def mask(self, present=None):
        """bool [total]: the elements of the (present) tensors"""
        m = np.zeros(self.total, dtype=bool)
        for k, sl in enumerate(self.slices()):
            if present is None or present[k]:
                m[sl] = True
        return m

    def tensor_of(self):
        """int [total]: the tensor an element belongs to, -1 outside every tensor"""
        t = np.full(self.total, -1, dtype=np.int64)
        for k, sl in enumerate(self.slices()):
            t[sl] = k
        return t

    def buffer(self, name, scale=1.0, positive=False):
        """float32 [total]: seeded normals (squared if positive) times scale in the tensors, the sentinel everywhere else"""
        x = torch.randn(self.total, generator=gen(name))
        x = (x * x if positive else x) * scale
        x[torch.from_numpy(~self.mask())] = SENTINEL
        return x


def list_layout(entry):
    name, chunk, absent, misaligned = entry
    present = np.ones(NT, dtype=bool)
    present[list(absent)] = False
    return Layout(SIZES, chunk, misaligned), present


def chunk_regimes(n, chunk, misaligned):
    """tags of one tensor of n elements: per chunk the 16-byte pieces n4, the trips of each loop family, a partial last trip (some thread
    holds a first piece but not all of its later ones: the clamped load), a scalar tail"""
    tags = set()
    nch = -(-n // chunk)
    tags.add("chunks 1" if nch == 1 else "chunks > 1")
    if n < 4:
        tags.add("under one piece")
    for off in range(0, n, chunk):
        ln = min(chunk, n - off)
        if misaligned:
            tags.add("misaligned: scalar path")
            continue
        n4 = ln // 4
        if ln % 4:
            tags.add("scalar tail")
        if ln == chunk:
            tags.add("full chunk")
        elif off:
            tags.add("short last chunk")
        for fam, trip in TRIP.items():
            pieces = trip // 4
            trips = -(-n4 // pieces)
            tags.add("%s trips %s" % (fam, "0" if trips == 0 else "1" if trips == 1 else "> 1"))
            if fam != "single" and n4 % pieces:
                tags.add("%s partial last trip" % fam)
                if (n4 % pieces) % THREADS:
                    tags.add("%s clamped load inside a wave of pieces" % fam)
    return tags


def list_regimes(entry):
    name, chunk, absent, misaligned = entry
    tags = set()
    for k, n in enumerate(SIZES):
        if k in absent:
            tags.add("absent " + ("first" if k == 0 else "last" if k == NT - 1 else "middle"))
        else:
            tags |= chunk_regimes(n, chunk, misaligned)
    if any(n % 4 for n in SIZES):
        tags.add("padding canaries")
    return tags


# ---- balance -----------------------------------------------------------------------------------------------------------------------------------
# name, nt, nsets, kind. kinds: "mixed" = random sums with planted all-zero gradients (tensors 1 and nt - 2: the replacement mean), all-zero
# stashed tensors, absent stashed tensors and absent gradients; "all_zero_grad" = every gradient sum 0 (zc = 0: every coefficient 0)
BALANCE_CASES = [("nt%d_s%d" % (nt, ns), nt, ns, "mixed") for nt in (1, 255, 256, 257, 300) for ns in (1, 2, 8)] + [("zc0", 300, 2, "all_zero_grad")]


def balance_inputs(case):
    """-> sum_d [nt], sum_r [nsets][nt] float64, numel [nt] int64, grad_present [nt], r_present [nsets][nt] bool, xs [nsets] float32"""
    name, nt, ns, kind = case
    g = gen("balance_" + name)
    numel = torch.randint(1, 70000, (nt,), generator=g).numpy().astype(np.int64)
    sum_d = (torch.rand(nt, generator=g).double() * 1e-2 + 1e-5).numpy() * numel
    sum_r = (torch.rand(ns, nt, generator=g).double() * 1e-1 + 1e-6).numpy() * numel[None, :]
    grad_present, r_present = np.ones(nt, dtype=bool), np.ones((ns, nt), dtype=bool)
    xs = np.array([0.5, -1.0, 2.0, 0.25, 1.0, 3.0, 0.1, 0.7][:ns], dtype=np.float32)
    if kind == "all_zero_grad":
        sum_d[:] = 0.0
    else:
        for t in {1 % nt, (nt - 2) % nt}:
            if nt > 2:
                sum_d[t] = 0.0                                     # an all-zero gradient: its mean is replaced
        for k in range(ns):
            sum_r[k, (3 + 5 * k) % nt] = 0.0                       # an all-zero stashed tensor
            if nt > 1:
                r_present[k, (7 + 11 * k) % nt] = False            # an absent one
        if nt > 4:
            grad_present[nt // 2] = False                          # no gradient: the tensor counts nowhere
            r_present[:, nt // 2] = False
    return sum_d, sum_r, numel, grad_present, r_present, xs


def balance_regimes(case):
    name, nt, ns, kind = case
    sum_d, sum_r, numel, gp, rp, xs = balance_inputs(case)
    tags = {"nsets %d" % ns, "nt %s 256" % ("<" if nt < 256 else "=" if nt == 256 else ">")}
    if nt == 1:
        tags.add("nt 1")
    if ns * nt > 256:
        tags.add("coefficient loop strides")
    if bool((gp & (sum_d == 0)).any()) and bool((gp & (sum_d != 0)).any()):
        tags.add("zero mean replaced")
    if not bool((gp & (sum_d != 0)).any()):
        tags.add("zc = 0")
    if bool((rp & (sum_r == 0)).any()):
        tags.add("stashed all zero")
    if bool((~rp & gp[None, :]).any()):
        tags.add("stashed absent")
    if bool((~gp).any()):
        tags.add("gradient absent")
    return tags


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------------------
ADAM_EPS, ADAM_LR, ADAM_CLIP = 1e-8, 2e-4, 2.0
ADAM_STEPS = (1, 2, 10, 1000)                 # tensor k of a case is at step ADAM_STEPS[(k + rotation) % 4]
# name, betas, gradient scale. 1e-6: sqrt(v) is of eps' size; 1e3: every element clips
ADAM_CASES = [("b%s_g%s" % (str(b[0])[2:], s), b, float(s)) for b in ((0.5, 0.999), (0.9, 0.999)) for s in ("1", "1e-6", "1e3")]


def adam_inputs(case, layout):
    """-> p, g, m, v float32 [total] with planted elements: buffer positions i % 97 == 0 hold g = m = v = 0 (the update is exactly 0),
    i % 89 == 1 / i % 83 == 2 hold g = +clip / -clip exactly (clipping leaves them unchanged); steps [nt]"""
    name, betas, gs = case
    p = layout.buffer("adam_p_" + name)
    g = layout.buffer("adam_g_" + name, gs)
    m = layout.buffer("adam_m_" + name, 0.3 * min(gs, ADAM_CLIP))
    v = layout.buffer("adam_v_" + name, min(gs, ADAM_CLIP) ** 2, positive=True)
    i = torch.arange(layout.total)
    inside = torch.from_numpy(layout.mask())
    zero = inside & (i % 97 == 0)
    for t in (g, m, v):
        t[zero] = 0.0
    g[inside & ~zero & (i % 89 == 1)] = ADAM_CLIP
    g[inside & ~zero & (i % 83 == 2)] = -ADAM_CLIP
    rot = zlib.crc32(name.encode()) % 4
    steps = np.array([ADAM_STEPS[(k + rot) % 4] for k in range(layout.nt)], dtype=np.int64)
    return p, g, m, v, steps, zero


def adam_regimes(case, layout):
    name, betas, gs = case
    p, g, m, v, steps, zero = adam_inputs(case, layout)
    inside = torch.from_numpy(layout.mask())
    tags = {"betas %s" % (betas,), "scale %g" % gs} | {"step %d" % s for s in steps.tolist()}
    if bool(zero.any()):
        tags.add("g = v = 0")
    if bool((g[inside] == ADAM_CLIP).any()) and bool((g[inside] == -ADAM_CLIP).any()):
        tags.add("exactly at the clip")
    planted = zero | (g.abs() == ADAM_CLIP)
    frac = float((g[inside & ~planted].abs() > ADAM_CLIP).float().mean())
    tags.add("clips all" if frac > 0.99 else "clips some" if frac > 0 else "clips none")
    if float(v[inside & ~zero].sqrt().median()) < 100 * ADAM_EPS:
        tags.add("eps matters")
    return tags


# the three HipAdam steps against torch.optim.Adam: which tensors have a gradient in each (step counts diverge)
HIPADAM_STEPS = [lambda k: True, lambda k: k % 2 == 0, lambda k: k % 3 != 1]
HIPADAM_BETAS = (0.5, 0.999)


# ---- Philox ----------------------------------------------------------------------------------------------------------------------------------------
RNG_GRID_ELEMS = 4 * 2048 * 256                  # elements one pass of hwg_stream_grid's capped grid writes
RNG_STREAMS = [
    ("zero", 0, 0),
    ("high_seed", 0x9E3779B97F4A7C15, 12345),                 # a seed with a non-zero high word
    ("carry", 1234, 2 ** 32 - 2),                             # with n = 16 the counter's low word wraps: the carry enters the second word
    ("offset40", 987654321, 2 ** 40 + 5),                     # an offset past 32 bits
]
RNG_SIZES = [1, 2, 3, 4, 5, 16, 4097, 2098379]                # 16: the carry case's four blocks; the last one past RNG_GRID_ELEMS
DROP_PS = (0.0, 0.1, 0.5, 0.999)
DROP_SIZES = (5, 4097)
DROP_MULTI = [1, 3, 16]                                       # segments; 17 are refused


def drop_multi_segments(nseg):
    sizes = [4 * (1 + (37 * j) % 300) for j in range(nseg)]
    ps = [DROP_PS[j % 4] if j % 5 else 0.3 for j in range(nseg)]
    return sizes, ps


def rng_regimes(name, seed, offset, n):
    tags = set()
    if seed >> 32:
        tags.add("seed high word")
    if offset >> 32:
        tags.add("offset high word")
    last = offset + (n + 3) // 4 - 1
    if (offset >> 32) != (last >> 32):
        tags.add("carry into the second counter word")
    if n % 4:
        tags.add("partial last block")
    if n > RNG_GRID_ELEMS:
        tags.add("grid-stride second trip")
    if n < 4:
        tags.add("under one block")
    return tags


# ---- insert_spaces -----------------------------------------------------------------------------------------------------------------------------------
INSERT_CLASSES = 80
# name, L, B, label lengths, count_std, dup_std, count_duplicates, counts kind, seed, offset, T cut (None: the wrapper's own T).
# counts kinds: "model" = blanks around 1.5, repeats around 2.5 (what the spacing network predicts); "ties" = 0.5 / 1.5 / 2.5 cycling (with
# std 0 the output is rint(c): round half to even gives 0 / 2 / 2); "negative" = means below zero (clamped to 0)
INSERT_CASES = [
    ("one", 1, 1, [1], 0.1, 0.1, True, "model", 11, 0, None),
    ("l12", 12, 2, [12, 0], 0.1, 0.1, True, "model", 12, 7, None),                                  # label lengths 0 and L
    ("l40_nodup", 40, 8, [40, 33, 1, 0, 17, 40, 25, 8], 0.1, 0.1, False, "model", 13, 2 ** 32 - 100, None),    # repeats fixed at 1; a carry
    ("l130", 130, 3, [130, 77, 129], 0.1, 0.1, True, "model", 14, 100, None),                       # L * B = 390 > 256: the loops stride
    ("ties_std0", 12, 2, [12, 9], 0.0, 0.0, True, "ties", 15, 0, None),
    ("negative", 12, 2, [12, 5], 0.1, 0.1, True, "negative", 16, 3, None),
    ("truncated", 12, 2, [12, 12], 0.1, 0.1, True, "model", 17, 0, "cut"),                          # T inside the last run of line 0
]
INSERT_NEAR_TIE = 1e-4                         # a pre-rounding value this close to a half-integer may round either way on the device


def insert_inputs(case):
    """-> counts float32 [L][B][2], label int32 [L][B] (classes 1 .. INSERT_CLASSES - 1), lens int32 [B]"""
    name, L, B, lens, cs, ds, dup, kind, seed, offset, cut = case
    g = gen("insert_" + name)
    if kind == "ties":
        tie = torch.tensor([0.5, 1.5, 2.5])
        counts = torch.stack([tie[torch.arange(L * B) % 3], tie[(torch.arange(L * B) + 1) % 3]], dim=1).reshape(L, B, 2)
    elif kind == "negative":
        counts = -torch.rand(L, B, 2, generator=g) - 0.7
        counts[0, 0, 1] = 2.2                                        # one run survives: the fill has something to write
    else:
        counts = torch.tensor([1.5, 2.5]) + 0.8 * torch.randn(L, B, 2, generator=g)
    label = torch.randint(1, INSERT_CLASSES, (L, B), generator=g, dtype=torch.int32)
    return counts.float().contiguous(), label, torch.tensor(lens, dtype=torch.int32)


def insert_near_ties(pre, lens, count_duplicates):
    """bool [B][2L]: elements whose pre-rounding value lies within INSERT_NEAR_TIE of a half-integer (they may be left out of the comparison)"""
    B, L = pre.shape[:2]
    out = np.zeros((B, 2 * L), dtype=bool)
    for b in range(B):
        n = int(lens[b])
        frac = np.abs(pre[b, :n] - np.floor(pre[b, :n]) - 0.5) < INSERT_NEAR_TIE
        out[b, 0:2 * n:2] = frac[:, 0]
        if count_duplicates:
            out[b, 1:2 * n:2] = frac[:, 1]
    return out


def insert_regimes(case):
    name, L, B, lens, cs, ds, dup, kind, seed, offset, cut = case
    tags = {"duplicates " + ("on" if dup else "off")}
    if L * B > 256:
        tags.add("L * B > 256")
    if L * B == 1:
        tags.add("one character")
    if 0 in lens:
        tags.add("length 0")
    if L in lens:
        tags.add("length L")
    if cs == 0 and ds == 0 and kind == "ties":
        tags.add("std 0 ties")
    if kind == "negative":
        tags.add("negative means")
    if cut:
        tags.add("T truncates")
    return tags


REQUIRED_REGIMES = {
    "lists": {"chunks 1", "chunks > 1", "under one piece", "scalar tail", "full chunk", "short last chunk", "misaligned: scalar path",
              "absent first", "absent middle", "absent last", "padding canaries"}
             | {"%s trips %s" % (f, t) for f in TRIP for t in ("0", "1", "> 1")}
             | {"%s partial last trip" % f for f in ("unary", "adam")} | {"%s clamped load inside a wave of pieces" % f for f in ("unary", "adam")},
    "balance": {"nsets 1", "nsets 2", "nsets 8", "nt < 256", "nt = 256", "nt > 256", "nt 1", "coefficient loop strides", "zero mean replaced",
                "zc = 0", "stashed all zero", "stashed absent", "gradient absent"},
    "adam": {"betas (0.5, 0.999)", "betas (0.9, 0.999)", "scale 1", "scale 1e-06", "scale 1000", "step 1", "step 2", "step 10", "step 1000",
             "g = v = 0", "exactly at the clip", "clips all", "clips some", "eps matters"},
    "rng": {"seed high word", "offset high word", "carry into the second counter word", "partial last block", "grid-stride second trip",
            "under one block"},
    "insert": {"duplicates on", "duplicates off", "L * B > 256", "one character", "length 0", "length L", "std 0 ties", "negative means",
               "T truncates"},
}
