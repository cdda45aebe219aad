"""Case table of tests/test_lstm_fp64_gpu.py: the LSTM kernels of csrc/lstm.hip (hwg_lstm_fwd, hwg_lstm_bwd, hwg_lstm_pack_whh) at the smallest
hidden sizes that reach each template instance, each kind of partly filled k-slice and each batch tile, the seeded inputs, the impulse inputs
and an fp32 restatement of the documented summation order. A case is a dict: name, kind ("step" | "e2e"), H, B, T, tags (the regimes it covers).

  H     NJ / nj       slice                                             batch tile (lines per LDS image)
  4     NJ 1          partial (lane 0 alone)                            32
  64    NJ 1          full                                              32
  68    NJ 2          second j live in lane 0 only                      32
  132   NJ 4, nj 3    j = 3 dead; j = 2 live in lane 0 only             32
  260   NJ 8, nj 5    j = 5..7 dead; j = 4 live in lane 0 only          32
  512   NJ 8          full; the 64 KB LDS image at B >= 32              32
  516   NJ 16, nj 9   j = 9..15 dead; j = 8 live in lane 0 only         31
  768   NJ 16, nj 12  j = 12..15 dead, every live j full                21 (no power of two, no multiple of 4)
  1024  NJ 16         full; 64 KB image                                 16

B per H, from its tile c: 1, 3, 16, 17, c - 1, c, c + 1, 2 c + 1 (one pass of four lines with clamps; the k0 / k1 boundary of the forward
kernel from both sides; a full tile; a second tile of one line; a third tile). T in {1, 2, 3} for the per-step cases (the first step alone; one
recurrent product; the ping-pong workspaces once round) and one T = 6 case per H for the end-to-end check.

The fp64 reference is tests/_lstm_ref.py (loaded from there, not copied)."""
import importlib.util
import os
import sys
import zlib

import numpy as np
import torch

UNITS = 4                 # hidden units per workgroup (hwg_lstm_unit_slice)
MAX_CHUNK = 32
LDS_FLOATS = 16384
INSTANCES = (1, 2, 4, 8, 16)
H_TABLE = (4, 64, 68, 132, 260, 512, 516, 768, 1024)
E2E_T = 6


def ref():
    """tests/_lstm_ref.py, the numpy fp64 reference (one module object, whoever imported it first)"""
    if "_lstm_ref" not in sys.modules:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "_lstm_ref.py")
        spec = importlib.util.spec_from_file_location("_lstm_ref", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["_lstm_ref"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["_lstm_ref"]


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------------------
def chunk(H):
    """lines per LDS image (lstm_chunk; hwg_lstm_batch_tile for 1 <= H <= 1024)"""
    return min(MAX_CHUNK, LDS_FLOATS // H)


def nj(H):
    return (H + 63) // 64


def instance(H):
    """the NJ the entry points dispatch to"""
    return next(n for n in INSTANCES if nj(H) <= n)


def tiles(H, B):
    """[(b0, nb)] of the entry points' chunk loop"""
    c = chunk(H)
    return [(b0, min(c, B - b0)) for b0 in range(0, B, c)]


def batches(H):
    c = chunk(H)
    return sorted({b for b in (1, 3, 16, 17, c - 1, c, c + 1, 2 * c + 1) if b >= 1})


def regimes(H, B, T):
    """what a run of (H, B, T) reaches in the two step kernels"""
    tags = {"NJ%d" % instance(H), "chunk%d" % chunk(H), "first_step", "both_directions"}
    if nj(H) < instance(H):
        tags.add("dead_j")                 # a whole trailing j of the template instance holds no k < H
    if H % 64:
        tags.add("lane_partial")           # only some lanes of the last live j hold a k < H
    for b0, nb in tiles(H, B):
        if nb <= 3:
            tags.add("nb1to3")
        if nb == 16:
            tags.add("nb16")
        if nb == 17:
            tags.add("nb17")
        if nb == chunk(H):
            tags.add("nb_chunk")
        if nb % 4:
            tags.add("clamped_pass")
        if b0 > 0:
            tags.add("multi_chunk")
        if b0 >= 2 * chunk(H):
            tags.add("third_tile")
    if T > 1:
        tags.add("later_steps")
    if T > 2:
        tags.add("pingpong_round")
    return tags


REGIMES = (["NJ%d" % n for n in INSTANCES] + ["chunk%d" % c for c in (32, 31, 21, 16)]
           + ["dead_j", "lane_partial", "nb1to3", "nb16", "nb17", "nb_chunk", "clamped_pass", "multi_chunk", "third_tile", "first_step", "later_steps",
              "pingpong_round", "both_directions"])

CASES = []


def _add(kind, H, B, T):
    name = "%s_H%d_B%d_T%d" % (kind, H, B, T)
    assert name not in [c["name"] for c in CASES], name
    CASES.append(dict(name=name, kind=kind, H=H, B=B, T=T, tags=regimes(H, B, T)))


for _hi, _H in enumerate(H_TABLE):
    for _bi, _B in enumerate(batches(_H)):
        # (not the cross product: the first step alone at one line, every other batch size with a recurrent product - T alternates between 2 and
        # 3 along the batch sizes, shifted per H; the widest batch - three tiles - gets T = 3 as well)
        _add("step", _H, _B, 1 if _bi == 0 else 2 + (_hi + _bi) % 2)
    if (_hi + len(batches(_H)) - 1) % 2 == 0:
        _add("step", _H, batches(_H)[-1], 3)
    _add("e2e", _H, chunk(_H) + 1, E2E_T)

BY_NAME = {c["name"]: c for c in CASES}
STEP_CASES = [c for c in CASES if c["kind"] == "step"]
E2E_CASES = [c for c in CASES if c["kind"] == "e2e"]
IMPULSE_H = (64, 68, 132, 260, 1024)          # one per template instance; 64 lines: every k mod 64 class, two or more batch tiles
IMPULSE_B = 64


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def make_case(T, B, H, seed):
    """xproj and dy normal, weights and biases uniform in +-1/sqrt(H) (torch.nn.LSTM's initialisation), float32"""
    g = np.random.RandomState(seed)
    s = 1.0 / np.sqrt(H)
    c = dict(xp=[g.randn(T, B, 4 * H).astype(np.float32) for _ in range(2)],
             w=[g.uniform(-s, s, (4 * H, H)).astype(np.float32) for _ in range(2)],
             b=[g.uniform(-s, s, (4 * H,)).astype(np.float32) for _ in range(2)],
             dy=g.randn(T, B, 2 * H).astype(np.float32))
    return c


def inputs(c):
    return make_case(c["T"], c["B"], c["H"], zlib.crc32(c["name"].encode()) & 0x7FFFFFFF)


def valid_state(x):
    """gates [2][T][B][4H] and c [2][T][B][H] of the fp64 forward of the case, rounded to float32: a state the backward kernel can be handed
    without running the forward kernel"""
    d = lambda a: [v.astype(np.float64) for v in a]
    _, (gates, cs, _, _) = ref().layer_forward(d(x["xp"]), d(x["w"]), d(x["b"]))
    return gates.astype(np.float32), cs.astype(np.float32)


def k_walk(n, H):
    """a k < H for index n whose class k mod 64 is n mod 64 (n mod H below 64 units) and whose j alternates between the last j that holds the
    class - the partly filled slice - and the others"""
    if H < 64:
        return n % H
    cls = n % 64
    jmax = (H - 1 - cls) // 64
    return cls + 64 * (jmax if n % 2 == 0 else (n // 2) % (jmax + 1))


def forward_impulse(H, B=IMPULSE_B):
    """T = 2. At a direction's first step the input projection saturates the gates so that h is a multiple of a one-hot vector (unit
    hot[b] of line b: i, g, o = sig / tanh(+40) there, o = sig(-200) = 0 elsewhere); at its second step xproj = 0, b_hh = 0 and W_hh[r][k] = 1
    at k = k_walk(r) and 0 elsewhere: the pre-activation of gate row r is h[hot[b]] where k_walk(r) == hot[b] and +0 elsewhere."""
    hot = np.array([k_walk(b, H) for b in range(B)])
    col = np.array([k_walk(r % H, H) for r in range(4 * H)])          # every gate block meets every class
    xp = []
    for d in range(2):
        a = np.zeros((2, B, 4 * H), np.float32)
        first = 0 if d == 0 else 1
        a[first, :, 3 * H:] = -200.0
        for q in (0, 2, 3):
            a[first, np.arange(B), q * H + hot] = 40.0
        xp.append(a)
    w = np.zeros((4 * H, H), np.float32)
    w[np.arange(4 * H), col] = 1.0
    return dict(xp=xp, w=[w, w.copy()], b=[np.zeros(4 * H, np.float32) for _ in range(2)], dy=np.zeros((2, B, 2 * H), np.float32)), hot, col


def backward_impulse(H, rot, B=IMPULSE_B, seed=3):
    """T = 2, a state chosen so that every product is exact: at the backward's first step (t = 1 forward, t = 0 reverse) dy = 8 at unit
    hot[b] and 0 elsewhere, o = 1/2, c = 0 (tanhf(0) = 0), and (i, f, g, c_prev) picked per line so that dgates is ONE 1 in gate block
    blk[b] = (b // 16 + rot) mod 4 at unit hot[b] (block o: 2 tanhf(1), read back from the device); at its second step dy = 0, c = 0, o = i = 1/2,
    g = f = 0: dgates there is dh_rec / 4 in block g and 0 elsewhere, and dh_rec[u] = W_hh[blk H + hot][u] (times the device's 2 tanhf(1) in block
    o), W_hh random. A line of block f needs f = 1/2 and c_prev = 1 at its hot unit: there dc f = 2 reaches the second step and c = 1 is that
    step's own c, so the ONE element (line b, unit hot[b]) of such a line is left out of the exact comparison. -> (dy, gates, c, w), hot, blk"""
    g = np.random.RandomState(seed + H + rot)
    s = 1.0 / np.sqrt(H)
    w = [g.uniform(-s, s, (4 * H, H)).astype(np.float32) for _ in range(2)]
    hot = np.array([k_walk(b, H) for b in range(B)])
    blk = (np.arange(B) // 16 + rot) % 4
    dy = np.zeros((2, B, 2 * H), np.float32)
    gates = np.zeros((2, 2, B, 4 * H), np.float32)
    cs = np.zeros((2, 2, B, H), np.float32)
    for d in range(2):
        t0, t1 = (1, 0) if d == 0 else (0, 1)              # the backward's first and second step
        gates[d, :, :, 3 * H:] = 0.5                       # o
        gates[d, t1, :, :H] = 0.5                          # i of the second step
        for b in range(B):
            u = hot[b]
            dy[t0, b, d * H + u] = 8.0
            if blk[b] == 0:      # dc = 8 * 1/2 * 1 = 4; dg_i = dc g i (1 - i) = 4 * 1 * 1/2 * 1/2
                gates[d, t0, b, u], gates[d, t0, b, 2 * H + u] = 0.5, 1.0
            elif blk[b] == 1:    # dg_f = dc c_prev f (1 - f) = 4 * 1 * 1/2 * 1/2
                gates[d, t0, b, H + u] = 0.5
                cs[d, t1, b, u] = 1.0                      # c_prev of t0 is c of the forward walk's earlier row t1
            elif blk[b] == 2:    # dg_g = dc i (1 - g g) = 4 * 1/4 * 1
                gates[d, t0, b, u] = 0.25
            else:                # dg_o = dh tanhf(c) o (1 - o) = 8 * tanhf(1) / 4; i = 0 and c_prev = 0 keep the other blocks 0
                cs[d, t0, b, u] = 1.0
    return (dy, gates, cs, w), hot, blk


# ---- the documented summation order in float32 ---------------------------------------------------------------------------------------------------
# numpy and torch have no fused multiply-add: one step of a lane's chain is float32(float64(a) * float64(b) + float64(acc)). The product is exact
# in fp64 (24 + 24 bits); the sum is rounded to fp64 and then to fp32, which differs from the one rounding of fmaf in rare last-place cases. The
# activations are numpy's, not the device's expf / tanhf. The restatement is therefore a YARDSTICK for the size of an fp32 evaluation's error
# and for seeded flaws - never a bit-exact oracle: no test compares bits against it.
def k_schedule(H):
    """[(j, i, live lanes)] in the order a lane walks them: lane s < live adds element k = 64 j + 4 s + i"""
    return [(j, i, min(16, (H - 64 * j) // 4)) for j in range(nj(H)) for i in range(4)]


def lane_ks(H, s):
    """the k lane s sums, in order"""
    return [64 * j + 4 * s + i for j, i, live in k_schedule(H) if s < live]


def lane_dot(w, x, H):
    """w [R, K], x [B, K] float32 with K = blocks * H -> [B, R] float32: sum_k w[r][k] x[b][k], the blocks outermost in one chain per lane from +0,
    then the xor butterfly over the lane distances 1, 2, 4, 8"""
    wt, xt = torch.from_numpy(np.ascontiguousarray(w)).double(), torch.from_numpy(np.ascontiguousarray(x)).double()
    R, K = wt.shape
    B = xt.shape[0]
    acc = torch.zeros(16, B, R, dtype=torch.float32)
    lanes = torch.arange(16)
    for blk in range(K // H):
        for j, i, live in k_schedule(H):
            k = blk * H + 64 * j + 4 * lanes[:live] + i
            wk, xk = wt[:, k].t().contiguous(), xt[:, k].t().contiguous()            # [live, R], [live, B]
            acc[:live] = torch.addcmul(acc[:live].double(), xk[:, :, None], wk[:, None, :]).float()
    for dist in (1, 2, 4, 8):
        acc = acc + acc[lanes ^ dist]
    return acc[0].numpy()


def sigmoid32(x):
    one = np.float32(1)
    with np.errstate(over="ignore"):
        return (one / (one + np.exp(-x.astype(np.float32)))).astype(np.float32)


def restate_forward(x, dot=lane_dot):
    """the forward kernel's arithmetic in float32: -> y [T,B,2H], gates [2,T,B,4H], c [2,T,B,H], hseq [2,T+1,B,H]"""
    T, B, G = x["xp"][0].shape
    H = G // 4
    y = np.zeros((T, B, 2 * H), np.float32)
    gates = np.zeros((2, T, B, G), np.float32)
    cs = np.zeros((2, T, B, H), np.float32)
    hseq = np.zeros((2, T + 1, B, H), np.float32)
    for d in range(2):
        order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        for step, t in enumerate(order):
            pre = x["xp"][d][t] + x["b"][d]
            cp = np.zeros((B, H), np.float32)
            if step > 0:
                tp = order[step - 1]
                pre = pre + dot(x["w"][d], y[tp, :, d * H:(d + 1) * H], H)
                cp = cs[d, tp]
            a = np.concatenate([sigmoid32(pre[:, :2 * H]), np.tanh(pre[:, 2 * H:3 * H]), sigmoid32(pre[:, 3 * H:])], axis=1).astype(np.float32)
            i, f, g, o = (a[:, q * H:(q + 1) * H] for q in range(4))
            c = f * cp + i * g
            h = o * np.tanh(c)
            gates[d, t], cs[d, t], y[t, :, d * H:(d + 1) * H] = a, c, h
            hseq[d, t + 1 if d == 0 else t] = h
    return dict(y=y, gates=gates, c=cs, hseq=hseq)


def restate_backward(dy, gates, cs, w, dot=lane_dot):
    """the backward kernel's arithmetic in float32: -> dgates [2,T,B,4H], dc_ws [2,2,B,H] (slot step & 1 of step = 0 .. T-1: dc f)"""
    _, T, B, G = gates.shape
    H = G // 4
    dgates = np.zeros((2, T, B, G), np.float32)
    ws = np.zeros((2, 2, B, H), np.float32)
    one = np.float32(1)
    for d in range(2):
        order = list(range(T - 1, -1, -1)) if d == 0 else list(range(T))
        wt = np.ascontiguousarray(w[d].T)                                             # [H][4H]: row u holds column u of W_hh
        for step, t in enumerate(order):
            i, f, g, o = (gates[d, t][:, q * H:(q + 1) * H] for q in range(4))
            c = cs[d, t]
            cp = cs[d, order[step + 1]] if step + 1 < T else np.zeros((B, H), np.float32)
            dh = dy[t][:, d * H:(d + 1) * H]
            dcn = np.zeros((B, H), np.float32)
            if step > 0:
                dh = dh + dot(wt, dgates[d, order[step - 1]], H)
                dcn = ws[(step + 1) & 1, d]
            tc = np.tanh(c)
            dc = dcn + dh * o * (one - tc * tc)
            dgates[d, t] = np.concatenate([dc * g * i * (one - i), dc * cp * f * (one - f), dc * i * (one - g * g), dh * tc * o * (one - o)], axis=1)
            ws[step & 1, d] = dc * f
    return dict(dgates=dgates, dc_ws=ws)
