"""Plain torch restatements of the style-path and expert-bank kernels (csrc/style_ops.hip, csrc/expert_bank.hip). Every function works in
the dtype of its floating-point arguments: float64 gives the reference value, float32 (on the CPU) the yardstick, and - for the functions
that are sums of products - the same call on the absolute values of the arguments gives the sum of |terms| the error bound is formed from
(tests/test_style_expert_fp64_gpu.py). Forward and backward passes are written out separately (no autograd), so that the backward passes
can be run on absolute values too; tests/test_style_expert_ref_cpu.py checks them against torch's own ops and autograd in fp64.
"""
import torch
import torch.nn.functional as F


# ---- windows ----------------------------------------------------------------------------------------------------------------------------
def gather_windows(x, idx_b, idx_pos, w):
    """x [B, Wx, C] -> [n, 2w+1, C]: rows pos - w .. pos + w of line b, zero outside [0, Wx); a window whose centre (b, pos) lies outside
    the tensor is all zeros"""
    B, Wx, C = x.shape
    b, p = idx_b.long(), idx_pos.long()
    pos = p[:, None] + torch.arange(-w, w + 1)[None, :]
    ok = (pos >= 0) & (pos < Wx) & ((p >= 0) & (p < Wx) & (b >= 0) & (b < B))[:, None]
    rows = x[b.clamp(0, B - 1)[:, None], pos.clamp(0, Wx - 1)]
    return torch.where(ok[:, :, None], rows, torch.zeros((), dtype=x.dtype))


def scatter_windows(dp, idx_b, idx_pos, w, B, Wx):
    """the gradient of gather_windows: dp [n, 2w+1, C] -> dx [B, Wx, C]; windows overlap (at most 2w+1 terms per element), centres outside
    the tensor are ignored"""
    n, WW, C = dp.shape
    b, p = idx_b.long(), idx_pos.long()
    pos = p[:, None] + torch.arange(-w, w + 1)[None, :]
    ok = (pos >= 0) & (pos < Wx) & ((p >= 0) & (p < Wx) & (b >= 0) & (b < B))[:, None]
    flat = (b[:, None] * Wx + pos)[ok]
    return dp.new_zeros(B * Wx, C).index_add_(0, flat, dp[ok]).reshape(B, Wx, C)


def gather_scores(x, idx_b, idx_pos, idx_cls):
    return torch.exp(x[idx_b.long(), idx_pos.long(), idx_cls.long()])


# ---- confidence-weighted per-line mean ------------------------------------------------------------------------------------------------
def segment_mean(v, wgt, seg, B):
    """-> out [B, C], wsum [B]: total = sum of wgt_i v_i over the members of a line, out = total / wsum, or total where wsum == 0"""
    n, C = v.shape
    seg = seg.long()
    tot = v.new_zeros(B, C).index_add_(0, seg, wgt[:, None] * v)
    ws = v.new_zeros(B).index_add_(0, seg, wgt)
    nz = ws != 0
    return torch.where(nz[:, None], tot / torch.where(nz, ws, torch.ones_like(ws))[:, None], tot), ws


def segment_mean_bwd(dout, wgt, seg, wsum):
    ws = wsum[seg.long()]
    nz = ws != 0
    return torch.where(nz, wgt / torch.where(nz, ws, torch.ones_like(ws)), wgt)[:, None] * dout[seg.long()]


# ---- bank of linear layers sharing one input -------------------------------------------------------------------------------------------
def linear_bank_fwd(x, Ws, bs, halves):
    """-> per layer a list of `halves` tensors [B, O_l / halves]"""
    out = []
    for W, b in zip(Ws, bs):
        C = W.shape[0] // halves
        y = x @ W.t() + b
        out.append([y[:, h * C:(h + 1) * C] for h in range(halves)])
    return out


def _bank_dy(x, Ws, dys, halves):
    """the layers' output gradients side by side [B, total outputs]; an unused output (None) counts as zero"""
    cols = []
    for W, parts in zip(Ws, dys):
        C = W.shape[0] // halves
        cols += [p if p is not None else x.new_zeros(x.shape[0], C) for p in parts]
    return torch.cat(cols, 1)


def linear_bank_bwd(x, Ws, dys, halves):
    """dys: per layer a list of `halves` gradients [B, O_l / halves] or None -> dx [B, I], [dW_l], [db_l]"""
    dy = _bank_dy(x, Ws, dys, halves)
    first = [0]
    for W in Ws:
        first.append(first[-1] + W.shape[0])
    dWs = [dy[:, first[l]:first[l + 1]].t() @ x for l in range(len(Ws))]
    dbs = [dy[:, first[l]:first[l + 1]].sum(0) for l in range(len(Ws))]
    return dy @ torch.cat(list(Ws), 0), dWs, dbs


# ---- chain of square linear layers with leaky ReLU ------------------------------------------------------------------------------------
def mlp_chain_fwd(x, Ws, bs, slope):
    """-> [h_0 = x, h_1, .. h_L]"""
    acts = [x]
    for W, b in zip(Ws, bs):
        a = acts[-1] @ W.t() + b
        acts.append(torch.where(a > 0, a, a * slope))
    return acts


def mlp_chain_bwd(dout, acts, Ws, slope):
    """-> dx, [dW_l], [db_l]; the derivative where h == 0 (a pre-activation of exactly 0) is `slope`"""
    L = len(Ws)
    d = dout
    dWs, dbs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        h = acts[l + 1]
        d = d * torch.where(h > 0, torch.ones((), dtype=d.dtype), torch.full((), slope, dtype=d.dtype))
        dWs[l] = d.t() @ acts[l]
        dbs[l] = d.sum(0)
        d = d @ Ws[l]
    return d, dWs, dbs


# ---- grouped ("one expert per window") Conv1d --------------------------------------------------------------------------------------------
def runs_of(cls):
    """cls: the expert id of every window, ascending -> [(expert, first window, one past the last)]"""
    cls = [int(c) for c in cls]
    out, i0 = [], 0
    for i in range(1, len(cls) + 1):
        if i == len(cls) or cls[i] != cls[i0]:
            out.append((cls[i0], i0, i))
            i0 = i
    return out


def _padded(t, pad):
    """[n, R, C] -> [n, R + 2 pad, C], zero rows at both ends of every window"""
    if pad == 0:
        return t
    n, R, C = t.shape
    z = t.new_zeros(n, pad, C)
    return torch.cat([z, t, z], 1)


def grouped_conv_fwd(x, cls, Ws, bs, S):
    """x [n, R, Cin], Ws[e] [Cout, Cin, S], bs[e] [Cout] or bs None -> y [n, R, Cout]; padding S // 2 inside every window"""
    n, R, Cin = x.shape
    pad = S // 2
    xp = _padded(x, pad)
    ys = []
    for e, i0, i1 in runs_of(cls):
        W = Ws[e]
        y = sum(xp[i0:i1, s:s + R] @ W[:, :, s].t() for s in range(S))
        ys.append(y + bs[e] if bs is not None else y)
    return torch.cat(ys, 0)


def grouped_conv_dgrad(dy, cls, Ws, S):
    """-> dx [n, R, Cin]"""
    n, R, Cout = dy.shape
    pad = S // 2
    dp = _padded(dy, pad)
    return torch.cat([sum(dp[i0:i1, 2 * pad - s:2 * pad - s + R] @ Ws[e][:, :, s] for s in range(S)) for e, i0, i1 in runs_of(cls)], 0)


def grouped_conv_wgrad(dy, x, cls, S):
    """-> {expert: (dW [Cout, Cin, S], db [Cout])} for the experts that have windows"""
    n, R, Cin = x.shape
    pad = S // 2
    xp = _padded(x, pad)
    out = {}
    for e, i0, i1 in runs_of(cls):
        d = dy[i0:i1]
        dW = torch.stack([torch.einsum("nro,nri->oi", d, xp[i0:i1, s:s + R]) for s in range(S)], 2)
        out[e] = (dW, d.sum((0, 1)))
    return out


def segment_accumulate(rows, cls):
    """-> {expert: sum of its windows' rows}"""
    return {e: rows[i0:i1].sum(0) for e, i0, i1 in runs_of(cls)}


# ---- one expert, as the reference runs it for the windows of one class ------------------------------------------------------------------
EXPERT_KINDS = ("w1", "b1", "g1", "be1", "w2", "b2", "w3", "b3", "g2", "be2", "w4", "b4", "w5", "b5")


def char_extractor(p, x, groups1, groups2, eps=1e-5):
    """p: {kind: tensor} of one expert, x [m, R, C] the windows of its class -> [m, style_dim]; torch's own ops (differentiable)"""
    m, R, C = x.shape
    xc = x.transpose(1, 2)                                       # [m, C, R]
    h = F.conv1d(F.relu(xc), p["w1"], p["b1"], padding=1)
    h = F.relu(F.group_norm(h, groups1, p["g1"], p["be1"], eps))
    h = F.conv1d(h, p["w2"], p["b2"], padding=1)
    h = F.relu(h + xc)
    h = F.relu(F.group_norm(F.conv1d(h, p["w3"], p["b3"]), groups2, p["g2"], p["be2"], eps))
    h = h.mean(2)
    h = F.relu(F.linear(h, p["w4"].reshape(p["w4"].shape[0], -1), p["b4"]))
    return F.linear(h, p["w5"].reshape(p["w5"].shape[0], -1), p["b5"])


# ---- error bounds ------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24          # unit roundoff of float32


def sum_bound(K, abs_terms):
    """an fp32 sum of K products, in any order, with or without FMA (matrix cores included), rounded once more on the way out, is within
    (K + 2) U sum|terms| of the exact value; abs_terms: that sum, from the same restatement run on absolute values"""
    return (K + 2) * U * abs_terms


def chain_fwd_bound(acts, Ws, bs):
    """bound on the L2 norm of the error of every ROW of h_L of mlp_chain_fwd (float64 acts of the reference) -> [B], propagated layer by
    layer: the error e_l of a row of the input passes through W (at most its 2-norm times e_l; leaky ReLU is 1-Lipschitz), the layer's
    own sums of D products and a bias add at most (D + 3) U (|W| (|h_l| + e_l) + |b|) per element, the multiplication by the slope one
    more rounding. (Per element through |W| instead, the bound grows by the row sums of |W| per layer: 4.5^6 for the inputs used.)"""
    D = Ws[0].shape[0]
    e = acts[0].new_zeros(acts[0].shape[0])
    for l, (W, b) in enumerate(zip(Ws, bs)):
        local = (D + 3) * U * ((acts[l].abs() + e[:, None]) @ W.abs().t() + b.abs()) + U * acts[l + 1].abs()
        e = torch.linalg.matrix_norm(W, 2) * e + local.norm(dim=1)
    return e


def segment_mean_bound(v, wgt, seg, B):
    """float64 inputs -> (bound on out [B, C], bound on the relative error of wsum [B]) for a line of K members: total and wsum are sums of K
    terms, within (K + 2) U of the sums of their absolute terms; out = total / wsum takes the error of total divided by |wsum|, the
    relative error r of wsum as |out| r / (1 - r) <= 2 |out| r, and one rounding of the division; where wsum == 0, out = total"""
    seg = seg.long()
    K = torch.bincount(seg, minlength=B).double()
    tot = v.new_zeros(B, v.shape[1]).index_add_(0, seg, wgt[:, None] * v)
    atot = v.new_zeros(B, v.shape[1]).index_add_(0, seg, (wgt[:, None] * v).abs())
    ws = v.new_zeros(B).index_add_(0, seg, wgt)
    aws = v.new_zeros(B).index_add_(0, seg, wgt.abs())
    nz = ws != 0
    safe = torch.where(nz, ws, torch.ones_like(ws))
    ws_rel = torch.where(nz, (K + 2) * U * aws / safe.abs(), torch.zeros_like(ws))
    d_tot = ((K + 2) * U)[:, None] * atot
    out_b = torch.where(nz[:, None], d_tot / safe.abs()[:, None] + (tot / safe[:, None]).abs() * (2 * ws_rel + U)[:, None], d_tot)
    return out_b, ws_rel
