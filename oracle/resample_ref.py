"""Plain torch restatements of the memory-bound kernels of csrc/pool_resample.hip (pools, resampling, padding, channel copies, one-hot,
permute, the FusedUpsample weight, col2im_taps) and of the glue kernels at the end of csrc/spectral_loss.hip (axpby, mul, channel_affine,
weighted_sum, style_mix). Forward and backward passes are written out (no autograd), in the dtype of their arguments: fp64 for the
reference, fp32 for the yardstick, fp64 on absolute values for the bounds. Tensors are NHWC like the kernels'.

The kernels that promise a fixed order of explicitly rounded fp32 operations have a second restatement here (`*_f32`), numpy float32, one
rounded operation at a time in the kernel's order: the GPU result is held to torch.equal against those.

tests/test_resample_glue_ref_cpu.py checks all of this against torch (autograd for the adjoints) and seeds flaws into copies."""
import itertools

import numpy as np
import torch

U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def sum_bound(K, abs_terms):
    """an fp32 sum of K terms (one more per scaling), in any order, contracted or not, is within (K + 2) U sum|terms| of the exact value"""
    return (K + 2) * U * abs_terms


# ---- average pooling (kernel == stride, floor) -----------------------------------------------------------------------------------------------
def avgpool_fwd(x, kh, kw):
    N, H, W, C = x.shape
    P, Q = H // kh, W // kw
    return x[:, :P * kh, :Q * kw].reshape(N, P, kh, Q, kw, C).sum((2, 4)) * (1.0 / (kh * kw))


def avgpool_bwd(dy, H, W, kh, kw):
    """remainder rows / columns get exactly zero"""
    N, P, Q, C = dy.shape
    dx = torch.zeros(N, H, W, C, dtype=dy.dtype)
    dx[:, :P * kh, :Q * kw] = dy.repeat_interleave(kh, 1).repeat_interleave(kw, 2) * (1.0 / (kh * kw))
    return dx


def _act(z, act, slope):
    if act == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == ACT_LRELU:
        return torch.where(z > 0, z, z * slope)
    return z


def act_avgpool_fwd(x, mask, act, slope, kh, kw):
    z = x if mask is None else x * mask[:, None, None, :]
    return avgpool_fwd(_act(z, act, slope), kh, kw)


def act_avgpool_bwd(dy, x, mask, act, slope, kh, kw):
    N, H, W, C = x.shape
    z = x if mask is None else x * mask[:, None, None, :]
    g = avgpool_bwd(dy, H, W, kh, kw)
    if act == ACT_RELU:
        g = torch.where(z > 0, g, torch.zeros_like(g))
    if act == ACT_LRELU:
        g = torch.where(z > 0, g, g * slope)
    return g if mask is None else g * mask[:, None, None, :]


def _act_f32(z, act, slope):
    if act == ACT_RELU:
        return np.where(z > 0, z, np.float32(0))
    if act == ACT_LRELU:
        return np.where(z > 0, z, z * np.float32(slope))
    return z


def act_avgpool_fwd_f32(x, mask, act, slope, kh, kw):
    """the kernel's order: window taps row major, mask product, activation, add - each rounded to fp32 -, then one product with 1 / (kh kw)"""
    x = x.numpy()
    N, H, W, C = x.shape
    P, Q = H // kh, W // kw
    k = None if mask is None else mask.numpy()[:, None, None, :]
    acc = np.zeros((N, P, Q, C), np.float32)
    for a in range(kh):
        for b in range(kw):
            v = x[:, a:P * kh:kh, b:Q * kw:kw]
            acc = acc + _act_f32(v if k is None else v * k, act, slope)
    return torch.from_numpy(acc * (np.float32(1) / np.float32(kh * kw)))


def act_avgpool_bwd_f32(dy, x, mask, act, slope, kh, kw):
    dy, x = dy.numpy(), x.numpy()
    N, H, W, C = x.shape
    P, Q = H // kh, W // kw
    k = None if mask is None else mask.numpy()[:, None, None, :]
    z = (x if k is None else x * k)[:, :P * kh, :Q * kw]
    g = np.repeat(np.repeat(dy, kh, 1), kw, 2) * (np.float32(1) / np.float32(kh * kw))
    if act == ACT_RELU:
        g = np.where(z > 0, g, g * np.float32(0))
    if act == ACT_LRELU:
        g = np.where(z > 0, g, g * np.float32(slope))
    if k is not None:
        g = g * k
    dx = np.zeros((N, H, W, C), np.float32)
    dx[:, :P * kh, :Q * kw] = g
    return torch.from_numpy(dx)


# ---- max pooling ---------------------------------------------------------------------------------------------------------------------------
def pool_out(H, k, s, p):
    return (H + 2 * p - k) // s + 1


def maxpool_fwd(x, kernel, stride, pad, relu=False):
    """-> y [N,P,Q,C], idx int32 [N,P,Q,C] = h * W + w of the FIRST maximum of the window (taps row major); a NaN wins and stays (ATen's
    rule). relu: y = max(y, 0) with a NaN folded to 0, as hwg_bias_act_fwd's ReLU does."""
    N, H, W, C = x.shape
    (kh, kw), (sh, sw), (ph, pw) = kernel, stride, pad
    P, Q = pool_out(H, kh, sh, ph), pool_out(W, kw, sw, pw)
    best = torch.full((N, P, Q, C), float("-inf"), dtype=x.dtype)
    idx = torch.full((N, P, Q, C), -1, dtype=torch.int64)
    for a in range(kh):
        h = torch.arange(P) * sh - ph + a
        for b in range(kw):
            w = torch.arange(Q) * sw - pw + b
            ok = ((h >= 0) & (h < H))[:, None] & ((w >= 0) & (w < W))[None, :]
            v = x[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)]
            take = ok[None, :, :, None] & ((v > best) | torch.isnan(v) | (idx < 0))
            best = torch.where(take, v, best)
            here = (h[:, None] * W + w[None, :])[None, :, :, None].expand_as(idx)
            idx = torch.where(take, here, idx)
    if relu:
        best = torch.where(best > 0, best, torch.zeros_like(best))
    return best, idx.to(torch.int32)


def maxpool_bwd(dy, idx, H, W, y=None):
    """dx[n, idx] += dy; y given: the ReLU variant, gated by y > 0"""
    N, P, Q, C = dy.shape
    g = dy if y is None else dy * (y > 0).to(dy.dtype)
    dx = torch.zeros(N, H * W, C, dtype=dy.dtype)
    dx.scatter_add_(1, idx.reshape(N, P * Q, C).long(), g.reshape(N, P * Q, C))
    return dx.reshape(N, H, W, C)


# ---- nearest upsample, blur, pad -----------------------------------------------------------------------------------------------------------
def upsample_fwd(x, fh, fw):
    return x.repeat_interleave(fh, 1).repeat_interleave(fw, 2)


def upsample_bwd(dy, fh, fw):
    N, P, Q, C = dy.shape
    return dy.reshape(N, P // fh, fh, Q // fw, fw, C).sum((2, 4))


def blur3(x):
    """[[1,2,1],[2,4,2],[1,2,1]] / 16 with zero padding; its own adjoint"""
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    y = torch.zeros_like(x)
    for a in range(3):
        for b in range(3):
            k = (2.0 if a == 1 else 1.0) * (2.0 if b == 1 else 1.0) / 16.0
            y = y + k * xp[:, a:a + H, b:b + W]
    return y


def _pad_index(H, pt, pb, replicate):
    h = torch.arange(H + pt + pb) - pt
    return (h.clamp(0, H - 1), None) if replicate else (h.clamp(0, H - 1), (h >= 0) & (h < H))


def pad2d_fwd(x, pt, pb, pl, pr, mode, value=0.0):
    """mode 0: constant (negative pads crop), mode 1: replicate"""
    N, H, W, C = x.shape
    h, okh = _pad_index(H, pt, pb, mode == 1)
    w, okw = _pad_index(W, pl, pr, mode == 1)
    y = x[:, h][:, :, w]
    if mode == 0:
        ok = (okh[:, None] & okw[None, :])[None, :, :, None]
        y = torch.where(ok, y, torch.full_like(y, value))
    return y


def pad2d_bwd(dy, H, W, pt, pb, pl, pr, mode):
    N, P, Q, C = dy.shape
    h, okh = _pad_index(H, pt, pb, mode == 1)
    w, okw = _pad_index(W, pl, pr, mode == 1)
    if mode == 0:
        dy = dy * (okh[:, None] & okw[None, :])[None, :, :, None].to(dy.dtype)
    t = torch.zeros(N, H, Q, C, dtype=dy.dtype).index_add_(1, h, dy)
    return torch.zeros(N, H, W, C, dtype=dy.dtype).index_add_(2, w, t)


# ---- channel copies --------------------------------------------------------------------------------------------------------------------------
def copy_channels(src, soff, dst, doff, Cn, HW=1, bcast=0, accumulate=0):
    """dst[row][doff + c] (+)= src[bcast ? row // HW : row][soff + c], c < Cn; src [rows_s, Cs], dst [rows, Cd]; -> the new dst"""
    out = dst.clone()
    rows = dst.shape[0]
    srow = torch.arange(rows) // HW if bcast else torch.arange(rows)
    v = src[srow, soff:soff + Cn]
    out[:, doff:doff + Cn] = out[:, doff:doff + Cn] + v if accumulate else v
    return out


def pad_channels(src, Cpad):
    rows, C = src.shape
    out = torch.zeros(rows, Cpad, dtype=src.dtype)
    out[:, :C] = src
    return out


def reduce_rows(src, soff, Cn, N, HW, out=None):
    """out[n][c] (+)= sum_hw src[n * HW + hw][soff + c]"""
    s = src.reshape(N, HW, -1)[:, :, soff:soff + Cn].sum(1)
    return s if out is None else out + s


def onehot(label, ncls, Cd=None, doff=0, out=None):
    """label int [L, B] (time major) -> [B, L, Cd] with the one-hot rows in channels doff .. doff + ncls (the rest of `out` kept); a label
    outside [0, ncls) gives a zero row"""
    Lr, B = label.shape
    Cd = Cd or ncls
    res = torch.zeros(B, Lr, Cd, dtype=torch.float64) if out is None else out.clone()
    res[:, :, doff:doff + ncls] = (label.t().long()[:, :, None] == torch.arange(ncls)[None, None, :]).to(res.dtype)
    return res


def onehot_both(label, ncls):
    blc = onehot(label, ncls)
    return blc, blc.transpose(0, 1).contiguous()


def permute4(x, dims, strides):
    return torch.as_strided(x.reshape(-1), tuple(dims), tuple(strides)).contiguous()


# ---- FusedUpsample weight: w4 = mean of the four 1-shifted copies of pad(w3 * mult, 1) -----------------------------------------------------
def fused_weight_fwd(w3, mult):
    AB = w3.shape[:-2]
    wp = torch.zeros(*AB, 5, 5, dtype=w3.dtype)
    wp[..., 1:4, 1:4] = w3 * mult
    acc = torch.zeros(*AB, 4, 4, dtype=w3.dtype)
    for dr in range(2):
        for ds in range(2):
            acc = acc + wp[..., dr:dr + 4, ds:ds + 4]
    return acc / 4


def fused_weight_bwd(dw4, mult, prev=None):
    acc = torch.zeros(*dw4.shape[:-2], 3, 3, dtype=dw4.dtype)
    for dr in range(2):
        for ds in range(2):
            acc = acc + dw4[..., 1 - dr:4 - dr, 1 - ds:4 - ds]
    v = acc * mult / 4
    return v if prev is None else prev + v


def fused_weight_bwd_f32(dw4, mult, prev=None):
    """the kernel's order: the four taps added (dr, ds) row major, one product with mult, one division by 4, one rounded add to what was there"""
    d = dw4.numpy()
    acc = np.zeros(d.shape[:-2] + (3, 3), np.float32)
    for dr in range(2):
        for ds in range(2):
            acc = acc + d[..., 1 - dr:4 - dr, 1 - ds:4 - ds]
    v = acc * np.float32(mult) / np.float32(4)
    return torch.from_numpy(v if prev is None else prev.numpy() + v)


# ---- col2im over the tap matrix ----------------------------------------------------------------------------------------------------------
def col2im_taps(t, H, W, R, S, ph, pw, dh=1, dw=1):
    """dx[n,ih,iw] = sum_{r,s} t[n, ih+ph-r*dh, iw+pw-s*dw, r*S+s]; t [N,P,Q,R*S] -> dx [N,H,W]"""
    N, P, Q, RS = t.shape
    dx = torch.zeros(N, H, W, dtype=t.dtype)
    ih, iw = torch.arange(H), torch.arange(W)
    for r in range(R):
        p = ih + ph - r * dh
        for s in range(S):
            q = iw + pw - s * dw
            ok = ((p >= 0) & (p < P))[:, None] & ((q >= 0) & (q < Q))[None, :]
            v = t[:, p.clamp(0, P - 1)][:, :, q.clamp(0, Q - 1)][..., r * S + s]
            dx = dx + v * ok[None].to(t.dtype)
    return dx


# ---- glue ------------------------------------------------------------------------------------------------------------------------------------
def axpby(x, a, y=None, b=0.0):
    return a * x if y is None else a * x + b * y


def channel_affine(x, scale=None, shift=None):
    y = x if scale is None else x * scale
    return y if shift is None else y + shift


def weighted_sum(xs, ws):
    """-> (left-to-right sum of the scaled terms, the scaled terms); a weight of exactly 1 multiplies nothing"""
    scaled = [x if w == 1.0 else x * w for x, w in zip(xs, ws)]
    acc = scaled[0]
    for v in scaled[1:]:
        acc = acc + v
    return acc, torch.stack(scaled)


def weighted_sum_f32(xs, ws):
    f = np.float32
    scaled = [f(x) if f(w) == f(1) else f(x) * f(w) for x, w in zip(xs, ws)]
    acc = scaled[0]
    for v in scaled[1:]:
        acc = f(acc + v)
    return torch.tensor(float(acc), dtype=torch.float32), torch.from_numpy(np.array(scaled, np.float32))


def weighted_sum_bwd(g, ws):
    return torch.stack([g if w == 1.0 else g * w for w in ws])


def weighted_sum_bwd_f32(g, ws):
    f = np.float32
    return torch.from_numpy(np.array([f(g) if f(w) == f(1) else f(g) * f(w) for w in ws], np.float32))


def style_mix(bank, ij, w):
    """out[b] = bank[ij[0][b]] * w[0][b] + bank[ij[1][b]] * w[1][b]"""
    return bank[ij[0].long()] * w[0][:, None] + bank[ij[1].long()] * w[1][:, None]


def style_mix_f32(bank, ij, w):
    bk, wn = bank.numpy(), w.numpy()
    a = bk[ij[0].numpy()] * wn[0][:, None]
    b = bk[ij[1].numpy()] * wn[1][:, None]
    return torch.from_numpy(a + b)


def all_perms4():
    return list(itertools.permutations(range(4)))
