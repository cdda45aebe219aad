"""Restatements of the forward-type convolution products of csrc/conv_mfma.hip, csrc/conv_direct.hip and csrc/conv_wino.hip (include/hwg.h:
hwg_conv_fwd, hwg_wino_conv_fwd, hwg_wino_s2_conv and their weight images) in plain torch on the CPU, no GPU and no torch convolution:
tap loops over shifted slices for the direct form, explicit tile transforms for the Winograd forms. Every function runs in the dtype of its
operands (fp64: the reference; fp32: the yardstick) and, with absolute=True, on absolute values with absolute transform matrices: the sum of
the absolute terms per output element, the scale of the per-element error bound.

Conventions: activations NHWC, x [N,H,W,C]; the LOGICAL weight of a product is w [R,S,K,C] (the engine image [R*S][K][C] unpadded), K the
channels of the output; geometry g = dict(stride=(sh,sw), pad=(ph,pw), dil=(dh,dw), P, Q, transposed) as in hwg_conv_desc.
(tests/test_conv_ref_cpu.py holds these against torch's own fp64 convolutions.)"""
import torch


def out_size(H, W, R, S, stride, pad, dil, transposed=0, opad=(0, 0)):
    """(P, Q) of hwg_conv_desc: convolution, or the fractionally strided product with opad rows / columns of slack"""
    if transposed:
        return ((H - 1) * stride[0] - 2 * pad[0] + R + opad[0], (W - 1) * stride[1] - 2 * pad[1] + S + opad[1])
    return ((H + 2 * pad[0] - dil[0] * (R - 1) - 1) // stride[0] + 1, (W + 2 * pad[1] - dil[1] * (S - 1) - 1) // stride[1] + 1)


def _finish(y, bias, y0, absolute):
    if bias is not None:
        y = y + (bias.abs() if absolute else bias).to(y.dtype)
    if y0 is not None:
        y = y + (y0.abs() if absolute else y0).to(y.dtype)
    return y


# ---- direct form --------------------------------------------------------------------------------------------------------------------------
def conv_direct(x, w, g, bias=None, y0=None, absolute=False, chunks=None):
    """y [N,P,Q,K] of hwg_conv_fwd. chunks: None, or a list of (channel-begin, channel-end) ranges summed one after the other as separate
    images (what a split contraction does) - the value is the same, the fp32 rounding differs"""
    if absolute:
        x, w = x.abs(), w.abs()
    N, H, W, C = x.shape
    R, S, K, _ = w.shape
    (sh, sw), (ph, pw), (dh, dw), P, Q = g["stride"], g["pad"], g["dil"], g["P"], g["Q"]
    y = None
    for c0, c1 in (chunks or [(0, C)]):
        xc, wc = x[..., c0:c1], w[..., c0:c1]
        if not g.get("transposed", 0):
            Hp, Wp = max(H + 2 * ph, (P - 1) * sh + dh * (R - 1) + 1), max(W + 2 * pw, (Q - 1) * sw + dw * (S - 1) + 1)
            xp = x.new_zeros((N, Hp, Wp, c1 - c0))
            xp[:, ph:ph + H, pw:pw + W] = xc
            part = x.new_zeros((N, P, Q, K))
            for r in range(R):
                for s in range(S):
                    part += xp[:, r * dh:r * dh + (P - 1) * sh + 1:sh, s * dw:s * dw + (Q - 1) * sw + 1:sw] @ wc[r, s].t()
        else:
            # out(p, q) += x(ih, iw) w(r, s) where ih * stride - pad + r == p; rows past the last contribution (the slack) stay zero
            full = x.new_zeros((N, (H - 1) * sh + R + sh + ph, (W - 1) * sw + S + sw + pw, K))
            for r in range(R):
                for s in range(S):
                    full[:, r:r + (H - 1) * sh + 1:sh, s:s + (W - 1) * sw + 1:sw] += xc @ wc[r, s].t()
            part = full[:, ph:ph + P, pw:pw + Q]
        y = part if y is None else y + part
    return _finish(y, bias, y0, absolute)


# ---- Winograd forms -----------------------------------------------------------------------------------------------------------------------
# F(2x2,3x3): points 0, 1, -1, inf
BT_23 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G_23 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
AT_23 = [[1, 1, 1, 0], [0, 1, -1, -1]]
# F(3x3,2x2): the same points, two taps, three outputs
BT_32 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]]
G_32 = [[1, 0], [.5, .5], [.5, -.5], [0, 1]]
AT_32 = [[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, 1]]


def _mat(rows, like, absolute):
    m = torch.tensor(rows, dtype=like.dtype)
    return m.abs() if absolute else m


def filter_transform(w, G, absolute=False):
    """U [4,4,K,C] = G g G^T of the taps w [R,S,K,C], the two 1-D stages one after the other (as csrc/wino_pack.h)"""
    Gm = _mat(G, w, absolute)
    t = torch.einsum("ir,rskc->iskc", Gm, w.abs() if absolute else w)
    return torch.einsum("js,iskc->ijkc", Gm, t)


def wino_stride1(x, w, pad, P, Q, m, BT, G, AT, absolute=False, chunks=None, U=None):
    """stride-1 convolution of x [N,H,W,C] with the taps w [r,r,K,C] (r = 5 - m) as F(m x m, r x r) on 4x4 patches: -> [N,P,Q,K] without bias.
    U: a transform-domain filter to use instead of G w G^T (the fp32 image a pack entry wrote). chunks: as conv_direct"""
    if absolute:
        x = x.abs()
    N, H, W, C = x.shape
    K = w.shape[2]
    TP, TQ = -(-P // m), -(-Q // m)
    xp = x.new_zeros((N, max(H + 2 * pad[0], m * TP + 4 - m), max(W + 2 * pad[1], m * TQ + 4 - m), C))
    xp[:, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = x
    d = xp.unfold(1, 4, m).unfold(2, 4, m)[:, :TP, :TQ]                 # [N,TP,TQ,C,4,4]
    Bm, Am = _mat(BT, x, absolute), _mat(AT, x, absolute)
    V = torch.einsum("ia,ntqcab->ntqcib", Bm, d)
    V = torch.einsum("jb,ntqcib->ntqcij", Bm, V)
    if U is None:
        U = filter_transform(w, G, absolute)
    elif absolute:
        U = U.abs()
    y = None
    for c0, c1 in (chunks or [(0, C)]):
        Mt = torch.einsum("ntqcij,ijkc->ntqkij", V[:, :, :, c0:c1], U[..., c0:c1].to(x.dtype))
        Y = torch.einsum("ai,ntqkij->ntqkaj", Am, Mt)
        Y = torch.einsum("bj,ntqkaj->ntqkab", Am, Y)                   # [N,TP,TQ,K,m,m]
        part = Y.permute(0, 1, 4, 2, 5, 3).reshape(N, TP * m, TQ * m, K)[:, :P, :Q]
        y = part if y is None else y + part
    return y


def wino_conv(x, w, g, bias=None, y0=None, absolute=False, chunks=None, U=None):
    """hwg_wino_conv_fwd: 3x3 stride 1 dilation 1 as F(2x2,3x3)"""
    return _finish(wino_stride1(x, w, g["pad"], g["P"], g["Q"], 2, BT_23, G_23, AT_23, absolute, chunks, U), bias, y0, absolute)


def space_to_depth(x, P, Q):
    """x' [N,P+1,Q+1,(a,b,c)] = x[2i+a, 2j+b, c]"""
    N, H, W, C = x.shape
    v = x[:, :2 * (P + 1), :2 * (Q + 1)].reshape(N, P + 1, 2, Q + 1, 2, C)
    return v.permute(0, 1, 3, 2, 4, 5).reshape(N, P + 1, Q + 1, 4 * C)


def s2_taps(w, dgrad):
    """the 2x2 taps of the two-tap product from the logical 4x4 weight w [4,4,K,C] of the descriptor: forward g2[u,v][k][(a,b,c)] =
    w[2u+a, 2v+b][k][c]; data gradient (descriptor transposed: K = the convolution's input channels, C = its output channels)
    g2[u,v][(a,b,k)][c] = w[2(1-u)+a, 2(1-v)+b][k][c]"""
    K, C = w.shape[2], w.shape[3]
    v = w.reshape(2, 2, 2, 2, K, C)                                    # [u, a, v, b, K, C]
    if not dgrad:
        return v.permute(0, 2, 4, 1, 3, 5).reshape(2, 2, K, 4 * C)
    return v.flip(0, 2).permute(0, 2, 1, 3, 4, 5).reshape(2, 2, 4 * K, C)


def wino_s2_conv(x, w, g, bias=None, y0=None, absolute=False, chunks=None):
    """hwg_wino_s2_conv: the 4x4 stride-2 pad-0 convolution (g transposed 0) as the two-tap convolution of the space-to-depth image, or its data
    gradient (g transposed 1: x = dy [N,H,W,C], output [N,2H+2,2W+2,K]) as the two-tap full correlation written depth-to-space, F(3x3,2x2)"""
    P, Q = g["P"], g["Q"]
    if not g.get("transposed", 0):
        y = wino_stride1(space_to_depth(x, P, Q), s2_taps(w, 0), (0, 0), P, Q, 3, BT_32, G_32, AT_32, absolute, chunks)
    else:
        N, H, W, C = x.shape
        K = w.shape[2]
        assert P == 2 * H + 2 and Q == 2 * W + 2
        yb = wino_stride1(x, s2_taps(w, 1), (1, 1), H + 1, W + 1, 3, BT_32, G_32, AT_32, absolute, chunks)       # [N,H+1,W+1,(a,b,k)]
        y = yb.reshape(N, H + 1, W + 1, 2, 2, K).permute(0, 1, 3, 2, 4, 5).reshape(N, P, Q, K)
    return _finish(y, bias, y0, absolute)


# ---- weight images ------------------------------------------------------------------------------------------------------------------------
def ceil16(n):
    return (n + 15) // 16 * 16


def gather_src(src, A, B, R, S, sa, sb, sr, ss, flip=0):
    """[A,B,R,S] from a flat source with element strides, flip mirrors the taps"""
    a, b = torch.arange(A).view(A, 1, 1, 1), torch.arange(B).view(1, B, 1, 1)
    r, s = torch.arange(R).view(1, 1, R, 1), torch.arange(S).view(1, 1, 1, S)
    if flip:
        r, s = R - 1 - r, S - 1 - s
    return src.reshape(-1)[a * sa + b * sb + r * sr + s * ss]


def pack_image(src, A, B, Bpad, R, S, sa, sb, sr, ss, flip):
    """hwg_conv_pack_weight: [R*S][A][Bpad], zeros past B"""
    out = src.new_zeros((R * S, A, Bpad))
    out[:, :, :B] = gather_src(src, A, B, R, S, sa, sb, sr, ss, flip).permute(2, 3, 0, 1).reshape(R * S, A, B)
    return out


def wino_layout(U, A, B):
    """U [4,4,A,B] -> the [ceil16(B)/16][16 positions][ceil16(A)][16] image, zeros in the padding"""
    Ap, Bp = ceil16(A), ceil16(B)
    full = U.new_zeros((16, Ap, Bp))
    full[:, :A, :B] = U.reshape(16, A, B)
    return full.reshape(16, Ap, Bp // 16, 16).permute(2, 0, 1, 3).contiguous()


def wino_image(src, A, B, sa, sb, sr, ss, flip, absolute=False):
    """hwg_wino_pack_weight"""
    w = gather_src(src, A, B, 3, 3, sa, sb, sr, ss, flip).permute(2, 3, 0, 1)
    return wino_layout(filter_transform(w, G_23, absolute), A, B)


def wino_s2_image(src, Kc, Cc, sk, sc, dgrad, absolute=False):
    """hwg_wino_s2_pack_weight from the convolution's weight (kc, cc, r, s) at src[kc*sk + cc*sc + r*4 + s]: the F(3x3,2x2) filter transform of
    the two-tap product's taps with the entries that have exactly one index equal to 3 negated (the kernel's input transform is F(2x2,3x3)'s)"""
    wc = gather_src(src, Kc, Cc, 4, 4, sk, sc, 4, 1, 0)                # [Kc,Cc,4,4]
    w = wc.permute(2, 3, 0, 1) if not dgrad else wc.permute(2, 3, 1, 0)   # the descriptor's logical weight [4,4,K,C]
    U = filter_transform(s2_taps(w, dgrad), G_32, absolute)
    if not absolute:
        sign = torch.ones(4, 4, dtype=U.dtype)
        sign[3, :3] = -1
        sign[:3, 3] = -1
        U = U * sign.view(4, 4, 1, 1)
    return wino_layout(U, U.shape[2], U.shape[3])


def unlayout(img, A, B):
    """the inverse of wino_layout: -> [4,4,A,B]"""
    Ap, Bp = ceil16(A), ceil16(B)
    return img.reshape(Bp // 16, 16, Ap, 16).permute(1, 2, 0, 3).reshape(16, Ap, Bp)[:, :A, :B].reshape(4, 4, A, B)


def sum_bound(terms, absval):
    """|err| <= terms * 2^-24 * (sum of absolute terms): a sum of rounded products / rounded partial sums, `terms` rounded operations deep"""
    return terms * 2.0 ** -24 * absval.double()


# ---- weight gradients (hwg_conv_wgrad, hwg_wino_wgrad, hwg_colsum; tests/test_wgrad_ref_cpu.py holds these against autograd) ----------------
# The operands are the C ABI's: u the ANCHOR tensor [N,P,Q,K], v the GATHERED one [N,H,W,C], g = dict(stride, pad, dil, R, S); the logical
# gradient is dw [R,S,K,C]. A convolution layer has u = dy, v = x; a transposed layer u = x, v = dy (just another descriptor).
def gathered(v, g, P, Q, r, s):
    """v[n, p*sh - ph + r*dh, q*sw - pw + s*dw, :] for every anchor pixel, zero outside the image: [N,P,Q,C]"""
    N, H, W, C = v.shape
    (sh, sw), (ph, pw), (dh, dw) = g["stride"], g["pad"], g["dil"]
    Hp = max(H + 2 * ph, (P - 1) * sh + dh * (g["R"] - 1) + 1)
    Wp = max(W + 2 * pw, (Q - 1) * sw + dw * (g["S"] - 1) + 1)
    vp = v.new_zeros((N, Hp, Wp, C))
    vp[:, ph:ph + H, pw:pw + W] = v
    return vp[:, r * dh:r * dh + (P - 1) * sh + 1:sh, s * dw:s * dw + (Q - 1) * sw + 1:sw]


def wgrad_direct(u, v, g, dw0=None, absolute=False, ranges=None):
    """dw[r,s,k,c] = sum_m u[m,k] v[gather(m,r,s),c] (+ dw0). ranges: None, or (begin, end) ranges of the anchor pixels m = (n,p,q), summed one
    after the other as separate images (what the pixel split does) - the value is the same, the fp32 rounding differs"""
    if absolute:
        u, v = u.abs(), v.abs()
    N, P, Q, K = u.shape
    C, R, S = v.shape[3], g["R"], g["S"]
    M = N * P * Q
    um = u.reshape(M, K)
    cols = [gathered(v, g, P, Q, r, s).reshape(M, C) for r in range(R) for s in range(S)]
    dw = None
    for m0, m1 in (ranges or [(0, M)]):
        part = torch.stack([um[m0:m1].t() @ col[m0:m1] for col in cols]).reshape(R, S, K, C)
        dw = part if dw is None else dw + part
    if dw0 is not None:
        dw = dw + (dw0.abs() if absolute else dw0).to(dw.dtype)
    return dw


def wgrad_terms(g, N, P, Q, H, W):
    """[R,S,1,1] (fp64): the anchor pixels whose tap (r,s) falls inside the image - the contraction length of dw[r,s]"""
    one = torch.ones(N, P, Q, 1, dtype=torch.float64)
    return wgrad_direct(one, torch.ones(N, H, W, 1, dtype=torch.float64), g)


def colsum(u, db0=None, absolute=False):
    """the column sums of u [..., K] (the fused bias gradient; hwg_colsum) (+ db0)"""
    if absolute:
        u = u.abs()
    out = u.reshape(-1, u.shape[-1]).sum(0)
    if db0 is not None:
        out = out + (db0.abs() if absolute else db0).to(out.dtype)
    return out


def _wino_wgrad_tiles(dy, xv, pad, m, BT, G, AT, absolute):
    """the stride-1 weight gradient of r x r taps (r = 5 - m) over m x m gradient tiles, as csrc/conv_wino_wgrad.hip: Z = A dY A^T (4x4 from
    the m x m tile of dy, A = AT^T), V = B^T d B (4x4 input patch), dU = sum over tiles Z . V, dg = G^T dU G: -> [r,r,K,Cv]"""
    if absolute:
        dy, xv = dy.abs(), xv.abs()
    N, P, Q, K = dy.shape
    H, W, C = xv.shape[1:]
    TP, TQ = -(-P // m), -(-Q // m)
    dyp = dy.new_zeros((N, TP * m, TQ * m, K))
    dyp[:, :P, :Q] = dy
    t = dyp.reshape(N, TP, m, TQ, m, K)                                  # [n, tp, a, tq, b, k]
    xp = xv.new_zeros((N, max(H + 2 * pad[0], m * TP + 4 - m), max(W + 2 * pad[1], m * TQ + 4 - m), C))
    xp[:, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = xv
    d = xp.unfold(1, 4, m).unfold(2, 4, m)[:, :TP, :TQ]                  # [n, tp, tq, c, 4, 4]
    Am, Bm, Gm = _mat(AT, dy, absolute).t(), _mat(BT, dy, absolute), _mat(G, dy, absolute)
    Z = torch.einsum("ia,ntaqbk->ntqkib", Am, t)
    Z = torch.einsum("jb,ntqkib->ntqkij", Am, Z)
    V = torch.einsum("ia,ntqcab->ntqcib", Bm, d)
    V = torch.einsum("jb,ntqcib->ntqcij", Bm, V)
    dU = torch.einsum("ntqkij,ntqcij->ijkc", Z, V)
    out = torch.einsum("ir,ijkc->rjkc", Gm, dU)
    return torch.einsum("js,rjkc->rskc", Gm, out)


def wino_wgrad(dy, x, g, dw0=None, absolute=False):
    """hwg_wino_wgrad: 3x3 stride 1 dilation 1 as F(3x3 taps, 2x2 gradient tiles); 4x4 stride 2 pad 0 as F(2x2 taps, 3x3 gradient tiles) on the
    virtual input [N,P+1,Q+1,4C] (space to depth), virtual channel (a,b,c) of tap (u,v) being tap (2u+a, 2v+b) of the 4x4 filter: -> [R,S,K,C]"""
    N, P, Q, K = dy.shape
    C = x.shape[3]
    if g["R"] == 3:
        dw = _wino_wgrad_tiles(dy, x, g["pad"], 2, BT_23, G_23, AT_23, absolute)
    else:
        assert g["R"] == 4 and g["stride"] == (2, 2) and g["pad"] == (0, 0)
        d2 = _wino_wgrad_tiles(dy, space_to_depth(x, P, Q), (0, 0), 3, BT_32, G_32, AT_32, absolute)      # [u, v, K, (a,b,c)]
        dw = d2.reshape(2, 2, K, 2, 2, C).permute(0, 3, 1, 4, 2, 5).reshape(4, 4, K, C)
    if dw0 is not None:
        dw = dw + (dw0.abs() if absolute else dw0).to(dw.dtype)
    return dw
