"""fp64 restatements of the sequence, loss and spectral-norm family (csrc/seq_ops.hip, csrc/spectral_loss.hip), for the tests that hold the
HIP kernels against them. Plain CPU torch on float64 tensors, gradients by autograd, written from the operations' definitions:

  log_softmax_tbc:  [B, 1, T, C] logits -> [T, B, C] log-probabilities
  ctc:              mean_b( nll_b / max(tg_len_b, 1) ), nll_b = -log( alpha[in_len_b - 1][2 S_b] + alpha[in_len_b - 1][2 S_b - 1] ) of the
                    blank-interleaved target (blank = 0), alpha by the forward recursion in log space. This project's contract for an
                    infinite mean (some item has no alignment): the loss is 0 and every gradient is exactly 0 (the reference model/loss.py
                    back-propagates through a torch.where there and gets NaN; csrc/seq_ops.hip documents zeros).
  ctc_grad_on_simplex:  the kernels report d loss / d log-probs as ATen's ctc_loss does - the gradient g projected through the log-softmax
                    the log-probs came from, g - exp(lp) * sum_c g - not the free gradient g itself. Both give the same d loss / d logits.
  loss:             scale * mean(term): 0 |a - b|, 1 (a - b)^2, 2 a, 3 relu(1 - a), 4 relu(1 + a); the derivative at a tie is 0
  spectral:         one power iteration v' = W^T u / (|W^T u| + eps), u' = W v' / (|W v'| + eps), sigma = u' . (W v'), W / sigma;
                    sigma is a function of W with u', v' held constant
  pixel_norm:       x / sqrt(mean_c(x^2) + eps) over the rows of [rows, C]
  argmax_first:     the smallest index holding the row maximum"""
import torch

NEG = float("-inf")


def log_softmax_tbc(x):
    z = x[:, 0]                                                    # [B, T, C]
    m = z.detach().max(dim=2, keepdim=True).values
    lse = m + torch.log(torch.exp(z - m).sum(dim=2, keepdim=True))
    return (z - lse).permute(1, 0, 2)


def log_softmax_rows(x):
    """the same without the transpose (transpose_bt = 0 of hwg_log_softmax_fwd / _bwd): [B, 1, T, C] logits -> [B * T, C] log-probabilities,
    rows in the input's own (b, t) order"""
    return log_softmax_tbc(x).permute(1, 0, 2).reshape(-1, x.shape[-1])


def _lse_rows(rows):
    """log(sum(exp(rows), dim 0)) of [k, n]; a column of -inf gives -inf and passes no gradient (no 0 * inf anywhere)"""
    m = rows.detach().max(dim=0).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    s = torch.exp(rows - m).sum(dim=0)
    live = s > 0
    return torch.where(live, torch.log(torch.where(live, s, torch.ones_like(s))) + m, torch.full_like(s, NEG))


def ctc_nll(lp, targets, in_len, tg_len):
    """lp [T, B, C] log-probs, targets [B, Lmax] ints, lengths [B] -> nll [B] (inf where an item has no alignment)"""
    T, B, C = lp.shape
    out = []
    for b in range(B):
        S, Tb = int(tg_len[b]), int(in_len[b])
        assert 1 <= Tb <= T and 0 <= S <= targets.shape[1]
        ext = torch.zeros(2 * S + 1, dtype=torch.long)
        ext[1::2] = targets[b, :S].long()
        skip = torch.zeros(2 * S + 1, dtype=torch.bool)            # s - 2 -> s: only between two different characters
        skip[2:] = ext[2:] != ext[:-2]
        minus = lp.new_full((2,), NEG)
        alpha = lp.new_full((2 * S + 1,), NEG)
        alpha = torch.cat((lp[0, b, ext[:2]], alpha[2:]))          # states 0 (blank) and 1 (first character) at t = 0
        for t in range(1, Tb):
            a1 = torch.cat((minus[:1], alpha[:-1]))
            a2 = torch.where(skip, torch.cat((minus, alpha[:-2]))[: 2 * S + 1], minus[:1])
            alpha = _lse_rows(torch.stack((alpha, a1, a2))) + lp[t, b, ext]
        out.append(-_lse_rows(alpha[-2:].reshape(-1, 1))[0])
    return torch.stack(out)


def ctc(lp, targets, in_len, tg_len):
    """-> (loss, nll [B] detached); the loss of an infinite mean is an exact 0 whose gradient is an exact 0"""
    nll = ctc_nll(lp, targets, in_len, tg_len)
    div = torch.as_tensor(tg_len).clamp(min=1).to(nll.dtype)
    mean = (nll / div).sum() / nll.shape[0]
    if bool(torch.isinf(mean)):
        mean = (lp * 0.0).sum()
    return mean, nll.detach()


def ctc_grad_on_simplex(lp, grad):
    """the free gradient `grad` of a function of lp [T, B, C] as the kernels (and ATen) report it: g - exp(lp) * sum_c g"""
    return grad - torch.exp(lp.detach()) * grad.sum(dim=2, keepdim=True)


def loss(a, b, mode, scale):
    zero = torch.zeros((), dtype=a.dtype)
    if mode == 0:
        term = (a - b).abs()
    elif mode == 1:
        term = (a - b) ** 2
    elif mode == 2:
        term = a
    elif mode == 3:
        term = torch.where(1 - a > 0, 1 - a, zero)
    else:
        term = torch.where(1 + a > 0, 1 + a, zero)
    return scale * (term.sum() / term.numel())


def loss_accumulate(out0, a, b, mode, scale):
    """accumulate = 1 of hwg_loss_fwd: out0 + scale * mean(term). Backward with accumulate = 1 likewise adds to what da / db hold:
    da0 + d loss / d a and db0 + d loss / d b (the latter is db0 - d loss / d a for the pair losses)."""
    return out0 + loss(a, b, mode, scale)


def spectral(w_bar, u, v, eps):
    """-> (u', v', sigma, w_bar / sigma); u, v are not modified: pass u', v' to the next call (v itself is not read, as in the kernels)"""
    W = w_bar.reshape(w_bar.shape[0], -1)
    Wc = W.detach()
    t = Wc.t() @ u
    v1 = t / (t.norm() + eps)
    s = Wc @ v1
    u1 = s / (s.norm() + eps)
    sigma = u1 @ (W @ v1)
    return u1, v1, sigma, w_bar / sigma


def pixel_norm(x, eps):
    return x / torch.sqrt((x * x).mean(dim=1, keepdim=True) + eps)


def argmax_first(x):
    rows, C = x.shape
    top = x.max(dim=1, keepdim=True).values
    idx = torch.arange(C).expand(rows, C)
    return torch.where(x == top, idx, torch.full_like(idx, C)).min(dim=1).values
