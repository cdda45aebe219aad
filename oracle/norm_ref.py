"""fp64 restatements of the normalisation / activation family (csrc/norm_act.hip, tanh in csrc/spectral_loss.hip), for the tests that hold the
HIP kernels against them. Plain CPU autograd on NCHW float64 tensors, written from the operations' definitions:

  GroupNorm / BatchNorm (train) / InstanceNorm:  y = act(mask[n, c] * (gamma[c] * (x - mean) / sqrt(var + eps) + beta[c]))
      with the biased variance over the statistic group (GN: C/groups channels x H x W of one sample, BN: N x H x W of one channel,
      IN: H x W of one sample and channel), the Dropout2d channel mask applied after the affine and before the activation
  BatchNorm running statistics:  r <- (1 - momentum) r + momentum s, with the unbiased variance (count / (count - 1))
  frozen BatchNorm:  y = act(gamma * (x - running_mean) / sqrt(running_var + eps) + beta)
  generator epilogue (AdaIN):  y = gamma[n, c] * IN(lrelu(x + nw[c] * scale * noise)) + beta[n, c]
  bias_act:  y = act(mask[n, c] * (x + bias[c]))

Activations: 0 none, 1 relu, 2 leaky relu (slope), 3 tanh. relu / leaky relu are `z * gate` with the gate held constant, gate = 1 for z > 0 and
0 / slope otherwise - torch's own convention at z = 0 (relu'(0) = 0, lrelu'(0) = slope). `hint` = (where, positive): at the elements of `where`
the gate is taken from `positive` instead of the sign of the fp64 z (an fp32 kernel may fall on the other side of 0 where z is within its
rounding of 0; the tests pass the kernel's own forward output there)."""
import torch

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3


def act_ref(z, act, slope=0.0, hint=None):
    if act == ACT_NONE:
        return z
    if act == ACT_TANH:
        return torch.tanh(z)
    neg = slope if act == ACT_LRELU else 0.0
    pos = z.detach() > 0
    if hint is not None:
        where, positive = hint
        pos = torch.where(where, positive, pos)
    gate = torch.where(pos, torch.ones((), dtype=z.dtype), torch.full((), neg, dtype=z.dtype))
    return z * gate


def _cv(v):
    """a per-channel vector [C] as [1, C, 1, 1], a per-sample one [N, C] as [N, C, 1, 1]"""
    return v.reshape(1, -1, 1, 1) if v.dim() == 1 else v.reshape(v.shape[0], v.shape[1], 1, 1)


def moments(x, mode, groups=1):
    """(mean, biased variance) of x [N, C, H, W], broadcastable to x; mode "in" / "gn" / "bn" """
    N, C, H, W = x.shape
    if mode == "bn":
        m = x.mean((0, 2, 3), keepdim=True)
        return m, ((x - m) ** 2).mean((0, 2, 3), keepdim=True)
    if mode == "in":
        m = x.mean((2, 3), keepdim=True)
        return m, ((x - m) ** 2).mean((2, 3), keepdim=True)
    xg = x.reshape(N, groups, -1)
    m = xg.mean(2, keepdim=True)
    v = ((xg - m) ** 2).mean(2, keepdim=True)
    rep = lambda t: t.expand(N, groups, C // groups).reshape(N, C, 1, 1)     # noqa: E731
    return rep(m), rep(v)


def norm_pre(x, mode, groups=1, gamma=None, beta=None, mask=None, eps=1e-5):
    """the pre-activation z = mask * (gamma * xhat + beta) of a training-mode normalisation"""
    m, v = moments(x, mode, groups)
    z = (x - m) / torch.sqrt(v + eps)
    if gamma is not None:
        z = z * _cv(gamma)
    if beta is not None:
        z = z + _cv(beta)
    if mask is not None:
        z = z * _cv(mask)
    return z


def norm(x, mode, groups=1, gamma=None, beta=None, mask=None, act=ACT_NONE, slope=0.0, eps=1e-5, hint=None):
    return act_ref(norm_pre(x, mode, groups, gamma, beta, mask, eps), act, slope, hint)


def norm_per_sample(x, mode, groups, gamma, beta, mask=None, act=ACT_NONE, slope=0.0, eps=1e-5, hint=None):
    """InstanceNorm / GroupNorm with one affine per sample (affine_per_sample = 1 of hwg_norm_fwd / hwg_norm_bwd): gamma, beta [N, C],
    y[n] = act(mask[n, c] * (gamma[n, c] * xhat[n] + beta[n, c])); autograd leaves d gamma, d beta as [N, C] - no sum over the samples.
    Batch statistics with a per-sample affine are not defined (the entries refuse them)."""
    assert mode in ("in", "gn") and gamma.shape == beta.shape == (x.shape[0], x.shape[1]), (mode, tuple(gamma.shape))
    return norm(x, mode, groups, gamma, beta, mask, act, slope, eps, hint)


def running_stats(x, running_mean, running_var, momentum):
    """BatchNorm's running statistics after one training-mode call on x [N, C, H, W] (new tensors)"""
    cnt = x.shape[0] * x.shape[2] * x.shape[3]
    m = x.mean((0, 2, 3))
    v = ((x - m.reshape(1, -1, 1, 1)) ** 2).sum((0, 2, 3)) / (cnt - 1 if cnt > 1 else 1)
    return (1 - momentum) * running_mean + momentum * m, (1 - momentum) * running_var + momentum * v


def frozen_norm(x, running_mean, running_var, gamma=None, beta=None, act=ACT_NONE, slope=0.0, eps=1e-5):
    z = (x - _cv(running_mean)) / torch.sqrt(_cv(running_var) + eps)
    if gamma is not None:
        z = z * _cv(gamma)
    if beta is not None:
        z = z + _cv(beta)
    return act_ref(z, act, slope)


def adain_pre(x, noise, noise_w, scale):
    """t = x + nw * scale * noise, the input of the epilogue's leaky relu (noise_w [C] or [1, C, 1, 1])"""
    return x + (noise_w.reshape(1, -1, 1, 1) * scale) * noise


def adain(x, noise, noise_w, gamma, beta, scale, slope=0.2, eps=1e-5, hint=None):
    u = act_ref(adain_pre(x, noise, noise_w, scale), ACT_LRELU, slope, hint)
    return norm_pre(u, "in", 1, gamma, beta, None, eps)


def bias_act(x, bias=None, mask=None, act=ACT_NONE, slope=0.0, hint=None):
    z = x if bias is None else x + _cv(bias)
    if mask is not None:
        z = z * _cv(mask)
    return act_ref(z, act, slope, hint)


def to_nchw(t):
    """an NHWC kernel tensor [N, H, W, C] ([N, W, C] for 1-D layers) as NCHW float64 on the CPU"""
    t = t.detach().cpu().double()
    if t.dim() == 3:
        t = t.unsqueeze(1)
    return t.permute(0, 3, 1, 2).contiguous()
