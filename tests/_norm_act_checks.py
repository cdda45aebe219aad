"""What the normalisation / activation tests share (not collected by pytest): the bounds per kernel family, the constants of the calls, the
gate hint of the fp64 backward and the norm inputs. tests/test_norm_act_fp64_gpu.py (through ops) and tests/test_norm_abi_fp64_gpu.py (at
the C ABI) hold the same kernels to the same BOUNDS; tests/test_abi_cases_cpu.py seeds its flaws against them."""
import torch

from oracle import norm_ref as R
from _fp64 import _gen


# (relative L2, max|err| / max|ref|) per family: 4x the worst case measured on an MI355X (in brackets), rounded down.
# An off-by-one count, a dropped chunk, the biased running variance or a lost pre-filled gradient move some case by 1e-3 or more.
BOUNDS = {
    "norm_fwd": (2.2e-7, 1.7e-6),         # [5.7e-8, 4.3e-7]  GN / BN / IN forward (tanh: tanhf's ulps)
    "norm_grad": (4.3e-7, 6.7e-7),        # [1.1e-7, 1.7e-7]  dx, dgamma, dbeta
    "norm_stats": (2.5e-7, 4.7e-7),       # [7.1e-8, 1.3e-7]  running_mean, running_var after two updates
    "offset16": (2.7e-6, 4.9e-6),         # [6.9e-7, 1.2e-6]  mean 16 sigma, forward and gradients (fp32 lane sums of x^2)
    "adain_fwd": (2.0e-7, 5.9e-7),        # [5.2e-8, 1.5e-7]
    "adain_grad": (6.0e-7, 1.0e-6),       # [1.5e-7, 2.6e-7]  dx, dgamma, dbeta, d(noise weight)
    "frozen": (2.3e-7, 1.0e-6),           # [5.9e-8, 2.7e-7]
    "bias_act_fwd": (1.4e-7, 2.7e-7),     # [3.7e-8, 6.8e-8]
    "bias_act_grad": (4.3e-7, 4.5e-7),    # [1.1e-7, 1.1e-7]  dx, dbias
    "tanh_fwd": (9.4e-8, 3.2e-7),         # [2.4e-8, 8.1e-8]
    "tanh_grad": (2.6e-7, 3.2e-7),        # [6.6e-8, 8.1e-8]
}
NEAR = 1e-6          # |z64| < NEAR * max|z64|: the gate comes from the kernel's forward output
MAX_FLIPS = 8        # gates where that differs from the sign of the fp64 pre-activation
EPS, MOMENTUM = 1e-5, 0.1


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _gate_hint(z, y_kernel, act):
    """(hint for R.act_ref, gates taken from the kernel, of those where the kernel's sign differs from fp64's) - relu / leaky relu only"""
    if act not in (R.ACT_RELU, R.ACT_LRELU):
        return None, 0, 0
    zd = z.detach()
    near = (zd.abs() < NEAR * float(zd.abs().max())) & (zd != 0)
    positive = y_kernel > 0
    return (near, positive), int(near.sum()), int((near & (positive != (zd > 0))).sum())


FEW_PIXELS = 16


def norm_inputs(c, per_sample=False):
    """x = 2 randn + 0.5, the inputs of tests/test_norm_act_fp64_gpu.py. With fewer than FEW_PIXELS pixels per channel an InstanceNorm
    statistic is formed from 3 or 5 values, and among 2048 such groups of 2 randn + 0.5 the smallest sample variance is 1e-3 of the group's
    mean square: there the kernels' variance E[x^2] - E[x]^2 from fp32 lane sums keeps four digits (measured at C 1024, HW 3: y 5e-5, dx 2e-3
    of the tensor's maximum - the arithmetic whose cost the "offset16" family of that file measures at mean = 16 sigma), and fp64 itself moves
    by 1e-6 when x moves by an ulp. That is the conditioning of the drawn problem, not the one-chunk regime these shapes are here for: below
    FEW_PIXELS every (n, c) row is standardised to a sample deviation s in [0.5, 2] and a mean of s / 4, whatever the mode pools."""
    N, HW, C = c["N"], c["HW"], c["C"]
    g = _gen(c["name"])
    t = dict(x=torch.randn(N, C, 1, HW, generator=g) * 2 + 0.5)
    if HW < FEW_PIXELS:
        z = t["x"].double()
        s = torch.rand(N, C, 1, 1, generator=g).double() * 1.5 + 0.5
        t["x"] = (((z - z.mean(3, keepdim=True)) / z.std(3, unbiased=False, keepdim=True) + 0.25) * s).float()
    ash = (N, C) if per_sample else (C,)
    t["gamma"] = torch.rand(ash, generator=g) + 0.5
    t["beta"] = torch.randn(ash, generator=g)
    t["mask"] = ((torch.rand(N, C, generator=g) > 0.3).float() / 0.7) if c["mask"] else None
    t["gy"] = torch.randn(N, C, 1, HW, generator=g)
    t["rm0"] = torch.randn(C, generator=g) * 0.3 + 0.2
    t["rv0"] = torch.rand(C, generator=g) + 0.5
    scale = (N * HW) ** 0.5
    t["dgamma0"] = torch.randn(ash, generator=g) * scale
    t["dbeta0"] = torch.randn(ash, generator=g) * scale
    return t
