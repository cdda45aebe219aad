"""The bounds of the optimizer-tail and Philox kernels' fp64 tests (not collected by pytest): what the number formats allow (DERIVED,
RANDN_*), the per-element bounds of one Adam step and the distance its fp32 betas put between the kernel and fp64. tests/test_optim_rng_fp64_gpu.py
holds the device to them, tests/test_optim_rng_ref_cpu.py seeds its flaws against them."""
import math

import torch

from _fp64 import _f32

ULP = 2.0 ** -23          # spacing of fp32 at 1
E = 2.0 ** -24            # one fp32 rounding, relative
SLACK = 1.01              # second-order terms of the first-order error sums below
DERIVED = {
    # per tensor: the 16-byte path adds |a| + |b| in fp32 (one rounding per pair, relative to the pair: terms are non-negative, so relative
    # to the sum) and accumulates in double; the scalar path is exact in double. n * 2^-53 of double accumulation: 2e5 * 1.1e-16 < 1e-10
    "abs_sum_rel": E + 1e-10,
    # dst + c * src as one fused multiply-add (0.5 ulp of the result) or as a rounded product and a rounded sum: at most
    # ulp * (|result| + |c * src|) per element, as stated by the definition of the kernel
    "axpy_ulps": 1.0,
    # coef = x * (d / r): d and r are each an fp64-exact mean rounded to fp32, then one division and one product: four roundings; where the
    # mean was replaced, d is (float)sum / (float)count of fp32 means added in double: three more. 7 * 2^-24 < 4 ulp
    "coef_rel": 4 * ULP,
    # 1.f / (1.f - p): the difference is rounded (exact for p >= 0.5), then the quotient
    "drop_keep_ulps": 1.0,
}
# |error| of hwg_randn against the fp64 Box-Muller of the same fp32 uniforms: 4 x the worst absolute error measured on an MI355X over every
# (seed, offset, n) of the table (in brackets). The error is fp32 logf / sqrtf / sincosf with the argument 2 pi u rounded to fp32.
RANDN_ABS = None          # [UNMEASURED]
# Until it is measured the test holds hwg_randn to what the number formats allow, derived: z = r cos(a) with r = sqrt(-2 ln u) <= 5.89
# (u >= 2^-25). The angle fl(fl(2 pi) u) is off by at most 2 pi (2.8e-8 + 2^-24) = 5.5e-7 (the fp32 constant, the product's rounding), sincosf
# adds 2 ulp of 1 (2.4e-7); logf's 1 ulp halves under the root and the root and the final product round once each: 1.5 * 2^-23 relative.
RANDN_DERIVED = 5.89 * (2 * math.pi * (2.8e-8 + E) + 2 * ULP + 1.5 * ULP)          # 5.7e-6


def adam_bounds(p0, g, m0, v0, ss, bc2, b1, b2, eps, ref):
    """per-element bounds (float64 tensors) on |m|, |v|, |p| errors of one kernel step against R.adam_step's `ref` = (p, g, m, v); g is the
    gradient the moments see (clamped). Every operation is one fp32 rounding (E, relative to its result); division and square root are
    budgeted two (the compiler may pick a 1-ulp expansion).
      m = m0 + (g - m0) c1:   the difference (E |g - m0| c1), the product (E |g - m0| c1, absent when fused) and the sum (E |m|)
      v = v0 b2 + (c2 g) g:   all terms non-negative: two roundings on the second term, one on the first, one on the sum, each relative to v
                              at most: 3 E v (the fourth is absorbed when either product is fused; 3.5 keeps it)
      u = ss (m / (sqrt(v) / bc2 + eps)):   v's 3.5 E halves under the root (1.75), root 2, quotient 2, sum with eps 1, m / denom 2, the
                              product with ss 1: 9.75 E |u|, plus m's own error carried through ss / denom
      p = p0 - u:             E |p|"""
    pr, _, mr, vr = ref
    c1 = 1.0 - b1
    bm = SLACK * E * (2 * ((g - m0) * c1).abs() + mr.abs())
    bv = SLACK * 3.5 * E * vr
    denom = vr.sqrt() / bc2 + eps
    u = ss * mr / denom
    bp = SLACK * (E * pr.abs() + 9.75 * E * u.abs() + ss * bm / denom)
    return bm, bv, bp


def fp32_beta_distance(g, m0, v0, ss, bc2, b1, b2, eps, ref):
    """per-element bound on |contract - torch| of the update and of the moments: the kernels form 1 - beta from the fp32-rounded beta
    (for 0.999: 1.3e-5 below the double 0.001, relative), torch from the double; step_size and bc2_sqrt travel as fp32 (one rounding each)"""
    pr, _, mr, vr = ref
    d1 = abs((1.0 - _f32(b1)) - (1.0 - b1))
    d2 = abs((1.0 - _f32(b2)) - (1.0 - b2))
    dm = d1 * (g - m0).abs()
    dv = abs(_f32(b2) - b2) * v0 + d2 * g * g
    denom = vr.sqrt() / bc2 + eps
    u = ss * mr / denom
    safe_v = torch.where(vr > 0, vr, torch.ones_like(vr))
    du = SLACK * (u.abs() * (0.5 * dv / safe_v + 2 * E) + ss * dm / denom)
    return dm, dv, du
