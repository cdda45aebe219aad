"""What torchvision.utils.save_image(1 - images, nrow=nrow, normalize=True) writes for a [B,1,H,W] fp32 batch, restated with torch CPU
tensor operations in torchvision's documented order (utils.py: make_grid -> norm_range -> norm_ip, then save_image's quantisation), one
channel. torchvision is not installed, so this restatement is the yardstick of the sample-sheet kernels (csrc/sample_sheet.hip): for
finite input every step is a correctly rounded fp32 operation on both sides, so the comparison is byte equality.

    norm_ip(t, low, high):  t.clamp_(min=low, max=high); t.sub_(low).div_(max(high - low, 1e-5))     low, high Python floats
    make_grid:              B == 1 -> the image itself; else xmaps = min(nrow, B), ymaps = ceil(B / xmaps), padding 2, pad_value 0
    save_image:             grid.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
"""
import math

import torch


def default_nrow(W):
    return max(1, 2048 // W)


def normalised_grid(v, nrow, value_range=None):
    """v = 1 - images [B,1,H,W] fp32 (CPU) -> the normalised fp32 grid [Hs, Ws]"""
    t = v.clone()
    if value_range is not None:
        low, high = float(value_range[0]), float(value_range[1])
    else:
        low, high = float(t.min()), float(t.max())
    t.clamp_(min=low, max=high)
    t.sub_(low).div_(max(high - low, 1e-5))
    B, _, H, W = t.shape
    if B == 1:
        return t[0, 0]
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    height, width = H + 2, W + 2
    grid = t.new_full((height * ymaps + 2, width * xmaps + 2), 0.0)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= B:
                break
            grid.narrow(0, y * height + 2, height - 2).narrow(1, x * width + 2, width - 2).copy_(t[k, 0])
            k += 1
    return grid


def sheet_of_v(v, nrow=None, value_range=None):
    nrow = default_nrow(v.shape[3]) if nrow is None else nrow
    return normalised_grid(v, nrow, value_range).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def sheet(images, nrow=None):
    """the uint8 [Hs, Ws] sheet of a CPU fp32 batch `images` [B,1,H,W]"""
    return sheet_of_v(1 - images, nrow)


def sheet_fused(images, nrow=None):
    """the variant a contracted kernel would compute: n * 255 + 0.5 with ONE rounding (evaluated in fp64, where the product of an fp32
    and 255 and the sum with 0.5 are exact or far below half an fp32 ulp off, then rounded once to fp32)"""
    nrow = default_nrow(images.shape[3]) if nrow is None else nrow
    grid = normalised_grid(1 - images, nrow)
    return (grid.double() * 255.0 + 0.5).float().clamp_(0, 255).to(torch.uint8)


def sheet_nonfinite(images, nrow=None):
    """the project's rule for values that are not finite, from the finite restatement: lo / hi over the finite v = 1 - images; NaN ->
    hi + 1, +inf -> hi, -inf -> lo, normalised over (lo, hi); the NaN pixels then 0. No finite value at all: an all-0 sheet."""
    nrow = default_nrow(images.shape[3]) if nrow is None else nrow
    v = 1 - images
    finite = torch.isfinite(v)
    B, _, H, W = v.shape
    if not bool(finite.any()):
        return torch.zeros_like(sheet_of_v(torch.zeros_like(v), nrow))
    lo, hi = float(v[finite].min()), float(v[finite].max())
    nan = torch.isnan(v)
    w = v.clone()
    w[nan] = hi + 1
    w[v == float("inf")] = hi
    w[v == float("-inf")] = lo
    out = sheet_of_v(w, nrow, (lo, hi))
    mask = sheet_of_v(torch.where(nan, torch.zeros_like(v), torch.ones_like(v)), nrow, (0.0, 1.0)) == 0      # NaN pixels (and the borders, 0 anyway)
    out[mask] = 0
    return out
