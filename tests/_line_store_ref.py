"""numpy fp64 restatement of hwg_store_batch (csrc/line_store.hip): the horizontal stretch + shear of a grey line (the reference's
augmentation.affine_trans, cv2.warpAffine with INTER_LINEAR and a constant border) with 1 - p / 128 and the collate padding, in the kernel's
operation order - every intermediate below is one fp64 rounding, numpy never contracts. The kernel's output equals this bit for bit."""
import math

import numpy as np


def _taps(img, H, out_w, strech, m):
    """-> (in0, in1, i0, i1, f): per output pixel the two source columns (clipped for indexing), whether each is inside the line, and the
    blend weight"""
    w = img.shape[1]
    h = H / 2.0
    y = np.arange(H, dtype=np.float64)[:, None]
    x = np.arange(out_w, dtype=np.float64)[None, :]
    t = np.float64(m) * (y - h)
    num = x - t
    sx = num / np.float64(strech)
    x0 = np.floor(sx)
    f = sx - x0
    x1 = x0 + 1.0
    in0 = (x0 >= 0.0) & (x0 < float(w))
    in1 = (x1 >= 0.0) & (x1 < float(w))
    i0 = np.where(in0, x0, 0.0).astype(np.int64)
    i1 = np.where(in1, x1, 0.0).astype(np.int64)
    return in0, in1, i0, i1, f


def warp_levels(img, out_w, strech, m, want_interior=False):
    """uint8 [H, w] line -> uint8 [H, out_w] levels (border 255); want_interior: also the pixels whose two source columns are inside the line"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H = img.shape[0]
    in0, in1, i0, i1, f = _taps(img, H, out_w, strech, m)
    rows = np.arange(H)[:, None]
    src = img.astype(np.float64)
    p0 = np.where(in0, src[rows, i0], 255.0)
    p1 = np.where(in1, src[rows, i1], 255.0)
    d = p1 - p0
    fd = f * d
    v = p0 + fd
    q = np.floor(v + 0.5)
    level = np.minimum(np.maximum(q, 0.0), 255.0).astype(np.uint8)
    return (level, in0 & in1) if want_interior else level


def warp_line(img, out_w, strech, m):
    """-> float32 [H, out_w]: 1 - level / 128"""
    level = warp_levels(img, out_w, strech, m).astype(np.float32)
    return np.float32(1.0) - level / np.float32(128.0)


def warp_mask(mask, out_w, strech, m):
    """uint8 [H, w] mask (0 / 255) -> float32 [H, out_w]: p = byte / 255, border 0, (float)(p0 + f * (p1 - p0))"""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2
    H = mask.shape[0]
    in0, in1, i0, i1, f = _taps(mask, H, out_w, strech, m)
    rows = np.arange(H)[:, None]
    src = mask.astype(np.float64)
    p0 = np.where(in0, src[rows, i0], 0.0) / 255.0
    p1 = np.where(in1, src[rows, i1], 0.0) / 255.0
    d = p1 - p0
    fd = f * d
    v = p0 + fd
    return v.astype(np.float32)


def store_batch(lines, rows, W, masks=None):
    """lines: list of uint8 [H, w_k]; rows: [(line, out_w, strech, m)] -> out float32 [B, 1, H, W] (and out_mask with `masks`)"""
    H = lines[0].shape[0]
    out = np.full((len(rows), 1, H, W), -1.0, dtype=np.float32)
    om = np.zeros((len(rows), 1, H, W), dtype=np.float32) if masks is not None else None
    for b, (k, ow, s, m) in enumerate(rows):
        out[b, 0, :, :ow] = warp_line(lines[k], ow, s, m)
        if masks is not None:
            om[b, 0, :, :ow] = warp_mask(masks[k], ow, s, m)
    return out if masks is None else (out, om)


def tan(skew):
    """m as the host computes it"""
    return math.tan(skew)
