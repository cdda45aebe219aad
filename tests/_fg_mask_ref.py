"""numpy restatement of the foreground masks (csrc/fg_mask.hip; reference: datasets/author_hw_dataset.py:216-219 - cv2.threshold(BINARY + OTSU),
255 - that, cv2.dilate with getStructuringElement(MORPH_ELLIPSE, (9, 9))) and of the foreground-masked L1 loss (trainer :596-601) for the
tests. The threshold is tests/_augment_ref.otsu_variances' (exact integers, two fp64 roundings, lowest level on ties); the dilation is an
explicit OR over the element's 57 offsets, nothing of the kernel's bit-column arithmetic. Test infrastructure, not product code."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as AR  # noqa: E402

# half-width of the 9 x 9 ellipse per row offset dy = -4 .. 4: OpenCV fills columns c - dx .. c + dx with dx = round(4 sqrt((16 - dy^2) / 16))
HALF_WIDTHS = [0, 3, 3, 4, 4, 4, 3, 3, 0]
OFFSETS = [(dy, dx) for dy in range(-4, 5) for dx in range(-HALF_WIDTHS[dy + 4], HALF_WIDTHS[dy + 4] + 1)]
assert len(OFFSETS) == 57 and HALF_WIDTHS == [int(np.rint(4 * np.sqrt((16 - dy * dy) / 16.0))) for dy in range(-4, 5)]


def element():
    """the structuring element as a 9 x 9 uint8 array (what cv2.getStructuringElement returns)"""
    e = np.zeros((9, 9), dtype=np.uint8)
    for dy, dx in OFFSETS:
        e[dy + 4, dx + 4] = 1
    return e


def threshold(line):
    """Otsu level of a uint8 [H, w] line: lowest level of the best split, 0 for a constant line"""
    hist = np.bincount(np.asarray(line, dtype=np.uint8).reshape(-1), minlength=256)
    var, _ = AR.otsu_variances(hist)
    return int(np.argmax(var))


def dilate(binary):
    """bool [H, w] -> bool [H, w]: out(y, x) = OR over the 57 cells of binary(y + dy, x + dx), cells outside the line never count"""
    b = np.asarray(binary, dtype=bool)
    H, w = b.shape
    out = np.zeros((H, w), dtype=bool)
    for dy, dx in OFFSETS:
        ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), w + min(dx, 0))         # source rows / columns that stay inside
        yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), w + min(-dx, 0))
        if ys.start < ys.stop and xs.start < xs.stop:
            out[yd, xd] |= b[ys, xs]
    return out


def dilate_scipy(binary):
    """the same through scipy.ndimage (None where scipy is absent): the cross-check of the explicit loop"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    return ndimage.binary_dilation(np.asarray(binary, dtype=bool), structure=element().astype(bool), border_value=0)


def fg_mask(line):
    """uint8 [H, w] grey line -> (uint8 mask of 0 / 255, threshold)"""
    line = np.asarray(line, dtype=np.uint8)
    t = threshold(line)
    return np.where(dilate(line <= t), 255, 0).astype(np.uint8), t


def _text_line(rs, H, w):
    """light noisy paper with dark strokes"""
    img = rs.randint(190, 256, size=(H, w))
    for _ in range(max(w // 14, 1)):
        x, y = int(rs.randint(0, max(w - 3, 1))), int(rs.randint(0, max(H - 8, 1)))
        img[y:y + int(rs.randint(3, 22)), x:x + int(rs.randint(2, 9))] = rs.randint(10, 110)
    return img.astype(np.uint8)


def pool_lines(H):
    """[(name, uint8 [H, w] line)]: the widths around the kernel's 64-lane rows and its 4-column halo, ink on every border and corner, constant
    lines, a two-level line (every level between the two gives the same split: the lowest must be reported), a three-level line whose two
    splits tie EXACTLY (counts n, m, n at levels 0, 100, 200: the integers of both splits are the same), a noisy scan-like line. H = 64: all
    of them, with one line wider than the kernel's 1024-column chunk; H = 16: a few."""
    rs = np.random.RandomState(64 + H)
    out = []
    for w in ([1, 3, 4, 8, 9, 63, 64, 65, 130, 700, 1100] if H == 64 else [1, 9, 65]):
        line = _text_line(rs, H, w)
        if w <= 4:
            line = np.where(rs.rand(H, w) < 0.3, 30, 220).astype(np.uint8)
            line[0, 0], line[H - 1, w - 1] = 30, 220
        out.append(("w%d" % w, line))
    corners = np.full((H, 33), 230, dtype=np.uint8)
    for y, x in ((0, 0), (0, 32), (H - 1, 0), (H - 1, 32)):
        corners[y, x] = 20
    out.append(("corners", corners))
    borders = np.full((H, 40), 225, dtype=np.uint8)
    borders[0, 7:12] = borders[H - 1, 25:31] = 40
    borders[5:9, 0] = borders[H - 7:H - 3, 39] = 35
    out.append(("borders", borders))
    if H == 64:
        out.append(("all255", np.full((H, 20), 255, dtype=np.uint8)))
        out.append(("all0", np.zeros((H, 20), dtype=np.uint8)))
        two = np.full((H, 12), 200, dtype=np.uint8)
        two[20:30, 3:6] = 60
        out.append(("two_level", two))
        tie = np.full((H, 30), 100, dtype=np.uint8)
        tie[:, :7], tie[:, 23:] = 0, 200
        out.append(("tie", tie))
    scan = np.clip(rs.normal(205, 18, size=(H, 257)), 0, 255)
    for _ in range(14):
        x, y = int(rs.randint(0, 250)), int(rs.randint(0, H - 6))
        scan[y:y + int(rs.randint(3, 30)), x:x + int(rs.randint(2, 6))] = rs.normal(70, 25)
    out.append(("scan", np.clip(np.rint(scan), 0, 255).astype(np.uint8)))
    return out


GUARD = 0xA5


def pool(H):
    """the lines of pool_lines(H) at unaligned byte offsets, every line between guard bytes -> (names, lines, pixels uint8 1-D, offsets [B+1], widths [B])"""
    named = pool_lines(H)
    gaps = [3, 1, 5, 2, 7, 1, 6, 3, 9, 1, 2, 5, 11, 1, 3, 7, 2, 5, 1]
    offsets, pos = [], 0
    for k, (_, line) in enumerate(named):
        pos += gaps[k % len(gaps)]
        offsets.append(pos)
        pos += line.size
    total = pos + 13
    pixels = np.full(total, GUARD, dtype=np.uint8)
    for o, (_, line) in zip(offsets, named):
        pixels[o:o + line.size] = line.reshape(-1)
    return [n for n, _ in named], [l for _, l in named], pixels, np.array(offsets + [total], dtype=np.int64), [l.shape[1] for _, l in named]


def pad_mask(mask, W):
    """[B,1,H,Wm] -> [B,1,H,W] with zero columns (the reference's F.pad(fg_mask, (0, toPad), value=0))"""
    mask = np.asarray(mask)
    out = np.zeros(mask.shape[:3] + (W,), dtype=mask.dtype)
    out[..., :mask.shape[3]] = mask
    return out


def masked_l1(recon, image, mask, dtype=np.float64, gout=1.0):
    """-> (value, d recon). The products r m and x m are rounded to float32 in either precision - that IS the definition (the reference
    multiplies fp32 tensors) -; the difference, the sum, the mean and the gradient sign(rm - xm) m gout / N are evaluated in `dtype`."""
    r, x = np.asarray(recon, dtype=np.float32), np.asarray(image, dtype=np.float32)
    m = pad_mask(np.asarray(mask, dtype=np.float32), r.shape[3])
    rm, xm = (r * m).astype(dtype), (x * m).astype(dtype)
    n = r.size
    value = np.abs(rm - xm).sum(dtype=dtype) / dtype(n)
    grad = np.sign(rm - xm) * m.astype(dtype) * (dtype(gout) / dtype(n))
    return dtype(value), grad.astype(dtype)


def masked_l1_exact_products(recon, image, mask):
    """fp64 throughout, products NOT rounded to float32: how far the definition itself sits from real arithmetic (printed, never asserted)"""
    r, x = np.asarray(recon, dtype=np.float64), np.asarray(image, dtype=np.float64)
    m = pad_mask(np.asarray(mask, dtype=np.float64), r.shape[3])
    return float(np.abs(r * m - x * m).mean())
