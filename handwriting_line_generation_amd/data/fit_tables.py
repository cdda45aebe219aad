"""The host half of hwg_fit_lines (csrc/fit_lines.hip): the coefficient tables of PIL's 8-bit bicubic resize, computed in fp64 in the order
of Pillow's Resample.c (precompute_coeffs, then normalize_coeffs_8bpc), and the width rule of the loaders' `_resize`. The kernel does the
integer sums only, so its bytes are PIL's as long as these tables are PIL's; tests/test_fit_lines_cpu.py holds them to PIL itself.

For an axis of `in_size` pixels resized to `out_size` (bicubic, a = -0.5, support 2):
    scale = in_size / out_size;  fs = max(scale, 1.0);  support = 2.0 * fs;  ss = 1.0 / fs
    center = (xx + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0);  n = min(int(center + support + 0.5), in_size) - xmin
    w[x] = bicubic((x + xmin - center + 0.5) * ss), summed left to right, each divided by the sum (where the sum is not 0)
    k[x] = int(w * 2^22 + 0.5), or int(w * 2^22 - 0.5) for w < 0 (conversion truncates toward zero)
A pass computes acc = 2^21 + sum(pixel * k) in 32-bit integers and writes clamp(acc >> 22, 0, 255); the horizontal pass runs first into
an 8-bit intermediate; a pass whose in_size == out_size is skipped. One exception to the order, made by Image.resize itself in the
Pillow this was checked against (12.x): a picture more than 100 times as tall as wide that shrinks vertically gets the vertical pass
first (vertical_first)."""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def fitted_width(h, w, H):
    """the width `_resize(img, float(H) / h)` (data/author_hw_dataset.py) gives an h x w picture"""
    return max(int(round(w * (float(H) / h))), 1)


def vertical_first(h, w, H):
    """Image.resize's own rule (`self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`): such a picture is resized to (w, H) first
    and to (out_w, H) second, so the intermediate rounding falls on other bytes"""
    return h > w * 100 and H < h


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=256)
def resample_table(in_size, out_size):
    """-> (xmin int32 [out], count int32 [out], k int32 [out, ksize]) of one axis: output index xx is
    clamp((2^21 + sum_{x < count[xx]} pixel[xmin[xx] + x] * k[xx, x]) >> 22, 0, 255); k is 0 behind count. Cached per (in, out) pair - the
    arrays are shared and read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resample_table: sizes must be positive, got %d -> %d" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0)
    count = np.minimum(np.trunc(center + support + 0.5), float(in_size)) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    live = x < count[:, None]
    w = np.where(live, _bicubic((x + xmin[:, None] - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                       # left to right; the zeros behind `count` add nothing
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    scaled = w * float(1 << PRECISION_BITS)
    k = np.trunc(np.where(w < 0, scaled - 0.5, scaled + 0.5)).astype(np.int32)
    out = (xmin.astype(np.int32), count.astype(np.int32), k)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=512)
def axis_block(in_size, out_size):
    """-> (int32 1-D block first[out], count[out], k[out][ks] padded with zeros to a multiple of 4 elements, ks): the layout hwg_fit_lines
    reads an axis table in. ks = 0 and an empty block where in_size == out_size (the pass is skipped)."""
    if in_size == out_size:
        return np.zeros(0, dtype=np.int32), 0
    xmin, count, k = resample_table(in_size, out_size)
    n = xmin.size + count.size + k.size
    block = np.zeros(-(-n // 4) * 4, dtype=np.int32)
    block[:n] = np.concatenate([xmin, count, k.reshape(-1)])
    block.setflags(write=False)
    return block, k.shape[1]


ENTRY = 10                                                  # int64 words of a line's entry in hwg_fit_lines' table


def batch_tables(shapes, H, widths=None):
    """the device tables of hwg_fit_lines for pictures of `shapes` [(h, w)] lying back to back in one pool -> (lines int64 [B, ENTRY]:
    {byte offset, h, w, out_w, htab, hks, vtab, vks, order, 0}, coef int32 1-D: one axis_block per distinct (in, out) pair of the batch,
    each at a multiple of 4 elements; never empty). widths: the output widths (default: fitted_width)."""
    if widths is None:
        widths = [fitted_width(h, w, H) for h, w in shapes]
    lines = np.zeros((len(shapes), ENTRY), dtype=np.int64)
    blocks, where, pos, off = [], {}, 0, 0
    for b, (h, w) in enumerate(shapes):
        entry = [off, h, w, widths[b]]
        for pair in ((w, widths[b]), (h, H)):
            block, ks = axis_block(*pair)
            if ks and pair not in where:
                where[pair] = pos
                blocks.append(block)
                pos += block.size
            entry += [where[pair] if ks else 0, ks]
        lines[b] = entry + [int(vertical_first(h, w, H)), 0]
        off += h * w
    coef = np.concatenate(blocks) if blocks else np.zeros(4, dtype=np.int32)
    return lines, coef


def resample_axis(img, out_size, axis):
    """numpy restatement of one pass over `axis` (0: vertical, 1: horizontal) of a uint8 picture, driven by resample_table"""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    xmin, count, k = resample_table(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    acc = np.full((out_size,) + src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for x in range(k.shape[1]):                              # tap by tap over all outputs; k is 0 behind `count`, so the clamped index adds 0
        acc += src[np.minimum(xmin + x, in_size - 1)] * k[:, x].reshape((-1,) + (1,) * (src.ndim - 1))
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def fit_line_host(img, H, out_w=None):
    """the integer restatement of Image.fromarray(img).resize((out_w, H), Image.BICUBIC) on a uint8 [h, w] picture: horizontal pass first,
    but for vertical_first pictures"""
    if out_w is None:
        out_w = fitted_width(img.shape[0], img.shape[1], H)
    if vertical_first(img.shape[0], img.shape[1], H):
        return resample_axis(resample_axis(img, H, 0), out_w, 1)
    return resample_axis(resample_axis(img, out_w, 1), H, 0)
