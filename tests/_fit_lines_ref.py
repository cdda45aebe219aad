"""hwg_fit_lines as include/hwg.h states it, restated in numpy and unbounded Python integers over the very tables the entry reads (not
collected by pytest): the pictures of tests/test_fit_lines_cpu.py and tests/test_fit_lines_gpu.py, and `emulate`, which turns a pool, a
per-line table and a coefficient buffer into the batch the kernel has to write - a bad entry into padding."""
import numpy as np

HEIGHTS = [1, 2, 7, 31, 63, 64, 65, 100, 128, 129, 200, 300, 511]
WIDTHS = [1, 3, 5, 37, 64, 97, 333, 1000, 2000]
KINDS = ["random", "two-level", "stripe"]
MAX_IN_H, MAX_W, MAX_KS, TILE = 1024, 1 << 20, 1 << 16, 64      # the limits include/hwg.h documents for hwg_fit_lines


def picture(h, w, kind, seed=0):
    g = np.random.RandomState((seed * 7919 + h * 2003 + w) % (1 << 31))
    if kind == "random":
        return g.randint(0, 256, (h, w)).astype(np.uint8)
    if kind == "two-level":
        return ((g.rand(h, w) < 0.5) * 255).astype(np.uint8)
    img = np.full((h, w), 255, dtype=np.uint8)                  # a black stripe on white
    img[h // 3:h // 3 + max(1, h // 5)] = 0
    return img


def levels(p):
    assert p.dtype == np.uint8
    return np.float32(1.0) - p.astype(np.float32) / np.float32(128.0)


def pil_fit(img, H, out_w):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((out_w, H), Image.BICUBIC))


def expected_batch(images, H, W, widths):
    """1 - PIL / 128 on the fitted columns, -1 beyond"""
    want = np.full((len(images), 1, H, W), -1.0, dtype=np.float32)
    for b, (im, w) in enumerate(zip(images, widths)):
        want[b, 0, :, :w] = levels(pil_fit(im, H, w))
    return want


def pool_of(images):
    return np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])


def _axis_ok(coef, tab, ks, n, size):
    """the table of an axis of `size` pixels resized to n at element `tab`: inside coef, aligned, every window inside the axis"""
    if ks == 0:
        return size == n
    if not (0 <= tab and tab % 4 == 0 and tab <= len(coef) and n * (2 + ks) <= len(coef) - tab):
        return False
    first, count = coef[tab:tab + n].astype(np.int64), coef[tab + n:tab + 2 * n].astype(np.int64)
    return bool(((first >= 0) & (count >= 0) & (count <= ks) & (first + count <= size)).all())


def entry_ok(entry, coef, pixel_bytes, max_in_h, H, W):
    off, h, w, ow, htab, hks, vtab, vks, order = (int(v) for v in entry[:9])
    if not (1 <= h <= max_in_h and 1 <= w <= MAX_W and 1 <= ow <= W and 0 <= hks <= MAX_KS and 0 <= vks <= MAX_KS):
        return False
    if not (order == 0 or (order == 1 and w <= TILE)):
        return False
    if not (0 <= off <= pixel_bytes and h * w <= pixel_bytes - off):
        return False
    return _axis_ok(coef, htab, hks, ow, w) and _axis_ok(coef, vtab, vks, H, h)


def _pass(pic, coef, tab, ks, n, axis):
    if ks == 0:
        return pic
    first, count = coef[tab:tab + n], coef[tab + n:tab + 2 * n]
    k = coef[tab + 2 * n:tab + 2 * n + n * ks].reshape(n, ks).astype(np.int64)
    src = np.moveaxis(pic, axis, 0).astype(np.int64)
    out = np.empty((n,) + src.shape[1:], dtype=np.uint8)
    for i in range(n):
        f, c = int(first[i]), int(count[i])
        acc = (1 << 21) + np.tensordot(k[i, :c], src[f:f + c], axes=(0, 0))
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)         # 32-bit integers
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def emulate(pixels, lines, coef, max_in_h, H, W):
    B = lines.shape[0]
    out = np.full((B, 1, H, W), -1.0, dtype=np.float32)
    for b in range(B):
        if not entry_ok(lines[b], coef, pixels.size, max_in_h, H, W):
            continue
        off, h, w, ow, htab, hks, vtab, vks, order = (int(v) for v in lines[b, :9])
        pic = pixels[off:off + h * w].reshape(h, w)
        if order == 1:
            pic = _pass(_pass(pic, coef, vtab, vks, H, 0), coef, htab, hks, ow, 1)
        else:
            pic = _pass(_pass(pic, coef, htab, hks, ow, 1), coef, vtab, vks, H, 0)
        out[b, 0, :, :ow] = levels(pic)
    return out
