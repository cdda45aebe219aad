"""Numpy restatement of hwg_eval_pairs (csrc/eval_pictures.hip), written from its description: the per-line evaluation picture of new_eval.py -
the real line above its reconstruction, framed, optionally with a caption strip - as uint8 RGB. tests/test_eval_pictures_cpu.py checks it
against arrays recorded from the reference's evaluators/hwdataset_eval.py (tests/golden/eval_pictures.npz); the GPU tests check the kernel
against it."""
import numpy as np

STRIP = 50
GREEN = (0, 255, 0)
BLUE = (0, 0, 255)


def levels(x):
    """fp32 array -> uint8: v = 1 - (1 + x) / 2 in fp32, trunc of the exact v * 255, clamped to [0, 255], NaN -> 0"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.float32(1) - (np.float32(1) + x) / np.float32(2)
        assert v.dtype == np.float32
        p = v.astype(np.float64) * 255.0
        p = np.where(np.isnan(p), 0.0, np.clip(p, 0.0, 255.0))
    return p.astype(np.uint8)


def edge_values():
    """the 2304 values x = fp32(1 - 2k/255) and its +-1..4 ulp neighbours, k = 0..255, clipped to [-1, 1]"""
    base = (1.0 - 2.0 * np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    out = []
    for x in base:
        row = [x]
        up = dn = x
        for _ in range(4):
            up = np.nextafter(up, np.float32(2))
            dn = np.nextafter(dn, np.float32(-2))
            row += [up, dn]
        out += row
    return np.clip(np.asarray(out, dtype=np.float32), -1.0, 1.0)


def shape(H, Wi, Wr, strip):
    return 2 * H + 2 + (STRIP if strip else 0), max(Wi, Wr)


def eval_pairs(image, recon, captions=None, atlas=None):
    """image [B,1,H,Wi], recon [B,1,H,Wr] fp32; captions [B, L] int (a negative code ends a caption) with atlas [G, gh, gw] uint8, or None
    (no strip) -> uint8 [B, Hp, Wp, 3] RGB"""
    image, recon = np.asarray(image, dtype=np.float32), np.asarray(recon, dtype=np.float32)
    B, _, H, Wi = image.shape
    Wr = recon.shape[3]
    strip = captions is not None
    Hp, Wp = shape(H, Wi, Wr, strip)
    dif = abs(Wi - Wr)
    pr = dif // 2 if Wi < Wr else 0
    pg = dif // 2 if Wr < Wi else 0
    out = np.zeros((B, Hp, Wp, 3), dtype=np.uint8)
    out[:, 0:H, pr:pr + Wi, :] = levels(image[:, 0])[..., None]
    out[:, H + 2:2 * H + 2, pg:pg + Wr, :] = levels(recon[:, 0])[..., None]
    for r in (0, H):
        out[:, r, pr:Wp - pr] = GREEN
    for c in (pr, Wp - 1 - pr):
        out[:, 0:H, c] = GREEN
    for r in (H + 1, 2 * H + 1):
        out[:, r, pg:Wp - pg] = BLUE
    for c in (pg, Wp - 1 - pg):
        out[:, H + 2:2 * H + 2, c] = BLUE
    if strip:
        atlas = np.asarray(atlas, dtype=np.uint8)
        G, gh, gw = atlas.shape
        top = 2 * H + 2 + (STRIP - gh) // 2
        for b in range(B):
            for j, code in enumerate(captions[b]):
                code = int(code)
                if code < 0:
                    break
                x0 = 2 + j * gw
                if x0 >= Wp:
                    break
                w = min(gw, Wp - x0)
                out[b, top:top + gh, x0:x0 + w, :] = atlas[code][:, :w, None]
    return out
