"""Helpers of the warp-mode line store tests (tests/test_line_store_warp_cpu.py, tests/test_line_store_warp_gpu.py): fabricated dataset
directories, fabricated line pictures, a pool of them and the collated batch the old path is handed. Test infrastructure, not product code.

The yardstick of these tests is code that exists: ops.augment_lines on the uploaded collated batch and DeviceAugment(ShardedLoader(...)),
which tests/_augment_ref.py ties to fp64. The store's path adds no arithmetic of its own, so every comparison is bit equality."""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 64
POOL_WIDTHS = (5, 6, 63, 64, 65, 130, 333)      # not warped / just warped / around one 64-column tile edge / across one / several tiles
HWR_CFG = {"iam": "cf_IAM_hwr_cnnOnly_batchnorm_aug.json", "rimes": "cf_RIMESLines_hwr_cnnOnly_batchnorm_aug.json",
           "synth": "cf_IAM_hwr_cnnOnly_batchnorm_aug_synth.json"}


def fabricate(which, root):
    """a fabricated IAM / RIMES directory in the reference's layout (the recipe of tests/test_augment_gpu.py and the data tests)"""
    from oracle import collate_items
    os.makedirs(root)
    if which == "iam":
        collate_items.fake_iam(root, n_pages=6, with_images=True)
    else:
        collate_items.fake_rimes(root)


def hwr_config(which, root, tmp_path, **data_loader):
    from handwriting_line_generation_amd.harness import CHAR_FILES
    cfg = json.load(open(os.path.join(ROOT, "configs", HWR_CFG[which])))
    chars = CHAR_FILES["rimes" if which == "rimes" else "iam"]
    cfg["data_loader"].update(data_dir=root, batch_size=4, num_workers=0, char_file=chars, **data_loader)
    cfg["validation"].update(batch_size=4, num_workers=0)
    cfg["trainer"].update(save_dir=str(tmp_path / "saved"), save_step=10 ** 6, save_step_minor=10 ** 6, log_step=10 ** 6, val_step=10 ** 6, iterations=6)
    cfg["seed"] = 5
    cfg["cuda"], cfg["gpu"] = True, 0
    return cfg


def text_line(rs, w):
    """a line-like image: light paper with noise, dark strokes (tests/test_augment_gpu.py's recipe: its Otsu split margin is far above 1e-9)"""
    img = rs.randint(190, 256, size=(H, w))
    for _ in range(max(w // 14, 1)):
        x, y = int(rs.randint(0, max(w - 3, 1))), int(rs.randint(4, 40))
        img[y:y + int(rs.randint(6, 22)), x:x + int(rs.randint(2, 9))] = rs.randint(10, 110)
    return img.astype(np.int64)


def pool_lines(widths=POOL_WIDTHS, seed=33):
    rs = np.random.RandomState(seed)
    return [text_line(rs, w) for w in widths]


def make_pool(lines, device, gaps=True):
    """the lines (levels [H, w]) as an ops.LinePool on `device`. With H = 64 lines laid back to back begin at multiples of 64 whatever
    their widths (only their ROWS begin at odd addresses), so line k is preceded by k + 1 bytes of filler (value 7, darker than any
    stroke): the offsets take every residue mod 2 and mod 4, and a read outside a line would show"""
    from handwriting_line_generation_amd import ops
    widths = np.array([l.shape[1] for l in lines], dtype=np.int64)
    offsets = np.zeros(len(lines), dtype=np.int64)
    parts, at = [], 0
    for k, l in enumerate(lines):
        gap = k + 1 if gaps else 0
        parts += [np.full(gap, 7, dtype=np.uint8), l.astype(np.uint8).reshape(-1)]
        offsets[k] = at + gap
        at += gap + l.size
    pixels = np.concatenate(parts)
    return ops.LinePool(torch.from_numpy(pixels).to(device), offsets, widths, height=H)


def collate(lines, W, x_off=None):
    """what collate hands the old path: 1 - level / 128 at [x_off, x_off + w), -1 elsewhere -> fp32 [B,1,H,W] (host)"""
    x = np.full((len(lines), 1, H, W), -1.0, dtype=np.float32)
    for b, l in enumerate(lines):
        o = 0 if x_off is None else x_off[b]
        x[b, 0, :, o:o + l.shape[1]] = 1.0 - l.astype(np.float32) / 128.0
    return torch.from_numpy(x)


def draws(rs, w, sigma=1.5):
    """explicit displacements for a line of width w (None for a line too narrow to be warped)"""
    from handwriting_line_generation_amd import ops
    if w <= 5:
        return None
    sy, sx = ops.warp_lattice(H, w)
    n = (len(sy), len(sx))
    return (rs.normal(0.0, sigma, size=n), rs.normal(0.0, sigma, size=n))
