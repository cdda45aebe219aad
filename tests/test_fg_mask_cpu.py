"""CPU: what the foreground-only reconstruction loss decides on the host - the numpy restatement of the masks on hand-written cases (the
yardstick of tests/test_fg_mask_gpu.py), the pool that test uses, the switch (data/fg_masks.wants_fg_masks: the reference's literal lookup
plus data_loader.fg_masks_dir), and the refusals: a dataset constructed directly without a complete cache, `train.py --synthetic`."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as AR  # noqa: E402
import _fg_mask_ref as F  # noqa: E402

GAN_CFG = "cf_IAMslant_noMask_charSpecSingleAppend_GANMedMT_autoAEMoPrcp2tightNewCTCUseGen_balB_hCF0.75_sMG.json"


def test_single_ink_pixel_reproduces_the_element():
    line = np.full((21, 25), 240, dtype=np.uint8)
    line[10, 12] = 15
    mask, t = F.fg_mask(line)
    assert t == 15 and set(np.unique(mask)) == {0, 255} and int((mask == 255).sum()) == 57
    assert np.array_equal(mask[6:15, 8:17] == 255, F.element().astype(bool))
    rows = [int((mask[10 + dy] == 255).sum()) for dy in range(-4, 5)]
    assert rows == [2 * h + 1 for h in F.HALF_WIDTHS] == [1, 7, 7, 9, 9, 9, 7, 7, 1]
    e = F.element()
    assert np.array_equal(e[::-1], e) and np.array_equal(e[:, ::-1], e) and not np.array_equal(e.T, e)      # mirror-symmetric (a dilation needs no flip), not its own transpose


def test_ink_at_a_corner_is_clipped_by_the_lines_edge():
    line = np.full((12, 10), 240, dtype=np.uint8)
    line[0, 0] = 15
    mask, _ = F.fg_mask(line)
    want = np.zeros((12, 10), dtype=bool)
    want[:5, :5] = F.element()[4:, 4:].astype(bool)          # the element's lower-right quadrant is all that fits
    assert np.array_equal(mask == 255, want) and int(want.sum()) == 5 + 5 + 4 + 4 + 1
    line[11, 9] = 15                                          # and the opposite corner
    mask, _ = F.fg_mask(line)
    want[7:, 5:] = F.element()[:5, :5].astype(bool)
    assert np.array_equal(mask == 255, want)


def test_constant_lines_and_the_lowest_level_on_ties():
    assert F.threshold(np.full((8, 8), 255, dtype=np.uint8)) == 0 and not F.fg_mask(np.full((8, 8), 255, dtype=np.uint8))[0].any()
    assert F.threshold(np.zeros((8, 8), dtype=np.uint8)) == 0 and F.fg_mask(np.zeros((8, 8), dtype=np.uint8))[0].all()
    two = np.full((8, 8), 200, dtype=np.uint8)
    two[2, 2] = 60
    assert F.threshold(two) == 60                              # every level in [60, 199] is the same split


@pytest.mark.parametrize("H", [64, 16])
def test_the_gpu_tests_pool_never_rests_on_a_last_bit(H):
    """every line of the pool tests/test_fg_mask_gpu.py compares: the explicit 57-offset dilation agrees with scipy's, and the gap between
    the best split and the runner-up is exactly 0 (the tie line: the integers of the two splits are the same, so is every fp64 rounding) or
    many orders above an fp64 rounding error"""
    names, lines, pixels, offsets, widths = F.pool(H)
    assert len(set(names)) == len(names) and (H == 16 or {1, 3, 4, 8, 9, 63, 64, 65, 130, 700} <= set(widths))
    for name, line, o in zip(names, lines, offsets):
        assert pixels[o - 1] == F.GUARD and pixels[o + line.size] == F.GUARD and np.array_equal(pixels[o:o + line.size].reshape(line.shape), line)
        margin = AR.split_margin(np.bincount(line.reshape(-1), minlength=256))
        assert (margin == 0.0) if name == "tie" else (margin > 1e-6), (name, margin)
        mask, t = F.fg_mask(line)
        sc = F.dilate_scipy(line <= t)
        if sc is not None:
            assert np.array_equal(sc, mask == 255), name
    if H == 64:
        tie = lines[names.index("tie")]
        mask, t = F.fg_mask(tie)
        assert t == 0 and not (mask[:, 11:] == 255).any() and (mask[:, :11] == 255).all()         # the {0} | {100, 200} split, not {0, 100} | {200}
        assert sum(1 for o in offsets[:-1] if o % 4) >= len(lines) // 2                            # unaligned offsets


def test_masked_l1_restatement():
    rs = np.random.RandomState(0)
    r, x = rs.uniform(-1, 1, (2, 1, 4, 7)).astype(np.float32), rs.uniform(-1, 1, (2, 1, 4, 7)).astype(np.float32)
    ones = np.ones((2, 1, 4, 7), dtype=np.float32)
    v, g = F.masked_l1(r, x, ones)
    assert abs(v - np.abs(r.astype(np.float64) - x).mean()) < 1e-15 and np.array_equal(g, np.sign(r.astype(np.float64) - x) / r.size)
    m = rs.uniform(0, 1, (2, 1, 4, 5)).astype(np.float32)
    v, g = F.masked_l1(r, x, m, gout=0.5)
    assert not g[..., 5:].any() and abs(v - F.masked_l1_exact_products(r, x, m)) < 1e-7
    v32, _ = F.masked_l1(r, x, m, np.float32)
    assert v32.dtype == np.float32 and abs(float(v32) - float(v)) < 1e-6


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------
def test_wants_fg_masks_truth_table():
    from handwriting_line_generation_amd.data.fg_masks import loss_on, wants_fg_masks
    base = {"trainer": {"no_bg_loss": True}, "data_loader": {"fg_masks_dir": "masks"}}
    assert not wants_fg_masks(base) and not loss_on(base)                                      # trainer key only: the reference's lookup says no
    assert wants_fg_masks(dict(base, no_bg_loss=True)) and loss_on(dict(base, no_bg_loss=True))
    assert wants_fg_masks(dict(base, no_bg_loss=False))                                        # `'no_bg_loss' in config`: the key's presence counts
    assert not wants_fg_masks({"no_bg_loss": True, "trainer": {"no_bg_loss": False}, "data_loader": {"fg_masks_dir": "masks"}})
    assert not wants_fg_masks({"no_bg_loss": True, "trainer": {}, "data_loader": {"fg_masks_dir": "masks"}})
    no_dir = {"no_bg_loss": True, "trainer": {"no_bg_loss": True}, "data_loader": {}}
    assert loss_on(no_dir) and not wants_fg_masks(no_dir)
    assert not wants_fg_masks(dict(no_dir, data_loader={"fg_masks_dir": None}))


def test_every_shipped_config_leaves_the_switch_off():
    from handwriting_line_generation_amd.data.fg_masks import loss_on, wants_fg_masks
    paths = sorted(glob.glob(os.path.join(ROOT, "configs", "*.json")))
    assert len(paths) >= 7
    named = 0
    for p in paths:
        cfg = json.load(open(p))
        assert not wants_fg_masks(cfg) and not loss_on(cfg), p
        named += bool(cfg["trainer"].get("no_bg_loss"))
    assert named >= 2                                          # both GAN configs ask for it one level too low


def _fake_iam(tmp_path):
    from oracle import collate_items
    from handwriting_line_generation_amd.harness import CHAR_FILES
    root = str(tmp_path / "iam")
    os.makedirs(root)
    collate_items.fake_iam(root, n_pages=6, with_images=True)
    return root, {"img_height": 64, "a_batch_size": 2, "max_width": 640, "char_file": CHAR_FILES["iam"], "augmentation": "affine",
                  "fg_masks_dir": str(tmp_path / "masks")}


def test_dataset_constructed_directly_without_a_cache_refuses(tmp_path):
    from handwriting_line_generation_amd.data.author_hw_dataset import AuthorHWDataset
    root, dcfg = _fake_iam(tmp_path)
    ds = AuthorHWDataset(root, "train", dcfg)                                                  # fg_masks_dir alone: as before, no masks, no directory
    assert ds.fg_masks_dir is None and "fg_mask" not in ds[0] and not os.path.exists(str(tmp_path / "masks_640"))
    with pytest.raises(NotImplementedError, match="getDataLoader"):
        AuthorHWDataset(root, "train", dict(dcfg, no_bg_loss=True))
    assert not glob.glob(str(tmp_path / "masks_640" / "*"))


def test_dataset_reads_a_complete_cache_and_warps_the_mask_with_the_line(tmp_path):
    """a cache some other run wrote (here: the restatement) is read as it is; the items carry fg_mask of the image's shape, equal to the
    cached PNG / 255 without augmentation, warped with the line's own coefficients (bilinear, border 0) under `affine`; the draw order of
    the augmentation parameters is what it is without masks"""
    from PIL import Image
    from handwriting_line_generation_amd.data import fg_masks
    from handwriting_line_generation_amd.data.author_hw_dataset import AuthorHWDataset
    root, dcfg = _fake_iam(tmp_path)
    plain = AuthorHWDataset(root, "train", dict(dcfg, augmentation=None))
    plain.fg_masks_dir = fg_masks.cache_dir(dcfg["fg_masks_dir"], 640)
    assert plain.fg_masks_dir == str(tmp_path / "masks_640") == fg_masks.cache_dir(dcfg["fg_masks_dir"] + "/", 640)
    todo = fg_masks.missing(plain)
    assert len(todo) == len({(a, l) for a, ls in plain.lineIndex for l in ls})
    os.makedirs(plain.fg_masks_dir)
    fitted = {}
    for author, line in todo:
        path, lb, _ = plain.authors[author][line]
        img = plain._fit(plain._page(path)[max(lb[0], 0):lb[1], max(lb[2], 0):lb[3]])
        fitted[(author, line)] = img
        Image.fromarray(F.fg_mask(img)[0]).save(fg_masks.mask_path(plain, author, line))
        assert fg_masks.png_size(fg_masks.mask_path(plain, author, line)) == img.shape
    assert fg_masks.missing(plain) == []
    # a mask of another size than the fitted line is stale
    a0, l0 = todo[0]
    Image.fromarray(np.zeros((64, fitted[todo[0]].shape[1] + 1), dtype=np.uint8)).save(fg_masks.mask_path(plain, a0, l0))
    assert fg_masks.missing(plain) == [todo[0]]
    Image.fromarray(F.fg_mask(fitted[todo[0]])[0]).save(fg_masks.mask_path(plain, a0, l0))

    ds = AuthorHWDataset(root, "train", dict(dcfg, augmentation=None, no_bg_loss=True))      # complete cache: no device needed
    item, ref = ds[0], plain[0]
    assert np.array_equal(item["image"].numpy(), ref["image"].numpy()) and item["fg_mask"].shape == item["image"].shape
    author, lines = ds.lineIndex[0]
    for i, line in enumerate(lines):
        m = F.fg_mask(fitted[(author, line)])[0].astype(np.float32) / 255
        assert np.array_equal(item["fg_mask"][i, 0, :, :m.shape[1]].numpy(), m) and not item["fg_mask"][i, 0, :, m.shape[1]:].any()

    aug, aug_plain = AuthorHWDataset(root, "train", dict(dcfg, no_bg_loss=True)), AuthorHWDataset(root, "train", dcfg)
    np.random.seed(4)
    item = aug[1]
    after = np.random.get_state()[2]
    np.random.seed(4)
    ref = aug_plain[1]
    assert after == np.random.get_state()[2] and np.array_equal(item["image"].numpy(), ref["image"].numpy())
    fg = item["fg_mask"].numpy()
    assert fg.shape == item["image"].shape and fg.min() >= 0 and fg.max() <= 1 and 0 < fg.mean() < 1


def test_train_cli_refuses_synthetic_batches_with_the_switch_on(tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "configs", GAN_CFG)))
    cfg["no_bg_loss"] = True
    path = str(tmp_path / ("cf_" + cfg["name"] + ".json"))
    json.dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-c", path, "--synthetic", "--iterations", "1"], cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "synthetic" in r.stderr and "no foreground masks" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "saved"))
