"""CPU: the line-per-item IAM dataset of the recogniser pre-training configs (data/hw_dataset.py) against what the unmodified reference's
HWDataset + collate produce on the fabricated IAM directory (tests/golden/hwdataset_index.json, tools/gen_golden_hwdataset.py), its routing
through getDataLoader, and the numpy restatement of the mesh warp (tests/_augment_ref.py) against the maps the reference's
grid_distortion.warp_image hands to cv2.remap (tests/golden/warp_maps.npz)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as R  # noqa: E402
from oracle import collate_items  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CHAR_FILE = os.path.join(ROOT, "handwriting_line_generation_amd", "data", "IAM_char_set.json")
WARP_CASES = ["w150", "w263", "w420", "w300_low"]


@pytest.fixture()
def iam_dir(tmp_path):
    root = str(tmp_path / "iam")
    os.makedirs(root)
    collate_items.fake_iam(root, with_images=True)
    return root


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("split", ["train", "valid", "test"])
def test_hwdataset_items_and_collate_equal_the_reference(iam_dir, split, center, monkeypatch):
    from handwriting_line_generation_amd.data import hw_dataset as D
    gold = json.load(open(os.path.join(GOLD, "hwdataset_index.json")))["splits"][split]["center" if center else "left"]
    resized = []
    real = D._resize
    monkeypatch.setattr(D, "_resize", lambda img, percent: (resized.append((list(img.shape[:2]), percent)), real(img, percent))[1])
    ds = D.HWDataset(iam_dir, split, {"img_height": 64, "char_file": CHAR_FILE, "center_pad": center, "augmentation": None})
    assert len(ds) == gold["len"] and [[a, l] for a, l in ds.lineIndex] == gold["lineIndex"]
    items = []
    for g in gold["items"]:
        del resized[:]
        it = ds[g["idx"]]
        items.append(it)
        author, line = ds.lineIndex[g["idx"]]
        assert it["name"] == g["name"] and it["gt"] == g["gt"] and it["author"] == g["author"] and it["center"] == g["center"]
        assert it["gt_label"].tolist() == g["label"]
        assert list(ds.authors[author][line][1]) == g["crop_box"]
        assert list(it["image"].shape) == g["image_shape"] and it["image"].dtype == np.float32
        assert float(it["image"].min()) >= 1 - 255 / 128 and float(it["image"].max()) <= 1
        calls = [c for c in g["calls"] if c[0] == "resize"]
        assert len(calls) == len(resized)
        for c, (shape, percent) in zip(calls, resized):       # ["resize", source shape, dsize, fx, fy, interpolation, [h, w]]
            assert c[1] == shape and c[3] == percent and c[4] == percent and c[5] == "INTER_CUBIC" and c[6] == g["image_shape"][:2]
    gc = gold["collate"]
    batch = D.collate([None if i is None else items[i] for i in gc["of"]])
    assert sorted(batch) == gc["keys"]
    img = batch["image"]
    assert list(img.shape) == gc["image_shape"] and str(img.numpy().dtype) == gc["image_dtype"]
    for b, (c0, c1) in enumerate(gc["valid_columns"]):
        assert bool((img[b, :, :, :c0] == -1).all()) and bool((img[b, :, :, c1:] == -1).all()) and bool((img[b, :, :, c0:c1] != -1).all())
        assert torch.equal(img[b, 0, :, c0:c1], torch.from_numpy(items[gc["of"][b]]["image"][:, :, 0]))
    assert batch["label"].tolist() == gc["label"] and str(batch["label"].dtype) == gc["label_dtype"] == "torch.int32"
    assert isinstance(batch["label_lengths"], torch.IntTensor) and batch["label_lengths"].tolist() == gc["label_lengths"]
    assert batch["gt"] == gc["gt"] and batch["name"] == gc["name"] and batch["author"] == gc["author"]


def test_hwdataset_quirks(iam_dir):
    from handwriting_line_generation_amd.data.hw_dataset import HWDataset, collate
    base = {"img_height": 64, "char_file": CHAR_FILE, "center_pad": False}
    assert len(HWDataset(iam_dir, "train", dict(base, overfit=True))) == 10
    # the reference looks the misspelt key up (hw_dataset.py:105): `add_spaces` alone changes nothing
    assert HWDataset(iam_dir, "train", dict(base, add_spaces=True))[0]["gt"] == HWDataset(iam_dir, "train", base)[0]["gt"]
    sp = HWDataset(iam_dir, "train", dict(base, add_spaces=True, add_spces=1))[0]["gt"]
    assert sp.startswith(" ") and sp.endswith(" ")
    ds = HWDataset(iam_dir, "train", base)
    author, line = ds.lineIndex[2]
    path, lb, _ = ds.authors[author][line]
    ds.authors[author][line] = (path, lb, "")            # an empty transcription: the item is None and collate drops it
    assert ds[2] is None
    assert len(collate([ds[0], ds[2], ds[1]])["gt"]) == 2
    assert all(ds.estimated_width(i) > 0 for i in range(len(ds)))


@pytest.mark.parametrize("aug", [True, "warp", "warp low", "normalization", 1])
def test_hwdataset_itself_never_augments(iam_dir, aug):
    from handwriting_line_generation_amd.data.hw_dataset import HWDataset
    with pytest.raises(NotImplementedError, match="augmentation"):
        HWDataset(iam_dir, "train", {"img_height": 64, "char_file": CHAR_FILE, "center_pad": False, "augmentation": aug})


def _hwr_config(iam_dir, **over):
    cfg = json.load(open(os.path.join(ROOT, "configs", "cf_IAM_hwr_cnnOnly_batchnorm_aug.json")))
    cfg["data_loader"].update(data_dir=iam_dir, char_file=CHAR_FILE, batch_size=4, num_workers=0)
    cfg["validation"].update(batch_size=3)
    cfg["data_loader"].update(over)
    return cfg


def test_getdataloader_serves_the_hwr_config(iam_dir):
    from handwriting_line_generation_amd.data.author_hw_dataset import ShardedLoader, getDataLoader
    from handwriting_line_generation_amd.data.hw_dataset import HWDataset
    cfg = _hwr_config(iam_dir, augmentation=None)
    assert cfg["data_loader"]["data_set_name"] == "HWDataset"
    cfg["cuda"] = False
    tl, vl = getDataLoader(cfg, "train")
    assert isinstance(tl, ShardedLoader) and isinstance(vl, ShardedLoader) and isinstance(tl.dataset, HWDataset)      # no augmentation wrapper
    assert tl.batch_size == 4 and vl.batch_size == 3 and len(tl) == 3 and len(vl) == 2
    n = 0
    for loader, bs in ((tl, 4), (vl, 3)):
        for inst in loader:       # what HWWithStyleTrainer.run_hwr / _valid_epoch read
            img, lab = inst["image"], inst["label"]
            assert img.dtype == torch.float32 and img.shape[:3] == (bs, 1, 64) and not img.is_cuda
            assert lab.dtype == torch.int32 and lab.shape[1] == bs and inst["label_lengths"].tolist() == [len(g) for g in inst["gt"]]
            assert int(lab.shape[0]) == max(len(g) for g in inst["gt"]) and len(inst["name"]) == len(inst["author"]) == bs
            n += 1
    assert n == 5
    # rank sharding and width bucketing as for the author datasets
    cfg["data_loader"]["width_bucket"] = 128
    a, _ = getDataLoader(cfg, "train", 0, 2)
    b, _ = getDataLoader(cfg, "train", 1, 2)
    na, nb = [i["name"] for i in a], [i["name"] for i in b]
    assert len(na) == len(nb) >= 1 and not set(sum(na, [])) & set(sum(nb, []))
    assert all(i["image"].shape[3] % 128 == 0 for i in a)


def test_getdataloader_refuses_device_augmentation_without_a_gpu(iam_dir, monkeypatch):
    from handwriting_line_generation_amd.data.author_hw_dataset import getDataLoader
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(NotImplementedError, match="augmentation"):
        getDataLoader(_hwr_config(iam_dir), "train")                 # augmentation: true as shipped, no GPU here


def test_getdataloader_refuses_device_augmentation_with_cuda_false(iam_dir):
    from handwriting_line_generation_amd.data.author_hw_dataset import getDataLoader
    cfg = _hwr_config(iam_dir)
    cfg["cuda"] = False
    with pytest.raises(NotImplementedError, match="augmentation"):
        getDataLoader(cfg, "train")
    cfg["data_loader"]["augmentation"] = "normalization"            # never routed to the GPU: the dataset refuses
    cfg["cuda"] = True
    with pytest.raises(NotImplementedError, match="augmentation"):
        getDataLoader(cfg, "train")


def test_device_variant_follows_the_reference():
    from handwriting_line_generation_amd.data.device_augment import device_variant as v
    assert [v("HWDataset", a) for a in (None, True, "warp", "warp low", "affine", "normalization", "normalization warp")] == [None, "full", "full", "low", None, None, None]
    for name in ("AuthorHWDataset", "AuthorRIMESLinesDataset"):
        assert [v(name, a) for a in (None, True, "warp", "low", "affine", "affine warp", "normalization")] == [None, "full", "full", "full", None, None, None]


# ---- the mesh warp restatement against the reference's maps --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WARP_CASES)
def test_restated_map_equals_the_reference_map(case):
    from handwriting_line_generation_amd import ops
    g = np.load(os.path.join(GOLD, "warp_maps.npz"))
    img, src, dst = g[case + "/image"], g[case + "/source"], g[case + "/destination"]
    gy, gx = (int(v) for v in g[case + "/grid"])
    H, W = img.shape
    sy, sx = R.lattice(H, W)
    py, px = ops.warp_lattice(H, W)
    assert len(sy) == gy and len(sx) == gx and np.array_equal(sy, py) and np.array_equal(sx, px)
    S = src.reshape(gy, gx, 2)
    assert np.array_equal(S[:, :, 0], np.broadcast_to(sy[:, None], (gy, gx))) and np.array_equal(S[:, :, 1], np.broadcast_to(sx[None, :], (gy, gx)))
    disp = (dst - src).reshape(gy, gx, 2)
    mp = R.warp_map(H, W, sy, sx, disp[:, :, 0], disp[:, :, 1], np.float64)
    inside = mp["inside"]
    assert inside.mean() >= 0.97
    gold_y, gold_x = g[case + "/map_y"], g[case + "/map_x"]
    assert gold_y.dtype == np.float32 and int(g[case + "/interpolation"]) == 1
    assert not np.isnan(gold_y[inside]).any() and not np.isnan(gold_x[inside]).any()     # the lattice mesh lies inside the reference's hull
    worst = 0.0
    for mine, gold in ((mp["map_y"], gold_y), (mp["map_x"], gold_x)):
        d = np.abs(mine[inside].astype(np.float32).astype(np.float64) - gold[inside].astype(np.float64))
        ulp = np.spacing(np.abs(gold[inside])).astype(np.float64)
        worst = max(worst, float((d / ulp).max()))
        assert (d <= ulp).all(), (case, float((d / ulp).max()))
    print(case, "inside %.4f" % inside.mean(), "worst difference %.2f ulp (float32)" % worst)
    # the border level: the mean the reference hands to remap, saturated to a level
    t, lut, m = R.stats(img.astype(np.int64), 0.0, 0.0)
    assert np.array_equal(lut, np.arange(256)) and m == int(np.rint(float(g[case + "/border_value"][0])))


def test_brightness_lut_is_the_reference_arithmetic():
    """augmentation.py:11-22 on arrays (float32 image + (1 - th) * fg + th * bg, clamp, astype(uint8)) == the per-level LUT"""
    rs = np.random.RandomState(3)
    img = np.concatenate([rs.randint(0, 90, size=(20, 300)), rs.randint(170, 256, size=(44, 300))]).astype(np.uint8)
    for fg, bg in ((12.3456789, -40.25), (-70.5, 61.999), (300.0, -300.0), (0.0, 0.0)):
        t, lut, m = R.stats(img.astype(np.int64), fg, bg)
        th = (img > t).astype(np.float32)[..., None]
        x = img[..., None].astype(np.float32)
        x = x + (1.0 - th) * fg
        x = x + th * bg
        x[x > 255] = 255
        x[x < 0] = 0
        want = x.astype(np.uint8)[..., 0]
        assert np.array_equal(lut[img], want)
        assert m == int(np.rint(want.mean()))
        assert 89 <= t < 170 and R.split_margin(np.bincount(img.reshape(-1), minlength=256)) > 0
