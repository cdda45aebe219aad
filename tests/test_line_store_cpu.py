"""CPU: the device-resident line store without a device - (a) the fp64 restatement of hwg_store_batch (tests/_line_store_ref.py) against the
bytes of the line and against the host path's affine_trans (PIL); (b) StoreLoader's host side on a fabricated IAM directory with a stub in
place of the launch: the row tables against what dataset[idx] draws and produces, the instance fields against collate; (c) the pool cache
file; (d) the refusals of getDataLoader and of the entry point in front of its launch.

Bound of (a): on a pixel whose two source columns are inside the line both sides blend the same two bytes with weights that differ by the
rounding of PIL's fixed-point coordinate; PIL truncates the blend where cv2.warpAffine (and the restatement) rounds to nearest -> at most 1
level (measured on exactly these cases: maximum 1 over 1.4 M interior pixels, about 40 % of them differ by that level). Pixels with a
source column outside the line differ by design: PIL fills, cv2 blends the border in."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _line_store_ref as R  # noqa: E402

WIDTHS = (1, 3, 5, 64, 65, 257, 900)
STRECH = (0.6, 1.0, 1.37, 1.4)
SKEW = (0.0, 0.3, math.pi / 4, -math.pi / 4)


def _line(w, H=64):
    return np.random.RandomState(1000 + w).randint(0, 256, (H, w)).astype(np.uint8)


@pytest.mark.parametrize("w", WIDTHS)
def test_restatement_at_rest_returns_the_bytes(w):
    img = _line(w)
    img[:, 0], img[:, -1] = 0, 255 if w > 1 else 0
    assert np.array_equal(R.warp_levels(img, w, 1.0, R.tan(0.0)), img)
    assert np.array_equal(R.warp_line(img, w, 1.0, 0.0), np.float32(1.0) - img.astype(np.float32) / np.float32(128.0))
    mask = np.where(img > 100, 255, 0).astype(np.uint8)
    assert np.array_equal(R.warp_mask(mask, w, 1.0, 0.0), (mask / 255).astype(np.float32))


@pytest.mark.parametrize("w", WIDTHS)
def test_restatement_within_one_level_of_affine_trans_inside_the_line(w):
    from handwriting_line_generation_amd.data.author_hw_dataset import affine_trans
    img = _line(w)
    seen = 0
    for strech in STRECH:
        for skew in SKEW:
            pil = affine_trans(img, skew, strech)
            got, interior = R.warp_levels(img, int(w * strech), strech, R.tan(skew), want_interior=True)
            assert got.shape == pil.shape == (64, int(w * strech)), (w, strech, skew, got.shape, pil.shape)
            d = np.abs(got.astype(np.int64) - pil.astype(np.int64))[interior]
            seen += d.size
            worst = int(d.max()) if d.size else 0
            print("w %4d strech %.2f skew %+.3f: %7d interior pixels, max |restatement - PIL| %d" % (w, strech, skew, d.size, worst))
            assert worst <= 1, (w, strech, skew, worst)
    assert seen > 0 or w == 1               # a line of one column has no pixel with both columns inside


# ---- (b) StoreLoader's host side ---------------------------------------------------------------------------------------------------------
def _dataset(tmp_path, augmentation="affine", max_width=300, **extra):
    from oracle import collate_items
    from handwriting_line_generation_amd.data.author_hw_dataset import AuthorHWDataset
    from handwriting_line_generation_amd.harness import CHAR_FILES
    root = str(tmp_path / "iam")
    if not os.path.exists(root):
        os.makedirs(root)
        collate_items.fake_iam(root, n_pages=6, with_images=True)
    cfg = dict(img_height=64, a_batch_size=2, char_file=CHAR_FILES["iam"], max_width=max_width, augmentation=augmentation, **extra)
    return AuthorHWDataset(root, "train", cfg)


def _stub(loader):
    calls = []

    def launch(rows, W):
        calls.append((list(rows), W))
        return torch.zeros((len(rows), 1, loader.store.height, W))
    loader._launch = launch
    return calls


def _same_fields(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key in ("mask", "top_and_bottom", "center_line", "style", "spaced_label"):
        assert got[key] is None and want[key] is None, key
    for key in ("gt", "name", "author", "author_idx", "a_batch_size"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ("label", "label_lengths"):
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    assert got["image"].shape == want["image"].shape, (got["image"].shape, want["image"].shape)


@pytest.mark.parametrize("batch_size,width_bucket", [(2, 0), (1, 0), (2, 128)])
def test_store_loader_tables_and_fields_equal_the_host_path(tmp_path, monkeypatch, batch_size, width_bucket):
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.line_store import StoreLoader
    ds = _dataset(tmp_path)
    if batch_size == 2:                     # one line without a transcription: its item is dropped by collate, after its draws
        author, lines = ds.lineIndex[1]
        path, lb, _ = ds.authors[author][lines[0]]
        ds.authors[author][lines[0]] = (path, lb, "")
    warps = []
    plain = D.affine_trans

    def spy(img, skew, strech, fg_mask=None):
        out = plain(img, skew, strech, fg_mask)
        warps.append((img.copy(), skew, strech, out.shape[1]))
        return out
    monkeypatch.setattr(D, "affine_trans", spy)
    host = D.ShardedLoader(ds, batch_size, True, 0, seed=3, width_bucket=width_bucket)
    store = StoreLoader(ds, batch_size, True, 0, seed=3, width_bucket=width_bucket, device=None)
    calls = _stub(store)
    assert len(store) == len(host) and store.dataset is ds and store.batch_size == batch_size
    clamped = dropped = 0
    for epoch in range(2):
        np.random.seed(11 + epoch)
        del warps[:]
        want = list(host)
        host_warps = list(warps)
        np.random.seed(11 + epoch)
        del calls[:]
        got = list(store)
        assert store.epoch == host.epoch == epoch + 1 and len(got) == len(want) == len(calls) >= 2
        rows = [r for c, _ in calls for r in c]
        names = [n for inst in got for n in inst["name"]]
        # a dropped item warps the lines in front of its empty one on the host before it is dropped: those calls have no row
        kept = []
        for inst in want:
            kept += list(inst["name"])
        assert names == kept
        hw = iter(host_warps)
        for (k, out_w, strech, m), name in zip(rows, names):
            author, line = name.rsplit("_", 1)
            fitted = store.store.line(author, int(line))
            for img, skew, s, w_out in hw:      # skip the warps of dropped items
                if img.shape == fitted.shape and np.array_equal(img, fitted):
                    break
            else:
                raise AssertionError("no host warp for %s" % name)
            assert store.store.index[(author, int(line))] == k
            assert (out_w, strech, m) == (w_out, s, math.tan(skew)), (name, out_w, strech, m, w_out, s, math.tan(skew))
            clamped += strech == ds.max_width / fitted.shape[1] and out_w <= ds.max_width
        for g, w, (c, W) in zip(got, want, calls):
            _same_fields(g, w)
            assert W == w["image"].shape[3] and len(c) == w["image"].shape[0]
            dropped += len(c) < batch_size * ds.batch_size
            if batch_size == 1:
                assert g["a_batch_size"] == ds.batch_size and g["label"].shape[1] == ds.batch_size
    assert clamped > 0, "no item went through the max_width clamp"
    assert dropped > 0 or batch_size == 1


def test_store_loader_consumes_the_draws_of_the_host_path(tmp_path):
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.line_store import StoreLoader
    ds = _dataset(tmp_path)
    host = D.ShardedLoader(ds, 2, False, 0)
    store = StoreLoader(ds, 2, False, 0, device=None)
    _stub(store)
    np.random.seed(5)
    list(host)
    after_host = np.random.random()
    np.random.seed(5)
    list(store)
    assert np.random.random() == after_host
    # no augmentation: no draw, the line's own width, strech 1 and m 0
    plain = StoreLoader(_dataset(tmp_path, augmentation=None), 2, False, 0, device=None)
    calls = _stub(plain)
    np.random.seed(5)
    first = np.random.RandomState(5).random_sample()
    list(plain)
    assert np.random.random() == first
    for rows, W in calls:
        assert all(s == 1.0 and m == 0.0 and ow == plain.store.widths[k] for k, ow, s, m in rows) and W == max(r[1] for r in rows)


# ---- (c) the pool cache file --------------------------------------------------------------------------------------------------------------
def test_pool_cache_is_loaded_without_opening_a_page(tmp_path, monkeypatch):
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.line_store import LineStore
    opened = []
    plain = D._read_gray
    monkeypatch.setattr(D, "_read_gray", lambda path: (opened.append(path), plain(path))[1])
    cache = str(tmp_path / "pool_cache")
    ds = _dataset(tmp_path)
    first = LineStore(ds, None, cache)
    pages = {ds.authors[a][l][0] for a, l in first.index}
    assert sorted(opened) == sorted(pages) and not first.from_cache          # every page once
    assert os.listdir(cache) == [os.path.basename(first.cache_file)] and first.cache_file.endswith(".npz")
    for (author, line), k in first.index.items():
        path, lb, _ = ds.authors[author][line]
        assert np.array_equal(first.line(author, line), ds._fit(plain(path)[max(lb[0], 0):lb[1], max(lb[2], 0):lb[3]]))
    del opened[:]
    second = LineStore(_dataset(tmp_path), None, cache)
    assert not opened and second.from_cache and second.cache_file == first.cache_file
    assert np.array_equal(second.pixels, first.pixels) and np.array_equal(second.widths, first.widths) and np.array_equal(second.offsets, first.offsets)
    other = LineStore(_dataset(tmp_path, max_width=280), None, cache)
    assert opened and not other.from_cache and other.cache_file != first.cache_file and len(os.listdir(cache)) == 2
    assert int(other.widths.max()) <= 280 < int(first.widths.max())
    without = LineStore(ds, None)
    assert without.cache_file is None and np.array_equal(without.pixels, first.pixels)


# ---- (d) refusals --------------------------------------------------------------------------------------------------------------------------
def test_get_data_loader_refuses_with_the_reason(tmp_path):
    from handwriting_line_generation_amd.data import author_hw_dataset as D

    def cfg(name, **dl):
        return {"cuda": True, "data_loader": dict(dl, data_set_name=name, data_dir=str(tmp_path / "nothing_here"), batch_size=1, device_store=True)}
    with pytest.raises(NotImplementedError, match="author-grouped line datasets.*not HWDataset"):
        D.getDataLoader(cfg("HWDataset"), "train")
    for name in ("AuthorHWDataset", "AuthorRIMESLinesDataset"):
        for aug in (True, "warp", "affine warp", "low"):
            with pytest.raises(NotImplementedError, match="device_store with augmentation=.*affine augmentation only"):
                D.getDataLoader(cfg(name, augmentation=aug), "train")
    with pytest.raises(NotImplementedError, match="affine augmentation only"):         # the validation config's own value counts too
        D.getDataLoader(dict(cfg("AuthorHWDataset", augmentation="affine"), validation={"augmentation": "warp"}), "train")
    with pytest.raises(NotImplementedError, match='device_store with "cuda": false'):
        D.getDataLoader(dict(cfg("AuthorHWDataset", augmentation="affine"), cuda=False), "train")
    with pytest.raises(NotImplementedError, match='device_store with "cuda": false'):
        D.getDataLoader(dict(cfg("AuthorHWDataset"), cuda=False), "valid")


def test_store_batch_entry_point_refuses_bad_arguments_before_any_launch():
    """the checks run on the host side of the entry point, in front of the launch: with arguments they refuse, the call returns its status
    without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20          # any 16-byte aligned address
    good = dict(pixels=p, masks=p, pixel_bytes=4096, offsets=p, widths=p, n_lines=1, line=p, out_w=p, strech=p, m=p, B=2, H=7, W=5, out=p,
                out_mask=p, out_elems=72, stream=0)

    def args(**kw):
        return tuple(kw.get(k, v) for k, v in good.items())
    for a, word in [(args(pixels=None), "null"), (args(offsets=None), "null"), (args(widths=None), "null"), (args(line=None), "null"),
                    (args(out_w=None), "null"), (args(strech=None), "null"), (args(m=None), "null"), (args(out=None), "null"),
                    (args(masks=None), "go together"), (args(out_mask=None), "go together"), (args(B=0), "bad sizes"), (args(H=0), "bad sizes"),
                    (args(W=0), "bad sizes"), (args(n_lines=0), "bad sizes"), (args(pixel_bytes=0), "bad sizes"), (args(out=p + 4), "aligned"),
                    (args(out_mask=p + 8), "aligned"), (args(strech=p + 4), "aligned"), (args(out_elems=71), "rounded up to 4"),
                    (args(out_elems=70), "rounded up to 4"), (args(B=1 << 30, H=1 << 30, W=1 << 30, out_elems=1 << 62), "does not fit")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_store_batch", *a)
        assert word in str(e.value), (a, str(e.value))
