"""CPU: the warp mode of the device-resident line store (`data_loader.device_store: "warp"`) without a device - (a) the refusals of
getDataLoader on a path that needs no data; (b) the pool of HWDataset lines against dataset[i], one decode per page, the cache file and its
separation from the author datasets' caches; (c) StoreLoader's host side with a stub in place of the launch against hw_dataset.collate +
pad_width: labels, names, W and the lines' extents; (d) the two entry points' refusals in front of their launches."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _line_store_warp_ref as S  # noqa: E402


# ---- (a) routing -----------------------------------------------------------------------------------------------------------------------
def test_get_data_loader_refuses_the_warp_mode_with_the_reason(tmp_path):
    from handwriting_line_generation_amd.data import author_hw_dataset as D

    def cfg(name, **dl):
        return {"cuda": True, "data_loader": dict(dl, data_set_name=name, data_dir=str(tmp_path / "nothing_here"), batch_size=1, device_store="warp")}
    # an augmentation value that is None, affine-only or "normalization"
    for name, augs in (("HWDataset", (None, "affine", "low", "normalization", "warp normalization")),
                       ("AuthorHWDataset", (None, "affine", "affine warp", "normalization")),
                       ("AuthorRIMESLinesDataset", (None, "affine", "normalization"))):
        for aug in augs:
            with pytest.raises(NotImplementedError, match='device_store: "warp" with augmentation=.*brightness \\+ mesh-warp'):
                D.getDataLoader(cfg(name, augmentation=aug), "train")
    with pytest.raises(NotImplementedError, match='device_store: "warp" with augmentation=None'):       # the validation config's own value counts too
        D.getDataLoader(dict(cfg("HWDataset", augmentation=True), validation={"augmentation": None}), "train")
    with pytest.raises(NotImplementedError, match='device_store with "cuda": false'):
        D.getDataLoader(dict(cfg("HWDataset", augmentation=True), cuda=False), "train")
    with pytest.raises(NotImplementedError, match='device_store with "cuda": false'):
        D.getDataLoader(dict(cfg("AuthorRIMESLinesDataset", augmentation="warp"), cuda=False), "valid")
    # the foreground-only loss in effect: no warped masks
    masked = dict(cfg("AuthorHWDataset", augmentation="warp", fg_masks_dir=str(tmp_path / "fg")), trainer={"no_bg_loss": True}, no_bg_loss=True)
    with pytest.raises(NotImplementedError, match='device_store: "warp" with no_bg_loss / fg_masks_dir in effect'):
        D.getDataLoader(masked, "train")
    # `true` keeps its refusals (tests/test_line_store_cpu.py pins them); the ones the new value would serve say so
    with pytest.raises(NotImplementedError, match='author-grouped line datasets.*not HWDataset.*device_store: "warp"'):
        D.getDataLoader({"cuda": True, "data_loader": dict(cfg("HWDataset", augmentation=True)["data_loader"], device_store=True)}, "train")
    with pytest.raises(NotImplementedError, match='affine augmentation only.*device_store: "warp"'):
        D.getDataLoader({"cuda": True, "data_loader": dict(cfg("AuthorRIMESLinesDataset", augmentation="warp")["data_loader"], device_store=True)}, "train")
    assert not os.path.exists(str(tmp_path / "nothing_here"))


# ---- (b) the pool of HWDataset lines ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iam_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("warp_store") / "iam")
    S.fabricate("iam", root)
    return root


def _hw(iam_dir, center=False, **extra):
    from handwriting_line_generation_amd.data.hw_dataset import HWDataset
    from handwriting_line_generation_amd.harness import CHAR_FILES
    return HWDataset(iam_dir, "train", dict(img_height=64, char_file=CHAR_FILES["iam"], center_pad=center, augmentation=None, **extra))


def test_pool_holds_every_hwdataset_line_as_getitem_makes_it(iam_dir, tmp_path, monkeypatch):
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.author_hw_dataset import AuthorHWDataset
    from handwriting_line_generation_amd.data.line_store import LineStore
    from handwriting_line_generation_amd.harness import CHAR_FILES
    ds = _hw(iam_dir)
    want = [ds[i]["image"] for i in range(len(ds))]          # (before the spy: the dataset's own page cache)
    opened = []
    plain = D._read_gray
    monkeypatch.setattr(D, "_read_gray", lambda path: (opened.append(path), plain(path))[1])
    store = LineStore(ds, None)
    pages = {ds.authors[a][l][0] for a, l in ds.lineIndex}
    assert sorted(opened) == sorted(pages) and len(store.widths) == len(ds) > 6       # every page once
    resized = 0
    for i, (author, line) in enumerate(ds.lineIndex):
        got = store.line(author, line)
        assert got.dtype == np.uint8 and got.shape == want[i].shape[:2] and got.shape[0] == 64
        assert np.array_equal(got.astype(np.float32), (1 - want[i][:, :, 0]) * 128), (i, author, line)
        lb = ds.authors[author][line][1]
        resized += (lb[1] - max(lb[0], 0)) != 64
    assert resized > 0, "no line went through the resize"
    # the cache round-trips, and a cache written for AuthorHWDataset is not picked up
    cache = str(tmp_path / "pool_cache")
    first = LineStore(ds, None, cache)
    assert not first.from_cache and os.listdir(cache) == [os.path.basename(first.cache_file)]
    del opened[:]
    second = LineStore(_hw(iam_dir), None, cache)
    assert not opened and second.from_cache and second.cache_file == first.cache_file
    assert np.array_equal(second.pixels, store.pixels) and np.array_equal(second.widths, store.widths) and np.array_equal(second.offsets, store.offsets)
    ads = AuthorHWDataset(iam_dir, "train", dict(img_height=64, a_batch_size=1, char_file=CHAR_FILES["iam"], max_width=10 ** 6, augmentation=None))
    other = LineStore(ads, None, cache)
    assert opened and not other.from_cache and other.cache_file != first.cache_file and len(os.listdir(cache)) == 2
    del opened[:]
    third = LineStore(_hw(iam_dir), None, cache)             # with the author datasets' file next to it
    assert not opened and third.from_cache and np.array_equal(third.pixels, store.pixels)


# ---- (c) the host side ----------------------------------------------------------------------------------------------------------------------
def _stub(loader):
    calls = []

    def launch(lines, mesh, W):
        calls.append((list(lines), list(mesh.x_off), list(mesh.widths), W))
        return torch.zeros((len(lines), 1, loader.store.height, W))
    loader._launch_warp = launch
    return calls


@pytest.mark.parametrize("center,width_bucket", [(False, 0), (True, 0), (True, 96), (False, 96)])
def test_host_side_equals_collate_and_pad_width(iam_dir, center, width_bucket):
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.device_augment import line_extents
    from handwriting_line_generation_amd.data.line_store import StoreLoader
    ds = _hw(iam_dir, center)
    author, line = ds.lineIndex[2]                          # one line without a transcription: collate drops its item
    path, lb, _ = ds.authors[author][line]
    ds.authors[author][line] = (path, lb, "")
    host = D.ShardedLoader(ds, 4, True, 0, seed=3, width_bucket=width_bucket)
    store = StoreLoader(ds, 4, True, 0, seed=3, width_bucket=width_bucket, device=None, variant="low")
    calls = _stub(store)
    assert len(store) == len(host) and store.dataset is ds
    dropped = shifted = 0
    for epoch in range(2):
        want = list(host)
        random.seed(4 + epoch)
        del calls[:]
        got = list(store)
        flips = random.random()
        assert len(got) == len(want) == len(calls) >= 2 and store.epoch == host.epoch
        n_lines = 0
        for g, w, (lines, x_off, widths, W) in zip(got, want, calls):
            assert set(w) <= set(g) and set(g) - set(w) == {"line_extents"}
            for key in ("gt", "name", "author"):
                assert g[key] == w[key], key
            for key in ("label", "label_lengths"):
                assert g[key].dtype == w[key].dtype and torch.equal(g[key], w[key]), key
            assert g["image"].shape == w["image"].shape and W == w["image"].shape[3]
            if width_bucket:
                assert W % width_bucket == 0
            first, valid = line_extents(w["image"])
            assert x_off == first.tolist() and widths == valid.tolist(), (x_off, first, widths, valid)
            assert g["line_extents"] == (x_off, widths)
            assert [store.store.index[(n.rsplit("_", 1)[0], int(n.rsplit("_", 1)[1]))] for n in g["name"]] == lines
            dropped += len(lines) < 4
            shifted += any(o > 0 for o in x_off)
            n_lines += len(lines)
        random.seed(4 + epoch)                              # the "low" variant's coin flips: two per remaining line, nothing else
        for _ in range(2 * n_lines):
            random.random()
        assert random.random() == flips
    assert dropped > 0
    assert (shifted > 0) == center


def test_author_datasets_go_through_the_existing_host_batch(tmp_path):
    from handwriting_line_generation_amd.data.author_rimeslines_dataset import AuthorRIMESLinesDataset
    from handwriting_line_generation_amd.data.line_store import StoreLoader
    from handwriting_line_generation_amd.harness import CHAR_FILES
    root = str(tmp_path / "rimes")
    S.fabricate("rimes", root)
    ds = AuthorRIMESLinesDataset(root, "train", dict(img_height=64, a_batch_size=2, char_file=CHAR_FILES["rimes"], max_width=2000, augmentation=None))
    store = StoreLoader(ds, 2, False, 0, device=None, variant="full")
    calls = _stub(store)
    state = np.random.RandomState(1).get_state()
    np.random.set_state(state)
    got = list(store)
    assert np.random.get_state()[2] == state[2]             # no numpy draw on the host side (strech 1, m 0: nothing is drawn for them)
    assert len(got) == len(calls) >= 1
    for g, (lines, x_off, widths, W) in zip(got, calls):
        assert x_off == [0] * len(lines) and widths == [int(store.store.widths[k]) for k in lines] and W == max(widths)
        assert g["a_batch_size"] == 2 and len(g["name"]) == len(lines)


# ---- (d) the entry points -------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch():
    """the checks run on the host side of the entry points, in front of the launch: with arguments they refuse, the call returns its status
    without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20          # any 16-byte aligned address
    good = dict(pixels=p, pixel_bytes=4096, offsets=p, widths=p, n_lines=3, H=64, thr=p, hist=p, stream=0)

    def args(**kw):
        return tuple(kw.get(k, v) for k, v in good.items())
    for a, word in [(args(pixels=None), "null"), (args(offsets=None), "null"), (args(widths=None), "null"), (args(thr=None), "null"),
                    (args(hist=None), "null"), (args(n_lines=0), "bad sizes"), (args(pixel_bytes=0), "bad sizes"), (args(H=0), "bad sizes"),
                    (args(offsets=p + 4), "aligned"), (args(hist=p + 2), "aligned")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_store_line_stats", *a)
        assert word in str(e.value), (a, str(e.value))
    good = dict(pixels=p, pixel_bytes=4096, offsets=p, widths=p, n_lines=3, thr=p, hist=p, line=p, lines_i=p, lines_f=p, lf_stride=4 + 7 + 9,
                draws=p, draw_stride=2 + 2 * 7 * 9, B=2, H=64, W=101, GY=7, GX=9, out=p, map_out=p, out_elems=2 * 64 * 101, stream=0)
    for a, word in [(args(pixels=None), "null"), (args(offsets=None), "null"), (args(widths=None), "null"), (args(thr=None), "null"),
                    (args(hist=None), "null"), (args(line=None), "null"), (args(lines_i=None), "null"), (args(lines_f=None), "null"),
                    (args(draws=None), "null"), (args(out=None), "null"), (args(B=0), "bad sizes"), (args(H=0), "bad sizes"),
                    (args(W=0), "bad sizes"), (args(n_lines=0), "bad sizes"), (args(pixel_bytes=0), "bad sizes"), (args(B=65536), "too large"),
                    (args(GY=17, lf_stride=64, draw_stride=1024), "lattice"), (args(GY=-1), "lattice"), (args(GX=-1), "lattice"),
                    (args(lf_stride=19), "strides too small"), (args(draw_stride=127), "strides too small"), (args(offsets=p + 4), "aligned"),
                    (args(out=p + 2), "aligned"), (args(map_out=p + 1), "aligned"), (args(lines_f=p + 3), "aligned"),
                    (args(out_elems=2 * 64 * 101 - 1), "needs"), (args(B=65535, H=1 << 30, W=1 << 30, out_elems=1 << 62), "does not fit")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_store_warp_batch", *a)
        assert word in str(e.value), (a, str(e.value))
