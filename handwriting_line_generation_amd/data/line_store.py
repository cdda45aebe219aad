"""Device-resident line store for the author-grouped line datasets (`data_loader.device_store: true`, off by default).

The host path decodes a whole form page per line in DataLoader workers (AuthorHWDataset.__getitem__: crop, PIL resize, PIL affine warp,
1 - p / 128, pad; collate pads again; the trainer uploads fp32) - a GAN step consumes batch_size * a_batch_size lines in about 10 ms, a page
decode alone costs about ten times that. With the store the split's fitted lines are decoded ONCE (LineStore: grouped by page, the dataset's
own `_fit`), live in GPU memory as one ragged uint8 pool (the layout of ops.fg_masks; a second pool holds the cached foreground masks when
the foreground-only loss is on), and every batch is one table upload and one launch (ops.store_batch, csrc/line_store.hip): the affine warp
of the reference's augmentation.affine_trans in cv2.warpAffine's arithmetic, 1 - p / 128, the collate padding and the warped mask.

StoreLoader has ShardedLoader's surface and its `_batches()`: rank sharding, width bucketing and the epoch order are unchanged. Per batch
it restates the host side of __getitem__ and collate without touching a pixel: the two np.random.random() draws per item (strech, then
skew) in the main process in batch order, the sequential max_width clamp over the author's lines, out_w = int(width * strech), items
with an empty transcription dropped after their draws, labels / names / authors built on the host as before.

`device_store: "warp"` is the same store for recogniser pre-training (HWDataset and the author datasets with an `augmentation` value that
means brightness + mesh warp, data/device_augment.py): HWDataset's lines are stored as its __getitem__ makes them, the Otsu level and the
histogram of every line are computed once when the pool is built (ops.store_line_stats), and a batch is one table upload and one launch
(ops.store_warp_batch, csrc/store_warp.hip) that equals DeviceAugment over ShardedLoader bit for bit - no decoded page, no collated fp32
batch, no image upload, no statistics launch. The host side restates hw_dataset.collate (or the author datasets' collate with strech 1,
m 0) without touching a pixel and consumes `random`, numpy's generator and the device generator exactly as DeviceAugment does."""
import hashlib
import json
import logging
import math
import os
import time

import numpy as np
import torch

from ..utils import string_utils
from . import author_hw_dataset as D
from . import fg_masks

REFUSAL_DATASET = ("data_loader.device_store: the device-resident line store serves the author-grouped line datasets (AuthorHWDataset, "
                   "AuthorRIMESLinesDataset), not %s")
REFUSAL_AUG = ("data_loader.device_store with augmentation=%r: the store's kernel executes the affine augmentation only (None or 'affine'); "
               "the brightness / mesh-warp augmentation of the author datasets is not moved to the device")
REFUSAL_WARP_HINT = '; data_loader.device_store: "warp" serves that augmentation'
REFUSAL_WARP_DATASET = ('data_loader.device_store: "warp" serves HWDataset, AuthorHWDataset and AuthorRIMESLinesDataset, not %s')
REFUSAL_WARP_AUG = ('data_loader.device_store: "warp" with augmentation=%r: this mode executes the brightness + mesh-warp augmentation; for None or '
                    "'affine' use device_store: true, and 'normalization' is not implemented")
REFUSAL_WARP_MASKS = ('data_loader.device_store: "warp" with no_bg_loss / fg_masks_dir in effect: the warp path produces no warped foreground '
                      "masks (the reference's has none either)")
REFUSAL_CUDA = 'data_loader.device_store with "cuda": false: the lines live in GPU memory and are collated by a GPU kernel, there is no CPU execution'


def check_config(data_set_name, cfgs, device):
    """the refusals of getDataLoader for the loader configs that carry `device_store`, before anything is built"""
    from .device_augment import device_variant
    if any(cfg["device_store"] == "warp" for cfg in cfgs):
        if data_set_name not in ("HWDataset", "AuthorHWDataset", "AuthorRIMESLinesDataset"):
            raise NotImplementedError(REFUSAL_WARP_DATASET % data_set_name)
        for cfg in cfgs:
            if cfg["device_store"] == "warp" and device_variant(data_set_name, cfg.get("augmentation")) is None:
                raise NotImplementedError(REFUSAL_WARP_AUG % (cfg.get("augmentation"),))
    for cfg in cfgs:
        if cfg["device_store"] == "warp":
            continue
        if data_set_name not in ("AuthorHWDataset", "AuthorRIMESLinesDataset"):
            raise NotImplementedError(REFUSAL_DATASET % data_set_name + (REFUSAL_WARP_HINT if data_set_name == "HWDataset" else ""))
        aug = cfg.get("augmentation")
        if aug is not None and aug != "affine":
            raise NotImplementedError(REFUSAL_AUG % (aug,) + (REFUSAL_WARP_HINT if device_variant(data_set_name, aug) else ""))
    if device is None or not torch.cuda.is_available():
        raise NotImplementedError(REFUSAL_CUDA)


def _single(dataset):
    """True for a dataset whose items are single lines (HWDataset: lineIndex holds (author, line)), False for the author-grouped ones"""
    return bool(dataset.lineIndex) and not isinstance(dataset.lineIndex[0][1], (list, tuple))


def _keys(dataset):
    """every distinct (author, line) the dataset's items use, in item order"""
    if not _single(dataset):
        return list(fg_masks._lines(dataset))                  # with the (line + 37) % len wrap of the author datasets
    return list(dict.fromkeys((author, int(line)) for author, line in dataset.lineIndex))


def _fit_single(dataset, img):
    """HWDataset.__getitem__'s height normalisation: one uniform factor, no max_width, no vertical padding"""
    if img.shape[0] != dataset.img_height:
        img = D._resize(img, float(dataset.img_height) / img.shape[0])
    return img


def _resolve(dataset, author, line):
    """the dataset's own wrap of a line index past the author's lines (__getitem__)"""
    n = len(dataset.authors[author])
    return (line + 37) % n if line >= n else line


class LineStore:
    """The fitted lines of `dataset` as one ragged uint8 pool: `.index[(author, line)]` -> k, `.widths[k]`, `.offsets[k]`, host `.pixels`
    (and `.masks` when dataset.fg_masks_dir is set), and `.pool`, the ops.LinePool on `device` (None: host arrays only, nothing can be
    launched). The author datasets' lines are fitted by their `_fit`, HWDataset's as its __getitem__ makes them (crop, one uniform resize
    to img_height). cache_dir: the pixel pool is kept there as .npz under a digest of (page paths, boxes, img_height, max_width) - for
    HWDataset of (page paths, boxes, img_height, no max_width, the name of its fit), so a pool cached for one kind of dataset is never
    loaded for the other; a file whose digest matches is loaded instead of decoding."""

    def __init__(self, dataset, device, cache_dir=None):
        t0 = time.perf_counter()
        self.height = H = dataset.img_height
        keys = _keys(dataset)                                  # distinct (author, line) in item order
        if not keys:
            raise ValueError("device_store: the dataset has no lines")
        self.index = {k: i for i, k in enumerate(keys)}
        self.cache_file, self.from_cache = None, False
        lines = None
        if cache_dir:
            spec = [[dataset.authors[a][l][0], [int(v) for v in dataset.authors[a][l][1]]] for a, l in keys]
            what = [spec, int(H), None, "HWDataset.__getitem__"] if _single(dataset) else [spec, int(H), dataset.max_width]
            digest = hashlib.sha256(json.dumps(what, sort_keys=True).encode()).hexdigest()[:24]
            self.cache_file = os.path.join(cache_dir, "line_store_%s.npz" % digest)
            lines = self._load(len(keys))
        if lines is None:
            lines = self._decode(dataset, keys)
            if self.cache_file:
                self._save(lines)
        else:
            self.from_cache = True
        self.widths = np.array([img.shape[1] for img in lines], dtype=np.int64)
        self.offsets = np.zeros(len(lines), dtype=np.int64)
        np.cumsum(H * self.widths[:-1], out=self.offsets[1:])
        self.pixels = np.concatenate([img.reshape(-1) for img in lines])
        self.masks = None
        if getattr(dataset, "fg_masks_dir", None) is not None:
            from PIL import Image
            parts = []
            for (author, line), img in zip(keys, lines):
                path = fg_masks.mask_path(dataset, author, line)
                mask = np.asarray(Image.open(path).convert("L"))
                if mask.shape != img.shape:
                    raise ValueError("device_store: foreground mask %s is %s, its line %s" % (path, mask.shape, img.shape))
                parts.append(mask.reshape(-1))
            self.masks = np.concatenate(parts)
        self.pool = None
        if device is not None:
            from .. import ops
            self.pool = ops.LinePool(ops.h2d(torch.from_numpy(self.pixels), device), self.offsets, self.widths, height=H,
                                     masks=None if self.masks is None else ops.h2d(torch.from_numpy(self.masks), device))
        self.build_s = time.perf_counter() - t0
        logging.getLogger("LineStore").info("device store: %d lines, %d bytes%s, built in %.2f s%s", len(lines), self.pixels.size,
                                            "" if self.masks is None else " (+ as many of masks)", self.build_s,
                                            " (pool loaded from %s)" % self.cache_file if self.from_cache else "")

    @staticmethod
    def _decode(dataset, keys):
        fit = (lambda img: _fit_single(dataset, img)) if _single(dataset) else dataset._fit
        by_page = {}
        for k, (author, line) in enumerate(keys):
            by_page.setdefault(dataset.authors[author][line][0], []).append(k)
        lines = [None] * len(keys)
        for path, ks in by_page.items():                       # every page is decoded once
            page = D._read_gray(path)
            for k in ks:
                lb = dataset.authors[keys[k][0]][keys[k][1]][1]
                img = np.ascontiguousarray(fit(page[max(lb[0], 0):lb[1], max(lb[2], 0):lb[3]]))                  # as __getitem__
                assert img.dtype == np.uint8 and img.ndim == 2 and img.shape[0] == dataset.img_height and img.shape[1] >= 1, (img.dtype, img.shape)
                lines[k] = img
        return lines

    def _load(self, n):
        try:
            with np.load(self.cache_file) as z:
                widths, pixels = z["widths"], z["pixels"]
        except (OSError, KeyError, ValueError):
            return None
        H = self.height
        if widths.shape != (n,) or pixels.dtype != np.uint8 or (widths < 1).any() or int(H * widths.sum()) != pixels.size:
            return None
        ends = np.cumsum(H * widths.astype(np.int64))
        return [pixels[e - H * int(w):e].reshape(H, int(w)) for e, w in zip(ends, widths)]

    def _save(self, lines):
        os.makedirs(os.path.dirname(self.cache_file), exist_ok=True)
        tmp = "%s.%d.tmp" % (self.cache_file, os.getpid())     # data-parallel ranks may write the same file: every one writes the same bytes
        with open(tmp, "wb") as f:
            np.savez(f, widths=np.array([img.shape[1] for img in lines], dtype=np.int64), pixels=np.concatenate([img.reshape(-1) for img in lines]))
        os.replace(tmp, self.cache_file)

    def line(self, author, line):
        """the fitted line (uint8 [H, w]) as the store holds it"""
        k = self.index[(author, line)]
        return self.pixels[self.offsets[k]:self.offsets[k] + self.height * self.widths[k]].reshape(self.height, self.widths[k])


class StoreLoader(D.ShardedLoader):
    """ShardedLoader's surface (.dataset, .batch_size, len(), epoch, _batches()) over a LineStore: no worker, no decoded pixel on the host."""

    def __init__(self, dataset, batch_size, shuffle, num_workers=0, rank=0, world=1, seed=0, width_bucket=0, bucket_window=16, device=None,
                 cache_dir=None, variant=None):
        super().__init__(dataset, batch_size, shuffle, 0, rank, world, seed, width_bucket, bucket_window)
        assert variant in (None, "full", "low")
        self.variant = variant                                 # device_augment.device_variant: the warp mode, else None (affine GAN batches)
        self.store = LineStore(dataset, device, cache_dir)
        self.want_mask = self.store.masks is not None
        assert not (variant and self.want_mask), "the warp mode produces no foreground masks"
        self.stats_s = 0.0
        if variant and self.store.pool is not None:            # Otsu level and histogram of every line: once, they never change
            from .. import ops
            t0 = time.perf_counter()
            ops.store_line_stats(self.store.pool)
            torch.cuda.synchronize(device)
            self.stats_s = time.perf_counter() - t0
            logging.getLogger("LineStore").info("device store: per-line statistics of %d lines in %.3f s", len(self.store.widths), self.stats_s)

    def _launch(self, rows, W):
        from .. import ops
        return ops.store_batch(self.store.pool, rows, W, want_mask=self.want_mask)

    def _item(self, idx):
        """the host side of dataset[idx] -> (fields, [(k, out_w, strech, m)] per line), or None for a dropped item (after its draws)"""
        ds = self.dataset
        affine = ds.augmentation == "affine"
        strech, skew = 1.0, 0.0
        if affine:                                             # the reference's order: strech, then skew
            strech = (ds.max_strech * 2) * np.random.random() - ds.max_strech + 1
            skew = (ds.max_rot_rad * 2) * np.random.random() - ds.max_rot_rad
        author, lines = ds.lineIndex[idx]
        picked = []
        for line in lines:
            line = _resolve(ds, author, line)
            gt = ds.authors[author][line][2]
            if ds.no_spaces:
                gt = gt.replace(" ", "")
            k = self.store.index[(author, line)]
            width = int(self.store.widths[k])
            if affine and width * strech > ds.max_width:       # sequential: all of the author's lines use the final value
                strech = ds.max_width / width
            picked.append((line, gt, k, width))
        if any(len(gt) == 0 for _, gt, _, _ in picked):
            return None
        m = math.tan(skew) if affine else 0.0
        rows = [(k, int(width * strech) if affine else width, float(strech), m) for _, _, k, width in picked]
        labels = [string_utils.str2label_single(gt, ds.char_to_idx) for _, gt, _, _ in picked]
        label = np.zeros((max(l.shape[0] for l in labels), len(picked)), dtype=np.int32)
        for i, l in enumerate(labels):
            label[:l.shape[0], i] = l
        fields = {"label": torch.from_numpy(label), "label_lengths": torch.IntTensor([l.shape[0] for l in labels]),
                  "gt": [gt for _, gt, _, _ in picked], "author": [author] * len(picked),
                  "author_idx": [ds.author_list.index(author)] * len(picked), "name": ["%s_%d" % (author, line) for line, _, _, _ in picked]}
        return fields, rows

    def _host_batch(self, indices):
        """collate's host side -> (instance without pictures, rows, W)"""
        items = [self._item(int(i)) for i in indices]
        if len(items) > 1:                                     # (a batch of one item is handed through by collate as it is)
            items = [it for it in items if it is not None]
        if not items or items[0] is None:
            raise ValueError("device_store: every item of the batch %s has a line with an empty transcription" % (list(indices),))
        A = len(items[0][0]["gt"])
        if len(items) == 1:
            f = items[0][0]
            inst = {"label": f["label"], "label_lengths": f["label_lengths"], "gt": f["gt"], "author": f["author"], "author_idx": f["author_idx"],
                    "name": f["name"]}
        else:
            label = torch.zeros((max(f["label"].size(0) for f, _ in items), len(items) * A), dtype=torch.int32)
            for i, (f, _) in enumerate(items):
                label[:f["label"].size(0), i * A:(i + 1) * A] = f["label"]
            inst = {"label": label, "label_lengths": torch.cat([f["label_lengths"] for f, _ in items], dim=0)}
            for key in ("gt", "author", "author_idx", "name"):
                inst[key] = [v for f, _ in items for v in f[key]]
        inst.update(image=None, mask=None, top_and_bottom=None, center_line=None, style=None, spaced_label=None, a_batch_size=A)
        rows = [r for _, rs in items for r in rs]
        W = max(r[1] for r in rows)
        if self.width_bucket:
            W = -(-W // self.width_bucket) * self.width_bucket             # pad_width
        return inst, rows, W

    def _launch_warp(self, lines, mesh, W):
        """the draws as DeviceAugment.augment takes them: the device generator's (one randn of (B, 2 + 2 GY GX)), or numpy's in host mode"""
        from .. import ops, rng
        from .device_augment import host_draws
        if rng.mode() == "device":
            return ops.store_warp_batch(self.store.pool, lines, mesh, W, rng=rng.device_rng())
        return ops.store_warp_batch(self.store.pool, lines, mesh, W, fg_bg=host_draws(mesh))

    def _single_host_batch(self, indices):
        """hw_dataset.collate's host side (+ pad_width) -> (instance without the picture, pool lines, x_off, widths, W)"""
        ds = self.dataset
        picked = []
        for idx in indices:
            author, line = ds.lineIndex[int(idx)]
            gt = ds.authors[author][line][2]
            if ds.add_spaces:
                gt = " " + gt + " "
            if len(gt) == 0:                                   # __getitem__ returns None, collate drops it
                continue
            k = self.store.index[(author, int(line))]
            picked.append((author, line, gt, k, int(self.store.widths[k])))
        if not picked:
            raise ValueError("device_store: every item of the batch %s has an empty transcription" % (list(indices),))
        W = max(p[4] for p in picked)
        x_off = [(W - p[4]) // 2 if ds.center else 0 for p in picked]
        labels = [string_utils.str2label_single(p[2], ds.char_to_idx) for p in picked]
        lengths = torch.IntTensor([len(l) for l in labels])
        max_len = int(lengths.max())
        label = np.stack([np.pad(l, ((0, max_len - l.shape[0]),), "constant") for l in labels], axis=1)
        inst = {"image": None, "label": torch.from_numpy(label.astype(np.int32)), "label_lengths": lengths, "gt": [p[2] for p in picked],
                "name": ["%s_%d" % (p[0], p[1]) for p in picked], "author": [p[0] for p in picked]}
        if self.width_bucket:
            W = -(-W // self.width_bucket) * self.width_bucket                 # pad_width
        return inst, [p[3] for p in picked], x_off, [p[4] for p in picked], W

    def _warp_host_batch(self, indices):
        if _single(self.dataset):
            return self._single_host_batch(indices)
        inst, rows, W = self._host_batch(indices)              # the author datasets un-augmented: strech 1, m 0, every line at its own width
        return inst, [r[0] for r in rows], [0] * len(rows), [r[1] for r in rows], W

    def _generate(self, batches):
        if self.variant:
            from .device_augment import mesh_from_extents
            for indices in batches:
                inst, lines, x_off, widths, W = self._warp_host_batch(indices)
                mesh = mesh_from_extents(self.variant, self.store.height, x_off, widths)      # (the "low" variant's coin flips)
                inst["image"] = self._launch_warp(lines, mesh, W)
                inst["line_extents"] = (list(x_off), list(widths))             # (HWRWithSynthTrainer: where the augmented rows' lines are)
                yield inst
            return
        for indices in batches:
            inst, rows, W = self._host_batch(indices)
            out = self._launch(rows, W)
            if self.want_mask:
                inst["image"], inst["fg_mask"] = out
            else:
                inst["image"] = out
            yield inst

    def __iter__(self):
        batches = self._batches()
        self.epoch += 1
        # torch's DataLoader takes one 64-bit draw from torch's global generator for every iterator it builds (its workers' base seed), with 0
        # workers too: taken here as well, so that whatever draws from that generator afterwards (the trainer's host-side style noise) gets
        # what it got behind ShardedLoader
        torch.empty((), dtype=torch.int64).random_()
        return self._generate(batches)
