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
with an empty transcription dropped after their draws, labels / names / authors built on the host as before."""
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
REFUSAL_CUDA = 'data_loader.device_store with "cuda": false: the lines live in GPU memory and are collated by a GPU kernel, there is no CPU execution'


def check_config(data_set_name, cfgs, device):
    """the refusals of getDataLoader for the loader configs that carry `device_store`, before anything is built"""
    if data_set_name not in ("AuthorHWDataset", "AuthorRIMESLinesDataset"):
        raise NotImplementedError(REFUSAL_DATASET % data_set_name)
    for cfg in cfgs:
        aug = cfg.get("augmentation")
        if aug is not None and aug != "affine":
            raise NotImplementedError(REFUSAL_AUG % (aug,))
    if device is None or not torch.cuda.is_available():
        raise NotImplementedError(REFUSAL_CUDA)


def _resolve(dataset, author, line):
    """the dataset's own wrap of a line index past the author's lines (__getitem__)"""
    n = len(dataset.authors[author])
    return (line + 37) % n if line >= n else line


class LineStore:
    """The fitted lines of `dataset` as one ragged uint8 pool: `.index[(author, line)]` -> k, `.widths[k]`, `.offsets[k]`, host `.pixels`
    (and `.masks` when dataset.fg_masks_dir is set), and `.pool`, the ops.LinePool on `device` (None: host arrays only, nothing can be
    launched). cache_dir: the pixel pool is kept there as .npz under a digest of (page paths, boxes, img_height, max_width); a file whose
    digest matches is loaded instead of decoding."""

    def __init__(self, dataset, device, cache_dir=None):
        t0 = time.perf_counter()
        self.height = H = dataset.img_height
        keys = list(fg_masks._lines(dataset))                  # distinct (author, line) in item order, with the (line + 37) % len wrap
        if not keys:
            raise ValueError("device_store: the dataset has no lines")
        self.index = {k: i for i, k in enumerate(keys)}
        self.cache_file, self.from_cache = None, False
        lines = None
        if cache_dir:
            spec = [[dataset.authors[a][l][0], [int(v) for v in dataset.authors[a][l][1]]] for a, l in keys]
            digest = hashlib.sha256(json.dumps([spec, int(H), dataset.max_width], sort_keys=True).encode()).hexdigest()[:24]
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
        if dataset.fg_masks_dir is not None:
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
        by_page = {}
        for k, (author, line) in enumerate(keys):
            by_page.setdefault(dataset.authors[author][line][0], []).append(k)
        lines = [None] * len(keys)
        for path, ks in by_page.items():                       # every page is decoded once
            page = D._read_gray(path)
            for k in ks:
                lb = dataset.authors[keys[k][0]][keys[k][1]][1]
                img = np.ascontiguousarray(dataset._fit(page[max(lb[0], 0):lb[1], max(lb[2], 0):lb[3]]))        # as __getitem__
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
                 cache_dir=None):
        super().__init__(dataset, batch_size, shuffle, 0, rank, world, seed, width_bucket, bucket_window)
        self.store = LineStore(dataset, device, cache_dir)
        self.want_mask = self.store.masks is not None

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

    def _generate(self, batches):
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
