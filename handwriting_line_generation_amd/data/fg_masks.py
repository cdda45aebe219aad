"""Foreground masks for the GAN trainer's foreground-only reconstruction loss (`no_bg_loss`): the switch, and the mask cache on disk.

Reference: datasets/author_hw_dataset.py:190-220 (author_rimeslines_dataset.py has the same code). With `fg_masks_dir` set its datasets keep
one mask per line as `<fg_masks_dir>_<max_width>/<author>_<line>.png`: the fitted line Otsu-thresholded, inverted and dilated with a 9 x 9
ellipse (8-bit, 0 / 255), computed per line through OpenCV when the file is missing. Here the missing masks of a dataset are computed on
the GPU (ops.fg_masks, csrc/fg_mask.hip) from a ragged pool of the fitted lines, a chunk at a time; file names and content are the
reference's, so a directory either side wrote is read by the other as it is. What differs is what differs for the lines themselves
(INTEGRATION.md): PIL's resize arithmetic under the threshold, and the structuring element derived from OpenCV's construction, not pinned.

The switch. The reference's trainer reads `config['trainer']['no_bg_loss'] if 'no_bg_loss' in config else False`: the loss is
on only for a config that carries a top-level `no_bg_loss` key next to the trainer's. No shipped config does, so for all of them
wants_fg_masks() is False and nothing here runs."""
import os
import struct
import time

import numpy as np

CHUNK_BYTES = 32 << 20          # fitted lines uploaded per ops.fg_masks launch


def loss_on(config):
    """the reference trainer's literal lookup (trainer/hw_with_style_trainer.py:128)"""
    return bool(config["trainer"].get("no_bg_loss")) if "no_bg_loss" in config else False


def wants_fg_masks(config):
    """True iff the foreground-only loss is on AND data_loader.fg_masks_dir says where the masks live"""
    return loss_on(config) and bool(config.get("data_loader", {}).get("fg_masks_dir"))


def cache_dir(fg_masks_dir, max_width):
    """`<fg_masks_dir>_<max_width>` (reference :193-195: a trailing slash is dropped first)"""
    d = fg_masks_dir[:-1] if fg_masks_dir.endswith("/") else fg_masks_dir
    return "%s_%d" % (d, max_width)


def png_size(path):
    """(height, width) from the PNG header alone (signature + IHDR), None if the file is missing or no PNG"""
    try:
        with open(path, "rb") as f:
            head = f.read(24)
    except OSError:
        return None
    if len(head) < 24 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        return None
    w, h = struct.unpack(">II", head[16:24])
    return h, w


def fitted_shape(dataset, crop_h, crop_w):
    """the shape AuthorHWDataset._fit gives a crop of crop_h x crop_w, without touching a pixel"""
    H, mw = dataset.img_height, dataset.max_width
    size = lambda p: (max(int(round(crop_h * p)), 1), max(int(round(crop_w * p)), 1))        # noqa: E731  (_resize's rounding)
    h, w = crop_h, crop_w
    if h != H:
        percent = float(H) / h
        if w * percent > mw:
            percent = mw / w
        h, w = size(percent)
    elif w > mw:
        h, w = size(mw / w)
    return H, w


def _lines(dataset):
    """every distinct (author, line) the dataset's items use, in item order, with the wrap __getitem__ applies"""
    seen = set()
    for author, lines in dataset.lineIndex:
        for line in lines:
            if line >= len(dataset.authors[author]):
                line = (line + 37) % len(dataset.authors[author])
            if (author, line) not in seen:
                seen.add((author, line))
                yield author, line


def mask_path(dataset, author, line):
    return os.path.join(dataset.fg_masks_dir, "%s_%d.png" % (author, line))


def missing(dataset):
    """[(author, line)] whose cached mask is absent or of another size than the fitted line (headers only: of the mask and of the page)"""
    page_shape, out = {}, []
    for author, line in _lines(dataset):
        path, lb, _ = dataset.authors[author][line]
        have = png_size(mask_path(dataset, author, line))
        if have is not None:
            if path not in page_shape:
                page_shape[path] = png_size(path) or dataset._page(path).shape[:2]
            ph, pw = page_shape[path]
            ch = max(min(lb[1], ph) - max(lb[0], 0), 0)
            cw = max(min(lb[3], pw) - max(lb[2], 0), 0)
            if ch > 0 and cw > 0 and have == fitted_shape(dataset, ch, cw):
                continue
        out.append((author, line))
    return out


def build_cache(dataset, device, todo=None, chunk_bytes=CHUNK_BYTES):
    """Compute and write the masks `todo` (default: missing(dataset)) -> {"lines", "host_s", "gpu_s"}: wall time of decoding / cropping /
    resizing / PNG writing, and of upload + kernel + download. Files are written through a temporary name and os.replace: data-parallel
    ranks may build the same directory at the same time, and every one of them writes the same bytes."""
    import torch
    from PIL import Image

    from .. import ops
    os.makedirs(dataset.fg_masks_dir, exist_ok=True)
    todo = missing(dataset) if todo is None else list(todo)
    H = dataset.img_height
    stats = {"lines": len(todo), "host_s": 0.0, "gpu_s": 0.0}

    def flush(chunk):
        t0 = time.perf_counter()
        widths = [img.shape[1] for _, _, img in chunk]
        offsets = np.zeros(len(chunk) + 1, dtype=np.int64)
        np.cumsum([H * w for w in widths], out=offsets[1:])
        pool = np.concatenate([img.reshape(-1) for _, _, img in chunk])
        t1 = time.perf_counter()
        masks = ops.fg_masks(ops.h2d(torch.from_numpy(pool), device), offsets, widths, height=H).cpu().numpy()
        t2 = time.perf_counter()
        for k, (author, line, _) in enumerate(chunk):
            final = mask_path(dataset, author, line)
            tmp = "%s.%d.tmp" % (final, os.getpid())
            Image.fromarray(masks[offsets[k]:offsets[k + 1]].reshape(H, widths[k])).save(tmp, format="PNG")
            os.replace(tmp, final)
        stats["gpu_s"] += t2 - t1
        stats["host_s"] += (t1 - t0) + (time.perf_counter() - t2)

    chunk, nbytes = [], 0
    t0 = time.perf_counter()
    for author, line in todo:
        path, lb, _ = dataset.authors[author][line]
        img = np.ascontiguousarray(dataset._fit(dataset._page(path)[max(lb[0], 0):lb[1], max(lb[2], 0):lb[3]]))       # as __getitem__
        assert img.dtype == np.uint8 and img.shape[0] == H, (img.dtype, img.shape)
        chunk.append((author, line, img))
        nbytes += img.size
        if nbytes >= chunk_bytes:
            stats["host_s"] += time.perf_counter() - t0
            flush(chunk)
            chunk, nbytes = [], 0
            t0 = time.perf_counter()
    stats["host_s"] += time.perf_counter() - t0
    if chunk:
        flush(chunk)
    return stats


def read_mask(path):
    """cached mask -> float32 [H, W] in {0, 1} (reference :409-410: cv2.imread(path, 0) / 255)"""
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), dtype=np.float32) / np.float32(255)
