"""Transcription of line images a user hands over: a trained recogniser (CNN-only or CRNN) from a GAN or a recogniser pre-training checkpoint,
lines of any height fitted to the recogniser's height on the device (ops.fit_lines: PIL's bytes, the arithmetic the loaders train on),
batched by width, decoded and scored on the device (ops.ctc_error_rates / ops.ctc_beam_error_rates). The program around it: recognize.py."""
import time

import numpy as np
import torch

from . import ops
from .data.author_hw_dataset import PADDING_CONSTANT, _resize
from .data.fit_tables import fitted_width


def load_recogniser(checkpoint, gpu, add_to_config=None, averaged=False):
    """-> (hwr, idx_to_char, config): the recogniser of a checkpoint of this package or of the reference, in eval mode on `gpu`, with the
    character table of the checkpoint's data_loader.char_file. A GAN checkpoint (the recogniser rides in its state dict under `hwr.`) and
    a recogniser pre-training checkpoint (a HWWithStyle without generator) both load through generate.load_for_generation; `hwr` is what
    the checkpoint's config names ("CNNOnly batchnorm", "CRNN batchnorm", ...). add_to_config, averaged: as there."""
    from .evaluate import _char_set
    from .generate import load_for_generation
    model, config, _ = load_for_generation(checkpoint, None, gpu, add_to_config=add_to_config, averaged=averaged)
    hwr = getattr(model, "hwr", None)
    if hwr is None:
        raise ValueError("the checkpoint %s holds no recogniser (model.hwr is %r)" % (checkpoint, config["model"].get("hwr")))
    hwr.eval()
    return hwr, _char_set(config), config


def plan_batches(widths, batch=32, bucket=32):
    """lines sorted by fitted width (ties by index), neighbours batched -> [(indices, W)]: every index exactly once, at most `batch` per
    entry, W = the widest member rounded up to a multiple of `bucket` (itself a multiple of 4: the kernel's stores are 16 bytes)"""
    batch, bucket = int(batch), int(bucket)
    if batch < 1 or bucket < 4 or bucket % 4:
        raise ValueError("plan_batches: batch %d must be at least 1 and bucket %d a positive multiple of 4" % (batch, bucket))
    order = sorted(range(len(widths)), key=lambda i: (widths[i], i))
    out = []
    for k in range(0, len(order), batch):
        idx = order[k:k + batch]
        out.append((idx, -(-max(widths[i] for i in idx) // bucket) * bucket))
    return out


def host_batch(images, height, W):
    """the loaders' host path for a batch: `_resize` to `height` rows (PIL), 1 - p / 128, padded with -1 to W -> float32 numpy [B,1,H,W]"""
    out = np.full((len(images), 1, height, W), PADDING_CONSTANT, dtype=np.float32)
    for b, im in enumerate(images):
        if im.shape[0] != height:
            im = _resize(im, float(height) / im.shape[0])
        out[b, 0, :, :im.shape[1]] = np.float32(1.0) - im.astype(np.float32) / np.float32(128.0)
    return out


def transcribe(hwr, idx_to_char, images, gpu, batch=32, bucket=32, beam=0, host_fit=False, gt=None, height=64, casesensitive=True, timing=None):
    """images: list of 2-D uint8 arrays (grey line pictures of any height) -> texts in input order, or (texts, cers, wers) where `gt`
    (a list of reference texts, None for a line without one) is given - the values of string_utils.cer / wer, None where there is no
    reference. Every line is fitted to `height` rows (on the device; host_fit: with PIL on the host, same values), lines are sorted by
    fitted width and batched with their neighbours, each batch padded with -1 ("paper") to a multiple of `bucket` columns; a line's frames
    are decoded at its batch's T, as the validation loops do (batch=1 reads a line alone). Greedy CTC decode, or prefix beam search of
    width `beam` > 0, on the device; batch k's result is fetched while batch k + 1 runs. `timing`: a dict that collects the seconds spent
    in "fit", "recogniser" and "decode" - the device is synchronised around each stage then, so nothing overlaps."""
    n = len(images)
    widths = [fitted_width(im.shape[0], im.shape[1], height) for im in images]
    texts, cers, wers = [None] * n, [None] * n, [None] * n
    pending = []

    def clock(name, t0):
        if timing is not None:
            torch.cuda.synchronize()
            timing[name] = timing.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    def settle(keep):
        while len(pending) > keep:
            idx, handle = pending.pop(0)
            t0 = time.perf_counter()
            c, w, s = handle.result()
            for j, i in enumerate(idx):
                texts[i] = s[j]
                if gt is not None and gt[i] is not None:
                    cers[i], wers[i] = c[j], w[j]
            if timing is not None:
                timing["decode"] = timing.get("decode", 0.0) + time.perf_counter() - t0
    was_training = hwr.training
    hwr.eval()
    try:
        with torch.no_grad():
            for idx, W in plan_batches(widths, batch, bucket):
                t0 = time.perf_counter()
                lines = [images[i] for i in idx]
                if host_fit:
                    x = ops.h2d(host_batch(lines, height, W), gpu)
                else:
                    x, _ = ops.fit_lines(lines, height, W=W, device=gpu)
                t0 = clock("fit", t0)
                pred = hwr(x, None)
                t0 = clock("recogniser", t0)
                refs = [gt[i] if gt is not None and gt[i] is not None else "" for i in idx]
                if beam:
                    handle = ops.ctc_beam_error_rates(pred, refs, idx_to_char, casesensitive, beam)
                else:
                    handle = ops.ctc_error_rates(pred, refs, idx_to_char, casesensitive)
                clock("decode", t0)
                pending.append((idx, handle))
                settle(1)
            settle(0)
    finally:
        if was_training:
            hwr.train()
    return texts if gt is None else (texts, cers, wers)
