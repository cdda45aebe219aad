"""A pool of generated text lines that never leaves the GPU: what HWRWithSynthTrainer mixes into its real batches (the reference names that
trainer - train.py:40-44, 68-69, get_styles.py:119, new_eval.py:158 - and does not ship it; the experiment is the paper's recogniser trained
on real + generated lines).

The pool owns a generator (generate.load_for_generation; recogniser and style extractor dropped, as the reference's `gen_model.hwr = None`;
eval mode, no gradient anywhere), a style file (generate.load_style_file + sample_styles: the `R` action's draws) and a text source
(TextData's corpus). `refill(k)` draws `pool` texts and styles from random.Random("seed/rank/k"), renders them through
generate.render_lines_device and keeps the ragged 8-bit lines in ONE uint8 device buffer - the bytes `generate.py` would write for these
texts and styles - next to host tables (offsets, widths, texts, labels). `draw(n)` hands out n pool indices without replacement and refills,
synchronously, when fewer than n are left: a few tens of ms per thousand lines, no thread, no extra stream. ops.lines_from_u8 turns drawn
lines into rows of a collated fp32 batch; a generated pixel is never fetched."""
import logging
import os
import random

import numpy as np
import torch

from ..utils import string_utils

SYNTH_KEYS = ("checkpoint", "styles", "text_data", "per_batch", "pool", "gen_batch", "seed", "max_len", "max_width", "spacing_noise")
SYNTH_AUTHOR = "synth"


def validate_synth_config(config):
    """the `trainer.synth` block -> (per_batch, pool size); raises ValueError with the reason for what the trainer refuses. Runs before
    anything is built, so it needs no GPU."""
    synth = config["trainer"].get("synth") or {}
    unknown = sorted(set(synth) - set(SYNTH_KEYS))
    if unknown:
        raise ValueError("trainer.synth: unknown key(s) %s (known: %s)" % (unknown, ", ".join(SYNTH_KEYS)))
    per_batch = int(synth.get("per_batch", 0) or 0)
    if per_batch < 0:
        raise ValueError("trainer.synth.per_batch = %d: the number of generated lines per batch cannot be negative" % per_batch)
    if per_batch == 0:
        return 0, 0
    pool = int(synth.get("pool", 0) or 0)
    if pool < per_batch:
        raise ValueError("trainer.synth.pool = %d is smaller than per_batch = %d: one batch draws per_batch different lines from one pool" % (pool, per_batch))
    if config["data_loader"].get("center_pad"):
        raise ValueError("data_loader.center_pad with generated lines: a generated line can be wider than the real batch, and re-centring the "
                         "real rows in the wider batch needs their extents, which the collated batch no longer has")
    if int(synth.get("gen_batch", 64) or 0) < 1:
        raise ValueError("trainer.synth.gen_batch must be at least 1")
    for key, what in (("checkpoint", "generator checkpoint"), ("styles", "style file"), ("text_data", "text file")):
        path = synth.get(key)
        if not path:
            raise ValueError("trainer.synth.%s is missing: the pool needs a %s" % (key, what))
        if key == "styles":
            from glob import glob
            found = bool(glob(path if path.endswith("*") else path + "*"))       # (a prefix, as generate.load_style_file reads it)
        else:
            found = os.path.exists(path)
        if not found:
            raise ValueError("trainer.synth.%s: %s %r does not exist" % (key, what, path))
    return per_batch, pool


def first_refill(completed_iterations, per_batch, pool):
    """the number of the first refill of a run that starts behind `completed_iterations` iterations (0: a fresh run). Every iteration drew
    per_batch lines, a pool hands out `pool` of them: no pool that was used up is rendered again; the pool that was in use when the
    checkpoint was written is NOT continued where it stood (its position is not stored) but drawn again from its beginning."""
    return completed_iterations * per_batch // pool


def merge_labels(instance, texts, labels, names):
    """the collated real `instance` with generated lines appended -> its "label" [L, B] int32 zero padded, "label_lengths", "gt", "name" and
    "author" as hw_dataset.collate makes them for the real items followed by one item per generated line; every other entry is the
    instance's own ("image" is the caller's to replace)."""
    real = instance["label"]
    if real.is_cuda:            # (a loader that keeps its batches resident; the merged table is built on the host)
        real = real.cpu()
    L = max([real.size(0)] + [len(l) for l in labels])
    merged = torch.zeros((L, real.size(1) + len(labels)), dtype=torch.int32)
    merged[:real.size(0), :real.size(1)] = real
    for j, l in enumerate(labels):
        merged[:len(l), real.size(1) + j] = torch.from_numpy(np.asarray(l).astype(np.int32))
    out = dict(instance)
    out["label"] = merged
    out["label_lengths"] = torch.cat([instance["label_lengths"].to(torch.int32), torch.IntTensor([len(l) for l in labels])])
    out["gt"] = list(instance["gt"]) + list(texts)
    out["name"] = list(instance["name"]) + list(names)
    out["author"] = list(instance["author"]) + [SYNTH_AUTHOR] * len(labels)
    return out


class SynthLinePool:
    """synth: the `trainer.synth` block; char_to_idx: the RECOGNISER's character set (the labels); `render(texts, styles)`: an iterable of
    (text indices, pixels, offsets, widths) per bucket as generate.render_lines_device yields them - None: a generator is loaded from
    synth["checkpoint"] on `gpu`. After a refill: `pixels` (uint8, 1-D), `offsets` int64 [n], `widths` int32 [n], `texts`, `labels`, `ids`
    (the line's number in the refill's draw, left-out lines counted) of the n lines kept, and `drawn_texts` / `drawn_styles`: what was
    drawn for the refill, before anything was left out."""

    def __init__(self, synth, char_to_idx, gpu=None, rank=0, start=0, render=None):
        from ..generate import load_style_file
        from .text_data import TextData
        self.size, self.gen_batch = int(synth["pool"]), int(synth.get("gen_batch", 64) or 64)
        self.seed, self.rank = int(synth.get("seed", 0) or 0), int(rank)
        self.max_width = synth.get("max_width")
        self.spacing_noise = bool(synth.get("spacing_noise", False))
        self.char_to_idx = char_to_idx
        self.logger = logging.getLogger("SynthLinePool")
        self.text = TextData(textfile=synth["text_data"], max_len=int(synth.get("max_len") or 55))
        self.styles_by_author = load_style_file(synth["styles"])
        self.model = self.gen_char_to_idx = None
        if render is None:
            from ..generate import load_for_generation, render_lines_device
            model, _, self.gen_char_to_idx = load_for_generation(synth["checkpoint"], gpu=gpu)
            model.hwr = model.style_extractor = None
            for p in model.parameters():
                p.requires_grad_(False)
            model.eval()
            self.model = model

            def render(texts, styles):
                return render_lines_device(model, texts, styles, self.gen_char_to_idx, gpu, batch_lines=self.gen_batch,
                                           spacing_noise=self.spacing_noise)
        self._render = render
        self.next_refill, self.refills, self.left_out = int(start), [], 0
        self.pixels = self.offsets = self.widths = None
        self.texts, self.labels, self.ids, self._order = [], [], [], []
        self.drawn_texts, self.drawn_styles = [], None

    def _draw_text(self, rand):
        t = self.text
        length = rand.randint(t.min_len, t.max_len)
        at = rand.randrange(0, max(len(t.text) - length, 1))
        text = t.text[at:at + length]
        return t.text[at + 1:at + 2] if text == " " else text          # (TextData.getInstance's rule for a lone blank)

    def refill(self, k):
        """pool number k of this rank: a function of (seed, rank, k) and the text and style files alone, as far as texts, styles and draw
        order go (the generator's noise is the process's device stream)"""
        from ..generate import sample_styles
        rand = random.Random("%d/%d/%d" % (self.seed, self.rank, k))
        texts = [self._draw_text(rand) for _ in range(self.size)]
        styles = sample_styles(self.styles_by_author, self.size, rand)
        self.drawn_texts, self.drawn_styles = texts, styles
        chunks, offsets, widths, kept, base = [], [], [], [], 0
        for idx, pixels, offs, w in self._render(texts, torch.from_numpy(styles)):
            chunks.append(pixels)
            for b, i in enumerate(idx):
                label = string_utils.str2label_single(texts[i], self.char_to_idx)
                if len(label) == 0 or (self.max_width and w[b] > self.max_width):
                    continue            # (its bytes stay in the buffer, unused)
                kept.append((i, label))
                offsets.append(base + int(offs[b]))
                widths.append(int(w[b]))
            base += int(pixels.numel())
        left_out = self.size - len(kept)
        self.logger.info("pool %d: %d lines rendered, %d left out (no character of the character set%s)", k, self.size, left_out,
                         ", or wider than %d columns" % self.max_width if self.max_width else "")
        self.left_out += left_out
        self.pixels = chunks[0] if len(chunks) == 1 else torch.cat(chunks) if chunks else torch.empty((0,), dtype=torch.uint8)
        self.offsets, self.widths = np.asarray(offsets, dtype=np.int64), np.asarray(widths, dtype=np.int32)
        self.texts, self.labels, self.ids = [texts[i] for i, _ in kept], [l for _, l in kept], [i for i, _ in kept]
        self._order = list(range(len(kept)))
        rand.shuffle(self._order)
        self.refills.append(k)
        self.next_refill = k + 1

    def draw(self, n):
        """n different pool indices (into offsets / widths / texts / labels); they stay valid until the next draw"""
        if len(self._order) < n:
            self.refill(self.next_refill)
            if len(self._order) < n:
                raise RuntimeError("a pool of %d drawn lines kept only %d, fewer than the %d of one batch: the text file holds too few "
                                   "characters of the character set, or max_width = %r leaves too little" % (self.size, len(self._order), n, self.max_width))
        taken, self._order = self._order[:n], self._order[n:]
        return taken

    def name(self, index):
        return "synth_%d" % (self.refills[-1] * self.size + self.ids[index])
