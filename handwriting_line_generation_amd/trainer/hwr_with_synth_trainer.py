"""Recogniser training on real lines plus lines generated on the GPU (the paper's synthetic-data experiment). The reference names this
trainer three times (train.py:40-44, 68-69, get_styles.py:119, new_eval.py:158) and does not ship it: nothing here is a port.

The model stays the recogniser-only HWWithStyle of pre-training (`generator: none, style: none`), so a checkpoint written here has the
format of recogniser pre-training (`hwr.*` keys): `model.pretrained_hwr` and `get_styles.py --cer` take it as it is. The generator lives
in the pool (data/synth_lines.py), outside the model: it is in no optimizer and in no checkpoint.

Per iteration: the real instance of the inherited loader, `per_batch` lines drawn from the pool, ONE ops.lines_from_u8 launch that writes
the mixed batch (real rows first, then 1 - p / 128 of the drawn lines, all padded with -1 to a common width), labels merged as `collate`
would for the equivalent items, then the inherited run_hwr / _apply_step (device_cer, async_log and the data-parallel all-reduce are
theirs). Where getDataLoader wrapped the loader in DeviceAugment, the un-augmented inner loader is read and the MIXED batch is augmented
once with the same variant - two launches for all rows, extents from line_extents for the real rows and from the pool's widths for the
generated ones. Behind a warp-mode line store (`data_loader.device_store: "warp"`) the real rows arrive augmented from the store's one launch;
the mixed batch is then augmented with brightness and warp switched off for those rows, which returns them bit for bit. Validation reads
real lines only.

Resume: the pool is not part of a checkpoint. The first refill of a resumed run is number `iteration * per_batch // pool` (iteration:
what the checkpoint completed): no used-up pool is rendered again; the pool that was in use is drawn again from its beginning rather than
continued (with other noise: the device generator's stream goes on)."""
import json

import numpy as np

from .. import ops
from ..data.synth_lines import SynthLinePool, first_refill, merge_labels, validate_synth_config
from .hw_with_style_trainer import HWWithStyleTrainer


class HWRWithSynthTrainer(HWWithStyleTrainer):
    def __init__(self, model, loss, metrics, resume, config, data_loader, valid_data_loader=None, train_logger=None):
        self.per_batch, pool_size = validate_synth_config(config)        # (first: a refusal leaves no checkpoint directory behind)
        if self.per_batch and "curriculum" in config["trainer"]:
            raise ValueError("HWRWithSynthTrainer trains the recogniser alone: trainer.curriculum belongs to the GAN configs")
        super().__init__(model, loss, metrics, resume, config, data_loader, valid_data_loader, train_logger)
        self.pool = self._augment = self._store_variant = None
        if not self.per_batch:            # HWWithStyleTrainer, bit for bit
            return
        from ..data.device_augment import DeviceAugment
        if isinstance(data_loader, DeviceAugment):
            self._augment = data_loader
            self.data_loader = data_loader.loader
            self.data_loader_iter = iter(self.data_loader)
        elif getattr(data_loader, "variant", None):       # a warp-mode StoreLoader (data/line_store.py): its rows arrive augmented
            self._store_variant = data_loader.variant
        with open(config["data_loader"]["char_file"]) as f:
            char_to_idx = json.load(f)["char_to_idx"]
        start = first_refill(self.start_iteration - 1, self.per_batch, pool_size)
        self.pool = SynthLinePool(config["trainer"]["synth"], char_to_idx, gpu=self.gpu.index, rank=self.rank, start=start)

    def _next_instance(self, lesson):
        instance = super()._next_instance(lesson)
        return self.mix(instance) if self.pool is not None else instance

    def mix(self, instance):
        """the collated real `instance` (host image) + per_batch drawn pool lines -> one instance whose image is on the device"""
        pool = self.pool
        drawn = pool.draw(self.per_batch)
        real = instance["image"]
        Br = real.shape[0]
        select = [-1 - r for r in range(Br)] + drawn
        image = ops.lines_from_u8(pool.pixels, pool.offsets, pool.widths, select, real=ops.h2d(real, self.gpu))
        if self._augment is not None:
            from ..data.device_augment import line_extents
            x_off, widths = line_extents(real)
            x_off = np.concatenate([x_off, np.zeros(len(drawn), dtype=np.int64)])
            widths = np.concatenate([widths, pool.widths[drawn]])
            image = self._augment.augment(image, self._augment.mesh_from_extents(image.shape[2], x_off, widths))
        elif self._store_variant is not None:
            # the real rows are augmented already: one pass over the mixed batch whose real rows have brightness and warp off (the identity
            # LUT and no lattice return a row bit for bit), the generated rows the variant's lattices and coin flips
            from ..data.device_augment import augment_batch, mesh_from_extents
            x_off, widths = instance["line_extents"]
            H = image.shape[2]
            gen = mesh_from_extents(self._store_variant, H, [0] * len(drawn), pool.widths[drawn])
            mesh = ops.LineMesh(H, list(widths) + gen.widths, sigma=gen.sigma[0], x_off=list(x_off) + gen.x_off,
                                warp=[False] * Br + [src is not None for src in gen.src], bright=[False] * Br + gen.bright)
            image = augment_batch(image, mesh)
        out = merge_labels(instance, [pool.texts[i] for i in drawn], [pool.labels[i] for i in drawn], [pool.name(i) for i in drawn])
        out["image"] = image
        return out
