"""The reference's line augmentation - Tensmeyer brightness + mesh warp (utils/augmentation.py:5-31, utils/grid_distortion.py:11-66), applied per
line inside `__getitem__` of its datasets through OpenCV and scipy.interpolate.griddata (4-19 ms per line for griddata alone) - executed here on
the collated batch by two HIP launches (ops.augment_lines, csrc/augment.hip). getDataLoader wraps a loader in `DeviceAugment` when the
config's `augmentation` value is one the reference answers with brightness + warp; the datasets themselves are constructed un-augmented.

Randomness: with the device generator (rng.mode() == "device") the brightness shifts and the displacements are Philox draws of the process's
stream (rank-keyed seed; the offset is part of a checkpoint, so a resumed run continues the stream); in host mode they come from numpy's global
generator in the reference's order per line (fg, bg, all row displacements, all column displacements). The per-line coin flips of the "low"
variant (datasets/hw_dataset.py:145-149) are Python's `random`, as in the reference."""
import random

import numpy as np
import torch

REFUSAL = ("data option augmentation=%r: only None and 'affine' are implemented (the reference's 'warp' / brightness / "
           "'normalization' augmentations are OpenCV code outside the hot-path scope)")


def device_variant(data_set_name, augmentation):
    """"full" / "low" when the reference answers this `augmentation` value of this dataset with brightness + warp, else None
    (datasets/hw_dataset.py:138-152: not None and not a string, or a string with "warp"; the author datasets, author_hw_dataset.py:427-432:
    anything not None without "affine"). "normalization" is never routed here: the dataset classes refuse it."""
    aug = augmentation
    if aug is None or (isinstance(aug, str) and "normalization" in aug):
        return None
    if data_set_name == "HWDataset":
        if isinstance(aug, str) and "warp" not in aug:
            return None
        return "low" if isinstance(aug, str) and "low" in aug else "full"
    if isinstance(aug, str) and "affine" in aug:
        return None
    return "full"


def line_extents(image):
    """(first valid column, valid width) per line of a collated batch [B,1,H,W], from the top pixel row: padding is -1, which no pixel is
    (a pixel is 1 - p/128 with p <= 255)"""
    top = (image[:, 0, 0, :] != -1).numpy()
    first = top.argmax(axis=1)
    last = top.shape[1] - 1 - top[:, ::-1].argmax(axis=1)
    has = top.any(axis=1)
    return np.where(has, first, 0), np.where(has, last - first + 1, 0)


def mesh_from_extents(variant, H, x_off, widths):
    """the variant's lattices for lines of height H with these extents (the "low" variant's coin flips: two per line, in line order)"""
    from .. import ops
    if variant == "low":
        bright, warp = [], []
        for _ in range(len(widths)):
            bright.append(random.random() > 0.1)
            warp.append(random.random() > 0.01)
        return ops.LineMesh(H, widths, sigma=0.7, x_off=x_off, warp=warp, bright=bright)
    return ops.LineMesh(H, widths, sigma=1.5, x_off=x_off)


def host_draws(mesh):
    """host rng mode: numpy's global generator in the reference's order per line (fg / bg, all row displacements, all column
    displacements) -> fg_bg [B,2]; the displacements become mesh.disp"""
    from .. import ops
    fg_bg, disp = [], []
    for b, src in enumerate(mesh.src):
        fg_bg.append(np.random.normal(0, ops.AUG_BRIGHT_SIGMA, size=2))
        if src is None:
            disp.append(None)
            continue
        n = (len(src[0]), len(src[1]))
        dy = np.random.normal(0.0, mesh.sigma[b], size=n)
        disp.append((dy, np.random.normal(0.0, mesh.sigma[b], size=n)))
    mesh.disp = disp
    return np.asarray(fg_bg)


def augment_batch(dev_image, mesh):
    """the device batch `dev_image` [B,1,H,W] re-lit and warped over `mesh` -> a new device tensor (two launches); the draws are the device
    generator's, or numpy's in host mode"""
    from .. import ops, rng
    if rng.mode() == "device":
        return ops.augment_lines(dev_image, mesh, rng=rng.device_rng())
    return ops.augment_lines(dev_image, mesh, fg_bg=host_draws(mesh))


class DeviceAugment:
    """iterates `loader`; every batch's "image" is uploaded, augmented on the GPU and handed on as a device tensor (the trainers' `_to_tensor`
    passes device tensors through). `.dataset`, `.batch_size` and `len()` are the wrapped loader's."""

    def __init__(self, loader, variant, device, augmentation=None):
        if device is None or not torch.cuda.is_available():
            raise NotImplementedError(REFUSAL % (augmentation,))
        assert variant in ("full", "low")
        self.loader, self.variant, self.device = loader, variant, torch.device(device)

    @property
    def dataset(self):
        return self.loader.dataset

    @property
    def batch_size(self):
        return self.loader.batch_size

    def __len__(self):
        return len(self.loader)

    def mesh_for(self, image):
        x_off, widths = line_extents(image)
        return self.mesh_from_extents(image.shape[2], x_off, widths)

    def mesh_from_extents(self, H, x_off, widths):
        """the variant's lattices for lines of height H with these extents (the "low" variant's coin flips: two per line, in line order)"""
        return mesh_from_extents(self.variant, H, x_off, widths)

    def augment(self, dev_image, mesh):
        """the uploaded batch `dev_image` [B,1,H,W] re-lit and warped over `mesh` -> a new device tensor (two launches); the draws are the
        device generator's, or numpy's in host mode"""
        return augment_batch(dev_image, mesh)

    def apply(self, instance):
        from .. import ops
        image = instance["image"]
        mesh = self.mesh_for(image)
        out = self.augment(ops.h2d(image, self.device), mesh)
        instance = dict(instance)
        instance["image"] = out
        return instance

    def __iter__(self):
        for instance in self.loader:
            yield self.apply(instance)
