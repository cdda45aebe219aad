"""One line per item from IAM-style data on disk: the dataset of the recogniser pre-training configs (reference: datasets/hw_dataset.py:21-172,
utils/parseIAM.py:11-70), without OpenCV - decoding, cropping and the height normalisation go through PIL / numpy, with the caveat of
author_hw_dataset.py's module docstring: the interpolation ARITHMETIC is PIL's (bicubic, a = -0.5, antialiased), not cv2.INTER_CUBIC's, and
is not pinned to the reference; which pixels are cropped, the resize geometry, the normalisation 1 - p/128, the padding, the label encoding
and the item index are (tests/golden/hwdataset_index.json).

Directory layout as for AuthorHWDataset (`forms/`, `xmls/`, `sets.json`). Every line is resized by ONE uniform factor to `img_height`
(this class has no `max_width` and no vertical padding). The class itself never augments: the reference's brightness + mesh warp
(:143-152) runs on the GPU on the collated batch (data/device_augment.py, switched on by getDataLoader), so constructing the class with an
augmentation value the reference would act on raises NotImplementedError, like its siblings."""
import json
import os
from collections import defaultdict

import numpy as np
import torch

from ..utils import string_utils
from .author_hw_dataset import PADDING_CONSTANT, _read_gray, _resize, parse_iam_xml


def collate(batch):
    """items -> batch dict (hw_dataset.py:21-67): None items dropped, images padded with -1 to the widest line (left aligned, or centred
    when the items say `center`), labels [L, B] int32 zero padded"""
    batch = [b for b in batch if b is not None]
    assert len(set(b["image"].shape[0] for b in batch)) == 1
    assert len(set(b["image"].shape[2] for b in batch)) == 1
    dim0, dim1, dim2 = batch[0]["image"].shape[0], max(b["image"].shape[1] for b in batch), batch[0]["image"].shape[2]
    input_batch = np.full((len(batch), dim0, dim1, dim2), PADDING_CONSTANT).astype(np.float32)
    all_labels, label_lengths = [], []
    for i, b in enumerate(batch):
        img = b["image"]
        to_pad = dim1 - img.shape[1]
        to_pad = to_pad // 2 if batch[0].get("center") else 0
        input_batch[i, :, to_pad:to_pad + img.shape[1], :] = img
        all_labels.append(b["gt_label"])
        label_lengths.append(len(b["gt_label"]))
    label_lengths = torch.IntTensor(label_lengths)
    max_len = int(label_lengths.max())
    labels = np.stack([np.pad(l, ((0, max_len - l.shape[0]),), "constant") for l in all_labels], axis=1)
    return {"image": torch.from_numpy(input_batch.transpose([0, 3, 1, 2])), "label": torch.from_numpy(labels.astype(np.int32)),
            "label_lengths": label_lengths, "gt": [b["gt"] for b in batch], "name": [b["name"] for b in batch],
            "author": [b["author"] for b in batch]}


class HWDataset(torch.utils.data.Dataset):
    collate = staticmethod(collate)          # what ShardedLoader batches the items with

    def __init__(self, dirPath, split, config):
        self.img_height = config["img_height"]
        sets = None
        for cand in (os.path.join("data", "sets.json"), os.path.join(os.path.dirname(config["char_file"]), "sets.json"), os.path.join(dirPath, "sets.json")):
            if os.path.exists(cand):
                sets = json.load(open(cand))
                break
        if sets is None:
            raise FileNotFoundError("sets.json (train/valid/test page lists) not found in data/, next to the char set or in %s" % dirPath)
        pages = []
        for s in (split if isinstance(split, (list, tuple)) else [split]):
            pages += sets[s]
        self.authors = defaultdict(list)
        self.lineIndex = []
        for name in pages:
            lines, author = parse_iam_xml(os.path.join(dirPath, "xmls", name + ".xml"))
            n = len(self.authors[author])
            self.authors[author] += [(os.path.join(dirPath, "forms", name + ".png"),) + l for l in lines]
            self.lineIndex += [(author, i + n) for i in range(len(lines))]
        with open(config["char_file"]) as f:
            self.char_to_idx = json.load(f)["char_to_idx"]
        self.augmentation = config.get("augmentation")
        # the reference deskews / skeletonises for a string with "normalization" and re-lights + warps every line for any other non-None
        # value that is not a string without "warp" (:138-152); neither happens in this class (see the module docstring)
        aug = self.augmentation
        if aug is not None and (not isinstance(aug, str) or "warp" in aug or "normalization" in aug):
            raise NotImplementedError("data option augmentation=%r: only None and 'affine' are implemented (the reference's 'warp' / brightness / "
                                      "'normalization' augmentations are OpenCV code outside the hot-path scope)" % (aug,))
        if config.get("cache_normalized") is not None:
            raise NotImplementedError("data option 'cache_normalized' belongs to the 'normalization' augmentation, which is not implemented")
        if config.get("overfit"):
            self.lineIndex = self.lineIndex[:10]
        self.center = config["center_pad"]
        self.add_spaces = config["add_spaces"] if "add_spces" in config else False     # (sic: the reference looks the misspelt key up, :105)
        self._pages = {}

    def __len__(self):
        return len(self.lineIndex)

    def estimated_width(self, idx):
        """width (px) of item `idx` after height normalisation, from the line box alone (no image is read): what width bucketing sorts by"""
        author, line = self.lineIndex[idx]
        lb = self.authors[author][line][1]
        return (lb[3] - lb[2]) * self.img_height / max(lb[1] - lb[0], 1)

    def _page(self, path):
        if path not in self._pages:
            if len(self._pages) > 8:
                self._pages.clear()
            self._pages[path] = _read_gray(path)
        return self._pages[path]

    def __getitem__(self, idx):
        author, line = self.lineIndex[idx]
        path, lb, gt = self.authors[author][line]
        if self.add_spaces:
            gt = " " + gt + " "
        page = self._page(path)
        img = page[max(lb[0], 0):lb[1], max(lb[2], 0):lb[3]]
        if img.shape[0] != self.img_height:
            img = _resize(img, float(self.img_height) / img.shape[0])
        img = 1.0 - img.astype(np.float32)[..., None] / 128.0
        if len(gt) == 0:
            return None
        return {"image": img, "gt": gt, "gt_label": string_utils.str2label_single(gt, self.char_to_idx), "name": "%s_%d" % (author, line),
                "center": self.center, "author": author}
