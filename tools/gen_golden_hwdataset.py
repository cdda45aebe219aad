"""Known answers from the unmodified reference for the recogniser pre-training data path (build container only, tools/ref_bootstrap.py):

  * tests/golden/hwdataset_index.json: the reference's `HWDataset` + `collate` (datasets/hw_dataset.py:21-172) on the fabricated IAM
    directory of oracle/collate_items.fake_iam with augmentation None. cv2 is absent, so the class runs with a recording stand-in
    (a subclass of oracle/cv2_recorder.RecordingCv2): per split the `lineIndex`, per item name / gt / label / author / crop box (the line
    box the class slices the page with) / the `resize` call, and for `center_pad` false and true the collated batch's shape, labels,
    label_lengths and the padded columns of every line.
  * tests/golden/warp_maps.npz: `utils/grid_distortion.warp_image` called with `random_state=np.random.RandomState(seed)` on images of
    64 x W with `cv2.remap` replaced by a recorder and `griddata` wrapped: the source lattice, the destination points, map_x / map_y
    (float32, as the reference stores them), the interpolation flag and the borderValue it hands to remap. Chosen seeds: every lattice
    triangle (each cell split along its locally Delaunay diagonal) is a triangle of scipy.spatial.Delaunay(destination) - a seed where
    one is not is skipped and named in the file - and at least 97 % of the pixels lie inside the lattice mesh.

    python tools/gen_golden_hwdataset.py
"""
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")

WARP_CASES = [   # name, W, first seed to try, keyword arguments of warp_image
    ("w150", 150, 11, {}),
    ("w263", 263, 12, {}),          # not a multiple of 12
    ("w420", 420, 13, {}),
    ("w300_low", 300, 14, {"w_mesh_std": 0.7, "h_mesh_std": 0.7}),      # the "low" variant's sigma (datasets/hw_dataset.py:149)
]


def hwdataset_index():
    from oracle import collate_items, cv2_recorder
    from datasets import hw_dataset as ref

    class Rec(cv2_recorder.RecordingCv2):
        pass

    work = "/tmp/hwg_golden_hwdataset"
    shutil.rmtree(work, ignore_errors=True)
    root = os.path.join(work, "iam")
    os.makedirs(os.path.join(work, "data"))
    pages, sets = collate_items.fake_iam(root, with_images=True)
    shutil.copy(os.path.join(root, "sets.json"), os.path.join(work, "data", "sets.json"))
    char_file = os.path.join(ROOT, "handwriting_line_generation_amd", "data", "IAM_char_set.json")
    out = {"sets": sets, "splits": {}}
    cwd = os.getcwd()
    os.chdir(work)          # the reference opens data/sets.json relative to the working directory
    try:
        for split in ("train", "valid", "test"):
            per_center = {}
            for center in (False, True):
                rec = Rec(root)
                ref.cv2 = rec
                ds = ref.HWDataset(root, split, {"img_height": 64, "char_file": char_file, "center_pad": center, "augmentation": None})
                items, raw = [], []
                for idx in range(len(ds)):
                    del rec.calls[:]
                    it = ds[idx]
                    author, line = ds.lineIndex[idx]
                    raw.append(it)
                    items.append({"idx": idx, "name": it["name"], "gt": it["gt"], "label": it["gt_label"].tolist(), "author": it["author"],
                                  "crop_box": list(ds.authors[author][line][1]), "image_shape": list(it["image"].shape),
                                  "calls": [list(c) for c in rec.calls], "center": bool(it["center"])})
                batch = ref.collate(raw[:5] + [None])
                img = batch["image"].numpy()
                cols = []
                for b in range(img.shape[0]):
                    valid = np.nonzero(img[b, 0, 0] != -1)[0]
                    cols.append([int(valid[0]), int(valid[-1]) + 1])
                per_center["center" if center else "left"] = {
                    "lineIndex": [[a, int(l)] for a, l in ds.lineIndex], "len": len(ds), "items": items,
                    "collate": {"of": [0, 1, 2, 3, 4, None], "image_shape": list(img.shape), "image_dtype": str(img.dtype), "valid_columns": cols,
                                "padding_is_minus_one": bool(all((img[b, :, :, :c[0]] == -1).all() and (img[b, :, :, c[1]:] == -1).all() for b, c in enumerate(cols))),
                                "label": batch["label"].tolist(), "label_dtype": str(batch["label"].dtype), "label_lengths": batch["label_lengths"].tolist(),
                                "gt": batch["gt"], "name": batch["name"], "author": batch["author"], "keys": sorted(batch)}}
            out["splits"][split] = per_center
    finally:
        os.chdir(cwd)
    path = os.path.join(GOLD, "hwdataset_index.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("hwdataset_index.json", os.path.getsize(path) // 1024, "KiB", {k: v["left"]["len"] for k, v in out["splits"].items()})


def lattice_is_delaunay(dst, gy, gx):
    """every lattice triangle (cells split along the locally Delaunay diagonal of their four displaced corners) is a scipy Delaunay triangle"""
    from scipy.spatial import Delaunay
    P = dst.reshape(gy, gx, 2)
    idx = np.arange(gy * gx).reshape(gy, gx)
    tris = []
    for i in range(gy - 1):
        for j in range(gx - 1):
            a, b, c, d = idx[i, j], idx[i, j + 1], idx[i + 1, j + 1], idx[i + 1, j]
            pa, pb, pc, pd = dst[a], dst[b], dst[c], dst[d]
            orient = (pb[0] - pa[0]) * (pc[1] - pa[1]) - (pb[1] - pa[1]) * (pc[0] - pa[0])
            m = np.array([[p[0] - pd[0], p[1] - pd[1], (p[0] - pd[0]) ** 2 + (p[1] - pd[1]) ** 2] for p in (pa, pb, pc)])
            if np.linalg.det(m) * np.sign(orient) > 0:
                tris += [(a, b, d), (b, c, d)]
            else:
                tris += [(a, b, c), (a, c, d)]
    have = set(tuple(sorted(t)) for t in Delaunay(dst).simplices.tolist())
    missing = [t for t in tris if tuple(sorted(int(v) for v in t)) not in have]
    return not missing, np.array(tris)


def inside_fraction(dst, tris, h, w):
    inside = np.zeros((h, w), dtype=bool)
    yy, xx = np.mgrid[0:h, 0:w]
    for t in tris:
        p = dst[t]
        T = np.array([[p[0, 0] - p[2, 0], p[1, 0] - p[2, 0]], [p[0, 1] - p[2, 1], p[1, 1] - p[2, 1]]])
        Ti = np.linalg.inv(T)
        l0 = Ti[0, 0] * (yy - p[2, 0]) + Ti[0, 1] * (xx - p[2, 1])
        l1 = Ti[1, 0] * (yy - p[2, 0]) + Ti[1, 1] * (xx - p[2, 1])
        inside |= (l0 >= 0) & (l1 >= 0) & (1 - l0 - l1 >= 0)
    return float(inside.mean())


def warp_maps():
    from oracle import cv2_recorder
    from utils import grid_distortion as ref

    class RemapRecorder(cv2_recorder.RecordingCv2):
        def remap(self, src, map1, map2, interpolation, dst=None, borderMode=0, borderValue=0):
            self.calls.append(["remap", np.array(map1), np.array(map2), int(interpolation), [float(v) for v in np.ravel(borderValue)]])
            return src

    out, notes = {}, []
    for name, W, seed, kw in WARP_CASES:
        while True:
            rec = RemapRecorder("/")
            ref.cv2 = rec
            ref.INTERPOLATION = {"linear": rec.INTER_LINEAR, "cubic": rec.INTER_CUBIC}
            seen = {}
            orig = ref.griddata

            def wrapped(points, values, xi, method="linear", _orig=orig, _seen=seen):
                _seen["destination"], _seen["source"], _seen["method"] = np.array(points), np.array(values), method
                return _orig(points, values, xi, method=method)
            ref.griddata = wrapped
            img = np.random.RandomState(1000 + seed).randint(0, 256, size=(64, W)).astype(np.uint8)
            try:
                ref.warp_image(img, random_state=np.random.RandomState(seed), **kw)
            finally:
                ref.griddata = orig
            _, map_x, map_y, interp, border = rec.calls[-1]
            src, dst = seen["source"], seen["destination"]
            gy = len(np.unique(src[:, 0])); gx = len(np.unique(src[:, 1]))
            ok, tris = lattice_is_delaunay(dst, gy, gx)
            frac = inside_fraction(dst, tris, 64, W)
            if ok and frac >= 0.97:
                break
            notes.append("%s: seed %d skipped (lattice Delaunay %s, inside fraction %.4f)" % (name, seed, ok, frac))
            seed += 100
        assert map_x.dtype == np.float32 and map_y.dtype == np.float32 and seen["method"] == "linear"
        out[name + "/image"] = img
        out[name + "/seed"] = np.array(seed)
        out[name + "/source"] = src
        out[name + "/destination"] = dst
        out[name + "/grid"] = np.array([gy, gx])
        out[name + "/map_x"], out[name + "/map_y"] = map_x, map_y
        out[name + "/interpolation"] = np.array(interp)
        out[name + "/border_value"] = np.array(border, dtype=np.float64)
        out[name + "/sigma"] = np.array(kw.get("w_mesh_std", 1.5))
        print(name, "W", W, "seed", seed, "grid", gy, gx, "inside %.4f" % frac, "nan", int(np.isnan(map_x).sum()))
    out["notes"] = np.array(json.dumps(notes))
    path = os.path.join(GOLD, "warp_maps.npz")
    np.savez_compressed(path, **out)
    print("warp_maps.npz", os.path.getsize(path) // 1024, "KiB", notes)


if __name__ == "__main__":
    import ref_bootstrap
    ref_bootstrap.bootstrap()
    hwdataset_index()
    warp_maps()
