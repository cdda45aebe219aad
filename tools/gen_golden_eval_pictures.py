#!/usr/bin/env python
"""Records tests/golden/eval_pictures.npz: what the reference's evaluators/hwdataset_eval.py hands to cv2.imwrite for fabricated batches.

    python tools/gen_golden_eval_pictures.py --reference <checkout of the reference>

The reference's module is imported as it is, next to stand-in modules for what this machine lacks or what would start a whole trainer:
  cv2          cvtColor stacks the grey picture into three channels, putText does nothing (the caption's font is not reproduced), imwrite
               records (file name, array);
  trainer      empty classes HWWithStyleTrainer, AutoTrainer and HWRWithSynthTrainer (the reference tests `type(trainer) is ...` against
               the last name without ever defining it);
  skimage, editdistance   empty (imported by the reference's utils, not used on this path).
HWDataset_eval is then called with a fake trainer whose run_gen returns fabricated `recon` (and `pred`) tensors.

Cases: H = 5, B = 2, (Wi, Wr) in CASES, each without and with `pred` (with: the 50 caption rows are appended and the array becomes float64;
it is recorded as uint8 after checking that every value is an integer in [0, 255]). The pixels of image and recon walk through a fixed
permutation of the 2304 edge values of tests/_eval_pictures_ref.py (x = fp32(1 - 2k/255) and neighbours): 1600 of them fit the cases.
The file holds, per case i: c<i>_image, c<i>_recon (fp32), c<i>_pred (0 / 1), c<i>_names, c<i>_pic<b> (uint8 [Hp, Wp, 3] in the order the
reference hands to imwrite, which reads it as BGR). Only recorded data, nothing of the reference's text."""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _eval_pictures_ref as ref  # noqa: E402

H, B = 5, 2
CASES = [(7, 7), (12, 7), (7, 12), (8, 7), (1, 12)]
OUT = os.path.join(ROOT, "tests", "golden", "eval_pictures.npz")


def fabricate():
    """-> [(image [B,1,H,Wi], recon [B,1,H,Wr], with_pred)] over CASES x (False, True)"""
    values = ref.edge_values()
    values = values[np.random.RandomState(5).permutation(values.size)]
    at, out = 0, []
    for with_pred in (False, True):
        for wi, wr in CASES:
            n_i, n_r = B * H * wi, B * H * wr
            image = values[at:at + n_i].reshape(B, 1, H, wi).copy()
            recon = values[at + n_i:at + n_i + n_r].reshape(B, 1, H, wr).copy()
            at += n_i + n_r
            out.append((image, recon, with_pred))
    assert at <= values.size
    return out


class _Loose(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return None


class _Cv2(_Loose):                                   # (constants that other modules of the reference read at import: None)
    COLOR_GRAY2RGB = 8
    FONT_HERSHEY_SIMPLEX = 0
    LINE_AA = 16

    def __init__(self):
        super().__init__("cv2")
        self.written = []

    def cvtColor(self, img, code):
        assert code == self.COLOR_GRAY2RGB and img.ndim == 2
        return np.stack([img, img, img], axis=2)

    def putText(self, *a, **k):
        return None

    def imwrite(self, path, arr):
        self.written.append((os.path.basename(path), np.array(arr, copy=True)))
        return True


def load_reference(reference):
    cv2 = _Cv2()
    sys.modules["cv2"] = cv2
    trainer = types.ModuleType("trainer")
    for n in ("HWWithStyleTrainer", "AutoTrainer", "HWRWithSynthTrainer"):
        setattr(trainer, n, type(n, (), {}))
    sys.modules["trainer"] = trainer
    import importlib.abc
    import importlib.machinery

    class Absent(importlib.abc.MetaPathFinder, importlib.abc.Loader):      # skimage(.anything) and editdistance: empty modules
        def find_spec(self, name, path, target=None):
            if name.split(".")[0] in ("skimage", "editdistance"):
                return importlib.machinery.ModuleSpec(name, self, is_package=True)
            return None

        def create_module(self, spec):
            return _Loose(spec.name)

        def exec_module(self, module):
            pass
    sys.meta_path.insert(0, Absent())
    sys.path.insert(0, reference)
    datasets = types.ModuleType("datasets")            # the reference's directory has no __init__.py: an installed `datasets` would win
    datasets.__path__ = [os.path.join(reference, "datasets")]
    sys.modules["datasets"] = datasets
    spec = importlib.util.spec_from_file_location("reference_hwdataset_eval", os.path.join(reference, "evaluators", "hwdataset_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, cv2


def run_reference(reference, cases):
    import torch
    mod, cv2 = load_reference(reference)
    rs = np.random.RandomState(6)
    recorded = []
    for i, (image, recon, with_pred) in enumerate(cases):
        names = ["c%d_l%d" % (i, b) for b in range(B)]
        got = {"recon": torch.from_numpy(recon)}
        if with_pred:
            got["pred"] = torch.from_numpy(rs.randn(9, B, 6).astype(np.float32)).log_softmax(2)

        class FakeTrainer:
            idx_to_char = {k: "abcde"[k - 1] for k in range(1, 6)}
            curriculum = types.SimpleNamespace(getEval=lambda: ["auto", "eval"])

            def run_gen(self, instance, lesson, get):
                return {}, dict(got)

            def getCER(self, gt, pred, individual=False):
                return 0.3125, 0.75, ["ab", "c"], [0.125, 0.5]

        instance = {"image": torch.from_numpy(image), "gt": ["ab", "cd"], "name": names, "label": torch.tensor([[1, 3], [2, 4]]),
                    "author": ["w0", "w1"]}
        del cv2.written[:]
        with contextlib.redirect_stdout(io.StringIO()):
            mod.HWDataset_eval({}, instance, FakeTrainer(), [], outDir="out", toEval=["recon", "pred"] if with_pred else ["recon"])
        assert [n for n, _ in cv2.written] == ["%s_recon.png" % n for n in names], [n for n, _ in cv2.written]
        pics = []
        for _, arr in cv2.written:
            assert arr.dtype == (np.float64 if with_pred else np.uint8), arr.dtype
            u8 = arr.astype(np.uint8)
            assert np.array_equal(u8.astype(arr.dtype), arr)
            pics.append(u8)
        recorded.append((names, pics))
    return recorded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="directory of the reference checkout (holds evaluators/hwdataset_eval.py)")
    args = ap.parse_args()
    cases = fabricate()
    print("%d cases, %d pixels" % (len(cases), sum(i.size + r.size for i, r, _ in cases)))
    if args.reference is None:
        print("no --reference: nothing written")
        return
    recorded = run_reference(os.path.abspath(args.reference), cases)
    data = {}
    for i, ((image, recon, with_pred), (names, pics)) in enumerate(zip(cases, recorded)):
        data["c%d_image" % i] = image
        data["c%d_recon" % i] = recon
        data["c%d_pred" % i] = np.int32(with_pred)
        data["c%d_names" % i] = np.array(names)
        for b, p in enumerate(pics):
            data["c%d_pic%d" % (i, b)] = p
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
