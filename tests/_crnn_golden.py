"""The CRNN goldens under tests/golden/crnn/ (the reference's recorded float32 logits, made by tools/gen_golden_crnn.py): their list, one
case read back, and the seeded weights a case was recorded with (not collected by pytest)."""
import glob
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crnn")
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "*.npz")))


def golden_case(path):
    z = np.load(path)
    return dict(pixels=z["pixels"], logits=z["logits"], norm=str(z["norm"]), pad=(str(z["pad"]) or False), nclass=int(z["nclass"]), wseed=int(z["wseed"]),
                keys=[str(k) for k in z["keys"]], shapes=[tuple(int(d) for d in str(s).split(",") if d) for s in z["shapes"]], max_pre=float(z["max_pre"]))


def seeded_sd(keys, shapes, seed):
    """oracle.torch_ref.seeded_state_dict needs a module only for its key names and shapes: a stand-in built from the golden's recorded list,
    so that this works before (and independently of) the class under test"""
    from oracle import torch_ref

    class Stand:
        def __init__(self):
            self.sd = {k: (torch.zeros(s, dtype=torch.int64) if k.endswith("num_batches_tracked") else torch.zeros(s)) for k, s in zip(keys, shapes)}

        def named_parameters(self):
            return [(k, v) for k, v in self.sd.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]

        def state_dict(self):
            return self.sd
    return torch_ref.seeded_state_dict(Stand(), seed)
