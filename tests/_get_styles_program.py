"""get_styles.py on a fabricated IAM directory and the reduced reference checkpoint: the module-scoped `program` fixture and the child
process that runs the tool on it (not collected by pytest; a test module imports `program` by name to use it)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from _reference_checkpoint import unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(args, cwd, timeout=300):
    """one get_styles.py process; a non-zero or timed-out child fails the test at once (nothing more is started on the GPU)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "get_styles.py")] + args, cwd=cwd, timeout=timeout, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def program(cuda, tmp_path_factory):
    """-> dict(dir, ckpt, cfg path): the fabricated dataset, the checkpoint (its spacer spread out as tests/test_generate_cli_gpu.py explains,
    so that regenerated lines are not empty) and a config file that points the checkpoint's own config at the dataset"""
    from oracle import collate_items
    from handwriting_line_generation_amd.harness import CHAR_FILES
    from handwriting_line_generation_amd.logger import load_checkpoint
    d = tmp_path_factory.mktemp("get_styles")
    root = str(d / "iam")
    os.makedirs(root)
    collate_items.fake_iam(root, n_pages=6, with_images=True)
    ck = load_checkpoint(unpack("gan", d))
    ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
    ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
    path = str(d / "spread.pth")
    torch.save(ck, path)
    cfg = ck["config"]
    cfg["data_loader"].update(data_dir=root, batch_size=2, a_batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"], max_width=640, augmentation=None)
    cfg["validation"] = dict(cfg.get("validation", {}), batch_size=2, a_batch_size=2, num_workers=0, augmentation=None)
    cfg_path = str(d / "cfg.json")
    json.dump(cfg, open(cfg_path, "w"))
    return {"dir": d, "ckpt": path, "cfg": cfg_path, "iteration": ck["iteration"]}
