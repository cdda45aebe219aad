#!/usr/bin/env python
"""Measures the evaluation pictures of new_eval.py on the GPU (profiles/eval_pictures.txt).

    python tools/eval_pictures_bench.py --what kernels [--steps 200]
    python tools/eval_pictures_bench.py --what program [--rounds 6]

kernels: hwg_eval_pairs `--steps` times back to back between two device events (after 20 untimed launches) at 8 x 64 x 512 and
         16 x 64 x 1216, without and with the caption strip: us per launch in a loop and bytes moved (both inputs read, the pictures written)
         per second - next to hwg_sheet_compose's figures in profiles/sample_sheets.txt, measured the same way.
program: lines/s of new_eval.py's loop with -e [recon,pred] and -d on a fabricated IAM directory and the reduced GAN checkpoint of
         tests/golden: new_eval.setup once, then `--rounds` passes over both splits (begin of batch k + 1 before finish of batch k, the
         writer thread joined inside the timed region). Once composing on the device (the product), once composing on the HOST from
         downloaded fp32 tensors through the numpy restatement tests/_eval_pictures_ref.py - the reference's way; this tool replaces the
         evaluator's method for that, the product has no such switch."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kernels(steps):
    from handwriting_line_generation_amd import ops
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    atlas = torch.from_numpy(rs.randint(0, 256, size=(100, 14, 8)).astype(np.uint8)).to(dev)
    for B, H, W in ((8, 64, 512), (16, 64, 1216)):
        image = torch.from_numpy(rs.uniform(-1, 1, size=(B, 1, H, W)).astype(np.float32)).to(dev)
        recon = torch.from_numpy(rs.uniform(-1, 1, size=(B, 1, H, W - 3)).astype(np.float32)).to(dev)
        for strip in (False, True):
            captions = [rs.randint(0, 100, size=40).tolist() for _ in range(B)] if strip else None
            Hp, Wp = ops.eval_pairs_shape(H, W, W - 3, strip)
            out = torch.empty((-(-B * Hp * Wp * 3 // 4) * 4,), dtype=torch.uint8, device=dev)
            codes = ops.h2d(np.asarray(captions, dtype=np.int32), dev) if strip else None
            st = ops._stream()

            def launch():      # the launch alone: ops.eval_pairs' upload of the codes is not part of the kernel's time
                ops.L.call("hwg_eval_pairs", image, recon, B, H, W, W - 3, atlas if strip else None, 100 if strip else 0, 14 if strip else 0,
                           8 if strip else 0, codes, 40 if strip else 0, out, out.numel(), st)
            for _ in range(20):
                launch()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                launch()
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) * 1000.0 / steps
            moved = image.numel() * 4 + recon.numel() * 4 + B * Hp * Wp * 3
            print("%d x %d x %d / %d (pictures %d x %d x 3, %s) hwg_eval_pairs %8.2f us per launch, %.2f MB moved = %.2f TB/s"
                  % (B, H, W, W - 3, Hp, Wp, "caption strip" if strip else "no strip", us, moved / 1e6, moved / us / 1e6), flush=True)


def _fabricate(d):
    from oracle import collate_items
    from _reference_checkpoint import unpack
    from handwriting_line_generation_amd.harness import CHAR_FILES
    from handwriting_line_generation_amd.logger import load_checkpoint
    root = os.path.join(d, "iam")
    os.makedirs(root)
    collate_items.fake_iam(root, n_pages=6, with_images=True)
    ck = load_checkpoint(unpack("gan", d))
    ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
    ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
    path = os.path.join(d, "gan.pth")
    torch.save(ck, path)
    cfg = ck["config"]
    cfg["data_loader"].update(data_dir=root, batch_size=2, a_batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"], max_width=640, augmentation=None)
    cfg["validation"] = dict(cfg.get("validation", {}), batch_size=2, a_batch_size=2, num_workers=0, augmentation=None)
    cfg["trainer"]["save_dir"] = os.path.join(d, "saved")
    cfg_path = os.path.join(d, "gan.json")
    json.dump(cfg, open(cfg_path, "w"))
    return path, cfg_path


class _HostFetch:
    def __init__(self, array):
        self.array = array

    def get(self):
        return torch.from_numpy(self.array)


def _host_pair_pictures(self, names, cer, pred_str):
    """the reference's way: both fp32 tensors come to the host, the pictures are composed there with numpy on the calling thread"""
    import _eval_pictures_ref as ref
    from handwriting_line_generation_amd import evaluators
    image, recon = self.image.cpu().numpy(), self.out["recon"].cpu().numpy()
    atlas, codes_of = evaluators.glyph_atlas(self.trainer.idx_to_char, self.image.device)
    if not hasattr(_host_pair_pictures, "atlas"):
        _host_pair_pictures.atlas = atlas.cpu().numpy()
    codes = [evaluators.text_codes("CER: {:.3f}, T: {}".format(cer[b], pred_str[b]), codes_of) for b in range(len(names))]
    pictures = ref.eval_pairs(image, recon, codes, _host_pair_pictures.atlas)
    _, Hp, Wp, _ = pictures.shape
    files = [(os.path.join(self.outDir, "{}_recon.png".format(n)), k * Hp * Wp * 3, (Hp, Wp, 3)) for k, n in enumerate(names)]
    evaluators.writer.add(_HostFetch(pictures.reshape(-1)), files)


def program(rounds):
    import contextlib
    import io

    import new_eval
    from handwriting_line_generation_amd import evaluators
    with tempfile.TemporaryDirectory() as d:
        ckpt, cfg = _fabricate(d)
        with contextlib.redirect_stdout(io.StringIO()):
            config, trainer, train_loader, valid_loader, to_eval, _ = new_eval.setup(new_eval.parse_args(["-c", ckpt, "-f", cfg, "-v", "1", "-e", "[recon,pred]"]))
        device_way = evaluators.Pending._pair_pictures

        def one_pass(out_dir):
            lines, ahead = 0, None
            for loader in (valid_loader, train_loader):
                for instance in loader:
                    p = evaluators.begin(config, instance, trainer, [], out_dir, 0, to_eval, 1)
                    if ahead is not None:
                        ahead.finish()
                    ahead = p
                    lines += len(instance["gt"])
            ahead.finish()
            return lines

        for label, method in (("device composition (ops.eval_pairs, uint8 RGB fetched)", device_way),
                              ("host composition (fp32 tensors downloaded, numpy)", _host_pair_pictures),
                              ("device composition, again", device_way)):
            evaluators.Pending._pair_pictures = method
            out_dir = os.path.join(d, "out_%d" % len(os.listdir(d)))
            os.makedirs(out_dir)
            try:
                with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                    one_pass(out_dir)                       # untimed: first pinned buffers, PIL import, thread start
                    evaluators.wait()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    lines = sum(one_pass(out_dir) for _ in range(rounds))
                    evaluators.wait()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
            finally:
                evaluators.Pending._pair_pictures = device_way
            print("%-62s %4d lines in %7.3f s = %7.1f lines/s (%d pictures on disk)" % (label, lines, dt, lines / dt, len(os.listdir(out_dir))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernels", "program"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    if args.what == "kernels":
        kernels(args.steps)
    else:
        program(args.rounds)


if __name__ == "__main__":
    main()
