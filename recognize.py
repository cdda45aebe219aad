#!/usr/bin/env python
"""python recognize.py -c checkpoint.pth -i DIR_OR_LIST -o out.txt [-g gpu] [--beam K] [--batch 32] [--bucket 32] [--gt FILE] [--host-fit]
                    [--swa] [--readers 8] [--timing] [-a k=v,...]
Reads line images with a trained recogniser: the checkpoint is a GAN checkpoint or a recogniser pre-training checkpoint (CNN-only or CRNN)
of this package or of the reference. -i is a directory (every file PIL opens, sorted by name; a line is named by its file name) or a text
file with one path per line (a line is named as it is written there; the order of the file is kept). The images are decoded by a small
thread pool, fitted to the recogniser's height on the GPU (PIL's bicubic bytes, the loaders' arithmetic; --host-fit: with PIL on the host -
the same output, byte for byte), batched by width and decoded on the GPU, greedy or with --beam K by prefix beam search. -o gets one
`name<TAB>text` line per image in input order. --gt FILE (`name<TAB>text` per line) also prints the mean CER / WER and writes them with
the per-line values (string_utils.cer / wer's) to <out>.json. --timing synchronises the device around every stage and prints where the
time went."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MAX_READERS = 16
MAX_BEAM = 32


def read_gray(path):
    """one image file as a uint8 [h, w] grey picture"""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("L"), dtype=np.uint8))


def list_input(arg):
    """-i -> [(name, path)]: the files of a directory that PIL opens, sorted by name, or the paths of a list file in its order (a relative
    path that does not exist from here is tried beside the list file)"""
    from PIL import Image
    if os.path.isdir(arg):
        found = []
        for name in sorted(os.listdir(arg)):
            path = os.path.join(arg, name)
            if not os.path.isfile(path):
                continue
            try:
                with Image.open(path):
                    pass
            except Exception:  # noqa: BLE001 - not an image PIL knows: not a line
                continue
            found.append((name, path))
        return found
    if not os.path.isfile(arg):
        raise SystemExit("recognize.py: -i %r is neither a directory nor a list file" % arg)
    found = []
    with open(arg) as f:
        for line in f:
            name = line.rstrip("\r\n")
            if not name.strip():
                continue
            path = name
            if not os.path.exists(path) and not os.path.isabs(path):
                path = os.path.join(os.path.dirname(os.path.abspath(arg)), name)
            if not os.path.isfile(path):
                raise SystemExit("recognize.py: the list %s names %r, which does not exist" % (arg, name))
            found.append((name, path))
    return found


def read_gt(path, names):
    """`name<TAB>text` per line -> [text or None] in the order of `names`; a name that is no image of the input is refused"""
    if not os.path.isfile(path):
        raise SystemExit("recognize.py: --gt %r does not exist" % path)
    known, texts = set(names), {}
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line:
                continue
            if "\t" not in line:
                raise SystemExit("recognize.py: --gt %s line %d is not `name<TAB>text`: %r" % (path, no, line))
            name, text = line.split("\t", 1)
            if name not in known:
                raise SystemExit("recognize.py: --gt %s line %d names the image %r, which is not in the input" % (path, no, name))
            texts[name] = text
    return [texts.get(name) for name in names]


def mean(values):
    total = 0
    for v in values:
        total += v
    return total / max(len(values), 1)


def main(argv=None):
    from generate import parse_addtoconfig
    ap = argparse.ArgumentParser(description="MI355X-native transcription of line images with a trained recogniser")
    ap.add_argument("-c", "--checkpoint", type=str, default=None, help="GAN or recogniser checkpoint of this package or of the reference")
    ap.add_argument("-i", "--input", type=str, default=None, help="directory of line images, or a text file with one path per line")
    ap.add_argument("-o", "--out", type=str, default=None, help="file that gets one `name<TAB>text` line per image")
    ap.add_argument("-g", "--gpu", type=int, default=0)
    ap.add_argument("-a", "--addtoconfig", type=str, default=None, help="k1=v1,k2=k3=v2: config[k1]=v1, config[k2][k3]=v2")
    ap.add_argument("--beam", type=int, default=0, help="CTC prefix beam search of this width (0: greedy; at most %d)" % MAX_BEAM)
    ap.add_argument("--batch", type=int, default=32, help="lines per batch (1: every line is read alone)")
    ap.add_argument("--bucket", type=int, default=32, help="batch widths are multiples of this (a multiple of 4)")
    ap.add_argument("--gt", type=str, default=None, help="`name<TAB>text` per line: print CER / WER and write <out>.json")
    ap.add_argument("--host-fit", action="store_true", help="fit the lines with PIL on the host instead of the kernel (same output)")
    ap.add_argument("--swa", action="store_true", help="read with the averaged weights (the checkpoint's swa_state_dict)")
    ap.add_argument("--readers", type=int, default=8, help="image decoder threads (at most %d)" % MAX_READERS)
    ap.add_argument("--timing", action="store_true", help="synchronise around every stage and print the seconds spent in each")
    args = ap.parse_args(argv)

    if args.checkpoint is None:
        raise SystemExit("recognize.py: must provide a checkpoint (with -c)")
    if args.input is None:
        raise SystemExit("recognize.py: must provide the images to read (with -i: a directory or a list file)")
    if args.out is None:
        raise SystemExit("recognize.py: must provide a file to write the texts to (with -o)")
    if not 0 <= args.beam <= MAX_BEAM:
        raise SystemExit("recognize.py: --beam %d is outside 0 .. %d" % (args.beam, MAX_BEAM))
    if args.batch < 1 or args.bucket < 4 or args.bucket % 4:
        raise SystemExit("recognize.py: --batch must be at least 1 and --bucket a positive multiple of 4")
    if args.readers < 1:
        raise SystemExit("recognize.py: --readers must be at least 1")
    adds = parse_addtoconfig(args.addtoconfig)
    found = list_input(args.input)
    if not found:
        raise SystemExit("recognize.py: -i %s holds no image" % args.input)
    names = [name for name, _ in found]
    gt = read_gt(args.gt, names) if args.gt is not None else None
    if not os.path.isfile(args.checkpoint):
        raise SystemExit("recognize.py: the checkpoint %r does not exist" % args.checkpoint)

    t_start = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(args.readers, MAX_READERS)) as pool:
        images = list(pool.map(read_gray, [path for _, path in found]))
    t_read = time.perf_counter() - t_start

    import torch
    torch.set_num_threads(1)       # host side = many tiny CPU ops; the intra-op pool only adds latency (see bench.py)
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.recognize import load_recogniser, transcribe
    torch.cuda.set_device(args.gpu)
    gpu = torch.device("cuda", args.gpu)
    hwr, idx_to_char, config = load_recogniser(args.checkpoint, args.gpu, add_to_config=adds, averaged=args.swa)
    height = int(config.get("data_loader", {}).get("img_height", 64))
    casesensitive = config.get("trainer", {}).get("casesensitive", True)

    timing = {} if args.timing else None
    t0 = time.perf_counter()
    result = transcribe(hwr, idx_to_char, images, gpu, batch=args.batch, bucket=args.bucket, beam=args.beam, host_fit=args.host_fit, gt=gt,
                        height=height, casesensitive=casesensitive, timing=timing)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    texts, cers, wers = result if gt is not None else (result, None, None)

    with open(args.out, "w", encoding="utf-8") as f:
        for name, text in zip(names, texts):
            f.write("%s\t%s\n" % (name, text))
    n = len(names)
    print("lines %d  read seconds %.3f  transcribe seconds %.3f  lines/s %.1f (transcribe) %.1f (with reading)  fit %s  fallbacks %d" % (
        n, t_read, dt, n / dt if dt > 0 else 0.0, n / (dt + t_read) if dt + t_read > 0 else 0.0, "host" if args.host_fit else "device",
        ops.fit_fallbacks), flush=True)
    if timing is not None:
        print("timing (synchronised): " + "  ".join("%s %.3f s (%.1f %%)" % (k, timing.get(k, 0.0), 100.0 * timing.get(k, 0.0) / (dt + t_read))
                                                      for k in ("fit", "recogniser", "decode"))
              + "  read %.3f s (%.1f %%)" % (t_read, 100.0 * t_read / (dt + t_read)), flush=True)
    if gt is not None:
        scored = [i for i in range(n) if gt[i] is not None]
        summary = {"lines": n, "scored": len(scored), "beam": args.beam, "cer": mean([cers[i] for i in scored]),
                   "wer": mean([wers[i] for i in scored]), "fit_fallbacks": ops.fit_fallbacks,
                   "per_line": [{"name": names[i], "text": texts[i], "gt": gt[i], "cer": cers[i], "wer": wers[i]} for i in range(n)]}
        with open(args.out + ".json", "w", encoding="utf-8") as f:
            json.dump(summary, f, ensure_ascii=False, indent=1)
        print("CER %.6f  WER %.6f  over %d lines with a reference" % (summary["cer"], summary["wer"], len(scored)), flush=True)


if __name__ == "__main__":
    main()
