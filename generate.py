#!/usr/bin/env python
"""python generate.py -c checkpoint.pth -d out_dir [-g gpu] [-f config.json] [-a k=v,...] -s styles.pkl -r choice=R,num=N,text=...
python generate.py -c checkpoint.pth -d out_dir -r choice=f,path1=a.png,path2=b.png,text=...
python generate.py -c checkpoint.pth -d out_dir -s styles.pkl -r choice=u
python generate.py -c checkpoint.pth -d out_dir [-T] -r choice=s[,batch=i]
python generate.py -c checkpoint.pth -d out_dir [-T] -r choice=r,num_styles=K,step=0.1[,text=...][,start=i,stride=n]
python generate.py -c checkpoint.pth -d out_dir [-T] -r choice=A,author=<id>[,text=...][,max=5]
Non-interactive drop-in for the reference's generate.py flags: `R` writes N lines in styles sampled (and interpolated) from a style file,
`f` interpolates between the styles of two line images in 20 steps, `u` writes `deep` in the first 3 styles of every writer of a style
file, with the ordered.txt that umap_styles.py reads. The actions behind the paper's figures read the validation split of the checkpoint's
dataset (-T: the test split), one writer per batch: `s` renders batch i 79 times while its character spacing is stretched and squeezed
(gen<b>_<i>.png), `r` walks in a closed loop through the styles of K writers (gen<b>_<i>.png, styles<b>.pth), `A` writes a text in the mean
style of one writer's lines (gen_<author>.png). Lines are rendered in batches of equal label length, converted to
8-bit grey and cut to their own width on the GPU, and written as PNGs by a thread pool - or, with --shard N, as lines_%05d.npz arrays of N
lines each (pixels uint8 1-D, offsets int64 [n+1], widths int32 [n], index int64 [n]). The texts go to <savedir>/OUT.txt as `i:text`."""
import argparse
import collections
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PANGRAM = "The quick brown fox jumps over the lazy dog."
CHOICES = ("R", "f", "u", "s", "r", "A")
PER_AUTHOR = 3                 # pictures per writer of the `u` action
MAX_WRITERS = 16


def parse_addtoconfig(arg):
    """'-a k1=v1,k2=k3=v2' -> [[k1, v1], [k2, k3, v2]] (reference generate.py:941-946: items split at ',', keys and value at '='). An item
    without '=' (where the reference fails with an IndexError) is read as a key in front of the next item: 'k2,k3=v2' is 'k2=k3=v2'."""
    out, prefix = [], []
    for kv in (arg.split(",") if arg else []):
        parts = kv.split("=")
        if len(parts) == 1:
            prefix.append(parts[0])
        else:
            out.append(prefix + parts)
            prefix = []
    if prefix:
        raise SystemExit("generate.py: -a %r ends in keys without a value" % arg)
    return out


def parse_run(arg):
    """'-r key=value,...' -> dict (reference generate.py:953-958)"""
    out = {}
    for pair in arg.split(","):
        ss = pair.split("=")
        if len(ss) < 2:
            raise SystemExit("generate.py: -r takes key=value pairs, got %r" % pair)
        out[ss[0]] = ss[1]
    return out


def seed_everything(seed):
    """numpy, torch, Python's random, the device Philox stream -> the random.Random that samples the styles"""
    import torch
    from handwriting_line_generation_amd import rng
    rng.seed_process(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return random.Random(seed)


def write_png(path, line):
    """one uint8 [H, w] line as an 8-bit grey PNG"""
    from PIL import Image
    line = np.ascontiguousarray(line, dtype=np.uint8)
    Image.frombuffer("L", (line.shape[1], line.shape[0]), line, "raw", "L", 0, 1).save(path, format="PNG")


def write_shard(path, lines, index):
    """ragged uint8 lines [H, w_k] -> one .npz: pixels uint8 1-D (the lines back to back, row-major), offsets int64 [n+1], widths int32 [n],
    index int64 [n] (which text each line renders)"""
    sizes = np.asarray([l.size for l in lines], dtype=np.int64)
    offsets = np.zeros(len(lines) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    pixels = np.concatenate([np.ascontiguousarray(l, dtype=np.uint8).reshape(-1) for l in lines]) if lines else np.zeros(0, np.uint8)
    np.savez(path, pixels=pixels, offsets=offsets, widths=np.asarray([l.shape[1] for l in lines], dtype=np.int32),
             index=np.asarray(index, dtype=np.int64))


def read_shard(path, height=64):
    """-> [(index, uint8 [height, w])] of a file written by write_shard"""
    with np.load(path) as z:
        pixels, offsets, widths, index = z["pixels"], z["offsets"], z["widths"], z["index"]
    return [(int(index[k]), pixels[offsets[k]:offsets[k + 1]].reshape(height, int(widths[k]))) for k in range(len(widths))]


class LineSink:
    """takes (index, line) pairs and leaves files in `savedir`: `pattern % index` PNGs, or lines_%05d.npz per `shard` lines; the encoding
    runs on `writers` threads (zlib releases the GIL), with a bounded backlog so that the renderer cannot run away from the encoders"""

    def __init__(self, savedir, pattern, shard=0, writers=8):
        self.savedir, self.pattern, self.shard = savedir, pattern, int(shard)
        workers = min(max(int(writers), 1), MAX_WRITERS)
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.backlog = collections.deque()
        self.limit = 2 if self.shard else 64 * workers
        self.lines, self.index, self.n_shards, self.count = [], [], 0, 0

    def _submit(self, fn, *args):
        while len(self.backlog) >= self.limit:
            self.backlog.popleft().result()
        self.backlog.append(self.pool.submit(fn, *args))

    def _flush(self):
        if self.lines:
            self._submit(write_shard, os.path.join(self.savedir, "lines_%05d.npz" % self.n_shards), self.lines, self.index)
            self.lines, self.index, self.n_shards = [], [], self.n_shards + 1

    def add(self, index, line):
        self.count += 1
        if not self.shard:
            self._submit(write_png, os.path.join(self.savedir, self.pattern % index), line)
            return
        self.lines.append(line)
        self.index.append(index)
        if len(self.lines) == self.shard:
            self._flush()

    def close(self):
        self._flush()
        try:
            for f in self.backlog:
                f.result()
        finally:
            self.pool.shutdown(wait=True)


def pick_texts(text, num, config):
    """the `text` argument of the R action (reference generate.py:358-378) -> num texts"""
    from handwriting_line_generation_amd.data.text_data import TextData
    if len(text) == 0:
        return [PANGRAM] * num
    if text == "RANDOM":
        corpus = config.get("trainer", {}).get("text_data")
        if not corpus or not os.path.exists(corpus):
            raise SystemExit("generate.py: text=RANDOM samples the training corpus, but trainer.text_data %r does not exist; "
                             "pass text=<file>.txt" % corpus)
        return TextData(batch_size=num, max_len=55, textfile=corpus).getInstance()["gt"]
    if text.endswith(".txt"):
        return TextData(batch_size=num, max_len=55, textfile=text).getInstance()["gt"]
    return [text] * num


def run_R(model, config, char_to_idx, run, args, rand, gpu):
    from handwriting_line_generation_amd.generate import load_style_file, render_lines, sample_styles
    if args.style_loc is None:
        raise SystemExit("generate.py: choice=R samples its styles from a style file: pass -s path/to/styles.pkl")
    num = int(run.get("num", run.get("num_inst", 0)))
    if num < 1:
        raise SystemExit("generate.py: choice=R needs num=<lines to generate>")
    texts = pick_texts(run.get("text", ""), num, config)
    styles = sample_styles(load_style_file(args.style_loc), num, rand)
    sink = LineSink(args.savedir, "sample_%d.png", args.shard, args.writers)
    skipped = []
    try:
        for i, line in render_lines(model, texts, styles, char_to_idx, gpu, batch_lines=args.batch, skipped=skipped):
            sink.add(i, line)
    finally:
        sink.close()
    with open(os.path.join(args.savedir, "OUT.txt"), "w") as out:
        for i, text in enumerate(texts):
            if i not in skipped:
                out.write("%d:%s\n" % (i, text))
    return sink.count


def run_f(model, config, char_to_idx, run, args, gpu):
    import torch
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.generate import interpolate, style_from_images
    if "path1" not in run or "path2" not in run:
        raise SystemExit("generate.py: choice=f needs path1=<image>,path2=<image>")
    text = run["text_gen"] if "text_gen" in run else run.get("text", "")
    if len(text) == 0:
        raise SystemExit("generate.py: choice=f needs text=<text to write>")
    style = style_from_images(model, [run["path1"], run["path2"]], gpu)
    model.count_std = model.dup_std = 0          # reference generate.py:199-200
    sink = LineSink(args.savedir, "%s.png", args.shard, args.writers)
    try:
        with torch.no_grad():
            images, _ = interpolate(model, style[0:1].contiguous(), style[1:2].contiguous(), text, char_to_idx, gpu, step=0.05)
            for i, image in enumerate(images):
                B, _, H, W = image.shape
                pixels, offsets = ops.lines_to_u8(image, [W] * B)
                host = pixels.cpu().numpy()
                for b in range(B):
                    line = host[offsets[b]:offsets[b + 1]].reshape(H, W)
                    if args.shard:
                        sink.add(b * len(images) + i, line)
                    else:
                        sink.add("gen%d_%d" % (b, i), line)
    finally:
        sink.close()
    return sink.count


def run_u(model, config, char_to_idx, run, args, gpu):
    """the reference's `u` action (generate.py:698-722): the text `deep` in the first PER_AUTHOR styles of every writer of the style file,
    as <author>_<i>.png, and ordered.txt - the count per writer, then the file names, relative to the directory (the reference writes
    the joined path, which umap_styles.py joins once more). Picture i of a writer is that writer's i-th style of the file(s). A writer with
    fewer styles than that has no pictures (the reference stops with an IndexError there)."""
    import umap_styles
    from handwriting_line_generation_amd.generate import load_style_file, render_lines
    if args.style_loc is None:
        raise SystemExit("generate.py: choice=u renders the styles of a style file: pass -s path/to/styles.pkl")
    if args.shard:
        raise SystemExit("generate.py: choice=u writes the PNGs ordered.txt names; --shard does not apply")
    names, styles = [], []
    for author, rows in load_style_file(args.style_loc).items():
        author = author.item() if isinstance(author, np.generic) else author
        if len(rows) < PER_AUTHOR:
            print("writer %s has %d styles, fewer than %d: no pictures" % (author, len(rows), PER_AUTHOR), flush=True)
            continue
        for i in range(PER_AUTHOR):
            names.append(umap_styles.picture_name(author, i))
            styles.append(np.asarray(rows[i], dtype=np.float32).reshape(-1))
    if not names:
        raise SystemExit("generate.py: no writer of %s has %d styles" % (args.style_loc, PER_AUTHOR))
    sink = LineSink(args.savedir, "%s", 0, args.writers)
    try:
        for i, line in render_lines(model, ["deep"] * len(names), np.stack(styles), char_to_idx, gpu, batch_lines=args.batch):
            sink.add(names[i], line)
    finally:
        sink.close()
    if sink.count != len(names):
        raise SystemExit("generate.py: the character set of this checkpoint cannot write 'deep'")
    umap_styles.write_ordered(args.savedir, PER_AUTHOR, names)
    return sink.count


def dataset_loader(config, test):
    """the loader the reference's dataset actions iterate (generate.py:140-156): one writer per batch (batch_size 1) of the validation
    split, or with -T of the test split with one line per batch (a_batch_size 1)"""
    from handwriting_line_generation_amd.data.author_hw_dataset import getDataLoader
    dl = config["data_loader"]
    val = config.setdefault("validation", {})
    dl["batch_size"] = val["batch_size"] = 1
    if not os.path.exists(dl["char_file"]):
        dl["char_file"] = os.path.join(ROOT, "handwriting_line_generation_amd", "data", os.path.basename(dl["char_file"]))
    if test:
        dl["a_batch_size"] = val["a_batch_size"] = 1
        print("changed a_batch_size to 1", flush=True)
        loader, _ = getDataLoader(config, "test")
    else:
        _, loader = getDataLoader(config, "train")
    if loader is None or not len(loader.dataset):
        raise SystemExit("generate.py: the %s split of %s holds no lines" % ("test" if test else "validation", dl.get("data_dir")))
    return loader


def _write_frames(images, args, frame=None):
    """images: list of NCHW [B,1,H,W] device tensors (one per frame, widths may differ) -> gen<b>_<i>.png (--shard: index b * frames + i),
    converted to 8-bit on the GPU; `frame(i)` true: a 1-pixel black border, drawn on the host array"""
    from handwriting_line_generation_amd import ops
    sink = LineSink(args.savedir, "%s.png", args.shard, args.writers)
    try:
        for i, image in enumerate(images):
            B, _, H, W = image.shape
            pixels, offsets = ops.lines_to_u8(image, [W] * B)
            host = pixels.cpu().numpy()
            for b in range(B):
                line = host[offsets[b]:offsets[b + 1]].reshape(H, W)
                if frame is not None and frame(i):
                    line = line.copy()
                    line[0, :] = line[-1, :] = 0
                    line[:, 0] = line[:, -1] = 0
                sink.add(b * len(images) + i if args.shard else "gen%d_%d" % (b, i), line)
    finally:
        sink.close()
    return sink.count


def run_s(model, config, char_to_idx, run, args, gpu):
    """the reference's `s` action (generate.py:278-305)"""
    import torch
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.generate import get_style, interpolate_horz
    from handwriting_line_generation_amd.model.hw_with_style import correct_pred
    index = int(run["batch"]) if run.get("batch") else 0
    if index < 0:
        raise SystemExit("generate.py: choice=s takes batch=<index from 0>, got %d" % index)
    for i, instance in enumerate(dataset_loader(config, args.test)):      # (never empty: dataset_loader refuses a split without lines)
        if i == index:
            break
    else:
        print("the split holds %d batches: batch %d taken (as the reference takes the last)" % (i + 1, i), flush=True)
    model.count_std = model.dup_std = 0          # reference generate.py:199-200
    with torch.no_grad():
        style = get_style(config, model, instance, gpu)
        image, label = ops.h2d(instance["image"], gpu), ops.h2d(instance["label"], gpu)
        pred = model.hwr(image, None)
        aligned = pred if config.get("trainer", {}).get("use_hwr_pred_for_style", False) else correct_pred(pred, label)
        images = interpolate_horz(model, style, aligned)
        return _write_frames(images, args)


def run_r(model, config, char_to_idx, run, args, rand, gpu):
    """the reference's `r` action (generate.py:306-353)"""
    import torch
    from handwriting_line_generation_amd.generate import walk_film, walk_styles
    num_styles, step = int(run["num_styles"]), float(run.get("step", 0.1))
    if num_styles < 2 or not 0 < step <= 1:
        raise SystemExit("generate.py: choice=r needs num_styles of at least 2 and a step in (0, 1]")
    text = run.get("text", "") or PANGRAM
    start = int(run["start"]) if run.get("start") else None
    stride = int(run["stride"]) if run.get("stride") else None
    model.count_std = model.dup_std = 0
    with torch.no_grad():
        styles = walk_styles(dataset_loader(config, args.test), model, config, num_styles, rand, gpu, start, stride)
        images, frame_styles = walk_film(model, styles, text, char_to_idx, gpu, step)
        n = _write_frames(images, args, frame=(lambda i: i % 5 == 0) if step == 0.2 else None)
    for b in range(images[0].shape[0]):
        torch.save(frame_styles, os.path.join(args.savedir, "styles%d.pth" % b))
    return n


def run_A(model, config, char_to_idx, run, args, gpu):
    """the reference's `A` action (generate.py:501-527)"""
    import torch
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.generate import author_mean_style, generate
    text = run.get("text", "") or PANGRAM
    max_hits = int(run["max"]) if run.get("max") else 5
    model.count_std = model.dup_std = 0
    sink = LineSink(args.savedir, "%s.png", args.shard, args.writers)
    try:
        with torch.no_grad():
            style = author_mean_style(dataset_loader(config, args.test), model, config, run["author"], gpu, max_hits)
            image = generate(model, style, text, char_to_idx, gpu)
            _, _, H, W = image.shape
            pixels, offsets = ops.lines_to_u8(image, [W])
            sink.add(0 if args.shard else "gen_%s" % run["author"], pixels.cpu().numpy().reshape(H, W))
    finally:
        sink.close()
    return sink.count


def main(argv=None):
    ap = argparse.ArgumentParser(description="MI355X-native handwriting line generation from a checkpoint")
    ap.add_argument("-c", "--checkpoint", type=str, default=None, help="checkpoint of this package or of the reference")
    ap.add_argument("-d", "--savedir", type=str, default=None, help="directory the images are written to")
    ap.add_argument("-g", "--gpu", type=int, default=0)
    ap.add_argument("-f", "--config", type=str, default=None, help="config file to use instead of the checkpoint's")
    ap.add_argument("-a", "--addtoconfig", type=str, default=None, help="k1=v1,k2=k3=v2: config[k1]=v1, config[k2][k3]=v2 (int / float coerced, empty = null)")
    ap.add_argument("-r", "--run", type=str, default=None, help="choice=R,num=N,text=... | choice=f,path1=..,path2=..,text=.. | choice=u | choice=s[,batch=i] (the "
                    "stretch film of one validation batch: the aligned text is re-sampled by one HIP launch for all 79 frames; with "
                    "trainer.use_hwr_pred_for_style the recogniser's own output is stretched instead, through torch's F.interpolate, not "
                    "the kernel) | choice=r,num_styles=K,step=0.1[,text=..][,start=i,stride=n] | choice=A,author=<id>[,text=..][,max=5]")
    ap.add_argument("-T", "--test", action="store_true", help="choice=s|r|A: read the test split, one line per batch (default: validation)")
    ap.add_argument("-s", "--style_loc", type=str, default=None, help="style pickle (prefix) written by evaluate.dump_styles")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--batch", type=int, default=64, help="lines rendered per batch")
    ap.add_argument("--shard", type=int, default=0, help="write lines_%%05d.npz arrays of this many lines instead of PNGs")
    ap.add_argument("--writers", type=int, default=8, help="encoder threads (at most %d)" % MAX_WRITERS)
    ap.add_argument("--swa", action="store_true", help="generate with the averaged weights (the checkpoint's swa_state_dict)")
    args = ap.parse_args(argv)

    if args.run is None:
        raise SystemExit("generate.py: the interactive prompt is not built; pass -r choice=R,num=N,text=... (with -s styles) or "
                         "-r choice=f,path1=..,path2=..,text=..")
    run = parse_run(args.run)
    choice = run.get("choice", "")
    if choice not in CHOICES:
        raise NotImplementedError("generate.py: action %r is not built; the six that exist are 'R' (random interpolated styles from a style "
                                  "file), 'f' (interpolation between the styles of two line images), 'u' (the pictures umap_styles.py "
                                  "pastes into its map), 's' (stretch film of a validation batch), 'r' (walk through the styles of "
                                  "several writers) and 'A' (a writer's mean style)" % choice)
    if choice == "r" and not run.get("num_styles"):
        raise SystemExit("generate.py: choice=r needs num_styles=<writers to walk through> (and takes step=0.1,text=...,start=,stride=)")
    if choice == "A" and not run.get("author"):
        raise SystemExit("generate.py: choice=A needs author=<writer id of the split>")
    if args.checkpoint is None:
        raise SystemExit("generate.py: must provide a checkpoint (with -c)")
    if args.savedir is None:
        raise SystemExit("generate.py: must provide a directory to write to (with -d)")
    if args.batch < 1 or args.shard < 0:
        raise SystemExit("generate.py: --batch must be at least 1 and --shard non-negative")

    import torch
    torch.set_num_threads(1)       # host side = many tiny CPU ops; the intra-op pool only adds latency (see bench.py)
    from handwriting_line_generation_amd.generate import load_for_generation
    rand = seed_everything(args.seed)
    torch.cuda.set_device(args.gpu)
    gpu = torch.device("cuda", args.gpu)
    model, config, char_to_idx = load_for_generation(args.checkpoint, args.config, args.gpu, add_to_config=parse_addtoconfig(args.addtoconfig),
                                                     averaged=args.swa)
    os.makedirs(args.savedir, exist_ok=True)

    t0 = time.time()
    if choice == "R":
        n = run_R(model, config, char_to_idx, run, args, rand, gpu)
    elif choice == "f":
        n = run_f(model, config, char_to_idx, run, args, gpu)
    elif choice == "u":
        n = run_u(model, config, char_to_idx, run, args, gpu)
    elif choice == "s":
        n = run_s(model, config, char_to_idx, run, args, gpu)
    elif choice == "r":
        n = run_r(model, config, char_to_idx, run, args, rand, gpu)
    else:
        n = run_A(model, config, char_to_idx, run, args, gpu)
    torch.cuda.synchronize()
    dt = time.time() - t0
    print("lines %d  seconds %.3f  lines/s %.1f" % (n, dt, n / dt if dt > 0 else 0.0), flush=True)


if __name__ == "__main__":
    main()
