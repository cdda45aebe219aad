#!/usr/bin/env python
"""python eval_writer_id.py <style_loc> [-g gpu] [--dedupe] [--json FILE]
The reference's eval_writer_id.py on the GPU: over the style files get_styles.py writes (every file matching <style_loc>*, concatenated in
sorted order), is the nearest style to a line's style a line of the same writer? Prints top-1 / top-5 / top-20 retrieval accuracy under
squared-L2 and L1 distance in the reference's format, and in place of the reference's "rank" lines the mean first rank of a same-writer
line. --dedupe drops a line whose writer and style repeat the line above (get_styles.py writes a writer's style once per line of theirs,
which makes top-1 trivially 1). --json writes the result dictionary."""
import argparse
import glob
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="MI355X-native writer retrieval over style files")
    ap.add_argument("style_loc", type=str, help="prefix of the style files (a trailing * is optional)")
    ap.add_argument("-g", "--gpu", type=int, default=0)
    ap.add_argument("--dedupe", action="store_true", help="drop a line whose writer and style repeat the line above")
    ap.add_argument("--json", type=str, default=None, help="write the result dictionary to this file")
    return ap.parse_args(argv)


def load_styles(style_loc):
    """-> (styles float32 [N, D], authors list [N]) over every file matching style_loc*, in sorted order"""
    import numpy as np
    pattern = style_loc if style_loc.endswith("*") else style_loc + "*"
    files = sorted(glob.glob(pattern))
    if not files:
        raise SystemExit("eval_writer_id.py: no file matches %s" % pattern)
    styles, authors = [], []
    for loc in files:
        try:
            with open(loc, "rb") as f:
                data = pickle.load(f)
            s, a = np.asarray(data["styles"]), list(data["authors"])
        except Exception as e:
            raise SystemExit("eval_writer_id.py: %s is not a style file ({\"styles\", \"authors\"} pickle): %s" % (loc, e))
        if s.ndim == 4 and s.shape[2:] == (1, 1):
            s = s[:, :, 0, 0]
        if s.ndim != 2 or s.shape[0] == 0 or s.shape[1] == 0:
            raise SystemExit("eval_writer_id.py: %s holds no styles (shape %s)" % (loc, tuple(s.shape)))
        if len(a) != s.shape[0]:
            raise SystemExit("eval_writer_id.py: %s has %d authors for %d styles" % (loc, len(a), s.shape[0]))
        if styles and s.shape[1] != styles[0].shape[1]:
            raise SystemExit("eval_writer_id.py: %s has style_dim %d, %s has %d" % (loc, s.shape[1], files[0], styles[0].shape[1]))
        styles.append(s.astype(np.float32, copy=False))
        authors += a
    return np.concatenate(styles, axis=0), authors


def main(argv=None):
    args = parse_args(argv)
    styles, authors = load_styles(args.style_loc)
    print("styles: {}".format(styles.shape), flush=True)
    import torch
    from handwriting_line_generation_amd import evaluate
    torch.cuda.set_device(args.gpu)
    try:
        result = evaluate.writer_id(styles, authors, torch.device("cuda", args.gpu), tops=(1, 5, 20), dedupe=args.dedupe)
    except ValueError as e:
        raise SystemExit("eval_writer_id.py: %s" % e)
    if args.dedupe:
        print("dropped {} repeated lines, {} left".format(result["dropped"], result["lines"]))
    for name in ("l2", "l1"):
        r = result[name]
        print("{} mean first rank: {} (rows without a same-writer line: {})".format(name, r["mean_first_rank"], r["rows_without_match"]))
        print("{}\ttop1:{},\ttop5:\t{},\ttop20:\t{}".format(name, r["top1"], r["top5"], r["top20"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)
        print("saved %s" % args.json)


if __name__ == "__main__":
    main()
