#!/usr/bin/env python
"""python play_styles.py <style_loc> [-g gpu] [--dedupe] [--bins B] [-o PREFIX] [--json FILE]
The reference's play_styles.py on the GPU: over the style files get_styles.py writes (every file matching <style_loc>*, concatenated in
sorted order), are two lines of one writer closer in style space than two lines of two writers? All pairs are visited once on the device
(handwriting_line_generation_amd/csrc/style_pairs.hip); the reference's double Python loop takes hours at the size of a training split.
Prints the reference's two lines in its format and with ITS labels - which are swapped: `inter` is the set of same-writer pairs, `intra`
the set of different-writer pairs - and then the same numbers under plain names with the pair counts. --dedupe drops a line whose writer
and style repeat the line above (get_styles.py writes a writer's style once per line of theirs: such pairs have distance 0).
-o PREFIX writes PREFIX.npz (everything evaluate.style_distances returns), PREFIX_mean.png and PREFIX_std.png (the writer x writer heat
maps the reference builds behind its exit(): light to dark blue, grey where two writers have no pair) and PREFIX_hist.png (the two
histograms of the distances, each normalised to its own number of pairs). --json writes the scalar and histogram part. No window is opened."""
import argparse
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

RAMP_LIGHT, RAMP_DARK = (247, 251, 255), (8, 48, 107)       # the smallest and the largest value of a heat map
GREY = (128, 128, 128)                                      # a cell without pairs
HIST_SIZE = (640, 400)                                      # width, height of PREFIX_hist.png
HIST_MARGIN = 20
HIST_COLOURS = {"same": (31, 119, 180), "different": (255, 127, 14)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="MI355X-native same-writer / different-writer style distances over style files")
    ap.add_argument("style_loc", type=str, help="prefix of the style files (a trailing * is optional)")
    ap.add_argument("-g", "--gpu", type=int, default=0)
    ap.add_argument("--dedupe", action="store_true", help="drop a line whose writer and style repeat the line above")
    ap.add_argument("--bins", type=int, default=64, help="bins of the distance histograms (1..256)")
    ap.add_argument("-o", "--out", type=str, default=None, help="writes PREFIX.npz, PREFIX_mean.png, PREFIX_std.png and PREFIX_hist.png")
    ap.add_argument("--json", type=str, default=None, help="write the scalar and histogram part of the result to this file")
    return ap.parse_args(argv)


def load_styles(style_loc):
    """-> (styles float32 [N, D], authors list [N]): eval_writer_id.load_styles under this program's name"""
    import eval_writer_id
    try:
        return eval_writer_id.load_styles(style_loc)
    except SystemExit as e:
        raise SystemExit(str(e).replace("eval_writer_id.py:", "play_styles.py:", 1))


def cell_pixels(writers):
    """side of a heat-map cell in pixels"""
    return max(1, min(16, 1024 // writers))


def heat_pixels(matrix):
    """[A, A] float matrix -> uint8 [A * cell, A * cell, 3]: RAMP_LIGHT at the smallest finite value, RAMP_DARK at the largest (linear in
    between; RAMP_LIGHT everywhere when they are equal), GREY where the matrix is NaN"""
    import numpy as np
    m = np.asarray(matrix, dtype=np.float64)
    a = m.shape[0]
    known = np.isfinite(m)
    t = np.zeros_like(m)
    if known.any():
        lo, hi = m[known].min(), m[known].max()
        if hi > lo:
            t[known] = (m[known] - lo) / (hi - lo)
    light, dark = np.array(RAMP_LIGHT, dtype=np.float64), np.array(RAMP_DARK, dtype=np.float64)
    rgb = np.rint(light + t[:, :, None] * (dark - light)).astype(np.uint8)
    rgb[~known] = GREY
    cell = cell_pixels(a)
    return np.repeat(np.repeat(rgb, cell, axis=0), cell, axis=1)


def _png(array):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(array, "RGB").save(buf, format="PNG")
    return buf.getvalue()


def heat_map(matrix):
    """-> the bytes of an RGB PNG of heat_pixels(matrix)"""
    return _png(heat_pixels(matrix))


def hist_picture(same, different):
    """two lists of bin counts -> the bytes of an RGB PNG of HIST_SIZE: each histogram divided by its own total and drawn as the outline
    of its bars (no fill), both on one vertical scale, white ground"""
    import numpy as np
    from PIL import Image, ImageDraw
    width, height = HIST_SIZE
    im = Image.new("RGB", HIST_SIZE, (255, 255, 255))
    draw = ImageDraw.Draw(im)
    curves = {}
    for name, counts in (("same", same), ("different", different)):
        c = np.asarray(counts, dtype=np.float64)
        curves[name] = c / c.sum() if c.size and c.sum() > 0 else c
    top = max([float(c.max()) for c in curves.values() if c.size] + [0.0])
    x0, x1, y0, y1 = HIST_MARGIN, width - 1 - HIST_MARGIN, height - 1 - HIST_MARGIN, HIST_MARGIN
    draw.line([(x0, y0), (x1, y0)], fill=(0, 0, 0))
    for name in ("different", "same"):
        c = curves[name]
        if not c.size or top <= 0:
            continue
        xs = [x0 + (x1 - x0) * k / c.size for k in range(c.size + 1)]
        ys = [y0 - (y0 - y1) * float(v) / top for v in c]
        points = [(xs[0], y0)]
        for k in range(c.size):
            points += [(xs[k], ys[k]), (xs[k + 1], ys[k])]
        points.append((xs[-1], y0))
        draw.line(points, fill=HIST_COLOURS[name], width=2)
    buf = io.BytesIO()
    im.save(buf, format="PNG")
    return buf.getvalue()


def scalar_part(result):
    """the JSON-serialisable part of evaluate.style_distances' result (no writer x writer matrices)"""
    return {k: v for k, v in result.items() if k not in ("writer_names", "pair_count", "pair_mean", "pair_std")}


def npz_arrays(result):
    """evaluate.style_distances' result as the arrays of PREFIX.npz: the nested parts flattened to same_pairs, same_mean, same_std,
    different_*, hist_edges, hist_same, hist_different; a mean or std that does not exist (no pair) is NaN"""
    import numpy as np
    out = {k: np.asarray(result[k]) for k in ("lines", "dim", "writers", "dropped", "pair_count", "pair_mean", "pair_std") if k in result}
    for name in ("same", "different"):
        out[name + "_pairs"] = np.asarray(result[name]["pairs"])
        for k in ("mean", "std"):
            out["%s_%s" % (name, k)] = np.asarray(np.nan if result[name][k] is None else result[name][k])
    out["hist_edges"] = np.asarray(result["hist"]["edges"], dtype=np.float64)
    out["hist_same"] = np.asarray(result["hist"]["same"], dtype=np.int64)
    out["hist_different"] = np.asarray(result["hist"]["different"], dtype=np.int64)
    if "writer_names" in result:
        out["writer_names"] = np.asarray([str(a) for a in result["writer_names"]])
    return out


def _number(v):
    return "nan" if v is None else v


def main(argv=None):
    args = parse_args(argv)
    if not 1 <= args.bins <= 256:
        raise SystemExit("play_styles.py: --bins must lie in 1..256")
    styles, authors = load_styles(args.style_loc)
    print("styles: {}".format(styles.shape), flush=True)
    import numpy as np
    import torch
    from handwriting_line_generation_amd import evaluate
    from handwriting_line_generation_amd.trainer.sample_sheets import _atomic_write
    torch.cuda.set_device(args.gpu)
    try:
        result = evaluate.style_distances(styles, authors, torch.device("cuda", args.gpu), dedupe=args.dedupe, matrices=args.out is not None,
                                          bins=args.bins)
    except ValueError as e:
        raise SystemExit("play_styles.py: %s" % e)
    if args.dedupe:
        print("dropped {} repeated lines, {} left".format(result["dropped"], result["lines"]))
    same, different = result["same"], result["different"]
    # the reference's lines, with the reference's (swapped) labels: its `inter` list holds the pairs of one writer
    print("inter dist mean: {}, stddev: {}".format(_number(same["mean"]), _number(same["std"])))
    print("intra dist mean: {}, stddev: {}".format(_number(different["mean"]), _number(different["std"])))
    print("same writer: pairs {}, mean {}, std {}".format(same["pairs"], _number(same["mean"]), _number(same["std"])))
    print("different writers: pairs {}, mean {}, std {}".format(different["pairs"], _number(different["mean"]), _number(different["std"])))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(scalar_part(result), f)
        print("saved %s" % args.json)
    if args.out:
        buf = io.BytesIO()
        np.savez(buf, dedupe=np.bool_(args.dedupe), **npz_arrays(result))
        _atomic_write(args.out + ".npz", buf.getvalue())
        written = [args.out + ".npz"]
        if "pair_mean" in result:
            _atomic_write(args.out + "_mean.png", heat_map(result["pair_mean"]))
            _atomic_write(args.out + "_std.png", heat_map(result["pair_std"]))
            written += [args.out + "_mean.png", args.out + "_std.png"]
        _atomic_write(args.out + "_hist.png", hist_picture(result["hist"]["same"], result["hist"]["different"]))
        print("saved %s" % ", ".join(written + [args.out + "_hist.png"]))


if __name__ == "__main__":
    main()
