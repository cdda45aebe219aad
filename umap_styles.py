#!/usr/bin/env python
"""python umap_styles.py <style_loc> [image_dir] [add] [-g gpu] [--dedupe] [--n-neighbors 35] [--min-dist 0.2] [--epochs N] [--seed 42] [-o OUT]
The reference's umap_styles.py ("the umap plots used in the paper") without umap-learn, numba or matplotlib: the two-dimensional map of the
style vectors get_styles.py writes (every file matching <style_loc>*, concatenated in sorted order), neighbours and layout computed on the
GPU (handwriting_line_generation_amd/style_map.py), deterministic for a seed. Writes OUT.npz (embedding fp32 [N, 2], authors, the
parameters) and OUT.png: one dot per line, one colour per writer; with image_dir (what `generate.py -r choice=u` wrote: ordered.txt and its
pictures) each picture is pasted at the point of its style, at a tenth of its size. `add` appends 100 standard normal rows, as the
reference does, drawn black. --dedupe drops a line whose writer and style repeat the line above (get_styles.py writes a writer's style once
per line of theirs, and exact copies never come apart in a map). No window is opened."""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

EXTRA_AUTHOR = "N(0,1)"
DOT = 4                     # radius of a dot in pixels


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="MI355X-native UMAP of style files")
    ap.add_argument("style_loc", type=str, help="prefix of the style files (a trailing * is optional)")
    ap.add_argument("image_dir", type=str, nargs="?", default=None, help="directory written by generate.py -r choice=u (ordered.txt)")
    ap.add_argument("add", type=str, nargs="?", default=None, choices=["add"], help="the word `add`: append 100 N(0,1) rows")
    ap.add_argument("-g", "--gpu", type=int, default=0)
    ap.add_argument("--dedupe", action="store_true", help="drop a line whose writer and style repeat the line above")
    ap.add_argument("--n-neighbors", type=int, default=35)
    ap.add_argument("--min-dist", type=float, default=0.2)
    ap.add_argument("--epochs", type=int, default=None, help="layout epochs (default 500 up to 10000 lines, 200 above)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--size", type=int, default=1600, help="side of the picture in pixels")
    ap.add_argument("-o", "--out", type=str, default="umap_styles", help="writes OUT.npz and OUT.png")
    return ap.parse_args(argv)


def load_styles(style_loc):
    """-> (styles float32 [N, D], authors list [N]): eval_writer_id.load_styles under this program's name"""
    import eval_writer_id
    try:
        return eval_writer_id.load_styles(style_loc)
    except SystemExit as e:
        raise SystemExit(str(e).replace("eval_writer_id.py:", "umap_styles.py:", 1))


def read_ordered(image_dir):
    """ordered.txt of `generate.py -r choice=u` -> (pictures per writer, [file names relative to image_dir])"""
    path = os.path.join(image_dir, "ordered.txt")
    try:
        with open(path) as f:
            lines = [l.strip() for l in f.readlines()]
        return int(lines[0]), [l for l in lines[1:] if l]
    except (OSError, ValueError, IndexError) as e:
        raise SystemExit("umap_styles.py: cannot read %s: %s" % (path, e))


def write_ordered(image_dir, per_author, names):
    from handwriting_line_generation_amd.trainer.sample_sheets import _atomic_write
    _atomic_write(os.path.join(image_dir, "ordered.txt"), ("%d\n" % per_author + "".join("%s\n" % n for n in names)).encode())


def picture_name(author, i):
    return "%s_%d.png" % (author, i)


def writer_colours(authors):
    """-> {author: (r, g, b)}: one draw of three uniforms per writer, in order of first appearance, from a generator seeded with 42"""
    import numpy as np
    rs = np.random.RandomState(42)
    out = {}
    for a in authors:
        if a not in out:
            out[a] = (0, 0, 0) if a == EXTRA_AUTHOR else tuple(int(v) for v in (rs.rand(3) * 255).astype(np.uint8))
    return out


def map_points(embedding, size):
    """-> int [N, 2] pixel (x, y) of every row: the map's bounding box scaled (one scale for both axes) into the picture, 5 % margin, y up"""
    import numpy as np
    e = np.asarray(embedding, dtype=np.float64)
    lo, hi = e.min(axis=0), e.max(axis=0)
    span = float(max((hi - lo).max(), 1e-12))
    margin = 0.05 * size
    p = margin + (e - (lo + hi) / 2 + span / 2) / span * (size - 1 - 2 * margin)
    p[:, 1] = size - 1 - p[:, 1]
    return np.rint(p).astype(np.int64)


def draw_map(embedding, authors, size=1600, thumbs=()):
    """-> the bytes of an RGB PNG: white ground, a filled dot per row in its writer's colour, then the (row, path) thumbnails pasted
    centred on their rows' points at a tenth of their size"""
    from PIL import Image, ImageDraw
    points = map_points(embedding, size)
    colours = writer_colours(authors)
    im = Image.new("RGB", (size, size), (255, 255, 255))
    draw = ImageDraw.Draw(im)
    for (x, y), a in zip(points.tolist(), authors):
        draw.ellipse((x - DOT, y - DOT, x + DOT, y + DOT), fill=colours[a])
    for row, path in thumbs:
        pic = Image.open(path).convert("RGB")
        pic = pic.resize((max(pic.size[0] // 10, 1), max(pic.size[1] // 10, 1)), Image.BICUBIC)
        x, y = points[row].tolist()
        im.paste(pic, (x - pic.size[0] // 2, y - pic.size[1] // 2))
    buf = io.BytesIO()
    im.save(buf, format="PNG")
    return buf.getvalue()


def thumbnails(image_dir, raw_authors, row_of_raw):
    """[(row of the map, picture path)]: picture <author>_<i>.png belongs to the i-th line of that writer in the style files;
    row_of_raw[k] is the map row of line k (with --dedupe a dropped line's row is that of the line it repeats)"""
    per_author, names = read_ordered(image_dir)
    nth = {}
    count = {}
    for k, a in enumerate(raw_authors):
        i = count.get(str(a), 0)
        count[str(a)] = i + 1
        nth[(str(a), i)] = k
    out = []
    for name in names:
        stem = os.path.splitext(os.path.basename(name))[0]
        author, _, i = stem.rpartition("_")
        if not i.isdigit() or (author, int(i)) not in nth:
            raise SystemExit("umap_styles.py: %s names %r, which is not line <i> of a writer of the style files" % (
                os.path.join(image_dir, "ordered.txt"), name))
        out.append((int(row_of_raw[nth[(author, int(i))]]), os.path.join(image_dir, name)))
    return out


def prepare(args):
    """everything in front of the device -> (styles [N, D], authors [N], raw_authors, row_of_raw)"""
    import numpy as np
    from handwriting_line_generation_amd import evaluate, style_map
    styles, authors = load_styles(args.style_loc)
    authors = [a.item() if isinstance(a, np.generic) else a for a in authors]
    if args.add:
        np.random.seed(42)
        styles = np.concatenate([styles, np.random.normal(size=(100, styles.shape[1])).astype(np.float32)], axis=0)
        authors = authors + [EXTRA_AUTHOR] * 100
    raw_authors = list(authors)
    row_of_raw = np.arange(len(authors))
    if args.dedupe:
        keep = evaluate.dedupe_rows(styles, evaluate.author_ids(authors)[0])
        row_of_raw = np.cumsum(keep) - 1
        styles, authors = np.ascontiguousarray(styles[keep]), [a for a, k in zip(authors, keep) if k]
        print("dropped {} repeated lines, {} left".format(int((~keep).sum()), len(authors)))
    try:
        styles = style_map.check_styles(styles)
    except ValueError as e:
        raise SystemExit("umap_styles.py: %s" % e)
    return styles, authors, raw_authors, row_of_raw


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    styles, authors, raw_authors, row_of_raw = prepare(args)
    print("styles: {}".format(styles.shape), flush=True)
    thumbs = thumbnails(args.image_dir, raw_authors, row_of_raw) if args.image_dir else ()
    import torch
    from handwriting_line_generation_amd import style_map
    from handwriting_line_generation_amd.trainer.sample_sheets import _atomic_write
    torch.cuda.set_device(args.gpu)
    info = {}
    try:
        embedding = style_map.embed(styles, torch.device("cuda", args.gpu), n_neighbors=args.n_neighbors, min_dist=args.min_dist,
                                    n_epochs=args.epochs, seed=args.seed, info=info)
    except ValueError as e:
        raise SystemExit("umap_styles.py: %s" % e)
    buf = io.BytesIO()
    np.savez(buf, embedding=embedding, authors=np.asarray([str(a) for a in authors]), dedupe=np.bool_(args.dedupe),
             **{k: np.asarray(v) for k, v in info.items()})
    _atomic_write(args.out + ".npz", buf.getvalue())
    _atomic_write(args.out + ".png", draw_map(embedding, authors, args.size, thumbs))
    print("saved %s.npz and %s.png (%d points, %d edges, %d epochs)" % (args.out, args.out, len(authors), info["edges"], info["n_epochs"]))


if __name__ == "__main__":
    main()
