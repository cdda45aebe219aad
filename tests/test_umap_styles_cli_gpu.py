"""GPU: the programs around the style map - umap_styles.py from style files to OUT.npz / OUT.png, and `generate.py -r choice=u`, which
writes the pictures and the ordered.txt that umap_styles.py pastes into its map (on the reference-written, width-reduced checkpoint with
the spread-out spacer that tests/test_generate_cli_gpu.py uses, built here the same way). No umap-learn output serves as a golden file:
umap-learn is not installed where these tests were written."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from _reference_checkpoint import unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(program, args, cwd, timeout=300):
    """one process of a program of the repository; a non-zero or timed-out child fails the test at once (nothing more is started on the GPU)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, program)] + args, cwd=cwd, timeout=timeout, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def _style_files(d):
    """two files in get_styles.py's format: 12 writers with 5 styles each, every style written once per line of its 1..3 lines
    -> (prefix, styles [60, 16] without the repeats, authors [60])"""
    rs = np.random.RandomState(5)
    centres = 3 * rs.randn(12, 16)
    styles = (np.repeat(centres, 5, axis=0) + rs.randn(60, 16)).astype(np.float32)
    authors = ["w%02d" % (i // 5) for i in range(60)]
    repeats = rs.randint(1, 4, 60)
    rows = np.repeat(np.arange(60), repeats)
    cut = int(np.searchsorted(rows, 30))                  # the second file starts with a new style
    for name, part in (("styles_1.pkl", rows[:cut]), ("styles_2.pkl", rows[cut:])):
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump({"styles": styles[part][:, :, None, None], "authors": np.array([authors[i] for i in part]),
                         "ids": [["line%d" % i] for i in part]}, f)
    return os.path.join(d, "styles_"), styles, authors, int(repeats.sum())


def test_umap_styles_program(cuda, tmp_path):
    from PIL import Image
    from handwriting_line_generation_amd import style_map
    prefix, styles, authors, lines = _style_files(str(tmp_path))
    assert lines > 60

    def run(out, extra=()):
        stdout = _child("umap_styles.py", [prefix, "--dedupe", "-g", "0", "--epochs", "60", "--n-neighbors", "10", "-o", str(tmp_path / out)] + list(extra),
                        str(tmp_path))
        assert "dropped %d repeated lines, 60 left" % (lines - 60) in stdout and "styles: (60, 16)" in stdout, stdout[-2000:]
        with np.load(str(tmp_path / (out + ".npz"))) as z:
            return {k: z[k] for k in z.files}
    a = run("a")
    assert a["embedding"].dtype == np.float32 and a["embedding"].shape == (60, 2) and np.isfinite(a["embedding"]).all()
    assert a["authors"].tolist() == authors
    assert (int(a["n_neighbors"]), int(a["n_epochs"]), int(a["seed"]), int(a["neg"]), float(a["min_dist"]), bool(a["dedupe"])) == (10, 60, 42, 5, 0.2, True)
    im = Image.open(str(tmp_path / "a.png"))
    assert im.format == "PNG" and im.size == (1600, 1600)
    assert sorted(n for n in os.listdir(str(tmp_path)) if n.startswith("a.")) == ["a.npz", "a.png"]          # no temporary name left
    b = run("b")
    assert b["embedding"].tobytes() == a["embedding"].tobytes()
    assert open(str(tmp_path / "a.png"), "rb").read() == open(str(tmp_path / "b.png"), "rb").read()
    direct = style_map.embed(styles, cuda, n_neighbors=10, n_epochs=60)
    assert direct.tobytes() == a["embedding"].tobytes()
    assert style_map.embed(styles, cuda, n_neighbors=10, n_epochs=60, seed=7).tobytes() != direct.tobytes()
    # writers are apart in style space by construction: in the map most points have a neighbour of their writer
    import _umap_ref as ref
    assert ref.nearest_label_share(a["embedding"], authors) > 0.8


@pytest.fixture(scope="module")
def spread(cuda, tmp_path_factory):
    """-> path of the spread-out copy of the reference checkpoint (spacer.mean = (3, 1), spacer.std = (1.5, 0.5): lines ~4 columns per character)"""
    from handwriting_line_generation_amd.logger import load_checkpoint
    d = tmp_path_factory.mktemp("umap_ckpt")
    ck = load_checkpoint(unpack("gan", d))
    ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
    ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
    path = os.path.join(str(d), "spread.pth")
    torch.save(ck, path)
    return path


def test_generate_u_and_the_map_with_pictures(cuda, spread, tmp_path):
    from PIL import Image
    from handwriting_line_generation_amd.evaluate import dump_styles
    g = np.random.RandomState(3)
    authors = ["a01"] * 2 + ["b02"] * 2 + ["a01"] * 2 + ["c03"] * 4 + [507] * 3       # a01's third line comes after b02's
    styles = g.randn(len(authors), 128).astype(np.float32)
    dump_styles({"styles": styles, "authors": authors}, str(tmp_path / "styles.pkl"))
    out = str(tmp_path / "pictures")
    stdout = _child("generate.py", ["-c", spread, "-d", out, "-g", "0", "-s", str(tmp_path / "styles.pkl"), "-r", "choice=u"], ROOT)
    assert "lines 9 " in stdout and "writer b02 has 2 styles" in stdout, stdout[-2000:]
    names = ["%s_%d.png" % (a, i) for a in ("a01", "c03", "507") for i in range(3)]
    assert open(os.path.join(out, "ordered.txt")).read().splitlines() == ["3"] + names
    assert sorted(os.listdir(out)) == sorted(names + ["ordered.txt"])
    pictures = {}
    for n in names:
        im = Image.open(os.path.join(out, n))
        assert im.mode == "L" and im.size[1] == 64 and im.size[0] >= 16 and im.size[0] % 4 == 0, (n, im.size)
        pictures[n] = np.asarray(im).copy()
    assert len({p.tobytes() for p in pictures.values()}) == len(names)                   # nine styles, nine pictures
    # picture i of a writer is that writer's i-th style: the same line through render_lines, in this process
    from handwriting_line_generation_amd.generate import load_for_generation, render_lines
    import generate as cli
    model, _, cti = load_for_generation(spread, gpu=0)
    cli.seed_everything(1234)
    # (the CPU oracle's spacer counts for these styles: widths 64, 68, 72, 72, 64, 68, ... by row, none within 4e-3 of a rounding tie)
    rows = [0, 1, 4, 6, 7, 8, 10, 11, 12]                                                # a01's first lines are 0, 1 and 4; b02 (2, 3) has no pictures
    widths = {i: line.shape[1] for i, line in render_lines(model, ["deep"] * 9, styles[rows], cti, cuda)}
    assert [widths[i] for i in range(9)] == [pictures[n].shape[1] for n in names] and len(set(widths.values())) >= 2
    assert pictures["a01_2.png"].shape[1] == 64                                          # row 4; row 2 (b02's) would be 72 columns wide
    # the map of the same file with the pictures pasted in
    stdout = _child("umap_styles.py", [str(tmp_path / "styles.pkl"), out, "-g", "0", "--epochs", "30", "-o", str(tmp_path / "map")], str(tmp_path))
    assert "using 12" in stdout, stdout[-2000:]                                          # 35 neighbours clamped to N - 1
    with np.load(str(tmp_path / "map.npz")) as z:
        emb = z["embedding"]
        assert emb.shape == (13, 2) and int(z["n_neighbors"]) == 12 and z["authors"].tolist() == [str(a) for a in authors]
    import umap_styles
    px = np.asarray(Image.open(str(tmp_path / "map.png")))
    x, y = umap_styles.map_points(emb, 1600)[12].tolist()                                # 507's third style is the last row
    assert px.shape == (1600, 1600, 3)
    small = Image.open(os.path.join(out, "507_2.png")).convert("RGB")
    small = np.asarray(small.resize((small.size[0] // 10, small.size[1] // 10), Image.BICUBIC))
    h, w = small.shape[:2]
    assert h == 6 and np.array_equal(px[y - h // 2:y - h // 2 + h, x - w // 2:x - w // 2 + w], small)       # (pasted last: nothing lies above it)
