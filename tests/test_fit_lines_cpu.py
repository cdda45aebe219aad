"""CPU: the host half of hwg_fit_lines and of recognize.py. The coefficient tables of data/fit_tables.py, driven through a numpy integer
restatement, give PIL's bytes on a fixed list of pictures (PIL itself is the oracle, no tolerance); fitted_width is `_resize`'s width; the
device tables ops.fit_lines uploads, read the way include/hwg.h says the kernel reads them (tests/_fit_lines_ref.emulate), give PIL's
batch; the program refuses bad arguments with a sentence; the batching function returns every line once."""
import numpy as np
import pytest

from _fit_lines_ref import HEIGHTS, KINDS, WIDTHS, emulate, entry_ok, expected_batch, picture, pil_fit, pool_of


@pytest.mark.parametrize("H", [64, 32])
def test_tables_give_pils_bytes(H):
    from handwriting_line_generation_amd.data import fit_tables as FT
    bad, n = [], 0
    for h in HEIGHTS:
        for w in WIDTHS:
            for kind in KINDS:
                img = picture(h, w, kind, seed=H)
                out_w = FT.fitted_width(h, w, H)
                n += 1
                if not np.array_equal(FT.fit_line_host(img, H), pil_fit(img, H, out_w)):
                    bad.append((h, w, kind))
    assert n == len(HEIGHTS) * len(WIDTHS) * len(KINDS) and not bad, bad
    # the list reaches both skipped passes and the order Image.resize turns round
    assert 64 in HEIGHTS and any(FT.fitted_width(h, w, H) == w and h != H for h in HEIGHTS for w in WIDTHS)
    assert any(FT.vertical_first(h, w, H) and FT.fitted_width(h, w, H) != w for h in HEIGHTS for w in WIDTHS)


def test_fitted_width_is_resizes_width():
    from handwriting_line_generation_amd.data import fit_tables as FT
    from handwriting_line_generation_amd.data.author_hw_dataset import _resize
    for H in (64, 32):
        for h in HEIGHTS:
            for w in WIDTHS:
                got = _resize(np.zeros((h, w), dtype=np.uint8), float(H) / h)
                assert got.shape == (H, FT.fitted_width(h, w, H)), (h, w, H, got.shape)


def test_table_windows_and_weights():
    from handwriting_line_generation_amd.data import fit_tables as FT
    for n_in, n_out in [(1, 64), (2, 64), (64, 1), (511, 64), (1024, 64), (2000, 1280), (37, 37 * 64 // 31), (1000, 32)]:
        first, count, k = FT.resample_table(n_in, n_out)
        assert first.dtype == count.dtype == k.dtype == np.int32 and k.shape == (n_out, k.shape[1])
        assert (first >= 0).all() and (count >= 1).all() and (first + count <= n_in).all() and (count <= k.shape[1]).all()
        assert all((k[i, count[i]:] == 0).all() for i in range(n_out))
        assert (np.abs(k.sum(axis=1) - (1 << 22)) <= k.shape[1]).all()              # the weights sum to one up to their rounding
        assert int(np.abs(k.astype(np.int64)).sum(axis=1).max()) * 255 + (1 << 21) < (1 << 31)      # the sum fits 32-bit integers
        block, ks = FT.axis_block(n_in, n_out)
        assert ks == k.shape[1] and block.size % 4 == 0 and np.array_equal(block[:2 * n_out], np.concatenate([first, count]))
    assert FT.axis_block(64, 64)[1] == 0 and FT.resample_table(5, 3) is FT.resample_table(5, 3)
    with pytest.raises(ValueError):
        FT.resample_table(0, 4)


MIXED = [(1, 1), (2, 1000), (63, 257), (64, 5), (65, 3), (200, 257), (511, 3), (1024, 1000), (64, 64), (128, 1)]


def test_device_tables_read_as_the_header_says_give_pils_batch():
    from handwriting_line_generation_amd.data import fit_tables as FT
    H = 64
    images = [picture(h, w, KINDS[i % 3], seed=3) for i, (h, w) in enumerate(MIXED)] + [picture(63, 257, "random", seed=4)]
    widths = [FT.fitted_width(im.shape[0], im.shape[1], H) for im in images]
    keep = [i for i, w in enumerate(widths) if w <= 1024]                           # (2 x 1000 fits to 32000 columns: the CPU list above has it)
    images, widths = [images[i] for i in keep], [widths[i] for i in keep]
    W = -(-max(widths) // 4) * 4
    lines, coef = FT.batch_tables([im.shape for im in images], H)
    assert lines.dtype == np.int64 and lines.shape == (len(images), FT.ENTRY) and coef.dtype == np.int32 and coef.size % 4 == 0
    assert all(entry_ok(e, coef, sum(im.size for im in images), 1024, H, W) for e in lines)
    same = [i for i, im in enumerate(images) if im.shape == (63, 257)]
    assert len(same) == 2 and tuple(lines[same[0], 4:8]) == tuple(lines[same[1], 4:8])          # lines that share a pair share a table
    assert {int(e[8]) for e in lines} == {0, 1}
    got = emulate(pool_of(images), lines, coef, 1024, H, W)
    assert np.array_equal(got.view(np.int32), expected_batch(images, H, W, widths).view(np.int32))


def _cli():
    import recognize as cli
    return cli


def _png(path, h=40, w=90):
    from PIL import Image
    Image.fromarray(picture(h, w, "stripe")).save(path)


def test_program_refuses_bad_arguments_with_a_sentence(tmp_path):
    cli = _cli()
    d = tmp_path / "lines"
    d.mkdir()
    _png(str(d / "a.png"))
    (d / "notes.txt").write_text("not a picture")
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "notes.txt").write_text("not a picture")
    nolist = tmp_path / "none.txt"
    nolist.write_text("\n")
    gt = tmp_path / "gt.tsv"
    gt.write_text("a.png\thello\nb.png\tworld\n")
    ck, out = str(tmp_path / "absent.pth"), str(tmp_path / "out.txt")
    for argv, word in [(["-i", str(d), "-o", out], "-c"),
                       (["-c", ck, "-o", out], "-i"),
                       (["-c", ck, "-i", str(d)], "-o"),
                       (["-c", ck, "-i", str(empty), "-o", out], "holds no image"),
                       (["-c", ck, "-i", str(nolist), "-o", out], "holds no image"),
                       (["-c", ck, "-i", str(tmp_path / "nowhere"), "-o", out], "neither a directory nor a list"),
                       (["-c", ck, "-i", str(d), "-o", out, "--gt", str(gt)], "'b.png', which is not in the input"),
                       (["-c", ck, "-i", str(d), "-o", out, "--beam", "33"], "outside 0 .. 32"),
                       (["-c", ck, "-i", str(d), "-o", out, "--beam", "-1"], "outside 0 .. 32"),
                       (["-c", ck, "-i", str(d), "-o", out, "--bucket", "30"], "multiple of 4"),
                       (["-c", ck, "-i", str(d), "-o", out, "--batch", "0"], "at least 1"),
                       (["-c", ck, "-i", str(d), "-o", out], "does not exist")]:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert isinstance(e.value.code, str) and e.value.code.startswith("recognize.py: ") and word in e.value.code, (argv, e.value.code)
    assert not (tmp_path / "out.txt").exists()


def test_input_listing_and_gt_reading(tmp_path):
    cli = _cli()
    d = tmp_path / "lines"
    d.mkdir()
    for name in ("b.png", "a.png", "c.png"):
        _png(str(d / name))
    (d / "readme.txt").write_text("no picture")
    assert [n for n, _ in cli.list_input(str(d))] == ["a.png", "b.png", "c.png"]
    lst = tmp_path / "list.txt"
    lst.write_text("lines/c.png\n\n%s\nlines/a.png\n" % (d / "b.png"))
    found = cli.list_input(str(lst))                              # relative paths are found beside the list
    assert [n for n, _ in found] == ["lines/c.png", str(d / "b.png"), "lines/a.png"]
    assert all(cli.read_gray(p).shape == (40, 90) and cli.read_gray(p).dtype == np.uint8 for _, p in found)
    gt = tmp_path / "gt.tsv"
    gt.write_text("c.png\tthird line\twith a tab\na.png\tfirst\n")
    assert cli.read_gt(str(gt), ["a.png", "b.png", "c.png"]) == ["first", None, "third line\twith a tab"]
    with pytest.raises(SystemExit) as e:
        lst.write_text("lines/zzz.png\n")
        cli.list_input(str(lst))
    assert "does not exist" in e.value.code
    assert cli.mean([0.5, 0.25]) == (0 + 0.5 + 0.25) / 2 and cli.mean([]) == 0


@pytest.mark.parametrize("batch,bucket", [(1, 32), (4, 32), (32, 32), (5, 8), (3, 100)])
def test_batching_returns_every_line_once(batch, bucket):
    from handwriting_line_generation_amd.recognize import plan_batches
    widths = [int(v) for v in np.random.RandomState(batch * 100 + bucket).randint(1, 700, 23)] + [32, 32, 64, 1]
    plan = plan_batches(widths, batch, bucket)
    seen = [i for idx, _ in plan for i in idx]
    assert sorted(seen) == list(range(len(widths)))                                 # every index exactly once
    assert [widths[i] for i in seen] == sorted(widths)                              # neighbours in width share a batch
    for idx, W in plan:
        assert 1 <= len(idx) <= batch and W % bucket == 0 and W % 4 == 0
        assert max(widths[i] for i in idx) <= W < max(widths[i] for i in idx) + bucket
    restored = [None] * len(widths)
    for idx, _ in plan:
        for i in idx:
            restored[i] = widths[i]
    assert restored == widths                                                      # results scattered by index restore the input order
    for bad in [(0, 32), (4, 0), (4, 30)]:
        with pytest.raises(ValueError):
            plan_batches(widths, *bad)
    assert plan_batches([], 4, 32) == []
