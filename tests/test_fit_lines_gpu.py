"""GPU: hwg_fit_lines (csrc/fit_lines.hip) at the C ABI under the protocol of tests/_guarded.py - operands carved out of one allocation with
canaries, poisoned output, inputs bit-identical afterwards, a second call with the same bits, refusals that write nothing - and through
ops.fit_lines. The oracle is PIL itself: the output equals 1 - Image.resize((out_w, H), BICUBIC) / 128 bit for bit on the fitted columns
and is -1 beyond; no tolerance anywhere (integers, and levels that are exact in fp32).

The bad table entries name memory inside this file's one allocation only (the pool and the coefficient buffer are handed over MARGIN
bytes / elements into what is allocated and with zeros behind what is stated), so a guard that is wrong shows as a wrong byte, never
as a fault."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _fit_lines_ref import MAX_IN_H, emulate, expected_batch, picture, pool_of  # noqa: E402
from _guarded import HWG_ERR_ARG, Guarded, protocol, refused, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

H = 64
MARGIN = 64                     # bytes of the pool / elements of the coefficient buffer in front of what the entry is handed
SLACK = 4096                    # zeros behind what is stated
# heights {1, 2, 63, 64, 65, 200, the documented maximum} x widths {1, 3, 5, 257, 1000}: both passes, each pass alone, none (64 x 1000),
# a tile that ends off a multiple of 64 columns, more than one tile, the vertical-first order (1024 x 3), 64 KiB of LDS
SHAPES = [(1, 5), (2, 3), (63, 257), (64, 1000), (65, 1000), (200, 1), (MAX_IN_H, 1000), (MAX_IN_H, 3)]


def _lib():
    from handwriting_line_generation_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def batch():
    """the pictures, their tables and PIL's batch - computed once, shared, never changed"""
    from handwriting_line_generation_amd.data import fit_tables as FT
    images = [picture(h, w, ("random", "two-level", "stripe")[i % 3], seed=11) for i, (h, w) in enumerate(SHAPES)]
    widths = [FT.fitted_width(h, w, H) for h, w in SHAPES]
    W = -(-max(widths) // 4) * 4
    assert len(images) == 8 and W <= 1024 and W > 64
    lines, coef = FT.batch_tables(SHAPES, H)
    want = expected_batch(images, H, W, widths)
    for a in (lines, coef, want):
        a.setflags(write=False)
    return dict(images=images, widths=widths, W=W, lines=lines, coef=coef, want=want, pool=pool_of(images))


def _guarded(cuda, pool, lines, coef, B, W):
    px = np.zeros(-(-(MARGIN + pool.size + SLACK) // 4) * 4, dtype=np.uint8)
    px[MARGIN:MARGIN + pool.size] = pool
    cf = np.zeros(MARGIN + coef.size + SLACK, dtype=np.int32)
    cf[MARGIN:MARGIN + coef.size] = coef
    return Guarded(cuda, dict(pixels=torch.from_numpy(px), lines=torch.from_numpy(np.array(lines)), coef=torch.from_numpy(cf)),
                   dict(out=((B, 1, H, W), torch.float32)))


def _call(G, sizes, **kw):
    """sizes: (pixel_bytes, coef_elems, max_in_h, B, W) of the good call; kw: the arguments a refusal case replaces"""
    pool_bytes, coef_elems, max_in_h, B, W = sizes
    a = dict(pixels=G.t("pixels")[MARGIN:], pixel_bytes=pool_bytes, lines=G.t("lines"), coef=G.t("coef")[MARGIN:], coef_elems=coef_elems,
             max_in_h=max_in_h, B=B, H=H, W=W, out=G.f["out"])
    a.update(kw)
    return _lib().query("hwg_fit_lines", a["pixels"], a["pixel_bytes"], a["lines"], a["coef"], a["coef_elems"], a["max_in_h"], a["B"], a["H"],
                        a["W"], a["out"], G.st)


def _run(cuda, tag, pool, lines, coef, W, max_in_h=MAX_IN_H):
    B = lines.shape[0]
    G = _guarded(cuda, pool, lines, coef, B, W)
    got = protocol(G, tag, lambda ws, n: _call(G, (pool.size, coef.size, max_in_h, B, W)))
    return got["out"]


def test_mixed_batch_is_pils_batch_bit_for_bit(cuda, batch):
    got = _run(cuda, "fit_lines mixed", batch["pool"], batch["lines"], batch["coef"], batch["W"])
    want = torch.from_numpy(batch["want"])
    for b, w in enumerate(batch["widths"]):
        assert same_bits(got[b, 0, :, :w], want[b, 0, :, :w]), "line %d (%s -> %d columns) differs from PIL" % (b, SHAPES[b], w)
        assert bool((got[b, 0, :, w:] == -1.0).all()), "line %d: padding" % b
    assert same_bits(got, want)
    assert np.array_equal(emulate(batch["pool"], batch["lines"], batch["coef"], MAX_IN_H, H, batch["W"]).view(np.int32), batch["want"].view(np.int32))


def test_a_line_alone_and_in_the_batch_gives_the_same_bits(cuda, batch):
    from handwriting_line_generation_amd.data import fit_tables as FT
    whole = _run(cuda, "fit_lines mixed", batch["pool"], batch["lines"], batch["coef"], batch["W"])
    for b in (0, 2, 4, 6, 7):
        lines, coef = FT.batch_tables([SHAPES[b]], H)
        alone = _run(cuda, "fit_lines alone %d" % b, pool_of([batch["images"][b]]), lines, coef, batch["W"], max_in_h=SHAPES[b][0])
        assert same_bits(alone[0], whole[b]), "line %d alone differs from the line in the batch" % b


def _bad_tables(batch):
    """-> (lines, coef, {row: why}): the batch's tables with six entries made bad, the other two rows untouched"""
    lines, coef = batch["lines"].copy(), batch["coef"].copy()
    W, pool_bytes = batch["W"], batch["pool"].size
    why = {}
    lines[0, 0] = -4;                                   why[0] = "a negative offset"
    assert lines[1, 5] > 0
    lines[1, 4] += 2;                                   why[1] = "a coefficient table at no multiple of 4"
    h, w = SHAPES[7]
    assert lines[7, 0] + h * w == pool_bytes
    lines[7, 0] += 1;                                   why[7] = "a line that ends one byte behind pixel_bytes"
    lines[4, 3] = W + 4;                                why[4] = "out_w > W"
    # row 2 gets a private copy of its horizontal table whose last window leaves the picture by one pixel
    ow, ks, tab = int(lines[2, 3]), int(lines[2, 5]), int(lines[2, 4])
    n = -(-(ow * (2 + ks)) // 4) * 4
    private = coef[tab:tab + n].copy()
    private[ow - 1] += 1
    assert private[ow - 1] + private[2 * ow - 1] == SHAPES[2][1] + 1
    lines[2, 4] = coef.size
    coef = np.concatenate([coef, private])
    why[2] = "a tap window past the picture's edge"
    assert lines[5, 7] > 0
    lines[5, 6] = coef.size - 4;                        why[5] = "a vertical table that ends outside the coefficient buffer"
    return lines, coef, why


def test_bad_table_entries_become_padding_and_the_others_stay(cuda, batch):
    lines, coef, why = _bad_tables(batch)
    assert sorted(set(range(8)) - set(why)) == [3, 6]
    got = _run(cuda, "fit_lines bad entries", batch["pool"], lines, coef, batch["W"])
    want = torch.from_numpy(batch["want"])
    for b in range(8):
        if b in why:
            assert bool((got[b] == -1.0).all()), "row %d (%s) is not padding" % (b, why[b])
        else:
            assert same_bits(got[b], want[b]), "the good row %d differs from PIL next to bad rows" % b
    assert np.array_equal(emulate(batch["pool"], lines, coef, MAX_IN_H, H, batch["W"]).view(np.int32), got.numpy().view(np.int32))
    # a picture taller than the caller states: padding as well (the LDS is sized by max_in_h)
    got = _run(cuda, "fit_lines max_in_h 200", batch["pool"], batch["lines"], batch["coef"], batch["W"], max_in_h=200)
    for b, (h, _) in enumerate(SHAPES):
        assert bool((got[b] == -1.0).all()) if h > 200 else same_bits(got[b], want[b]), b


def test_calls_beyond_the_limits_are_refused(cuda, batch):
    W, B = batch["W"], 8
    G = _guarded(cuda, batch["pool"], batch["lines"], batch["coef"], B, W)
    n, m = batch["pool"].size, batch["coef"].size
    out = G.f["out"]
    for kw, word in [(dict(pixels=None), "null"), (dict(lines=None), "null"), (dict(coef=None), "null"), (dict(out=None), "null"),
                     (dict(B=0), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"), (dict(W=-4), "bad sizes"),
                     (dict(pixel_bytes=0), "bad sizes"), (dict(coef_elems=0), "bad sizes"), (dict(max_in_h=0), "bad sizes"),
                     (dict(B=65536), "beyond the limit"), (dict(H=1025), "beyond the limit"), (dict(W=(1 << 20) + 4), "beyond the limit"),
                     (dict(max_in_h=MAX_IN_H + 1), "beyond the limit"), (dict(W=W + 2), "multiple of 4"),
                     (dict(out=out.data_ptr() + 4), "aligned"), (dict(coef=G.t("coef")[MARGIN:].data_ptr() + 4), "aligned"),
                     (dict(lines=G.t("lines").data_ptr() + 4), "aligned")]:
        refused(G, "fit_lines %s" % kw, lambda: _call(G, (n, m, MAX_IN_H, B, W), **kw), HWG_ERR_ARG)
        assert word in _lib().last_error(), (kw, _lib().last_error())
    assert _call(G, (n, m, MAX_IN_H, B, W)) == 0                                      # and the good call still runs
    G.sync()
    assert same_bits(G.get("out"), torch.from_numpy(batch["want"])) and G.intact() and G.untouched()


def test_ops_fit_lines_in_limit_list_takes_no_fallback(cuda, batch):
    from handwriting_line_generation_amd import ops
    before = ops.fit_fallbacks
    got, widths = ops.fit_lines(batch["images"], H, device=cuda)
    torch.cuda.synchronize()
    assert widths == batch["widths"] and tuple(got.shape) == (8, 1, H, batch["W"]) and got.dtype == torch.float32
    assert same_bits(got, torch.from_numpy(batch["want"]))
    # a wider batch into a caller's buffer: the same columns, padding behind, nothing behind the batch
    W = batch["W"] + 24
    buf = torch.full((8 * H * W + 64,), float("nan"), dtype=torch.float32, device=cuda)
    got, _ = ops.fit_lines(batch["images"], H, W=W, out=buf)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and bool(torch.isnan(buf[8 * H * W:]).all())
    assert same_bits(got.cpu(), torch.from_numpy(expected_batch(batch["images"], H, W, batch["widths"])))
    assert ops.fit_fallbacks == before                                             # a condition, not a measurement
    with pytest.raises(ops.L.HwgError):
        ops.fit_lines(batch["images"], H, W=batch["W"] - 4, device=cuda)
    with pytest.raises(ops.L.HwgError):
        ops.fit_lines([batch["images"][0].astype(np.float32)], H, device=cuda)
    with pytest.raises(ops.L.HwgError):
        ops.fit_lines([], H, device=cuda)


def test_ops_fit_lines_sends_a_line_above_the_height_limit_through_the_host(cuda, batch, capfd):
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.data import fit_tables as FT
    tall = picture(MAX_IN_H + 1, 300, "random", seed=5)
    images = [batch["images"][2], tall, batch["images"][6]]
    widths = [FT.fitted_width(im.shape[0], im.shape[1], H) for im in images]
    before = ops.fit_fallbacks
    got, got_w = ops.fit_lines(images, H, device=cuda)
    torch.cuda.synchronize()
    assert ops.fit_fallbacks == before + 1 and got_w == widths
    assert same_bits(got.cpu(), torch.from_numpy(expected_batch(images, H, -(-max(widths) // 4) * 4, widths)))
    ops.fit_lines([tall], H, device=cuda)
    assert ops.fit_fallbacks == before + 2
    assert capfd.readouterr().err.count("fit_lines:") <= 1                           # said once per process
