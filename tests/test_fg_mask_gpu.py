"""GPU: hwg_fg_masks (csrc/fg_mask.hip) through ops.fg_masks - Otsu threshold, inversion and dilation with the 9 x 9 ellipse of every line of a
ragged 8-bit pool in one launch - bit for bit against the numpy restatement tests/_fg_mask_ref.py (explicit OR over the element's 57
offsets; cross-checked against scipy and on hand-written cases by tests/test_fg_mask_cpu.py, which also shows that no line of the pool
rests on a last-bit fp64 difference between two Otsu splits)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fg_mask_ref as F  # noqa: E402
from _gpu_tidy import leave_nothing_behind  # noqa: E402,F401  (module-scoped, autouse)


@pytest.fixture(scope="module", params=[64, 16], ids=["H64", "H16"])
def run(request, cuda):
    """the pool of tests/_fg_mask_ref.pool(H) once through the kernel (into an output buffer pre-filled with the guard value) and once
    through the restatement"""
    from handwriting_line_generation_amd import ops
    H = request.param
    names, lines, pixels, offsets, widths = F.pool(H)
    px = ops.h2d(torch.from_numpy(pixels), cuda)
    out = torch.full((pixels.size,), F.GUARD, dtype=torch.uint8, device=cuda)
    got, thr = ops.fg_masks(px, offsets, widths, height=H, out=out, want_thresholds=True)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return {"H": H, "names": names, "lines": lines, "pixels": pixels, "offsets": offsets, "widths": widths, "px_after": px.cpu().numpy(),
            "got": got.cpu().numpy(), "thr": thr.cpu().numpy(), "ref": [F.fg_mask(l) for l in lines]}


def test_masks_are_bit_equal_to_the_restatement(run):
    H = run["H"]
    for k, (name, line) in enumerate(zip(run["names"], run["lines"])):
        o, w = int(run["offsets"][k]), run["widths"][k]
        got = run["got"][o:o + H * w].reshape(H, w)
        want, t = run["ref"][k]
        assert int(run["thr"][k]) == t, "line %s: threshold %d, restatement %d" % (name, int(run["thr"][k]), t)
        bad = np.argwhere(got != want)
        assert not len(bad), "line %s (%d x %d, threshold %d): %d pixels differ, first at %s" % (name, H, w, t, len(bad), bad[0].tolist())
    print("\nfg masks H=%d: %d lines, widths %s, bit-equal; thresholds %s" % (H, len(run["lines"]), run["widths"], run["thr"].tolist()))


def test_guard_bytes_and_the_input_pool_come_back_untouched(run):
    H = run["H"]
    line_bytes = np.zeros(run["pixels"].size, dtype=bool)
    for k, w in enumerate(run["widths"]):
        line_bytes[int(run["offsets"][k]):int(run["offsets"][k]) + H * w] = True
    assert int((~line_bytes).sum()) > 2 * len(run["widths"])
    assert (run["got"][~line_bytes] == F.GUARD).all(), "bytes between the lines were written"
    assert set(np.unique(run["got"][line_bytes])) <= {0, 255}
    assert np.array_equal(run["px_after"], run["pixels"]), "the input pool was written"


def test_thresholds_are_the_augmentations(run, cuda):
    """the same pixels as a collated fp32 batch through ops.augment_lines (zero brightness shifts, zero displacements): its stats kernel
    reports the same Otsu level per line"""
    from handwriting_line_generation_amd import ops
    H, lines, widths = run["H"], run["lines"], run["widths"]
    W = max(widths)
    x = np.full((len(lines), 1, H, W), -1.0, dtype=np.float32)
    for b, l in enumerate(lines):
        x[b, 0, :, :l.shape[1]] = 1.0 - l.astype(np.float32) / 128.0
    disp = []
    for w in widths:
        src = ops.warp_lattice(H, w) if (H > 5 and w > 5) else None
        disp.append(None if src is None else (np.zeros((len(src[0]), len(src[1]))), np.zeros((len(src[0]), len(src[1])))))
    mesh = ops.LineMesh(H, widths, disp=disp)
    _, _, stats = ops.augment_lines(torch.from_numpy(x).to(cuda), mesh, fg_bg=np.zeros((len(lines), 2)), want_map=True)
    assert stats[:, 0].cpu().tolist() == run["thr"].tolist()


def test_default_output_is_zero_between_the_lines(cuda):
    from handwriting_line_generation_amd import ops
    names, lines, pixels, offsets, widths = F.pool(16)
    got = ops.fg_masks(ops.h2d(torch.from_numpy(pixels), cuda), offsets, widths, height=16).cpu().numpy()
    for k, line in enumerate(lines):
        o = int(offsets[k])
        assert np.array_equal(got[o:o + line.size].reshape(line.shape), F.fg_mask(line)[0])
        got[o:o + line.size] = 0
    assert not got.any()


def test_host_tables_are_validated_before_any_launch(cuda, monkeypatch):
    from handwriting_line_generation_amd import _lib as L, ops
    calls = []
    monkeypatch.setattr(L, "call", lambda *a, **k: calls.append(a[0]))
    px = torch.zeros(64 * 40, dtype=torch.uint8, device=cuda)
    bad = [
        ("negative width", dict(offsets=[0, 64 * 8, 64 * 40], widths=[8, -3])),
        ("zero width", dict(offsets=[0, 64 * 8, 64 * 40], widths=[8, 0])),
        ("overlapping offsets", dict(offsets=[0, 64 * 8 - 1, 64 * 40], widths=[8, 8])),
        ("overlapping, listed out of order", dict(offsets=[64 * 4, 0, 64 * 40], widths=[8, 8])),
        ("negative offset", dict(offsets=[-1, 64 * 8, 64 * 40], widths=[8, 8])),
        ("line behind the pool", dict(offsets=[0, 64 * 33, 64 * 40], widths=[8, 8])),
        ("pool behind the buffer", dict(offsets=[0, 64 * 8, 64 * 40 + 1], widths=[8, 8])),
        ("offsets of the wrong length", dict(offsets=[0, 64 * 8], widths=[8, 8])),
        ("H > 64", dict(offsets=[0, 65 * 8, 64 * 40], widths=[8, 8], height=65)),
        ("H < 1", dict(offsets=[0, 0, 64 * 40], widths=[8, 8], height=0)),
    ]
    for what, kw in bad:
        with pytest.raises(L.HwgError, match="fg_masks"):
            ops.fg_masks(px, **kw)
        assert not calls, what
    with pytest.raises(L.HwgError, match="fg_masks"):
        ops.fg_masks(px.cpu(), [0, 64 * 8], [8])
    with pytest.raises(L.HwgError, match="fg_masks"):
        ops.fg_masks(px, [0, 64 * 8], [8], out=px)
    assert not calls
    ops.fg_masks(px, [64 * 4, 0, 64 * 40], [8, 4])             # out of order without overlap is fine
    assert calls == ["hwg_fg_masks"]
