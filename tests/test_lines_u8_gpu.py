"""GPU: hwg_lines_to_u8 (csrc/lines_out.hip) through ops.lines_to_u8 - the generator's fp32 image to ragged 8-bit lines. The expectation
is numpy's ((1 - x) * 127.5).astype(uint8) in float32 on the very input that was uploaded: exact equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 64
FILL = 0xA5


def _numpy_u8(x):
    assert x.dtype == np.float32
    v = (np.float32(1.0) - x) * np.float32(127.5)
    assert v.dtype == np.float32
    return v.astype(np.uint8)


def _run(img, widths, slack=64, **kw):
    """-> (pixels as numpy, offsets, the `slack` bytes behind them); the output buffer is pre-filled with 0xA5"""
    from handwriting_line_generation_amd import ops
    total = H * int(sum(widths))
    out = torch.full((total + slack,), FILL, dtype=torch.uint8, device="cuda")
    pixels, offsets = ops.lines_to_u8(ops.h2d(torch.from_numpy(img), torch.device("cuda:0")), widths, out=out, **kw)
    torch.cuda.synchronize()
    assert pixels.dtype == torch.uint8 and pixels.dim() == 1 and pixels.numel() == total and pixels.data_ptr() == out.data_ptr()
    assert isinstance(offsets, np.ndarray) and offsets.dtype == np.int64 and offsets.shape == (len(widths) + 1,)
    host = out.cpu().numpy()
    return host[:total], offsets, host[total:]


def test_truncation_boundaries_match_numpy_exactly(cuda):
    """every point at which the truncation flips: fp32 1 - k / 127.5 and its two neighbours for k = 0..255, with exact 1, -1 and 0"""
    W = 1024
    k = np.arange(256, dtype=np.float64)
    t = (1.0 - k / 127.5).astype(np.float32)
    special = np.concatenate([t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf)),
                              np.asarray([1.0, -1.0, 0.0], dtype=np.float32)])
    x = np.random.RandomState(17).uniform(-1.0, 1.0, H * W).astype(np.float32)
    pos = np.random.RandomState(18).permutation(H * W)[:special.size]
    x[pos] = special
    img = x.reshape(1, 1, H, W)
    with np.errstate(invalid="ignore"):
        want = _numpy_u8(img[0, 0])
    got, offsets, tail = _run(img, [W])
    assert offsets.tolist() == [0, H * W]
    assert np.array_equal(got.reshape(H, W), want)
    assert got.min() == 0 and got.max() == 255
    assert (tail == FILL).all()


@pytest.mark.parametrize("W,widths", [(40, [40, 12, 4, 36]), (1040, [1040, 1028, 260])])
def test_ragged_packing(cuda, W, widths):
    """each line is its own crop, converted, back to back; nothing behind the last line is written; columns >= widths[b] (NaN here) never
    reach the output. The wide case crosses the 1024 columns a workgroup takes and ends off a multiple of 256 lanes."""
    B = len(widths)
    img = np.random.RandomState(W).uniform(-1.0, 1.0, (B, 1, H, W)).astype(np.float32)
    for b, w in enumerate(widths):
        img[b, 0, :, w:] = np.nan
    got, offsets, tail = _run(img, widths)
    assert offsets.tolist() == [0] + (H * np.cumsum(widths)).tolist()
    for b, w in enumerate(widths):
        line = got[offsets[b]:offsets[b + 1]].reshape(H, w)
        assert np.array_equal(line, _numpy_u8(np.ascontiguousarray(img[b, 0, :, :w]))), b
    assert (tail == FILL).all()


def test_outside_the_range_clamps(cuda):
    """numpy's astype wraps outside [-1, 1]; the kernel clamps, NaN is 0"""
    W = 8
    img = np.zeros((1, 1, H, W), dtype=np.float32)
    img[0, 0, 3, :5] = [-1.5, 1.5, np.inf, -np.inf, np.nan]
    got, _, tail = _run(img, [W])
    got = got.reshape(H, W)
    assert got[3, :5].tolist() == [255, 0, 0, 255, 0]
    assert (np.delete(got.reshape(-1), np.arange(3 * W, 3 * W + 5)) == 127).all()      # (1 - 0) * 127.5 truncates to 127
    assert (tail == FILL).all()


@pytest.mark.parametrize("W,widths,offsets", [
    (40, [40, 6, 4], None),            # a width that is no multiple of 4
    (40, [40, 0, 4], None),            # an empty line
    (40, [40, 44, 4], None),           # wider than the image
    (40, [40, 12, 4], [0, 2562, 3328, 3584]),      # a misaligned offset
    (40, [40, 12, 4], [0, 2560, 3328, 3400]),      # a line that ends behind the bytes in use
    (42, [40, 12, 4], None),           # an image width that is no multiple of 4
    (40, [40, 12], None),              # one width too few
])
def test_refusals_never_launch(cuda, W, widths, offsets):
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd._lib import HwgError
    img = torch.zeros((3, 1, H, W), dtype=torch.float32, device=cuda)
    out = torch.full((H * 3 * 48,), FILL, dtype=torch.uint8, device=cuda)
    calls, orig = [], ops.L.call

    def call(fn, *a):
        calls.append(fn)
        return orig(fn, *a)
    ops.L.call = call
    try:
        with pytest.raises(HwgError):
            ops.lines_to_u8(img, widths, out=out, offsets=offsets)
    finally:
        ops.L.call = orig
    torch.cuda.synchronize()
    assert calls == []                                   # refused on the host, before anything was uploaded or launched
    assert bool((out == FILL).all())


def test_entry_point_refuses_bad_sizes_itself(cuda):
    """the checks the entry point can make on its own arguments (the tables are device arrays: theirs are ops.lines_to_u8's)"""
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd._lib import HwgError
    img = torch.zeros((1, 1, H, 44), dtype=torch.float32, device=cuda)
    widths = torch.tensor([40], dtype=torch.int32, device=cuda)
    offsets = torch.tensor([0], dtype=torch.int64, device=cuda)
    out = torch.full((H * 48,), FILL, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    for args in [(img, 1, H, 42, widths, offsets, out), (img, 0, H, 44, widths, offsets, out), (img, 1, H, 44, None, offsets, out),
                 (img, 1, H, 44, widths, offsets, out.data_ptr() + 2), (img.data_ptr() + 4, 1, H, 40, widths, offsets, out)]:
        with pytest.raises(HwgError):
            ops.L.call("hwg_lines_to_u8", *args, st)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
