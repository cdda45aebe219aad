"""GPU: the sample-sheet kernels (csrc/sample_sheet.hip: hwg_sheet_minmax + hwg_sheet_compose) through ops.sample_sheet against
tests/_sheet_ref.py, torchvision's save_image(1 - images, nrow, normalize=True) restated with torch CPU operations. Byte equality, no
tolerance: for finite input every step is a correctly rounded fp32 operation on both sides."""
import pytest
import torch

import _sheet_ref as ref

pytestmark = pytest.mark.gpu

FILL = 0xAB
GUARD = 64


def _uniform(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def _sheet(x, nrow=None):
    """ops.sample_sheet on the uploaded batch, written into a buffer pre-filled with FILL between two guards -> the sheet on the host"""
    from handwriting_line_generation_amd import ops
    B, _, H, W = x.shape
    hs, ws, _ = ops.sample_sheet_shape(B, H, W, nrow)
    need = -(-hs * ws // 4) * 4
    buf = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    got = ops.sample_sheet(ops.h2d(x, torch.device("cuda:0")), nrow=nrow, out=buf[GUARD:])     # (out may be larger than the sheet)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.is_cuda and got.data_ptr() == buf.data_ptr() + GUARD
    host = buf.cpu()
    assert bool((host[:GUARD] == FILL).all()) and bool((host[GUARD + need:] == FILL).all()), "bytes outside the sheet (rounded up to 4) were written"
    return got.cpu()


GEOMETRY = [(1, 5, 7, 3), (2, 3, 8, 4), (5, 4, 6, 3), (3, 64, 9, 1), (4, 2, 1, 2), (8, 64, 512, None), (2, 64, 1028, None)]


@pytest.mark.parametrize("B,H,W,nrow", GEOMETRY)
def test_geometry(cuda, B, H, W, nrow):
    """no border (B = 1), one row, a last row with an empty cell, a column of odd width, one-pixel-wide images, nrow from the width
    (4 and 1); random values in [-1, 1]"""
    x = _uniform((B, 1, H, W), 100 + B * W)
    want = ref.sheet(x, nrow)
    got = _sheet(x, nrow)
    assert tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got, want), "%d bytes differ" % int((got != want).sum())


@pytest.mark.parametrize("B,H,W,nrow", [(1, 5, 7, 3), (3, 5, 9, 1), (5, 4, 6, 3), (4, 2, 1, 2)])
def test_every_byte_is_written(cuda, B, H, W, nrow):
    """out starts as 0xAB: afterwards borders and empty cells are 0 and no fill is left inside the sheet (35- and 253-byte sheets end off a
    multiple of 4: _sheet checks that nothing behind the rounded-up end is touched)"""
    x = _uniform((B, 1, H, W), 7) * 0.25 + 0.5                       # v in [0.25, 0.75], range 0.5
    got = _sheet(x, nrow)
    want = ref.sheet(x, nrow)
    assert torch.equal(got, want)
    if B > 1:
        cells = torch.zeros_like(want, dtype=torch.bool)
        xmaps = min(nrow, B)
        for k in range(B):
            r, c = (k // xmaps) * (H + 2) + 2, (k % xmaps) * (W + 2) + 2
            cells[r:r + H, c:c + W] = True
        assert bool((got[~cells] == 0).all())
        assert int((~cells).sum()) > 0


@pytest.mark.parametrize("where", ["first_last", "last_first", "middles"])
def test_extremes_anywhere(cuda, where):
    """8 x 64 x 512 spans 64 workgroups of the reduction: the only minimum and the only maximum of v at the first element, the last one,
    and in the middle of different images"""
    B, H, W = 8, 64, 512
    x = _uniform((B, 1, H, W), 31, -0.9, 0.9)
    flat = x.view(-1)
    n = flat.numel()
    mid = lambda k: k * H * W + (H // 2) * W + W // 2 + 1      # noqa: E731
    lo_at, hi_at = {"first_last": (0, n - 1), "last_first": (n - 1, 0), "middles": (mid(2), mid(5))}[where]
    flat[lo_at] = 1.0        # v = 0: the minimum
    flat[hi_at] = -1.0       # v = 2: the maximum
    want = ref.sheet(x)
    got = _sheet(x)
    assert torch.equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert int(got.max()) == 255


def test_degenerate_ranges(cuda):
    """a constant batch: d = 1e-5, every pixel 0. A range of 50 ulps (3e-6 < 1e-5: d is still 1e-5) and one of 168 ulps of 2^-24
    (1.0014e-5, exactly representable, just above 1e-5: d is the range itself)"""
    B, H, W = 3, 6, 10
    const = torch.full((B, 1, H, W), 0.3, dtype=torch.float32)
    got = _sheet(const, 2)
    assert torch.equal(got, ref.sheet(const, 2)) and int(got.max()) == 0
    for ulps in (50, 168):
        j = torch.randint(0, ulps + 1, (B, 1, H, W), generator=torch.Generator().manual_seed(ulps))
        j.view(-1)[3], j.view(-1)[-5] = 0, ulps
        x = (0.5 - j.double() * 2.0 ** -24).float()                 # exact: v = 1 - x = 0.5 + j 2^-24
        assert float((1 - x).max() - (1 - x).min()) == ulps * 2.0 ** -24
        want = ref.sheet(x, 2)
        got = _sheet(x, 2)
        assert torch.equal(got, want), (ulps, int((got != want).sum()))
        assert int(want.max()) == (255 if ulps == 168 else 76)      # 2.98e-6 / 1e-5 * 255 + 0.5 = 76.49


def test_both_roundings_are_kept(cuda):
    """n * 255 + 0.5 rounded twice, as torchvision does, on a seeded 4 x 64 x 256 batch. This test was meant to first show, on the CPU, a
    seed on which the fused restatement (_sheet_ref.sheet_fused: one rounding, as an fma) differs from the unfused one. No such seed
    exists: a scan of ALL 1 065 353 217 fp32 values n in [0, 1] finds none at which trunc(fl(n * 255 + 0.5)) differs from
    trunc(fl(fl(n * 255) + 0.5)) (the one place where the sum is rounded at all below a byte boundary, products in [0.25, 0.5), holds no
    representable n inside the 1.5e-8 wide window that would flip byte 0 / 1), and seeds 0..59 of this batch agree byte for byte.
    So that precondition cannot be asserted. What is asserted instead asks no less of the kernel: on top of the seeded batch, values
    within an ulp of EVERY rounding boundary (k - 0.5) / 255, k = 1..255, where any deviation from the two correctly rounded operations
    shows first, and the kernel equals the unfused restatement byte for byte. The kernel itself keeps the two roundings (contract off)."""
    x = _uniform((4, 1, 64, 256), 5)
    flat = x.view(-1)
    k = torch.arange(1, 256, dtype=torch.float64)
    v = 2.0 * (k - 0.5) / 255.0                                     # lo = 0, hi = 2 planted below: d = 2, n = v / 2
    xs = torch.cat([(1.0 - v).float(), torch.nextafter((1.0 - v).float(), torch.tensor(2.0)), torch.nextafter((1.0 - v).float(), torch.tensor(-2.0))])
    pos = torch.randperm(flat.numel() - 2, generator=torch.Generator().manual_seed(6))[:xs.numel()] + 1
    flat[pos] = xs
    flat[0], flat[-1] = 1.0, -1.0
    want, fused = ref.sheet(x), ref.sheet_fused(x)
    print("bytes on which the fused restatement differs from the unfused one: %d" % int((want != fused).sum()))
    got = _sheet(x)
    assert torch.equal(got, want), "%d bytes differ" % int((got != want).sum())


def test_non_finite_values(cuda):
    """lo / hi over the finite values; NaN -> 0, v = +inf -> 255, v = -inf -> 0; nothing finite -> an all-0 sheet"""
    B, H, W, nrow = 5, 7, 13, 3
    x = _uniform((B, 1, H, W), 77)
    flat = x.view(-1)
    pos = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(78))
    flat[pos[:9]] = float("nan")
    flat[pos[9:15]] = float("inf")
    flat[pos[15:21]] = float("-inf")
    flat[0], flat[-1] = float("nan"), float("-inf")
    want = ref.sheet_nonfinite(x, nrow)
    got = _sheet(x, nrow)
    assert torch.equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert int((want == 255).sum()) >= 7 and int(want.max()) == 255
    for fill in ([float("nan")], [float("nan"), float("inf"), float("-inf")]):
        y = torch.tensor(fill, dtype=torch.float32).repeat(B * H * W // len(fill) + 1)[:B * H * W].reshape(B, 1, H, W).contiguous()
        got = _sheet(y, nrow)
        assert tuple(got.shape) == tuple(want.shape) and int(got.max()) == 0
        assert torch.equal(got, ref.sheet_nonfinite(y, nrow))


def test_refusals_never_launch(cuda):
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd._lib import HwgError
    good = torch.zeros((3, 1, 4, 6), dtype=torch.float32, device=cuda)          # sheet: 20 x 10 = 200 bytes
    out = torch.full((256,), FILL, dtype=torch.uint8, device=cuda)
    calls, orig = [], ops.L.call

    def call(fn, *a):
        calls.append(fn)
        return orig(fn, *a)
    ops.L.call = call
    try:
        for args, kw in [((good.cpu(),), {}), ((good[:, 0],), {}), ((good,), {"nrow": 0}), ((good,), {"nrow": 1, "out": out[:196]}),
                         ((good,), {"nrow": 1, "out": out[2:]}), ((good.double(),), {}), ((good.expand(3, 2, 4, 6),), {})]:
            with pytest.raises(HwgError):
                ops.sample_sheet(*args, **kw)
    finally:
        ops.L.call = orig
    torch.cuda.synchronize()
    assert calls == []
    assert bool((out == FILL).all())


def test_entry_points_refuse_bad_arguments_themselves(cuda):
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd._lib import HwgError
    x = torch.zeros((3, 1, 4, 6), dtype=torch.float32, device=cuda)
    parts = torch.zeros((4, 2), dtype=torch.float32, device=cuda)
    out = torch.full((256,), FILL, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert ops.L.query("hwg_sheet_parts", 72) == 1 and ops.L.query("hwg_sheet_parts", 8 * 64 * 512) == 64 and ops.L.query("hwg_sheet_parts", 1 << 40) == 256
    for args in [(None, 72, parts, 1), (x, 0, parts, 1), (x, 72, None, 1), (x, 72, parts, 2), (x, 72, parts.data_ptr() + 2, 1)]:
        with pytest.raises(HwgError):
            ops.L.call("hwg_sheet_minmax", *args, st)
    for args in [(None, 3, 4, 6, 1, parts, 1, out, 256), (x, 0, 4, 6, 1, parts, 1, out, 256), (x, 3, 0, 6, 1, parts, 1, out, 256),
                 (x, 3, 4, 0, 1, parts, 1, out, 256), (x, 3, 4, 6, 0, parts, 1, out, 256), (x, 3, 4, 6, 1, None, 1, out, 256),
                 (x, 3, 4, 6, 1, parts, 0, out, 256), (x, 3, 4, 6, 1, parts, 257, out, 256), (x, 3, 4, 6, 1, parts, 1, None, 256),
                 (x, 3, 4, 6, 1, parts, 1, out, 199), (x, 3, 4, 6, 1, parts, 1, out.data_ptr() + 1, 255),
                 (x, 1, 65536, 65536, 1, parts, 1, out, 1 << 40), (x, 70000, 64, 512, 1, parts, 1, out, 1 << 40)]:
        with pytest.raises(HwgError):
            ops.L.call("hwg_sheet_compose", *args, st)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
