"""GPU: hwg_lines_from_u8 (csrc/lines_out.hip) through ops.lines_from_u8 - ragged 8-bit lines back into a collated fp32 batch, mixed with the
rows of a real batch. Every expectation is exact equality: the levels are integers and 1 - p / 128 is exact in fp32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 64
SLACK = 64


def _levels(p):
    assert p.dtype == np.uint8
    v = np.float32(1.0) - p.astype(np.float32) / np.float32(128.0)
    assert v.dtype == np.float32
    return v


def _pool(lines):
    """uint8 [H, w] lines -> (pixels host uint8 1-D, offsets int64, widths int32) in the layout hwg_lines_to_u8 writes"""
    widths = np.asarray([l.shape[1] for l in lines], dtype=np.int32)
    offsets = np.zeros(len(lines), dtype=np.int64)
    offsets[1:] = np.cumsum(H * widths.astype(np.int64))[:-1]
    return np.concatenate([l.reshape(-1) for l in lines]), offsets, widths


def _random_lines(widths, seed):
    g = np.random.RandomState(seed)
    return [g.randint(0, 256, (H, w)).astype(np.uint8) for w in widths]


def _run(lines, select, real=None, W=None):
    """-> (out as numpy [B,1,H,W], the SLACK floats behind it); the output buffer is pre-filled with NaN"""
    from handwriting_line_generation_amd import ops
    dev = torch.device("cuda:0")
    pixels, offsets, widths = _pool(lines)
    B = len(select)
    buf = torch.full((B * H * W + SLACK,), float("nan"), dtype=torch.float32, device=dev)
    real_d = None if real is None else ops.h2d(torch.from_numpy(real), dev)
    out = ops.lines_from_u8(ops.h2d(torch.from_numpy(pixels), dev), offsets, widths, select, real=real_d, out=buf)
    torch.cuda.synchronize()
    assert out.shape == (B, 1, H, W) and out.dtype == torch.float32 and out.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    return host[:B * H * W].reshape(B, 1, H, W), host[B * H * W:]


def _expect(lines, select, real, W):
    want = np.full((len(select), 1, H, W), -1.0, dtype=np.float32)
    for b, s in enumerate(select):
        if s >= 0:
            want[b, 0, :, :lines[s].shape[1]] = _levels(lines[s])
        else:
            want[b, 0, :, :real.shape[3]] = real[-1 - s, 0]
    return want


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_every_level_matches_numpy_exactly(cuda):
    W = 1024
    p = np.random.RandomState(3).randint(0, 256, H * W).astype(np.uint8)
    pos = np.random.RandomState(4).permutation(H * W)[:256]
    p[pos] = np.arange(256, dtype=np.uint8)
    line = p.reshape(H, W)
    got, tail = _run([line], [0], W=W)
    assert _same_bits(got[0, 0], _levels(line))
    assert got.max() == 1.0 and got.min() == np.float32(1.0) - np.float32(255.0) / np.float32(128.0)
    assert len(np.unique(got)) == 256 and np.isnan(tail).all()


@pytest.mark.parametrize("widths,select", [([40, 12, 4, 36], [3, 0, 0, 2]), ([1040, 1028, 260], [1, 2, 0, 1])])
def test_ragged_selection_with_repeats_and_permutation(cuda, widths, select):
    """rows are lines in any order, a line may be taken twice; padding is exactly -1, every element of the NaN-filled output is written and
    nothing behind it. The wide case crosses the 1024 columns a workgroup takes and ends off a multiple of 256 lanes."""
    lines = _random_lines(widths, seed=widths[0])
    W = max(widths[s] for s in select)
    got, tail = _run(lines, select, W=W)
    assert not np.isnan(got).any()
    assert _same_bits(got, _expect(lines, select, None, W))
    for b, s in enumerate(select):
        assert (got[b, 0, :, widths[s]:] == -1.0).all()
    assert np.isnan(tail).all()


@pytest.mark.parametrize("Wr,W", [(37, 40), (45, 48)])
def test_mixed_with_real_rows(cuda, Wr, W):
    """real [2,1,64,Wr] with an odd width (unaligned rows), interleaved with pool lines: once a pool line (40) is the widest row, once the
    real batch (45 -> W = 48)"""
    lines = _random_lines([40, 12, 36], seed=Wr)
    real = np.random.RandomState(Wr + 1).uniform(-1.0, 1.0, (2, 1, H, Wr)).astype(np.float32)
    select = [-1, 2, -2, 0]
    got, tail = _run(lines, select, real=real, W=W)
    assert not np.isnan(got).any()
    assert _same_bits(got, _expect(lines, select, real, W))
    assert (got[0, 0, :, Wr:] == -1.0).all() and (got[2, 0, :, Wr:] == -1.0).all() and (got[1, 0, :, 36:] == -1.0).all()
    assert np.isnan(tail).all()


def test_equals_collate_on_the_host(cuda):
    """the same lines and real items through data.hw_dataset.collate: images bit-equal apart from the <= 3 round-up columns (-1); labels,
    lengths, texts, names and authors equal"""
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd.data.hw_dataset import collate
    from handwriting_line_generation_amd.data.synth_lines import SYNTH_AUTHOR, merge_labels
    g = np.random.RandomState(9)
    real_items = [{"image": _levels(g.randint(0, 256, (H, w)).astype(np.uint8))[..., None], "gt": gt, "gt_label": np.asarray(lab, dtype=np.uint32),
                   "name": "a%d_0" % i, "center": False, "author": "a%d" % i}
                  for i, (w, gt, lab) in enumerate([(37, "abc", [1, 2, 3]), (21, "de", [4, 5])])]
    lines = _random_lines([40, 12, 52], seed=10)
    texts, labels = ["fghi", "j", "klmnop"], [np.asarray(l, dtype=np.uint32) for l in ([6, 7, 8, 9], [10], [11, 12, 13, 14, 15, 16])]
    drawn = [2, 0]
    synth_items = [{"image": _levels(lines[k])[..., None], "gt": texts[k], "gt_label": labels[k], "name": "synth_%d" % k, "center": False,
                    "author": SYNTH_AUTHOR} for k in drawn]
    want = collate(real_items + synth_items)
    inst = collate(real_items)
    dev = torch.device("cuda:0")
    pixels, offsets, widths = _pool(lines)
    image = ops.lines_from_u8(ops.h2d(torch.from_numpy(pixels), dev), offsets, widths, [-1, -2] + drawn, real=ops.h2d(inst["image"], dev)).cpu()
    got = merge_labels(inst, [texts[k] for k in drawn], [labels[k] for k in drawn], ["synth_%d" % k for k in drawn])
    Wc = want["image"].shape[3]
    assert Wc == 52 and image.shape == (4, 1, H, 52)
    assert _same_bits(image.numpy(), want["image"].numpy())
    assert got["label"].dtype == want["label"].dtype and torch.equal(got["label"], want["label"])
    assert got["label_lengths"].dtype == want["label_lengths"].dtype and torch.equal(got["label_lengths"], want["label_lengths"])
    assert got["gt"] == want["gt"] and got["name"] == want["name"] and got["author"] == want["author"]
    # a widest row of 37 columns: the batch is 40 wide, the 3 round-up columns are padding
    image = ops.lines_from_u8(ops.h2d(torch.from_numpy(pixels), dev), offsets, widths, [-1, 1, -2], real=ops.h2d(inst["image"], dev)).cpu()
    want = collate([real_items[0], {"image": _levels(lines[1])[..., None], "gt": "j", "gt_label": labels[1], "name": "s", "center": False,
                                    "author": SYNTH_AUTHOR}, real_items[1]])
    assert image.shape == (3, 1, H, 40) and want["image"].shape == (3, 1, H, 37)
    assert _same_bits(image[..., :37].contiguous().numpy(), want["image"].numpy()) and bool((image[..., 37:] == -1).all())


REFUSALS = [
    dict(select=[0, 3]),                                   # a select entry behind the pool
    dict(select=[0, -3], real=True),                       # a real row behind the real batch
    dict(select=[0, -1]),                                  # a negative entry without a real batch
    dict(select=[1], widths=[40, 6, 4]),                   # a width that is no multiple of 4
    dict(select=[1], widths=[40, 0, 4]),                   # an empty line
    dict(select=[1], offsets=[0, 2562, 3328]),             # a misaligned offset
    dict(select=[2], offsets=[0, 2560, 3584 - 4]),         # offsets[2] + 64 * 4 ends 252 bytes behind pixels
    dict(select=[0], offsets=[-4, 2560, 3328]),            # a negative offset
    dict(select=[]),                                       # an empty select
    dict(select=[0, 1, 2], out=3 * H * 40 - 1),            # an `out` that is too small
]


@pytest.mark.parametrize("case", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_never_launch(cuda, case):
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd._lib import HwgError
    widths = case.get("widths", [40, 12, 4])
    offsets = case.get("offsets", [0, 2560, 3328])
    pixels = torch.zeros((H * 56,), dtype=torch.uint8, device=cuda)               # 3584 bytes: the three lines back to back
    real = torch.zeros((2, 1, H, 37), dtype=torch.float32, device=cuda) if case.get("real") else None
    out = torch.full((case.get("out", 4 * H * 40),), float("nan"), dtype=torch.float32, device=cuda)
    calls, orig = [], ops.L.call

    def call(fn, *a):
        calls.append(fn)
        return orig(fn, *a)
    ops.L.call = call
    try:
        with pytest.raises(HwgError):
            ops.lines_from_u8(pixels, offsets, widths, case["select"], real=real, out=out)
    finally:
        ops.L.call = orig
    torch.cuda.synchronize()
    assert calls == []                                   # refused on the host, before anything was launched
    assert bool(torch.isnan(out).all())


def test_entry_point_refuses_bad_arguments_itself(cuda):
    """the checks the entry point can make on its own arguments (the tables are device arrays: theirs are ops.lines_from_u8's)"""
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd._lib import HwgError
    pixels = torch.zeros((H * 40,), dtype=torch.uint8, device=cuda)
    offsets = torch.tensor([0], dtype=torch.int64, device=cuda)
    widths = torch.tensor([40], dtype=torch.int32, device=cuda)
    select = torch.tensor([0], dtype=torch.int32, device=cuda)
    real = torch.zeros((1, 1, H, 45), dtype=torch.float32, device=cuda)
    out = torch.full((H * 48,), float("nan"), dtype=torch.float32, device=cuda)
    n = pixels.numel()
    st = torch.cuda.current_stream().cuda_stream
    good = [pixels, n, offsets, widths, 1, select, 0, None, 0, 0, 1, H, 40, out]

    def bad(**kw):
        names = ["pixels", "n", "offsets", "widths", "n_lines", "select", "min_select", "real", "Br", "Wr", "B", "H", "W", "out"]
        return [kw.get(k, v) for k, v in zip(names, good)]
    for args, word in [(bad(pixels=None), "null"), (bad(offsets=None), "null"), (bad(widths=None), "null"), (bad(select=None), "null"),
                       (bad(out=None), "null"), (bad(B=0), "bad sizes"), (bad(H=0), "bad sizes"), (bad(W=0), "bad sizes"), (bad(W=-4), "bad sizes"),
                       (bad(W=42), "multiple of 4"), (bad(out=out.data_ptr() + 4), "aligned"), (bad(pixels=pixels.data_ptr() + 2), "aligned"),
                       (bad(min_select=-1), "negative select"), (bad(real=real, Br=1, Wr=45, W=44), "real batch"),
                       (bad(real=real, Br=1, Wr=45, W=48, min_select=-2), "behind")]:
        with pytest.raises(HwgError) as e:
            ops.L.call("hwg_lines_from_u8", *args, st)
        assert word in str(e.value), (word, str(e.value))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
