"""GPU: ops.stretch_onehot (csrc/stretch.hip) against the numpy restatement of torch's CPU F.interpolate(mode='linear') (tests/_stretch_ref.py,
itself compared with torch bit for bit in tests/test_stretch_cpu.py): both layouts, np.array_equal, on buffers with NaN sentinels in front
of, between and behind the frames."""
import numpy as np
import pytest
import torch

import _stretch_ref as ref

pytestmark = pytest.mark.gpu

GAP = 8          # sentinel floats in front of every frame and behind the last (a multiple of 4: the frames stay 16-byte aligned)


def _labels(T, B, C, seed):
    g = np.random.RandomState(seed)
    lab = g.randint(0, C, (T, B))
    lab[g.rand(T, B) < 0.3] = 0          # blanks
    if T > 2:
        lab[1] = lab[0]                  # two neighbours of the same class
    return lab.astype(np.int32)


def _guarded(label, ncls, scales, cuda):
    """stretch_onehot into NaN-filled buffers with GAP sentinels around every frame -> (frames, host copies of both buffers, offsets, sizes)"""
    from handwriting_line_generation_amd import ops
    T, B = label.shape
    sizes = [B * ref.out_len(T, s) * ncls for s in scales]
    offsets, pos = [], GAP
    for n in sizes:
        offsets.append(pos)
        pos = (pos + n + 3) // 4 * 4 + GAP
    blc = torch.full((pos,), float("nan"), device=cuda)
    lbc = torch.full((pos,), float("nan"), device=cuda)
    # (the two layouts at different places of their buffers: the second buffer's frames in reverse order)
    off_lbc = [pos - o - (n + 3) // 4 * 4 for o, n in zip(offsets, sizes)]
    frames = ops.stretch_onehot(ops.h2d(torch.from_numpy(label), cuda), ncls, scales, out=(blc, lbc), offsets=(offsets, off_lbc))
    torch.cuda.synchronize()
    return frames, blc.cpu().numpy(), lbc.cpu().numpy(), (offsets, off_lbc), sizes


def _check(label, ncls, scales, cuda):
    from handwriting_line_generation_amd import ops
    T, B = label.shape
    frames, blc, lbc, (off_blc, off_lbc), sizes = _guarded(label, ncls, scales, cuda)
    assert len(frames) == len(scales)
    written_blc, written_lbc = np.zeros(blc.size, bool), np.zeros(lbc.size, bool)
    for k, s in enumerate(scales):
        want = ref.stretch(label, ncls, s)
        T_out = want.shape[0]
        got = frames[k]
        assert tuple(got.shape) == (T_out, B, ncls) and got.dtype == torch.float32
        twin = ops.nhwc_of(got)
        assert twin is not None and tuple(twin.shape) == (B, 1, T_out, ncls)
        assert np.array_equal(got.cpu().numpy(), want), (T, B, ncls, s)
        assert np.array_equal(twin.cpu().numpy()[:, 0], want.transpose(1, 0, 2)), (T, B, ncls, s)
        # the views are the frame's place in the buffers
        assert np.array_equal(lbc[off_lbc[k]:off_lbc[k] + sizes[k]].reshape(want.shape), want)
        assert np.array_equal(blc[off_blc[k]:off_blc[k] + sizes[k]].reshape(B, T_out, ncls), want.transpose(1, 0, 2))
        written_blc[off_blc[k]:off_blc[k] + sizes[k]] = True
        written_lbc[off_lbc[k]:off_lbc[k] + sizes[k]] = True
    # every sentinel survived: nothing outside the frames was written
    assert np.isnan(blc[~written_blc]).all() and np.isnan(lbc[~written_lbc]).all()
    assert (~written_blc).sum() >= GAP * (len(scales) + 1) and not np.isnan(blc[written_blc]).any() and not np.isnan(lbc[written_lbc]).any()


@pytest.mark.parametrize("ncls", [5, 78, 80])
@pytest.mark.parametrize("B", [1, 3])
def test_all_79_frames_in_one_call(cuda, B, ncls):
    for T in (2, 3, 33, 130):
        _check(_labels(T, B, ncls, seed=T * 10 + B), ncls, ref.film_scales(), cuda)
    # a line of one step can only be widened: the film's scales from 1 up
    _check(_labels(1, B, ncls, seed=B), ncls, [s for s in ref.film_scales() if s >= 1], cuda)


@pytest.mark.parametrize("ncls", [5, 78, 80])
@pytest.mark.parametrize("B", [1, 3])
def test_one_frame_per_call(cuda, B, ncls):
    for T, s in ((33, 1.01),           # identity although s != 1: floor(33.33) == 33
                 (130, 1.1),           # src < 0 at t = 0 (r < 1), and i0 reaches the last step: i1 clamped at the right edge
                 (130, 0.9),
                 (33, 0.95), (3, 1.1), (2, 0.9), (1, 1.1), (2, 1.0)):
        _check(_labels(T, B, ncls, seed=T + B), ncls, [s], cuda)


def test_the_cases_hold_the_edges_they_are_there_for():
    """host only: the properties the shapes above were chosen for (no device needed, but they belong to this file's cases)"""
    assert ref.out_len(33, 1.01) == 33 and ref.out_len(130, 1.1) == 143
    i0, i1, w0, w1 = ref.taps(130, 1.1)
    assert i0[-1] == 129 and i1[-1] == 129                                       # right edge: both taps on the last step
    r = np.float32(1.0 / 1.1)
    assert np.float64(r) * 0.5 - 0.5 < 0 and i0[0] == 0 and w1[0] == 0           # src < 0 at t = 0, clamped to 0
    lab = _labels(33, 1, 5, seed=34)
    i0, i1, w0, w1 = ref.taps(33, 0.95)
    both = (lab[i0, 0] == lab[i1, 0]) & (i0 != i1) & (w1 > 0)
    assert both.any()                                                            # two different steps of one class under one output step
    out = ref.stretch(lab, 5, 0.95)
    k = int(np.flatnonzero(both)[0])
    assert out[k, 0, lab[i0[k], 0]] == np.float32(w0[k] + w1[k])


def test_default_buffers_and_refusals(cuda):
    from handwriting_line_generation_amd import _lib as L, ops
    label = _labels(33, 3, 78, seed=7)
    dev = ops.h2d(torch.from_numpy(label), cuda)
    scales = [1.0, 1.05, 0.9]
    frames = ops.stretch_onehot(dev, 78, scales)
    for f, s in zip(frames, scales):
        want = ref.stretch(label, 78, s)
        assert np.array_equal(f.cpu().numpy(), want) and np.array_equal(ops.nhwc_of(f).cpu().numpy()[:, 0], want.transpose(1, 0, 2))
        assert f.data_ptr() % 16 == 0 and ops.nhwc_of(f).data_ptr() % 16 == 0
    # refused on the host, before anything is launched: the buffers keep their sentinels
    blc = torch.full((4096,), float("nan"), device=cuda)
    lbc = torch.full((4096,), float("nan"), device=cuda)
    one = ops.h2d(torch.from_numpy(_labels(1, 1, 5, seed=1)), cuda)
    with pytest.raises(ValueError, match="no step"):
        ops.stretch_onehot(one, 5, [1.0, 0.9], out=(blc, lbc), offsets=([0, 8], [0, 8]))
    bad = label.copy()
    bad[5, 1] = 78
    for value in (78, -1):
        bad[5, 1] = value
        with pytest.raises(ValueError, match="labels must lie"):
            ops.stretch_onehot(ops.h2d(torch.from_numpy(bad), cuda), 78, [1.0], out=(blc, lbc), offsets=([0], [0]))
    small = ops.h2d(torch.from_numpy(_labels(2, 1, 5, seed=2)), cuda)
    for offsets, word in ((([2], [0]), "multiples of 4"), (([4092], [0]), "inside the buffer"), (([0, 4], [0, 16]), "overlap")):
        with pytest.raises(L.HwgError, match=word):
            ops.stretch_onehot(small, 5, [1.0] * len(offsets[0]), out=(blc, lbc), offsets=offsets)
    torch.cuda.synchronize()
    assert torch.isnan(blc).all() and torch.isnan(lbc).all()
