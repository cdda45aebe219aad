"""CPU: the stretch rule the kernel hwg_stretch_onehot implements (tests/_stretch_ref.py) IS torch's F.interpolate(mode='linear') on the CPU, bit
for bit; the film's scale list; the batch selection of the `r` action; the argument errors of the new generate.py actions. No device."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stretch_ref as ref


def _labels(T, B, C, seed):
    """aligned-looking lines: blanks (0), runs of one class (two neighbours of the same class) and changes of class"""
    g = np.random.RandomState(seed)
    lab = g.randint(0, C, (T, B))
    lab[g.rand(T, B) < 0.3] = 0
    if T > 2:
        lab[1] = lab[0]
    return lab.astype(np.int32)


@pytest.mark.parametrize("C", [5, 78])
@pytest.mark.parametrize("B", [1, 3])
def test_the_rule_is_torchs_linear_interpolation_bit_for_bit(B, C):
    scales = ref.film_scales()
    assert len(scales) == 79
    identity_with_other_scale = clamped_left = clamped_right = same_class = 0
    for T in (1, 2, 3, 7, 33, 130, 257):          # (130: the one length of these at which i0 reaches the last step)
        lab = _labels(T, B, C, seed=T * 10 + B)
        onehot = F.one_hot(torch.from_numpy(lab.astype(np.int64)), C).float()          # [T, B, C]
        x = onehot.permute(1, 2, 0).contiguous()                                            # [B, C, T] as interpolate_horz lays it out
        for s in scales:
            if T == 1 and s < 1:
                continue                                                                    # (no step left: torch refuses as well)
            want = F.interpolate(x, scale_factor=s, mode="linear").permute(2, 0, 1).contiguous().numpy()
            assert ref.out_len(T, s) == want.shape[0], (T, s)
            got = ref.stretch(lab, C, s)
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got, want), (T, B, C, s)
            i0, i1, w0, w1 = ref.taps(T, s)
            identity_with_other_scale += int(want.shape[0] == T and s != 1.0)
            if want.shape[0] != T:
                r = np.float32(1.0 / s)
                clamped_left += int(np.float64(r) * 0.5 - 0.5 < 0)
                clamped_right += int((i0 == T - 1).any())
                same_class += int(((lab[i0] == lab[i1]) & (i0 != i1)[:, None] & (w1 > 0)[:, None]).any())
    assert identity_with_other_scale and clamped_left and clamped_right and same_class      # the edge cases are among the cases


def test_identity_frame_with_a_scale_that_is_not_one():
    """T = 33, s = 1.01: floor(33.33) = 33 = T, torch copies its input although the scale is not 1"""
    assert ref.out_len(33, 1.01) == 33
    lab = _labels(33, 2, 5, seed=1)
    x = F.one_hot(torch.from_numpy(lab.astype(np.int64)), 5).float().permute(1, 2, 0).contiguous()
    assert torch.equal(F.interpolate(x, scale_factor=1.01, mode="linear"), x)
    assert np.array_equal(ref.stretch(lab, 5, 1.01), np.eye(5, dtype=np.float32)[lab])


def test_host_frame_table_is_the_rule():
    from handwriting_line_generation_amd import ops
    scales = ref.film_scales()
    for T in (1, 2, 3, 33, 130, 257):
        use = [s for s in scales if T > 1 or s >= 1]
        frames = ops.stretch_frames(T, use)
        assert [f[0] for f in frames] == [ref.out_len(T, s) for s in use]
        assert all(f[1].dtype == np.float32 and f[1] == np.float32(1.0 / s) for f, s in zip(frames, use))
        assert [bool(f[2]) for f in frames] == [ref.out_len(T, s) == T for s in use]
    with pytest.raises(ValueError):
        ops.stretch_frames(1, [0.9])
    with pytest.raises(ValueError):
        ops.stretch_frames(5, [0.0])


def test_stretch_scales_are_the_references_79():
    from handwriting_line_generation_amd.generate import stretch_scales
    s = stretch_scales()
    assert len(s) == 79 and all(type(v) is float for v in s)
    a, b, c = np.arange(1, 1.11, 0.01), np.arange(1.1, 0.89, -0.01), np.arange(0.9, 1.01, 0.01)
    assert (len(a), len(b), len(c)) == (12, 22, 11)
    assert s[:12] == [float(v) for v in a]
    assert s[12:24] == [float(a[-1])] * 12              # the first "vertical" loop: the last label again
    assert s[24:46] == [float(v) for v in b]
    assert s[46:68] == [float(b[-1])] * 22
    assert s[68:] == [float(v) for v in c]
    assert s == ref.film_scales()


class _FakeLoader:
    def __init__(self, authors):
        self.authors, self.read = authors, 0

    def __iter__(self):
        for k, a in enumerate(self.authors):
            self.read = k + 1
            yield {"author": [a], "k": k}


def _reference_walk(authors, num_styles, rand):
    """the loop of the reference's `r` action (generate.py:314-329) on a list of writers -> the indices taken"""
    taken = []
    index = rand.randint(0, 20)
    last_author = None
    for i, author in enumerate(authors):
        if i >= index and author != last_author:
            taken.append(i)
            last_author = author
            index += rand.randint(20, 50)
        if len(taken) >= num_styles:
            break
    return taken


def test_walk_selection_draws_like_the_reference():
    from handwriting_line_generation_amd.generate import walk_batches, walk_styles
    g = random.Random(5)
    authors = []
    while len(authors) < 400:
        authors += ["w%d" % g.randint(0, 30)] * g.randint(1, 30)
    for seed in (0, 1, 2, 3):
        for num in (2, 4, 50):
            rand, ref_rand = random.Random(seed), random.Random(seed)
            loader = _FakeLoader(authors)
            got = [i for i, inst in walk_batches(loader, num, rand)]
            want = _reference_walk(authors, num, ref_rand)
            assert got == want and rand.getstate() == ref_rand.getstate()
            assert 2 <= len(got) <= num and loader.read == (got[-1] + 1 if len(got) == num else len(authors))      # stops reading once it has them
    # start / stride: no draw is made
    rand = random.Random(9)
    state = rand.getstate()
    got = [i for i, _ in walk_batches(_FakeLoader(["a", "a", "b", "c", "c", "d"]), 3, rand, start=0, stride=1)]
    assert got == [0, 2, 3] and rand.getstate() == state
    # walk_styles: the styles of the batches taken, in order; fewer than two found is refused with the number of batches read

    class Model:
        use_hwr_pred_for_style = False
        pred = spaced_label = spaced_label_index = None

        def extract_style(self, image, label, a_batch_size):
            return image.reshape(1, 1).repeat(a_batch_size, 4)

    def loader(authors):
        for k, a in enumerate(authors):
            yield {"author": [a], "image": torch.tensor(float(k)), "label": torch.zeros(1, 2), "a_batch_size": 2}
    styles = walk_styles(loader(["a", "a", "b", "c", "c", "d"]), Model(), {}, 3, random.Random(0), None, start=0, stride=1)
    assert [tuple(s.shape) for s in styles] == [(1, 4)] * 3 and [float(s[0, 0]) for s in styles] == [0.0, 2.0, 3.0]
    with pytest.raises(SystemExit) as e:
        walk_styles(loader(["a", "a", "a"]), Model(), {}, 3, random.Random(0), None, start=0, stride=1)
    assert "found 1 in the 3 batches" in str(e.value.code)


def test_new_actions_refuse_missing_arguments_before_a_checkpoint_is_opened(tmp_path):
    import generate as cli
    missing = str(tmp_path / "none.pth")
    with pytest.raises(SystemExit) as e:
        cli.main(["-c", missing, "-d", str(tmp_path / "out"), "-r", "choice=r,step=0.1"])
    assert "num_styles" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        cli.main(["-c", missing, "-d", str(tmp_path / "out"), "-r", "choice=A,text=hello"])
    assert "author" in str(e.value.code)
    assert not (tmp_path / "out").exists()
    # the refusal of the actions that are not built names the ones that are
    with pytest.raises(NotImplementedError) as e:
        cli.main(["-c", missing, "-d", str(tmp_path / "out"), "-r", "choice=t"])
    for name in ("'R'", "'f'", "'u'", "'s'", "'r'", "'A'", "'t'"):
        assert name in str(e.value)
