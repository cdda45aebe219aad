"""GPU: ops.eval_pairs (hwg_eval_pairs, csrc/eval_pictures.hip) against the numpy restatement tests/_eval_pictures_ref.py - which
tests/test_eval_pictures_cpu.py pins to arrays recorded from the reference -, byte for byte."""
import numpy as np
import pytest
import torch

import _eval_pictures_ref as ref

pytestmark = pytest.mark.gpu

WIDTHS = [(1, 1), (7, 7), (12, 7), (7, 12), (8, 7), (1, 12), (5, 2), (515, 509)]
GUARD = 64


@pytest.fixture(scope="module")
def material(cuda):
    """shared, read-only: the edge values, a random glyph atlas (no PIL) on host and device"""
    rs = np.random.RandomState(11)
    atlas = rs.randint(1, 256, size=(9, 7, 5)).astype(np.uint8)
    return {"edge": ref.edge_values(), "atlas": atlas, "atlas_d": torch.from_numpy(atlas).to(cuda), "rs_seed": 12}


def _inputs(material, B, H, Wi, Wr, seed):
    """pixels that walk through the edge values (both inputs), with NaN, +-inf and +-3 sprinkled in where there is room"""
    edge = material["edge"]
    rs = np.random.RandomState(seed)
    out = []
    for k, W in enumerate((Wi, Wr)):
        n = B * H * W
        start = (seed * 37 + k * 1151) % edge.size
        x = np.take(edge, np.arange(start, start + n), mode="wrap").astype(np.float32).reshape(B, 1, H, W)
        flat = x.reshape(-1)
        special = np.array([np.nan, np.inf, -np.inf, 3.0, -3.0], dtype=np.float32)
        if n >= 10:
            flat[rs.choice(n, size=5, replace=False)] = special
        else:
            flat[:] = np.take(special, np.arange(n) + k, mode="wrap")
        out.append(x)
    return out


def _captions(B, Wp, G, gw, rs):
    """per line another kind: empty, longer than the picture (clipped), end-marked early, plain"""
    kinds = []
    for b in range(B):
        kind = (b + Wp) % 4
        if kind == 0:
            kinds.append([])
        elif kind == 1:
            kinds.append(rs.randint(0, G, size=Wp // gw + 5).tolist())
        elif kind == 2:
            kinds.append(rs.randint(0, G, size=3).tolist() + [-1] + rs.randint(0, G, size=2).tolist())
        else:
            kinds.append(rs.randint(0, G, size=2).tolist())
    return kinds


def _run_guarded(image_d, recon_d, captions, atlas_d, shape):
    """eval_pairs into a buffer prefilled with 0xAA with a guard behind the rounded-up size -> (pictures, surplus, guard) on the host"""
    from handwriting_line_generation_amd import ops
    total = int(np.prod(shape))
    need = -(-total // 4) * 4
    buf = torch.full((need + GUARD,), 0xAA, dtype=torch.uint8, device=image_d.device)
    got = ops.eval_pairs(image_d, recon_d, captions, atlas_d, out=buf[:need])
    assert got.shape == shape and got.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    return host[:total].reshape(shape), host[total:need], host[need:]


@pytest.mark.parametrize("H", [1, 5, 64])
@pytest.mark.parametrize("strip", [False, True])
def test_against_the_restatement(cuda, material, H, strip):
    from handwriting_line_generation_amd import ops
    rs = np.random.RandomState(material["rs_seed"] + H)
    for Wi, Wr in WIDTHS:
        for B in (1, 3):
            image, recon = _inputs(material, B, H, Wi, Wr, seed=H * 100 + Wi * 3 + Wr + B)
            captions = _captions(B, max(Wi, Wr), material["atlas"].shape[0], material["atlas"].shape[2], rs) if strip else None
            Hp, Wp = ops.eval_pairs_shape(H, Wi, Wr, strip)
            assert (Hp, Wp) == ref.shape(H, Wi, Wr, strip)
            shape = (B, Hp, Wp, 3)
            got, surplus, guard = _run_guarded(torch.from_numpy(image).to(cuda), torch.from_numpy(recon).to(cuda), captions,
                                               material["atlas_d"] if strip else None, shape)
            want = ref.eval_pairs(image, recon, captions, material["atlas"] if strip else None)
            assert np.array_equal(got, want), (H, Wi, Wr, B, strip, np.argwhere(got != want)[:5].tolist())
            assert not surplus.any(), "the tail word's surplus bytes are 0"
            assert (guard == 0xAA).all(), "nothing behind the rounded-up size is touched"


def test_the_cases_hold_sizes_that_are_no_multiple_of_4():
    """3 B (2 H + 2 + S) Wp bytes: a multiple of 4 unless B, Wp and H + 1 + S / 2 are all odd - the tail word's path of the cases above"""
    odd = [(H, strip, w, B) for H in (1, 5, 64) for strip in (False, True) for w in WIDTHS for B in (1, 3)
           if (3 * B * ref.shape(H, w[0], w[1], strip)[0] * max(w)) % 4]
    assert len(odd) >= 12 and {o[0] for o in odd} == {1, 5, 64} and {o[1] for o in odd} == {False, True}


def test_edge_values_as_pixels(cuda, material):
    """all 2304 edge values as the pixels of both inputs: the three quantisations (this one, lines_to_u8's, round to nearest) differ on
    them (tests/test_eval_pictures_cpu.py counts where), so a kernel that took another one fails here"""
    from handwriting_line_generation_amd import ops
    edge = material["edge"]
    image = edge.reshape(2, 1, 4, 288).copy()
    recon = edge[::-1].reshape(2, 1, 4, 288).copy()
    got = ops.eval_pairs(torch.from_numpy(image).to(cuda), torch.from_numpy(recon).to(cuda)).cpu().numpy()
    assert np.array_equal(got, ref.eval_pairs(image, recon))
    inner = got[:, 1:4, 1:-1, 0]                      # real rows 1..3 inside the frame
    assert np.array_equal(inner, ref.levels(image[:, 0, 1:4, 1:-1]))


def test_refusals_before_any_launch(cuda, material):
    from handwriting_line_generation_amd import ops
    image = torch.zeros((2, 1, 5, 7), device=cuda)
    recon = torch.zeros((2, 1, 5, 9), device=cuda)
    atlas = material["atlas_d"]
    G = atlas.shape[0]
    Hp, Wp = ops.eval_pairs_shape(5, 7, 9, True)
    need = -(-2 * Hp * Wp * 3 // 4) * 4
    buf = torch.full((need + 8,), 0xAA, dtype=torch.uint8, device=cuda)
    E = ops.L.HwgError
    with pytest.raises(E, match="code %d" % G):
        ops.eval_pairs(image, recon, [[0, G], [1]], atlas, out=buf)
    with pytest.raises(E, match="code"):
        ops.eval_pairs(image, recon, [[0], [1] * 40 + [G + 3]], atlas, out=buf)        # beyond the picture's last cell: still refused
    with pytest.raises(E, match="aligned"):
        ops.eval_pairs(image, recon, [[0], [1]], atlas, out=buf[1:])
    with pytest.raises(E, match="at least"):
        ops.eval_pairs(image, recon, [[0], [1]], atlas, out=buf[:need - 4])
    with pytest.raises(E, match="float32"):
        ops.eval_pairs(image.double(), recon, [[0], [1]], atlas, out=buf)
    with pytest.raises(E, match="float32"):
        ops.eval_pairs(image, recon.half(), None, None, out=buf)
    with pytest.raises(E, match="atlas"):
        ops.eval_pairs(image, recon, [[0], [1]], None, out=buf)
    with pytest.raises(E, match="captions for"):
        ops.eval_pairs(image, recon, [[0]], atlas, out=buf)
    with pytest.raises(E, match="height"):
        ops.eval_pairs(image, recon[:, :, :4].contiguous(), None, None, out=buf)
    with pytest.raises(E, match="GPU"):
        ops.eval_pairs(image.cpu(), recon, None, None, out=buf)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xAA).all(), "a refused call has launched nothing"
    # the C entry point's own checks (what ops cannot get wrong is still checked there)
    with pytest.raises(E, match="out holds"):
        ops.L.call("hwg_eval_pairs", image, recon, 2, 5, 7, 9, None, 0, 0, 0, None, 0, buf, 16, ops._stream())
    with pytest.raises(E, match="aligned"):
        ops.L.call("hwg_eval_pairs", image, recon, 2, 5, 7, 9, None, 0, 0, 0, None, 0, buf.data_ptr() + 2, need, ops._stream())
    with pytest.raises(E, match="bad sizes"):
        ops.L.call("hwg_eval_pairs", image, recon, 2, 0, 7, 9, None, 0, 0, 0, None, 0, buf, need, ops._stream())
    with pytest.raises(E, match="atlas"):
        ops.L.call("hwg_eval_pairs", image, recon, 2, 5, 7, 9, None, 0, 0, 0, torch.zeros(4, dtype=torch.int32, device=cuda), 2, buf, need, ops._stream())
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xAA).all()


def test_stream_and_second_call(cuda, material):
    """the same bytes on a side stream, and from a second call into the buffer the first one filled"""
    from handwriting_line_generation_amd import ops
    image, recon = _inputs(material, 3, 5, 12, 7, seed=77)
    image_d, recon_d = torch.from_numpy(image).to(cuda), torch.from_numpy(recon).to(cuda)
    captions = [[1, 2, 3], [], [4]]
    want = ref.eval_pairs(image, recon, captions, material["atlas"])
    first = ops.eval_pairs(image_d, recon_d, captions, material["atlas_d"])
    assert np.array_equal(first.cpu().numpy(), want)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.eval_pairs(image_d, recon_d, captions, material["atlas_d"])
    side.synchronize()
    assert np.array_equal(other.cpu().numpy(), want)
    # a second call with other inputs into the buffer of the first: nothing of the first survives
    image2, recon2 = _inputs(material, 3, 5, 12, 7, seed=78)
    buf = first.view(-1)
    buf = torch.cat([buf, torch.zeros((-buf.numel()) % 4, dtype=torch.uint8, device=cuda)])
    again = ops.eval_pairs(torch.from_numpy(image2).to(cuda), torch.from_numpy(recon2).to(cuda), [[], [5], [6, 7]], material["atlas_d"], out=buf)
    assert np.array_equal(again.cpu().numpy(), ref.eval_pairs(image2, recon2, [[], [5], [6, 7]], material["atlas"]))
