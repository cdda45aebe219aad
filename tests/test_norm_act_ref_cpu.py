"""CPU: the fp64 restatements of the normalisation / activation family (oracle/norm_ref.py) against torch's own functional ops, and the
bookkeeping of the GPU case tables (oracle/norm_cases.py): each case's chunk count agrees with the library's workspace query (no launch), and
the tables together hit every geometry, statistics and activation regime of the kernels."""
import pytest
import torch
import torch.nn.functional as F

from oracle import norm_cases as NC
from oracle import norm_ref as R


def _leaf(t):
    return t.double().clone().requires_grad_(True)


def _same_autograd(fn_a, fn_b, inputs, gy):
    """outputs and input gradients of two functions of the same fp64 inputs agree"""
    a_in, b_in = [_leaf(t) if t is not None else None for t in inputs], [_leaf(t) if t is not None else None for t in inputs]
    ya, yb = fn_a(*a_in), fn_b(*b_in)
    torch.testing.assert_close(ya, yb, rtol=1e-12, atol=1e-12)
    ya.backward(gy.double()); yb.backward(gy.double())
    for ta, tb in zip(a_in, b_in):
        if ta is not None:
            torch.testing.assert_close(ta.grad, tb.grad, rtol=1e-10, atol=1e-10)


def _torch_act(z, act, slope):
    return {R.ACT_NONE: lambda t: t, R.ACT_RELU: F.relu, R.ACT_LRELU: lambda t: F.leaky_relu(t, slope), R.ACT_TANH: torch.tanh}[act](z)


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH])
@pytest.mark.parametrize("mode,groups", [("gn", 4), ("gn", 1), ("gn", 8), ("bn", 1), ("in", 1)])
def test_norm_reference_is_torch(mode, groups, act):
    g = torch.Generator().manual_seed(3 + groups + 7 * act)
    N, C, H, W = 3, 8, 5, 7
    x = torch.randn(N, C, H, W, generator=g) * 2 + 0.5
    x[:, 0, :2, :3] = 0.0
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    mask = (torch.rand(N, C, generator=g) > 0.3).double() / 0.7
    gy = torch.randn(N, C, H, W, generator=g)

    def ours(x, gm, bt):
        return R.norm(x, mode, groups, gm, bt, mask, act, 0.1, 1e-5)

    def theirs(x, gm, bt):
        if mode == "gn":
            z = F.group_norm(x, groups, gm, bt, 1e-5)
        elif mode == "bn":
            z = F.batch_norm(x, None, None, gm, bt, True, 0.0, 1e-5)
        else:
            z = F.instance_norm(x, eps=1e-5) * gm[None, :, None, None] + bt[None, :, None, None]
        return _torch_act(z * mask[:, :, None, None], act, 0.1)
    _same_autograd(ours, theirs, [x, gamma, beta], gy)


def test_running_statistics_are_torch():
    g = torch.Generator().manual_seed(5)
    for N, H, W in ((4, 3, 5), (1, 2, 9), (2, 1, 1), (7, 1, 1)):
        x = torch.randn(N, 6, H, W, generator=g, dtype=torch.float64) * 3 + 1
        rm, rv = torch.randn(6, generator=g, dtype=torch.float64), torch.rand(6, generator=g, dtype=torch.float64) + 0.5
        want_m, want_v = rm.clone(), rv.clone()
        F.batch_norm(x, want_m, want_v, None, None, True, 0.1, 1e-5)
        got_m, got_v = R.running_stats(x, rm, rv, 0.1)
        torch.testing.assert_close(got_m, want_m, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(got_v, want_v, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH])
def test_frozen_and_bias_act_references_are_torch(act):
    g = torch.Generator().manual_seed(11 + act)
    N, C, H, W = 2, 6, 3, 4
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.1
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    want = _torch_act(F.batch_norm(x, rm, rv, gamma, beta, False, 0.0, 1e-5), act, 0.2)
    torch.testing.assert_close(R.frozen_norm(x, rm, rv, gamma, beta, act, 0.2, 1e-5), want, rtol=1e-12, atol=1e-12)
    bias = torch.randn(C, generator=g)
    mask = (torch.rand(N, C, generator=g) > 0.4).double() / 0.6
    x0 = torch.where(torch.rand(N, C, H, W, generator=g) < 0.25, -bias.double()[:, None, None], x)     # exact zeros: relu'(0) = 0, lrelu'(0) = slope
    _same_autograd(lambda x, b: R.bias_act(x, b, mask, act, 0.2),
                   lambda x, b: _torch_act((x + b[None, :, None, None]) * mask[:, :, None, None], act, 0.2), [x0, bias], torch.randn(N, C, H, W, generator=g))


def test_adain_reference_is_torch():
    g = torch.Generator().manual_seed(13)
    N, C, H, W = 3, 8, 4, 9
    x, noise = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    nw = torch.randn(1, C, 1, 1, generator=g) * 0.5
    gamma, beta = torch.randn(N, C, generator=g) + 1, torch.randn(N, C, generator=g)
    scale = (2.0 / C) ** 0.5

    def theirs(x, nw, gm, bt):
        u = F.leaky_relu(x + (nw * scale) * noise.double(), 0.2)
        return gm[:, :, None, None] * F.instance_norm(u, eps=1e-5) + bt[:, :, None, None]
    _same_autograd(lambda x, nw, gm, bt: R.adain(x, noise.double(), nw, gm, bt, scale, 0.2, 1e-5), theirs, [x, nw, gamma, beta],
                   torch.randn(N, C, H, W, generator=g))


def test_gate_hint_overrides_only_the_marked_elements():
    z = torch.tensor([-2.0, -1e-9, 0.0, 1e-9, 3.0], dtype=torch.float64, requires_grad=True)
    where = torch.tensor([False, True, False, True, False])
    positive = torch.tensor([True, True, True, False, True])
    y = R.act_ref(z, R.ACT_LRELU, 0.25, (where, positive))
    y.backward(torch.ones(5, dtype=torch.float64))
    assert z.grad.tolist() == [0.25, 1.0, 0.25, 0.25, 1.0]


def _all_norm_geometries():
    geos = [(c[0], c[2], c[3] * c[4], c[5]) for c in NC.NORM_CASES]
    geos += [(c[0], c[1], c[2] * c[3], c[4]) for c in NC.ADAIN_CASES]
    return geos


def test_case_chunk_counts_match_the_library():
    """make_geo restated in Python gives every GPU case the chunk count the library plans (hwg_norm_workspace = 2 N chunks C 16 + 8 N C + 256)"""
    from handwriting_line_generation_amd import _lib as L
    for name, N, HW, C in _all_norm_geometries():
        got = NC.chunks_from_workspace(L.query("hwg_norm_workspace", N, HW, C), N, C)
        assert got == NC.make_geo(N, HW, C)["chunks"], (name, N, HW, C, got, NC.make_geo(N, HW, C))
    assert L.query("hwg_norm_workspace", 4, 100, 6) == 0          # C % 4 != 0: no normalisation kernel takes it


def test_case_tables_cover_every_regime():
    """removing the only case of a regime from a table fails here"""
    tags = set()
    for c in NC.NORM_CASES:
        tags |= NC.norm_case_regimes(c)
    assert NC.REQUIRED_NORM_REGIMES <= tags, sorted(NC.REQUIRED_NORM_REGIMES - tags)
    adain = set()
    for c in NC.ADAIN_CASES:
        adain |= NC.geometry_regimes(c[1], c[2] * c[3], c[4]) | {"noise " + c[5]}
    assert {"noise tensor", "noise virtual", "idle threads", "ragged last chunk", "chunks capped at 64"} <= adain, sorted(adain)
    assert {c[5] for c in NC.FROZEN_CASES} == {R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH}
    ba = set()
    for c in NC.BIAS_ACT_CASES:
        ba |= NC.bias_act_case_regimes(c)
    assert NC.REQUIRED_BIAS_ACT_REGIMES <= ba, sorted(NC.REQUIRED_BIAS_ACT_REGIMES - ba)
    assert max(a * b for a, b in NC.TANH_SIZES) > 2048 * 256
    # no case is larger than 128 MB of fp32
    for c in NC.NORM_CASES:
        assert c[2] * c[3] * c[4] * c[5] * 4 <= 128 << 20, c[0]
    for c in NC.ADAIN_CASES:
        assert c[1] * c[2] * c[3] * c[4] * 4 <= 128 << 20, c[0]
    for c in NC.BIAS_ACT_CASES:
        assert c[1] * c[2] * c[3] * c[4] * 4 <= 128 << 20, c[0]


@pytest.mark.parametrize("N,HW,C,want", [(16, 29696, 64, dict(chunks=64, cs=464, PP=16)), (65, 256, 1024, dict(chunks=32, cs=8, PP=1, halved=True)),
                                         (8, 1032, 512, dict(chunks=61, cs=17, PP=2)), (1, 1, 4, dict(chunks=1, cs=1, PP=256))])
def test_make_geo_restatement_known_answers(N, HW, C, want):
    got = NC.make_geo(N, HW, C)
    assert {k: got[k] for k in want} == want, got
