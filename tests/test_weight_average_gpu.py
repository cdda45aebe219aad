"""GPU: the two weight-averaging kernels (csrc/weight_avg.hip) behind FlatParams.average_into / exchange_average / averaged_state_dict.

Reference: the reference's moving_average (base/base_trainer.py:481-484), `a *= (1.0 - alpha); a += p * alpha`, run by torch on the CPU over
fp32 tensors. Both sides round the two scalars to fp32 and then perform one product per operand and one sum, each rounded to nearest: the
tolerance is ZERO (int32 views compared with torch.equal).

One statement of the plan this test was written from does not hold for the reference itself and is checked in the form the reference
satisfies: "the first step's result (alpha = 1) equals the parameters bit for bit" is true of every value except -0.0, which
`0 * 0 + (-0) * 1` turns into +0.0 on the CPU and on the GPU alike (round-to-nearest gives +0 for (+0) + (-0)). The first step is therefore
compared with the parameters bit for bit wherever they are not -0.0, and must be +0.0 where they are - exactly what `p + 0.0` gives."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SPECIALS = np.array([1e-40, -1e-42, 0.0, -0.0, 1.6e38, -1.7e38, 1.4e-45, -3e-39], dtype=np.float32)   # denormals, +-0, near FLT_MAX / 2


def _sizes():
    from handwriting_line_generation_amd.trainer.flat_params import CHUNK
    return [1, 3, 4, 5, 1023, CHUNK, CHUNK + 1, 2 * CHUNK + 7]


def _values(seed):
    """one fp32 array per tensor: normal draws with every third element replaced by a special value (the cycle starts elsewhere per tensor
    and per seed, so the one-element tensor sees different specials from step to step)"""
    rs = np.random.RandomState(seed)
    out = []
    for t, n in enumerate(_sizes()):
        v = (rs.standard_normal(n) * 10.0 ** rs.randint(-3, 4)).astype(np.float32)
        idx = np.arange(0, n, 3)
        v[idx] = SPECIALS[(idx // 3 + t + seed) % len(SPECIALS)]
        out.append(torch.from_numpy(v))
    return out


def _flat(dev, seed=0):
    """FlatParams over eight hand-made parameters; flat order 7, 2, 0 | 5, 3, 6 | 1, 4 differs from the parameter order; parameter 6 is frozen,
    parameters 1 and 4 are in no group"""
    from handwriting_line_generation_amd.trainer.flat_params import FlatParams
    params = [torch.nn.Parameter(v.to(dev), requires_grad=(i != 6)) for i, v in enumerate(_values(seed))]
    flat = FlatParams(params, {"main": [params[7], params[2], params[0]], "disc": [params[5], params[3], params[6]]})
    assert flat.order == [7, 2, 0, 5, 3, 6, 1, 4] and flat.group_range["rest"] == (6, 8)
    return flat, params


def _set(params, values):
    for p, v in zip(params, values):
        p.data.copy_(v)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _slices(flat):
    """per parameter index: the slice of the flat buffer that holds it; and the mask of the padding floats"""
    sl, pad = [], torch.ones(flat.total, dtype=torch.bool)
    for i in range(len(flat.params)):
        k = flat.pos[i]
        s = slice(int(flat.offsets[k]), int(flat.offsets[k] + flat.numel[k]))
        sl.append(s)
        pad[s] = False
    return sl, pad


def _check_padding(flat, pad):
    padding = _bits(flat.avg)[pad]
    assert padding.numel() > 0 and int(padding.abs().max()) == 0, "a padding float of avg was written"


def _cpu_step(avg, values, alpha):
    """the reference's moving_average, statement for statement"""
    for a, p in zip(avg, values):
        a *= (1.0 - alpha)
        a += p * alpha


def _run_recurrence(cuda, alphas):
    flat, params = _flat(cuda)
    sl, pad = _slices(flat)
    cpu_avg = [torch.zeros(n, dtype=torch.float32) for n in _sizes()]
    for step, alpha in enumerate(alphas):
        values = _values(100 + step)
        _set(params, values)
        flat.average_into(alpha)
        _cpu_step(cpu_avg, values, alpha)
        got = flat.avg.cpu()
        for i, s in enumerate(sl):
            assert torch.equal(_bits(got[s]), _bits(cpu_avg[i])), "step %d (alpha %r), tensor %d of %d elements" % (step, alpha, i, _sizes()[i])
            assert torch.equal(_bits(params[i]), _bits(values[i])), "averaging changed parameter %d" % i
            if step == 0:
                assert alpha == 1.0
                assert torch.equal(_bits(got[s]), _bits(values[i] + 0.0)), "the first step is not a copy (tensor %d)" % i
                keep = _bits(values[i]) != _bits(torch.tensor(-0.0))
                assert torch.equal(_bits(got[s])[keep], _bits(values[i])[keep])
        _check_padding(flat, pad)
    return flat


def test_averaging_recurrence_is_bit_identical_to_torch_cpu(cuda):
    _run_recurrence(cuda, [1.0, 1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 5])


def test_decay_form_is_bit_identical_to_torch_cpu(cuda):
    decay = 0.999
    _run_recurrence(cuda, [1.0] + [1.0 - decay] * 4)


def test_exchange_swaps_in_place_and_twice_restores(cuda):
    flat, params = _flat(cuda)
    sl, pad = _slices(flat)
    flat.average_into(1.0)
    _set(params, _values(7))
    flat.average_into(0.25)              # avg now differs from every parameter
    old_avg = flat.avg.cpu().clone()
    old_p = [p.detach().cpu().clone() for p in params]
    ptrs = [p.data_ptr() for p in params]
    flat.exchange_average()
    got = flat.avg.cpu()
    for i, s in enumerate(sl):
        assert torch.equal(_bits(params[i]), _bits(old_avg[s])), "parameter %d does not hold the old average" % i
        assert torch.equal(_bits(got[s]), _bits(old_p[i])), "avg does not hold the old parameter %d" % i
    _check_padding(flat, pad)
    flat.exchange_average()
    assert torch.equal(_bits(flat.avg), _bits(old_avg))
    for i, p in enumerate(params):
        assert torch.equal(_bits(p), _bits(old_p[i])) and p.data_ptr() == ptrs[i], i


def test_exchange_before_any_average_is_an_error(cuda):
    flat, _ = _flat(cuda)
    with pytest.raises(RuntimeError, match="average_into"):
        flat.exchange_average()


def test_forward_after_exchange_uses_the_averaged_weights(cuda):
    """a recogniser whose weights were packed by an earlier forward pass: after exchange_average() its output is that of a fresh model
    loaded from averaged_state_dict - stale packed weights (no cache invalidation) give the live model's output instead"""
    from oracle import cases, torch_ref
    from handwriting_line_generation_amd.model import CNNOnlyHWR
    from handwriting_line_generation_amd.trainer.flat_params import FlatParams
    case = cases.CASES["hwr"]
    x = cases.inputs("hwr")["image"].to(cuda)
    m = CNNOnlyHWR(**case["ctor"])
    m.load_state_dict(torch_ref.seeded_state_dict(m, case["wseed"]))
    m.to(cuda).eval()
    params = list(m.parameters())
    flat = FlatParams(params, {"main": params[: len(params) // 2]}, names=[n for n, _ in m.named_parameters()])
    with torch.no_grad():
        y_live0 = m(x, None).clone()                  # packs the weights
        flat.average_into(1.0)
        g = torch.Generator().manual_seed(3)
        for p in params:                               # perturb the live weights: avg (the old ones) and the live ones now differ
            # (p.add_, not p.data.add_: a write through .data leaves p._version alone, and the forward below would read stale packed weights)
            p.add_((torch.randn(p.shape, generator=g) * (0.05 * float(p.detach().abs().mean().cpu()) + 0.01)).to(cuda))
        flat.average_into(0.5)
        y_live = m(x, None).clone()                   # ... and pack the perturbed ones
        sd = flat.averaged_state_dict(m)
        for name, p in m.named_parameters():
            assert not torch.equal(sd[name], p.detach().cpu()), name
        for name, b in m.named_buffers():
            assert torch.equal(sd[name], b.cpu()), name
        flat.exchange_average()
        y_avg = m(x, None).clone()
        flat.exchange_average()
        y_back = m(x, None).clone()
        fresh = CNNOnlyHWR(**case["ctor"])
        fresh.load_state_dict(sd)
        fresh.to(cuda).eval()
        y_fresh = fresh(x, None)
    assert not torch.equal(y_live, y_live0) and not torch.equal(y_avg, y_live)
    assert torch.equal(_bits(y_avg), _bits(y_fresh)), "forward after the exchange did not use the averaged weights"
    assert torch.equal(_bits(y_back), _bits(y_live)), "forward after the exchange back did not use the live weights"
