"""ops.lstm_layer / ops.bilstm (csrc/lstm.hip) on the GPU against tests/_lstm_ref.py (numpy fp64).

Shapes: H = 512 (the only H that ships) plus H = one and two unit slices (4, 8); the kernels' batch tile is S = 32 lines at all three, so
B in {1, 3, 31, 32, 33, 16}; T in {1, 2, 3, 64}.

Toleranced tests. Yardstick: torch's own float32 CPU nn.LSTM on the same case (forward and autograd). For every compared tensor
err_hip = max|hip - fp64| must be at most 4 * max|torch_fp32 - fp64| + 4 * 2^-24 * scale (scale = the tensor's largest magnitude). For the
single-layer cases nn.LSTM is fed x = [xproj_f | xproj_r] with W_ih = [I | 0] / [0 | I] and b_ih = 0: products with 1 and 0 and sums with 0
are exact in float32, so its input projection IS xproj and its dx IS dxproj.
Observed err_hip / bound on the MI355X (296 compared tensors, per case in profiles/crnn_lstm.txt): worst 0.38 (single layer, H = 512),
0.36 (two layers through ops.bilstm, H = 512), 0.33 / 0.27 (H = 8 / 4) - the device's error is of the size of torch's own.

(d) - T = 1 against the closed form - is toleranced although the summation order is stated (csrc/lstm.hip; at T = 1 the recurrent sum is
+0): what stands between the device and a float32 numpy evaluation is not the order of a sum but the last-place rounding of expf / tanhf /
the division, which differ between libraries. Bound: every one of sigmoid, tanh is within 2 ulp of the exact function of its float32
argument in both implementations (|values| <= 1), h = sig(o) tanh(sig(i) tanh(g)) chains three of them with two products, each stage passing
on its input error with a factor <= 1: <= 8 ulp of 1 = 8 * 2^-24 per side, 16 * 2^-24 between the two.
"""
import numpy as np
import pytest
import torch

import _lstm_ref
from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)
from _lstm_layer import EPS, check_against_yardstick, ref_layer, run_layer, torch_layer
from oracle.lstm_cases import make_case  # (the seeded draw, shared with tests/test_lstm_fp64_gpu.py)

pytestmark = pytest.mark.gpu

LAYER_CASES = ([(512, B, T) for T in (1, 2, 3) for B in (1, 3, 31, 32, 33, 16)] + [(512, 3, 64), (512, 33, 64)]
               + [(H, B, T) for H in (4, 8) for B in (1, 33) for T in (1, 3, 64)])


@pytest.mark.parametrize("H,B,T", LAYER_CASES)
def test_layer_against_fp64_with_torch_float32_as_yardstick(cuda, H, B, T):
    c = make_case(T, B, H, seed=H + 10 * B + 1000 * T)
    bad = check_against_yardstick("layer H%d B%d T%d" % (H, B, T), run_layer(c, cuda), ref_layer(c), torch_layer(c))
    assert not bad, bad


def bilstm_params(I, H, seed, layers=2):
    g = np.random.RandomState(seed)
    s = 1.0 / np.sqrt(H)
    out = []
    for layer in range(layers):
        nin = I if layer == 0 else 2 * H
        out.append(tuple((g.uniform(-s, s, (4 * H, nin)).astype(np.float32), g.uniform(-s, s, (4 * H, H)).astype(np.float32),
                          g.uniform(-s, s, (4 * H,)).astype(np.float32), g.uniform(-s, s, (4 * H,)).astype(np.float32)) for _ in range(2)))
    return out


def run_bilstm(x, params, dy, dev, training=False, masks=None, p_drop=0.5):
    from handwriting_line_generation_amd import ops
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    pd = [tuple(tuple(torch.from_numpy(a).to(dev).requires_grad_(True) for a in d) for d in layer) for layer in params]
    md = None if masks is None else [torch.from_numpy(m.astype(np.float32)).to(dev) for m in masks]
    y = ops.bilstm(xd, pd, p_drop, training, md)
    if dy is not None:
        y.backward(torch.from_numpy(dy).to(dev))
    torch.cuda.synchronize()
    return y.detach().cpu(), (xd.grad.cpu() if dy is not None else None), ([[[p.grad.cpu() for p in d] for d in layer] for layer in pd] if dy is not None else None)


@pytest.mark.parametrize("H,I,T,B", [(512, 512, 3, 3), (512, 512, 64, 16), (8, 3, 2, 1), (8, 3, 3, 33)])
def test_bilstm_against_fp64_with_torch_float32_as_yardstick(cuda, H, I, T, B):
    g = np.random.RandomState(H + I + T + B)
    params = bilstm_params(I, H, seed=T * 7 + B)
    x = g.randn(T, B, I).astype(np.float32)
    dy = g.randn(T, B, 2 * H).astype(np.float32)
    y, dx, grads = run_bilstm(x, params, dy, cuda)
    p64 = [tuple(tuple(a.astype(np.float64) for a in d) for d in layer) for layer in params]
    yr, caches = _lstm_ref.forward(x.astype(np.float64), p64)
    dxr, gr = _lstm_ref.backward(dy.astype(np.float64), caches)
    m = torch.nn.LSTM(I, H, bidirectional=True, num_layers=2).eval()
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    with torch.no_grad():
        for layer in range(2):
            for d, suffix in enumerate(("", "_reverse")):
                for k, n in enumerate(names):
                    getattr(m, "%s_l%d%s" % (n, layer, suffix)).copy_(torch.from_numpy(params[layer][d][k]))
    xt = torch.from_numpy(x).requires_grad_(True)
    yt, _ = m(xt)
    yt.backward(torch.from_numpy(dy))
    got = dict(y=y, dx=dx); ref = dict(y=yr, dx=dxr); yard = dict(y=yt.detach(), dx=xt.grad)
    for layer in range(2):
        for d, suffix in enumerate(("", "_reverse")):
            for k, n in enumerate(names):
                key = "%s_l%d%s" % (n, layer, suffix)
                got[key], ref[key], yard[key] = grads[layer][d][k], gr[layer][d][k], getattr(m, key).grad
    bad = check_against_yardstick("bilstm H%d I%d T%d B%d" % (H, I, T, B), got, ref, yard)
    assert not bad, bad


def _same(a, b):
    return all(torch.equal(x, y) for k in a for x, y in (zip(a[k], b[k]) if isinstance(a[k], list) else [(a[k], b[k])]))


@pytest.mark.parametrize("H,B,T", [(512, 33, 3), (8, 33, 64)])
def test_two_runs_give_the_same_bits(cuda, H, B, T):
    c = make_case(T, B, H, seed=5)
    assert _same(run_layer(c, cuda), run_layer(c, cuda))


@pytest.mark.parametrize("H,B,T", [(512, 33, 3), (512, 3, 64), (4, 33, 2)])
def test_a_row_of_the_batch_equals_the_line_run_alone(cuda, H, B, T):
    """forward and the gradients w.r.t. that row: the summation order depends on neither B nor the batch tile a line falls in"""
    c = make_case(T, B, H, seed=6)
    full = run_layer(c, cuda)
    for row in sorted({0, B // 2, 31 if B > 31 else B - 1, B - 1}):
        one = dict(xp=[a[:, row:row + 1].copy() for a in c["xp"]], w=c["w"], b=c["b"], dy=c["dy"][:, row:row + 1].copy())
        alone = run_layer(one, cuda)
        assert torch.equal(alone["y"], full["y"][:, row:row + 1]), row
        for d in range(2):
            assert torch.equal(alone["dxp"][d], full["dxp"][d][:, row:row + 1]), (row, d)


@pytest.mark.parametrize("H,B,T", [(512, 3, 3), (512, 33, 64), (8, 1, 2)])
def test_reverse_direction_equals_forward_on_the_flipped_sequence(cuda, H, B, T):
    """the reverse half of y equals the forward half of a run on the time-flipped input with the two directions' weights swapped"""
    c = make_case(T, B, H, seed=7)
    a = run_layer(c, cuda)
    f = dict(xp=[c["xp"][1][::-1].copy(), c["xp"][0][::-1].copy()], w=c["w"][::-1], b=c["b"][::-1],
             dy=np.concatenate([c["dy"][::-1, :, H:], c["dy"][::-1, :, :H]], axis=2).copy())
    b = run_layer(f, cuda)
    assert torch.equal(a["y"][:, :, H:], torch.flip(b["y"][:, :, :H], [0]))
    assert torch.equal(a["y"][:, :, :H], torch.flip(b["y"][:, :, H:], [0]))
    # (the input gradients too; dW_hh / db_hh are sums over the T*B rows in row order, which the flip changes)
    assert torch.equal(a["dxp"][1], torch.flip(b["dxp"][0], [0])) and torch.equal(a["dxp"][0], torch.flip(b["dxp"][1], [0]))


@pytest.mark.parametrize("H,B", [(512, 33), (4, 1)])
def test_one_step_equals_the_closed_form(cuda, H, B):
    c = make_case(1, B, H, seed=8)
    got = run_layer(c, cuda)["y"].numpy()
    sig = lambda v: (np.float32(1) / (np.float32(1) + np.exp(-v))).astype(np.float32)
    for d in range(2):
        pre = (c["xp"][d][0] + c["b"][d]).astype(np.float32)          # (xproj + b_hh) + 0
        i, g_, o = sig(pre[:, :H]), np.tanh(pre[:, 2 * H:3 * H]).astype(np.float32), sig(pre[:, 3 * H:])
        want = (o * np.tanh((i * g_).astype(np.float32))).astype(np.float32)
        err = float(np.abs(got[0, :, d * H:(d + 1) * H] - want).max())
        print("closed form H%d B%d dir %d: err %.3e (bound %.3e)" % (H, B, d, err, 16 * EPS))
        assert err <= 16 * EPS


@pytest.mark.parametrize("H,B,T", [(512, 33, 3), (8, 3, 64)])
def test_frozen_weights_give_the_same_input_gradient(cuda, H, B, T):
    c = make_case(T, B, H, seed=9)
    a, b = run_layer(c, cuda, wgrad=True), run_layer(c, cuda, wgrad=False)
    assert torch.equal(a["y"], b["y"]) and all(torch.equal(x, y) for x, y in zip(a["dxp"], b["dxp"]))


def test_no_grad_forward_equals_the_recorded_forward(cuda):
    """under no_grad the kernel keeps two ping-pong c buffers instead of the gates: same bits"""
    from handwriting_line_generation_amd import ops
    c = make_case(5, 33, 512, seed=10)
    a = run_layer(c, cuda)["y"]
    with torch.no_grad():
        y = ops.lstm_layer([torch.from_numpy(t).to(cuda) for t in c["xp"]], [torch.from_numpy(t).to(cuda) for t in c["w"]],
                           [torch.from_numpy(t).to(cuda) for t in c["b"]], False)
    assert torch.equal(y.cpu(), a)


def test_no_grad_with_trainable_weights_keeps_no_gates(cuda):
    """a validation pass: nn.Parameter weights (requires_grad) under torch.no_grad() must take the ping-pong path - no gates / c / hseq buffers -
    and give the recorded forward's bits. T = 64, B = 16, H = 512: y is 4.2 MB and the c ping-pong lives in the shared scratch buffer, while
    the kept buffers would be 16.8 + 4.2 + 4.3 = 25.3 MB on top: the peak may rise by y plus allocator rounding (< 8 MB), not by 29 MB."""
    from handwriting_line_generation_amd import ops
    T, B, H = 64, 16, 512
    c = make_case(T, B, H, seed=12)
    want = run_layer(c, cuda)["y"]
    xp = [torch.from_numpy(t).to(cuda).requires_grad_(True) for t in c["xp"]]
    w = [torch.nn.Parameter(torch.from_numpy(t).to(cuda)) for t in c["w"]]
    b = [torch.nn.Parameter(torch.from_numpy(t).to(cuda)) for t in c["b"]]
    with torch.no_grad():
        y = ops.lstm_layer(xp, w, b, True)            # warm-up: the scratch buffer exists afterwards
        del y
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = ops.lstm_layer(xp, w, b, True)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    print("no_grad forward with Parameters: peak rose by %.1f MB" % (rise / 1e6))
    assert y.grad_fn is None and not y.requires_grad
    assert rise < 8e6, "peak rose by %.1f MB: the gates were written" % (rise / 1e6)
    assert torch.equal(y.cpu(), want)
    # and with autograd recording the same call does keep them
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y2 = ops.lstm_layer(xp, w, b, False)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base > 25e6 and y2.grad_fn is not None
    assert torch.equal(y2.detach().cpu(), want)


def test_limits_are_errors_not_fallbacks(cuda):
    from handwriting_line_generation_amd import ops
    from handwriting_line_generation_amd._lib import HwgError
    unit, tile = ops.lstm_limits(512)
    assert (unit, tile) == (4, 32) and ops.lstm_limits(4)[1] == 32
    for H in (6, 1028):
        c = make_case(2, 2, H, seed=1)
        with pytest.raises(HwgError):
            run_layer(c, cuda)


def test_supplied_dropout_multiplier(cuda):
    """training-mode output with a supplied multiplier == the eval-mode pipeline run with that multiplier between the layers (exact), and both
    == two single-layer runs with the product taken in between; also against fp64 with the same multiplier"""
    T, B, I, H = 3, 5, 16, 8
    g = np.random.RandomState(11)
    params = bilstm_params(I, H, seed=12)
    x = g.randn(T, B, I).astype(np.float32)
    mask = ((g.rand(T, B, 2 * H) < 0.5) * 2.0).astype(np.float32)
    y_train, _, _ = run_bilstm(x, params, None, cuda, training=True, masks=[mask])
    y_eval, _, _ = run_bilstm(x, params, None, cuda, training=False, masks=[mask])
    y0, _, _ = run_bilstm(x, params[:1], None, cuda)
    y1, _, _ = run_bilstm((y0.numpy() * mask).astype(np.float32), params[1:], None, cuda)
    assert torch.equal(y_train, y_eval) and torch.equal(y_train, y1)
    p64 = [tuple(tuple(a.astype(np.float64) for a in d) for d in layer) for layer in params]
    yr, _ = _lstm_ref.forward(x.astype(np.float64), p64, [mask.astype(np.float64)])
    assert float(np.abs(y_train.numpy() - yr).max()) <= 64 * EPS          # |y| < 1, two layers of 8/16-term sums
    y_nomask, _, _ = run_bilstm(x, params, None, cuda, training=False)
    assert not torch.equal(y_nomask, y_train)


def test_philox_dropout_multiplier(cuda):
    from handwriting_line_generation_amd import rng
    T, B, C = 16, 4, 1024
    try:
        rng.set_mode("device", seed=123)
        m1 = rng.seq_mask((T, B, C), 0.5, cuda)
        m2 = rng.seq_mask((T, B, C), 0.5, cuda)
        rng.set_mode("device", seed=123)
        m3 = rng.seq_mask((T, B, C), 0.5, cuda)
        assert m1.shape == (T, B, C) and set(torch.unique(m1).tolist()) == {0.0, 2.0}
        n = T * B * C
        keep = float((m1 != 0).double().mean())
        assert abs(keep - 0.5) <= 5 * 0.5 / np.sqrt(n)
        assert not torch.equal(m1, m2) and torch.equal(m1, m3)
        rng.set_mode("host")
        torch.manual_seed(3)
        mh = rng.seq_mask((T, B, C), 0.5, cuda)
        assert mh.is_cuda and set(torch.unique(mh).tolist()) == {0.0, 2.0}
    finally:
        rng.set_mode("device", seed=0)


def test_training_mode_draws_a_mask_between_the_layers(cuda):
    from handwriting_line_generation_amd import rng
    T, B, I, H = 3, 2, 16, 8
    g = np.random.RandomState(13)
    params = bilstm_params(I, H, seed=14)
    x = g.randn(T, B, I).astype(np.float32)
    try:
        rng.set_mode("device", seed=77)
        want_mask = rng.seq_mask((T, B, 2 * H), 0.5, cuda).cpu().numpy()
        rng.set_mode("device", seed=77)
        y, _, _ = run_bilstm(x, params, None, cuda, training=True)
        y_sup, _, _ = run_bilstm(x, params, None, cuda, training=False, masks=[want_mask])
        assert torch.equal(y, y_sup)
    finally:
        rng.set_mode("device", seed=0)
