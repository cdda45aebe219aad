"""CPU checks of the CRNN recogniser's references and plumbing (no GPU): the numpy fp64 LSTM against torch.nn.LSTM in fp64, the project's
fp64 CRNN restatement against the reference's recorded float32 logits, the new CRNN's state-dict keys and shapes, and the `hwr` config
parsing of HWWithStyle."""
import os

import numpy as np
import pytest
import torch

import _crnn_ref
import _lstm_ref
from _crnn_golden import GOLD, GOLDENS, golden_case, seeded_sd


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))


def torch_lstm_params(m):
    return [tuple(tuple(getattr(m, "%s_l%d%s" % (n, layer, suffix)).detach().numpy() for n in _crnn_ref.LSTM_NAMES) for suffix in ("", "_reverse"))
            for layer in range(m.num_layers)]


@pytest.mark.parametrize("H,I", [(4, 3), (4, 512), (512, 3), (512, 512)])
@pytest.mark.parametrize("T,B", [(1, 1), (2, 3), (7, 1), (7, 3), (1, 3), (2, 1)])
def test_lstm_ref_equals_torch_fp64(H, I, T, B):
    """forward and every gradient of tests/_lstm_ref.py against torch.nn.LSTM(bidirectional, 2 layers).double() in eval mode: 1e-12 relative"""
    torch.manual_seed(H * 1000 + I + T * 10 + B)
    m = torch.nn.LSTM(I, H, bidirectional=True, num_layers=2).double().eval()
    x = torch.randn(T, B, I, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(T, B, 2 * H, dtype=torch.float64)
    y, _ = m(x)
    y.backward(dy)
    yr, caches = _lstm_ref.forward(x.detach().numpy(), torch_lstm_params(m))
    dx, grads = _lstm_ref.backward(dy.numpy(), caches)
    assert _rel(yr, y.detach().numpy()) <= 1e-12
    assert _rel(dx, x.grad.numpy()) <= 1e-12
    for layer in range(2):
        for d, suffix in enumerate(("", "_reverse")):
            for k, n in enumerate(_crnn_ref.LSTM_NAMES):
                want = getattr(m, "%s_l%d%s" % (n, layer, suffix)).grad.numpy()
                assert _rel(grads[layer][d][k], want) <= 1e-12, (n, layer, suffix)


def test_lstm_ref_mask_is_applied_between_the_layers():
    g = np.random.RandomState(3)
    m = torch.nn.LSTM(5, 4, bidirectional=True, num_layers=2).double().eval()
    x = g.randn(3, 2, 5)
    mask = (g.rand(3, 2, 8) < 0.5) * 2.0
    p = torch_lstm_params(m)
    y1, _ = _lstm_ref.forward(x, p[:1])
    want, _ = _lstm_ref.forward(y1 * mask, [p[1]])        # layer 1 alone on the masked output of layer 0
    got, _ = _lstm_ref.forward(x, p, [mask])
    assert np.array_equal(got, want)


def test_goldens_are_recorded():
    names = {os.path.basename(p) for p in GOLDENS}
    assert names == {"crnn_%s_nopad_w%d.npz" % (n, w) for n in ("batch", "group") for w in (8, 40, 64)} | {"crnn_batch_less_w16.npz"}
    for p in GOLDENS:
        c = golden_case(p)
        assert c["max_pre"] < 6.0                       # no gate saturates on the recorded cases (asserted by the tool too)
        W = c["pixels"].shape[3] + (128 if c["pad"] == "less" else 0)
        assert c["logits"].shape == (max(W, 12) // 4 - 2, 2, c["nclass"])


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_crnn_ref_matches_the_reference_logits(path):
    """tests/_crnn_ref.py (fp64) against the logits the unmodified reference computed in float32 on the CPU. Bound: float32 accuracy of the
    reference itself - seven convolutions with up to 4608-term sums, two LSTM layers and a 1024-term linear layer, each a float32 sum with
    relative rounding error ~ sqrt(n) 2^-24 of its magnitude; 1e-4 of the logits' scale is several times that and far below any modelling
    difference (a wrong gate order or pooling shifts the logits by O(1))."""
    c = golden_case(path)
    sd = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in seeded_sd(c["keys"], c["shapes"], c["wseed"]).items()}
    x = torch.from_numpy(c["pixels"].astype(np.float32) / 127.5 - 1.0).double()
    with torch.no_grad():
        got = _crnn_ref.forward(sd, x, c["norm"], c["pad"]).numpy()
    scale = float(np.abs(c["logits"]).max())
    err = float(np.abs(got - c["logits"]).max())
    print("%s: |ref fp64 - reference fp32| = %.3e, scale %.3f" % (os.path.basename(path), err, scale))
    assert err <= 1e-4 * scale


@pytest.mark.parametrize("path", [p for p in GOLDENS if p.endswith("w8.npz")], ids=["batch", "group"])
def test_crnn_state_dict_keys_and_shapes_equal_the_reference(path):
    from handwriting_line_generation_amd.model.cnn_lstm import CRNN
    c = golden_case(path)
    m = CRNN(c["nclass"], norm=c["norm"])
    sd = m.state_dict()
    assert list(sd.keys()) == c["keys"]                 # same entries in the same order (optimizer state is keyed by position)
    assert [tuple(v.shape) for v in sd.values()] == c["shapes"]
    m.load_state_dict(seeded_sd(c["keys"], c["shapes"], c["wseed"]), strict=True)
    lstm = torch.nn.LSTM(512, 512, bidirectional=True, dropout=0.5, num_layers=2)
    assert [n for n, _ in m.rnn.rnn.named_parameters()] == [n for n, _ in lstm.named_parameters()]
    lstm.load_state_dict(m.rnn.rnn.state_dict(), strict=True)


def test_crnn_refuses_the_variants_that_are_not_built():
    from handwriting_line_generation_amd.model.cnn_lstm import CRNN, SmallCRNN
    for kw in (dict(leakyRelu=True), dict(small=True)):
        with pytest.raises(NotImplementedError, match="not used by any shipped config"):
            CRNN(80, **kw)
    with pytest.raises(NotImplementedError, match="not used by any shipped config"):
        SmallCRNN(80)


def _model_cfg(hwr):
    import json
    with open(os.path.join(os.path.dirname(GOLD), "model_config_iam.json")) as f:
        cfg = json.load(f)
    cfg = cfg.get("model", cfg)
    cfg = dict(cfg)
    cfg["pretrained_hwr"] = None
    if hwr is None:
        cfg.pop("hwr", None)
    else:
        cfg["hwr"] = hwr
    return cfg


@pytest.mark.parametrize("hwr,norm_kind,pad_cols", [("CRNN", "batch", 0), ("CRNN_group_norm_softmax", "group", 0), ("CRNN no_norm pad less", None, 64),
                                                    (None, "batch", 0), ("CRNN batchnorm pad", "batch", 128)])
def test_hw_with_style_builds_a_crnn(hwr, norm_kind, pad_cols):
    from handwriting_line_generation_amd.model import HWWithStyle
    from handwriting_line_generation_amd.model.cnn_lstm import CRNN
    m = HWWithStyle(_model_cfg(hwr))
    assert isinstance(m.hwr, CRNN) and m.hwr.use_softmax is True
    assert m.hwr.norm_kind == norm_kind and m.hwr.pad_cols == pad_cols
    assert ("cnn.batchnorm2.weight" in m.hwr.state_dict()) == (norm_kind == "batch")
    assert ("cnn.groupnorm2.weight" in m.hwr.state_dict()) == (norm_kind == "group")


@pytest.mark.parametrize("hwr", ["CRNN small", "CRNN sma32"])
def test_hw_with_style_refuses_the_small_crnns(hwr):
    from handwriting_line_generation_amd.model import HWWithStyle
    with pytest.raises(NotImplementedError):
        HWWithStyle(_model_cfg(hwr))
