"""One ops.lstm_layer case on the device, in fp64 and through torch's float32 nn.LSTM, and the yardstick comparison of the three (not
collected by pytest; used by tests/test_lstm_gpu.py, whose docstring states the condition, and tests/test_lstm_fp64_gpu.py)."""
import numpy as np
import torch

import _lstm_ref

EPS = 2.0 ** -24


def run_layer(c, dev, wgrad=True, training=True):
    from handwriting_line_generation_amd import ops
    xp = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in c["xp"]]
    w = [torch.from_numpy(a).to(dev).requires_grad_(wgrad) for a in c["w"]]
    b = [torch.from_numpy(a).to(dev).requires_grad_(wgrad) for a in c["b"]]
    y = ops.lstm_layer(xp, w, b, training)
    y.backward(torch.from_numpy(c["dy"]).to(dev))
    torch.cuda.synchronize()
    out = dict(y=y.detach().cpu(), dxp=[t.grad.cpu() for t in xp])
    if wgrad:
        out["dw"] = [t.grad.cpu() for t in w]
        out["db"] = [t.grad.cpu() for t in b]
    return out


def ref_layer(c):
    y, cache = _lstm_ref.layer_forward([a.astype(np.float64) for a in c["xp"]], [a.astype(np.float64) for a in c["w"]], [a.astype(np.float64) for a in c["b"]])
    dxp, dw, db = _lstm_ref.layer_backward(c["dy"].astype(np.float64), cache)
    return dict(y=y, dxp=list(dxp), dw=dw, db=db)


def torch_layer(c):
    """torch float32 CPU nn.LSTM on the same case (identity input projection, see the module docstring)"""
    T, B, G = c["xp"][0].shape
    H = G // 4
    m = torch.nn.LSTM(2 * G, H, bidirectional=True)
    with torch.no_grad():
        for d, suffix in enumerate(("", "_reverse")):
            wi = torch.zeros(G, 2 * G)
            wi[:, d * G:(d + 1) * G] = torch.eye(G)
            getattr(m, "weight_ih_l0" + suffix).copy_(wi)
            getattr(m, "bias_ih_l0" + suffix).zero_()
            getattr(m, "weight_hh_l0" + suffix).copy_(torch.from_numpy(c["w"][d]))
            getattr(m, "bias_hh_l0" + suffix).copy_(torch.from_numpy(c["b"][d]))
    x = torch.from_numpy(np.concatenate(c["xp"], axis=2)).requires_grad_(True)
    y, _ = m(x)
    y.backward(torch.from_numpy(c["dy"]))
    return dict(y=y.detach(), dxp=[x.grad[:, :, :G], x.grad[:, :, G:]], dw=[m.weight_hh_l0.grad, m.weight_hh_l0_reverse.grad],
                db=[m.bias_hh_l0.grad, m.bias_hh_l0_reverse.grad])


def check_against_yardstick(tag, got, ref, yard):
    """-> list of failures; prints err_hip / bound per tensor"""
    bad = []
    for k in ref:
        pairs = [(got[k], ref[k], yard[k])] if not isinstance(ref[k], list) else list(zip(got[k], ref[k], yard[k]))
        for j, (a, r, t) in enumerate(pairs):
            a = a.double().numpy(); t = np.asarray(t.detach().double().numpy() if hasattr(t, "detach") else t); r = np.asarray(r)
            err_hip = float(np.abs(a - r).max()); err_t = float(np.abs(t - r).max()); scale = float(np.abs(r).max())
            bound = 4 * err_t + 4 * EPS * scale
            print("LSTMRATIO %s %s[%d] err_hip %.3e err_torch %.3e scale %.3e ratio %.3f" % (tag, k, j, err_hip, err_t, scale, err_hip / max(bound, 1e-300)))
            if not err_hip <= bound:
                bad.append((tag, k, j, err_hip, bound))
    return bad
