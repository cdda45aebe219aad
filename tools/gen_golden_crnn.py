"""Generate tests/golden/crnn/*.npz by running the UNMODIFIED reference CRNN (model/cnn_lstm.py, imported read-only through ref_bootstrap)
on the CPU in float32, eval().

Run in the build container only:  python tools/gen_golden_crnn.py
Weights: oracle.torch_ref.seeded_state_dict(model, WSEED) - a function of key names, shapes and the seed, so the tests rebuild them from the
project's own CRNN (same keys) and nothing but inputs and logits is stored. Inputs are stored as uint8 pixels, the network sees
u8 / 127.5 - 1. Each file: pixels [2,1,64,W] uint8, logits [T,2,NCLASS] float32 (use_softmax=False), keys / shapes of the reference's
state dict, and `max_pre`: the largest |gate pre-activation| of the two LSTM layers on that case. The tool asserts max_pre < 6 - no gate
saturates, so the comparison exercises the recurrence rather than a clamp - on every recorded case; with the seeded weights as they are no
rescaling of the LSTM weights is needed (the test therefore applies none).
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
warnings.filterwarnings("ignore")

import ref_bootstrap  # noqa: E402

ref_bootstrap.bootstrap()

import torch  # noqa: E402

from oracle import torch_ref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "crnn")
NCLASS, WSEED = 80, 7
CASES = [("batch", False, 8), ("batch", False, 40), ("batch", False, 64), ("group", False, 8), ("group", False, 40), ("group", False, 64),
         ("batch", "less", 16)]


def max_preactivation(lstm, x):
    """largest |x W_ih^T + b_ih + b_hh + h W_hh^T| over both layers, directions and steps (eval mode: no dropout between the layers)"""
    worst = 0.0
    inp = x
    for layer in range(lstm.num_layers):
        outs = []
        for suffix in ("", "_reverse"):
            w_ih, w_hh, b_ih, b_hh = (getattr(lstm, "%s_l%d%s" % (n, layer, suffix)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            T, B, _ = inp.shape
            H = w_hh.shape[1]
            h = torch.zeros(B, H); c = torch.zeros(B, H)
            ys = [None] * T
            for t in (range(T) if not suffix else range(T - 1, -1, -1)):
                pre = inp[t] @ w_ih.t() + b_ih + b_hh + h @ w_hh.t()
                worst = max(worst, float(pre.abs().max()))
                i, f, g, o = pre.chunk(4, 1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                ys[t] = h
            outs.append(torch.stack(ys))
        inp = torch.cat(outs, 2)
    return worst, inp


def main():
    from model.cnn_lstm import CRNN
    os.makedirs(GOLD, exist_ok=True)
    for norm, pad, W in CASES:
        m = CRNN(NCLASS, norm=norm, use_softmax=False, pad=pad)
        sd = torch_ref.seeded_state_dict(m, WSEED)
        m.load_state_dict(sd)
        m.eval()
        g = np.random.RandomState(1000 + W + (7 if norm == "group" else 0))
        pix = g.randint(0, 256, size=(2, 1, 64, W)).astype(np.uint8)
        x = torch.from_numpy(pix.astype(np.float32) / 127.5 - 1.0)
        feats = []
        hook = m.rnn.rnn.register_forward_hook(lambda mod, inp, out: feats.append(inp[0].detach()))
        with torch.no_grad():
            logits = m(x)
        hook.remove()
        worst, restated = max_preactivation(m.rnn.rnn, feats[0])
        assert worst < 6.0, "case %s/%s/%d: a gate pre-activation reaches %.2f - rescale the LSTM weights" % (norm, pad, W, worst)
        T = logits.shape[0]
        name = "crnn_%s_%s_w%d.npz" % (norm, pad if pad else "nopad", W)
        keys = list(m.state_dict().keys())
        np.savez_compressed(os.path.join(GOLD, name), pixels=pix, logits=logits.numpy().astype(np.float32), max_pre=np.float32(worst),
                            keys=np.array(keys), shapes=np.array([",".join(str(d) for d in m.state_dict()[k].shape) for k in keys]),
                            norm=np.array(norm), pad=np.array(str(pad) if pad else ""), nclass=np.int32(NCLASS), wseed=np.int32(WSEED))
        print("%-28s T %2d  max |pre| %.2f  %d bytes" % (name, T, worst, os.path.getsize(os.path.join(GOLD, name))))


if __name__ == "__main__":
    main()
