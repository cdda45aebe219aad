"""This project's own fp64 restatement of the CRNN recogniser: torch conv / norm / pool functions for the trunk, tests/_lstm_ref.py (numpy
fp64, wrapped as an autograd function) for the recurrence. Held to the reference's float32 logits in tests/test_crnn_cpu.py."""
import numpy as np
import torch
import torch.nn.functional as F

import _lstm_ref

NORMED = (2, 4, 6)
PADS = [1, 1, 1, 1, 1, 0, 0]
POOLS = {0: ((2, 2), (2, 2), (0, 0)), 1: ((2, 2), (2, 2), (0, 0)), 3: ((2, 2), (2, 1), (0, 1)), 5: ((2, 2), (2, 1), (0, 1))}
LSTM_NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def lstm_params(sd, prefix="rnn.rnn.", layers=2):
    return [tuple(tuple(sd["%s%s_l%d%s" % (prefix, n, layer, suffix)] for n in LSTM_NAMES) for suffix in ("", "_reverse")) for layer in range(layers)]


class _LSTM(torch.autograd.Function):
    """_lstm_ref.forward / backward under torch autograd; flat: x, then 8 tensors per layer"""

    @staticmethod
    def forward(ctx, masks, x, *flat):
        params = [((flat[8 * l + 0], flat[8 * l + 1], flat[8 * l + 2], flat[8 * l + 3]), (flat[8 * l + 4], flat[8 * l + 5], flat[8 * l + 6], flat[8 * l + 7]))
                  for l in range(len(flat) // 8)]
        nparams = [tuple(tuple(p.detach().numpy() for p in d) for d in layer) for layer in params]
        y, caches = _lstm_ref.forward(x.detach().numpy(), nparams, masks)
        ctx.caches = caches
        return torch.from_numpy(y)

    @staticmethod
    def backward(ctx, dy):
        dx, grads = _lstm_ref.backward(dy.numpy(), ctx.caches)
        flat = [torch.from_numpy(np.ascontiguousarray(g)) for layer in grads for d in layer for g in d]
        return (None, torch.from_numpy(dx)) + tuple(flat)


def forward(sd, x, norm_kind, pad=False, use_softmax=False, masks=None, bn_training=False, torch_lstm=None):
    """sd: fp64 state dict (reference key names); x NCHW [B,1,64,W] fp64 -> [T,B,nclass]. torch_lstm: an nn.LSTM to run the recurrence with
    instead of _lstm_ref (the float32 yardstick: torch's own LSTM in the dtype of sd and x; its parameters are used, not sd's)"""
    if pad:
        c = 64 if pad == "less" else 128
        x = F.pad(x, (c, c, 0, 0))
    if x.shape[3] < 12:
        diff = 12 - x.shape[3]
        x = F.pad(x, (diff // 2, diff // 2 + diff % 2))
    h = x
    for i in range(7):
        h = F.conv2d(h, sd["cnn.conv%d.weight" % i], sd["cnn.conv%d.bias" % i], padding=PADS[i])
        if i in NORMED and norm_kind == "group":
            h = F.group_norm(h, 8, sd["cnn.groupnorm%d.weight" % i], sd["cnn.groupnorm%d.bias" % i])
        elif i in NORMED and norm_kind == "batch":
            p = "cnn.batchnorm%d." % i
            h = F.batch_norm(h, sd[p + "running_mean"].clone(), sd[p + "running_var"].clone(), sd[p + "weight"], sd[p + "bias"], bn_training)
        h = F.relu(h)
        if i in POOLS:
            h = F.max_pool2d(h, *POOLS[i])
    b, c, hh, w = h.shape
    assert hh == 1
    seq = h.view(b, c, w).permute(2, 0, 1).contiguous()
    flat = [p for layer in lstm_params(sd) for d in layer for p in d]
    rec = torch_lstm(seq)[0] if torch_lstm is not None else _LSTM.apply(masks, seq, *flat)
    T, b, hdim = rec.shape
    out = (rec.reshape(T * b, hdim) @ sd["rnn.embedding.weight"].t() + sd["rnn.embedding.bias"]).view(T, b, -1)
    return F.log_softmax(out, dim=2) if use_softmax else out
