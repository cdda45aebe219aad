"""numpy fp64 restatement of the bidirectional multi-layer LSTM (torch.nn.LSTM gate order i, f, g, o), forward and all gradients.

The dropout multiplier between the layers is an INPUT (`masks[l]`, [T,B,2H], applied to the output of layer l < last), so that a test can
hold the device pipeline to exactly the mask it drew. Pinned to torch.nn.LSTM(...).double() in tests/test_crnn_cpu.py.

Parameters: per layer a pair (forward, reverse) of (w_ih [4H,I], w_hh [4H,H], b_ih [4H], b_hh [4H]).
"""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def layer_forward(xp, w_hh, b_hh):
    """one bidirectional layer given its input projections: xp (fwd, rev) each [T,B,4H]; w_hh (fwd, rev) [4H,H]; b_hh (fwd, rev) [4H]
    -> y [T,B,2H], cache"""
    T, B, G = xp[0].shape
    H = G // 4
    y = np.zeros((T, B, 2 * H))
    gates = np.zeros((2, T, B, G))
    cs = np.zeros((2, T, B, H))
    hprev = np.zeros((2, T, B, H))
    for d in range(2):
        h = np.zeros((B, H)); c = np.zeros((B, H))
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            hprev[d, t] = h
            pre = (xp[d][t] + b_hh[d]) + h @ w_hh[d].T
            i, f, g, o = _sig(pre[:, :H]), _sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), _sig(pre[:, 3 * H:])
            c = f * c + i * g
            h = o * np.tanh(c)
            gates[d, t] = np.concatenate([i, f, g, o], axis=1)
            cs[d, t] = c
            y[t, :, d * H:(d + 1) * H] = h
    return y, (gates, cs, hprev, [np.asarray(w) for w in w_hh])


def layer_backward(dy, cache):
    """-> dxp (fwd, rev) [T,B,4H] (= the pre-activation gate gradients), dw_hh (fwd, rev), db_hh (fwd, rev)"""
    gates, cs, hprev, w_hh = cache
    _, T, B, G = gates.shape
    H = G // 4
    dgates = np.zeros_like(gates)
    for d in range(2):
        dh_rec = np.zeros((B, H)); dc_next = np.zeros((B, H))
        order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        for n, t in enumerate(reversed(order)):
            i, f, g, o = (gates[d, t][:, k * H:(k + 1) * H] for k in range(4))
            c = cs[d, t]
            later = len(order) - 1 - n            # position of t in the forward walk
            cp = cs[d, order[later - 1]] if later > 0 else np.zeros((B, H))
            dh = dy[t][:, d * H:(d + 1) * H] + dh_rec
            tc = np.tanh(c)
            dc = dc_next + dh * o * (1 - tc * tc)
            dg = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], axis=1)
            dgates[d, t] = dg
            dc_next = dc * f
            dh_rec = dg @ w_hh[d]
    dw = [dgates[d].reshape(T * B, G).T @ hprev[d].reshape(T * B, H) for d in range(2)]
    db = [dgates[d].reshape(T * B, G).sum(0) for d in range(2)]
    return (dgates[0], dgates[1]), dw, db


def forward(x, params, masks=None):
    """x [T,B,I] -> y [T,B,2H] of the last layer, cache"""
    T, B, _ = x.shape
    h = np.asarray(x, dtype=np.float64)
    caches = []
    for li, (pf, pr) in enumerate(params):
        rows = h.reshape(T * B, -1)
        xp = [(rows @ np.asarray(p[0], dtype=np.float64).T + np.asarray(p[2], dtype=np.float64)).reshape(T, B, -1) for p in (pf, pr)]
        y, cache = layer_forward(xp, [np.asarray(pf[1], dtype=np.float64), np.asarray(pr[1], dtype=np.float64)],
                                 [np.asarray(pf[3], dtype=np.float64), np.asarray(pr[3], dtype=np.float64)])
        m = masks[li] if (masks is not None and li + 1 < len(params)) else None
        caches.append((rows, cache, m, (pf, pr)))
        h = y * m if m is not None else y
    return h, caches


def backward(dy, caches):
    """-> dx [T,B,I], grads: per layer a pair (forward, reverse) of (dw_ih, dw_hh, db_ih, db_hh)"""
    grads = []
    d = np.asarray(dy, dtype=np.float64)
    T, B, _ = d.shape
    for rows, cache, m, (pf, pr) in reversed(caches):
        if m is not None:
            d = d * m
        dxp, dw_hh, db_hh = layer_backward(d, cache)
        drows = 0.0
        layer = []
        for k, p in enumerate((pf, pr)):
            g2 = dxp[k].reshape(T * B, -1)
            layer.append((g2.T @ rows, dw_hh[k], g2.sum(0), db_hh[k]))
            drows = drows + g2 @ np.asarray(p[0], dtype=np.float64)
        grads.append(tuple(layer))
        d = drows.reshape(T, B, -1)
    return d, grads[::-1]
