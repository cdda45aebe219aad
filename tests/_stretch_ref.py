"""numpy restatement of the stretch rule (include/hwg.h, hwg_stretch_onehot): what F.interpolate(x, scale_factor=s, mode='linear') computes
on the CPU for a one-hot x [B, C, T], from the label indices.

T_out = floor(double(T) * s); T_out == T: the plain one-hot (torch copies). Otherwise r = float32(1 / s) and per output step t
src = fl32(r * (t + 0.5) - 0.5) with ONE rounding - evaluated here exactly: r is an fp32 (24 significant bits) and t + 0.5 a half-integer
below 2^23 (24 bits), so their product has at most 48 significant bits and is exact in float64; for the scales used here r lies in
[0.5, 2), the product is a multiple of 2^-25 below 2^24, and so is the product minus 0.5: 49 bits, still exact in float64's 53. The cast
to float32 is then the single rounding, which is what fmaf does.
src = max(src, 0), i0 = min(int(src), T - 1), i1 = min(i0 + 1, T - 1), w1 = src - i0, w0 = 1 - w1 (fp32),
out[c] = w0 * [label[i0] == c] + w1 * [label[i1] == c] (fp32; the products are exact, the sum is rounded once)."""
import math

import numpy as np


def film_scales():
    """the 79 scale factors of the reference's film (generate.py:834-851), from the same np.arange calls; the two "vertical" loops render
    the label of the loop before them again"""
    a, b, c = np.arange(1, 1.11, 0.01), np.arange(1.1, 0.89, -0.01), np.arange(0.9, 1.01, 0.01)
    return [float(s) for s in a] + [float(a[-1])] * len(np.arange(1, 1.11, 0.01)) + [float(s) for s in b] + \
        [float(b[-1])] * len(np.arange(1.1, 0.89, -0.01)) + [float(s) for s in c]


def out_len(T, s):
    return int(math.floor(float(T) * float(s)))


def taps(T, s):
    """-> (i0 int64 [T_out], i1 int64 [T_out], w0 float32 [T_out], w1 float32 [T_out])"""
    T_out = out_len(T, s)
    assert T_out >= 1
    t = np.arange(T_out)
    if T_out == T:
        return t, t, np.ones(T_out, np.float32), np.zeros(T_out, np.float32)
    r = np.float32(1.0 / float(s))
    src = (np.float64(r) * (t.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    w1 = (src - i0.astype(np.float32)).astype(np.float32)
    w0 = (np.float32(1) - w1).astype(np.float32)
    return i0, i1, w0, w1


def stretch(label_TB, ncls, s):
    """label int [T, B] -> float32 [T_out, B, ncls], time major (its NHWC twin is .transpose(1, 0, 2)[:, None])"""
    label = np.asarray(label_TB)
    T, B = label.shape
    i0, i1, w0, w1 = taps(T, s)
    cls = np.arange(ncls)
    h0 = (label[i0][:, :, None] == cls).astype(np.float32)
    h1 = (label[i1][:, :, None] == cls).astype(np.float32)
    return (w0[:, None, None] * h0 + w1[:, None, None] * h1).astype(np.float32)
