"""Dispatch trace of the convolution family (ops._Conv2d): which C-ABI calls, with which descriptors, scalars, tensor shapes, streams and
scratch requests, every layer geometry of the tests becomes - recorded on CPU tensors with the launch seam faked, no GPU needed.

    python tools/gen_golden_conv_dispatch.py            # writes tests/golden/conv_dispatch.json.xz

tests/test_conv_dispatch_cpu.py records again and compares record for record. Only these seams are touched: L.call (records instead of
launching; hwg_tuning_reload passes through), ops._stream, ops._chk, ops._side_stream and the three workspace functions (recorders that
return CPU byte buffers); the module's side-stream bookkeeping containers are swapped for private ones so nothing leaks into a later GPU run.

One record per call: [entry point, arg, ...] with descriptor pointer -> its 16 fields, tensor -> ["t", shape], None, int / float parameters by
value (types from L.DECLS), the stream as "main" / "side", any other pointer as "ptr"; size_t arguments are left out (scratch buffer sizes
depend on what ran before). A scratch request is ["workspace" | "defer_workspace" | "side_workspace", bytes].
"""
import ctypes
import lzma
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ops_cases as T  # noqa: E402  (the geometries tests/test_ops_gpu.py runs)
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json.xz")
MAIN, SIDE = 0x5151515100, 0x5252525200        # stand-ins for the raw stream handles

TUNINGS = {"wino0": {"HWG_WINO": "0"}, "wino2": {"HWG_WINO": "2", "HWG_WINO_S2": "2", "HWG_WINO_WGRAD": "2"}}
FLAGS = {"plain": (False, False), "defer": (True, False), "side": (False, True), "defer_side": (True, True)}       # (DEFER_REDUCE, SIDE_WGRAD)


def cases():
    """[(name, variant, kind, geometry)]: variant = param (leaf parameters with bias) | nonleaf | nobias | sn_defer; kind = conv | conv1d |
    linear | linear_wgrad"""
    out = [(c[0], "param", "conv", c[1:]) for c in T.CONV_CASES + T.RANDOM_CONV_CASES]
    # 4x4 stride-2 pad-0 layers: the two-tap Winograd entries (no CONV_CASES row reaches them)
    for (N, H, W, C, K, _env) in T.WINO_S2_CASES:
        out.append(("s2_%dx%dx%dx%d_k%d" % (N, H, W, C, K), "param", "conv", (N, H, W, C, K, 4, 4, (2, 2), (0, 0), (1, 1), False)))
    by_name = {c[0]: c[1:] for c in T.CONV_CASES}
    extra = ["mfma128x32", "wino_pad0_k48", "stride2_4x4", "c1_5x5", "to1_3x3_c32_pad01", "convT_s2_4x4", "convT_s1_3x3", "rimes_conv1d_to78",
             "onerow_out_4x4_s21_h5"]
    for variant in ("nonleaf", "nobias", "sn_defer"):
        out += [(n, variant, "conv", by_name[n]) for n in extra]
    out.append(("conv1d_c64_k48_s5", "param", "conv1d", (3, 37, 64, 48, 5, 2, 2, 1)))      # N, L, C, K, S, stride, padding, dilation
    out.append(("linear_70x96_to_40", "param", "linear", (70, 96, 40)))                      # rows, I, O
    out.append(("linear_70x96_to_40", "nobias", "linear", (70, 96, 40)))
    out.append(("linear_70x96_to_78", "param", "linear_wgrad", (70, 96, 78)))
    return out


class Recorder:
    def __init__(self, ops, L, setattr_):
        """setattr_(object, name, value): how attributes are replaced (pytest's monkeypatch.setattr, or Patcher.setattr below)"""
        self.ops, self.L, self.records = ops, L, []
        real_call = L.call

        def call(name, *args):
            if name == "hwg_tuning_reload":
                return real_call(name)
            self.records.append([name] + self._encode(name, args))

        def ws(kind):
            def request(nbytes, device, *stream):
                self.records.append([kind, int(nbytes)])
                return torch.empty(max(int(nbytes), 1), dtype=torch.uint8)
            return request
        setattr_(L, "call", call)
        setattr_(ops, "_stream", lambda: MAIN)
        setattr_(ops, "_chk", lambda t, name, dtype=torch.float32: None)
        setattr_(ops, "_side_stream", lambda device: (None, SIDE, 0))
        setattr_(ops, "workspace", ws("workspace"))
        setattr_(ops, "_defer_workspace", ws("defer_workspace"))
        setattr_(ops, "_side_workspace", ws("side_workspace"))
        setattr_(ops, "_side_hold", [])
        setattr_(ops, "_side_dirty", set())

    def _encode(self, name, args):
        argtypes = self.L.DECLS[name][1]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        out = []
        for a, t in zip(args, argtypes):
            if t is ctypes.c_size_t:
                continue
            if isinstance(t, type) and issubclass(t, ctypes._Pointer):
                d = self.L.ConvDesc.from_address(int(a))
                out.append([int(getattr(d, f)) for f, _ in self.L.ConvDesc._fields_])
            elif t in (ctypes.c_void_p, ctypes.c_char_p):
                if a is None:
                    out.append(None)
                elif isinstance(a, torch.Tensor):
                    out.append(["t", list(a.shape)])
                else:
                    out.append("main" if a == MAIN else "side" if a == SIDE else "ptr")
            elif t in (ctypes.c_float, ctypes.c_double):
                out.append(float(a))
            else:
                out.append(int(a))
        return out

    def take(self):
        out, self.records = self.records, []
        return out


def _params(variant, wshape, K):
    """-> (weight, bias) as the op sees them, and the parameters behind them"""
    w0 = torch.nn.Parameter(torch.zeros(wshape))
    b0 = torch.nn.Parameter(torch.zeros(K)) if variant != "nobias" else None
    leaves = [p for p in (w0, b0) if p is not None]
    if variant in ("nonleaf", "sn_defer"):
        w, b = w0 * 1.0, b0 * 1.0
        if variant == "sn_defer":
            w._hwg_sn_defer = True
        return w, b, leaves
    return w0, b0, leaves


def _forward(ops, kind, geom, x, w, b):
    if kind == "conv":
        stride, pad, dil, transposed = geom[7:]
        if transposed:
            return ops.conv_transpose2d(x, w, b, stride=stride, padding=pad, dilation=dil)
        return ops.conv2d(x, w, b, stride=stride, padding=pad, dilation=dil)
    if kind == "conv1d":
        return ops.conv1d(x, w, b, stride=geom[5], padding=geom[6], dilation=geom[7])
    return ops.linear(x, w, b)


def _shapes(kind, geom):
    if kind == "conv":
        N, H, W, C, K, R, S, stride, pad, dil, transposed = geom
        return (N, H, W, C), ((C, K, R, S) if transposed else (K, C, R, S)), K
    if kind == "conv1d":
        N, Ln, C, K, S = geom[:5]
        return (N, 1, Ln, C), (K, C, S), K
    rows, I, O = geom
    return (rows, I), (O, I), O


def trace_case(ops, rec, case, mode):
    """records of one layer: forward, then autograd backward (mode "autograd") or a two-set Tape.backward_sets, set 0 redirected into a
    FlatParams stash and set 1 into the parameters (mode "sets"); None where the combination does not exist"""
    from handwriting_line_generation_amd.trainer.flat_params import FlatParams
    name, variant, kind, geom = case
    xshape, wshape, K = _shapes(kind, geom)
    rec.take()
    if kind == "linear_wgrad":
        if mode != "autograd":
            return None
        w = torch.nn.Parameter(torch.zeros(wshape))
        ops._linear_wgrad(torch.zeros(xshape), torch.zeros(xshape[0], K), w)
        return rec.take()
    if mode == "autograd":
        w, b, leaves = _params(variant, wshape, K)
        x = torch.zeros(xshape, requires_grad=True)
        y = _forward(ops, kind, geom, x, w, b)
        y.backward(torch.zeros(y.shape))
        return rec.take()
    if kind == "linear" or variant == "sn_defer":       # (linear returns a reshape the tape only adopts when another op consumes it)
        return None
    w, b, leaves = _params("nobias" if variant == "nobias" else "param", wshape, K)
    tape = ops.Tape()
    x = tape.watch(torch.zeros(xshape))
    if variant == "nonleaf":                               # plain tensors the tape watches: their gradients are returned per set, not accumulated
        w, b = tape.watch(torch.zeros(wshape)), tape.watch(torch.zeros(K))
        targets = [None, None]
    else:
        flat = FlatParams(leaves, {"main": leaves})
        targets = [(torch.zeros_like(flat.flat_grad), np.zeros(flat.nt, dtype=bool)), None]
    with ops.taping(tape), torch.no_grad():
        y = _forward(ops, kind, geom, x, w, b)
    tape.backward_sets(y, [torch.zeros(y.shape), torch.zeros(y.shape)], targets)
    return rec.take()


def record_all(ops, L, setattr_):
    """{"case|variant|tuning|flags|mode": [records]} for every case and setting"""
    rec = Recorder(ops, L, setattr_)
    out = {}
    try:
        for tname, env in TUNINGS.items():
            with ops.tuning(**env):
                for fname, (defer, side) in FLAGS.items():
                    setattr_(ops, "DEFER_REDUCE", defer)
                    setattr_(ops, "SIDE_WGRAD", side)
                    for case in cases():
                        for mode in ("autograd", "sets"):
                            got = trace_case(ops, rec, case, mode)
                            if got is not None:
                                out["|".join((case[0], case[1], tname, fname, mode))] = got
    finally:
        # nothing of the CPU tensors stays behind in the module's caches
        for cache in ("_pack_cache", "_ws_cache", "_set_views", "_pack_tables"):
            getattr(ops, cache).clear()
    return out


class Patcher:
    def __init__(self):
        self.saved = []

    def setattr(self, obj, name, value):
        self.saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def undo(self):
        for obj, name, value in reversed(self.saved):
            setattr(obj, name, value)
        del self.saved[:]


def dumps(traces):
    """the file's bytes: xz (the same traces give the same bytes) of a JSON object, one trace per line"""
    text = "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in traces.items()) + "\n}\n"
    return lzma.compress(text.encode(), preset=9)


def loads(data):
    return json.loads(lzma.decompress(data))


def main():
    sys.path.insert(0, ROOT)
    from handwriting_line_generation_amd import _lib as L, ops
    p = Patcher()
    try:
        traces = record_all(ops, L, p.setattr)
    finally:
        p.undo()
    with open(GOLDEN, "wb") as f:
        f.write(dumps(traces))
    names = sorted({r[0] for t in traces.values() for r in t})
    print("%d traces, %d records -> %s" % (len(traces), sum(len(t) for t in traces.values()), GOLDEN))
    print("entries:", " ".join(names))


if __name__ == "__main__":
    main()
