"""Guarded buffers and the C-ABI protocol that the *_fp64_gpu / *_abi_* / *_guards_* tests hold every entry to (not collected by pytest;
tests/test_guarded_cpu.py drives it on CPU tensors with fake entries and shows that it catches what it claims to catch).

Every operand, every output and the workspace are carved out of ONE allocation with GUARD floats of canary before, between and after them.
protocol(): before the call every owned output and the workspace are filled with NaN (an output the entry adds to: with its pre-filled
value). After the call: return code 0, canaries intact, every input bit-identical, every output the call does not own unchanged, every
documented output finite. A second call with the workspace filled with ZERO bytes instead of NaN gives the same bits. A call with
ws_bytes - 1, and one with ws = NULL, return HWG_ERR_WORKSPACE and leave outputs and canaries alone. Entries without a workspace get the
canary, input and repeatability parts."""
import numpy as np
import torch

GUARD = 64                   # floats of canary before, between and after the carved buffers
CANARY = -7.0e33
HWG_ERR_ARG, HWG_ERR_WORKSPACE = -1, -3      # include/hwg.h (held to the header by tests/test_guarded_cpu.py)
NAN = float("nan")


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def carve(dev, *numels):
    """-> ([flat float32 views of one allocation, 256-byte aligned, GUARD floats of canary around each], intact()): a 16-byte store past the
    end of a buffer, or before its start, lands in a canary"""
    offs, pos = [], GUARD
    for n in numels:
        offs.append(pos)
        pos += (n + 63) // 64 * 64 + GUARD
    buf = torch.full((pos,), CANARY, dtype=torch.float32, device=dev)
    views = [buf[o:o + n] for o, n in zip(offs, numels)]

    def intact():
        live = torch.zeros(pos, dtype=torch.bool, device=dev)
        for o, n in zip(offs, numels):
            live[o:o + n] = True
        return bool((buf[~live] == CANARY).all())
    return views, intact


def put(view, t):
    view.copy_(t.reshape(-1).to(view.device))
    return view


class Guarded:
    """inputs {name: CPU tensor}, outputs {name: (shape, dtype) - filled with NaN bits before a call - or a CPU tensor - pre-filled with it}
    and a workspace of exactly `ws_bytes`, all carved out of one allocation. 4- and 8-byte element types (and bytes, in multiples of 4)."""

    def __init__(self, dev, inputs, outputs, ws_bytes=0):
        self.dev = dev
        assert ws_bytes % 4 == 0, "workspace of %d bytes: not a multiple of 4" % ws_bytes
        self.need = int(ws_bytes)
        self.ins, self.outs = list(inputs), list(outputs)
        self.shape, self.dtype, self.init = {}, {}, {}
        floats = []
        for k, v in list(inputs.items()) + list(outputs.items()):
            shape, dtype = (tuple(v.shape), v.dtype) if torch.is_tensor(v) else (tuple(v[0]), v[1])
            nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
            assert nbytes % 4 == 0, (k, shape, dtype)
            self.shape[k], self.dtype[k] = shape, dtype
            self.init[k] = v.contiguous() if torch.is_tensor(v) else None
            floats.append(nbytes // 4)
        views, self.intact = carve(dev, *(floats + [self.need // 4]))
        self.f = dict(zip(self.ins + self.outs, views))                 # flat float32 views
        self.ws = views[-1] if self.need else None
        self._on_gpu = views[-1].is_cuda
        for k in self.ins:
            self.t(k).copy_(self.init[k])
        self.reset()
        self.sync()
        self.sent = {k: self.f[k].clone() for k in self.ins}

    @property
    def L(self):
        """the library, resolved on first use (a Guarded on CPU tensors needs none)"""
        from handwriting_line_generation_amd import _lib
        return _lib

    @property
    def st(self):
        if "_st" not in self.__dict__:
            from handwriting_line_generation_amd import ops
            self._st = ops._stream()
        return self._st

    def sync(self):
        if self._on_gpu:
            torch.cuda.synchronize()

    def t(self, k):
        """the buffer in its own type and shape"""
        return self.f[k].view(self.dtype[k]).view(self.shape[k])

    def set_input(self, k, value):
        self.t(k).copy_(value)
        self.sent[k] = self.f[k].clone()

    def reset(self, names=None):
        for k in self.outs if names is None else names:
            if self.init[k] is None:
                self.f[k].fill_(NAN)
            else:
                self.t(k).copy_(self.init[k])

    def ws_fill(self, value):
        if self.ws is not None:
            self.ws.fill_(value)

    def untouched(self):
        return all(same_bits(self.f[k], self.sent[k]) for k in self.ins)

    def as_reset(self, names=None):
        """the outputs that no longer hold what reset() put there"""
        bad = []
        for k in self.outs if names is None else names:
            ok = bool(torch.isnan(self.f[k]).all()) if self.init[k] is None else same_bits(self.f[k], self.init[k].view(torch.float32).reshape(-1))
            if not ok:
                bad.append(k)
        return bad

    def get(self, k):
        return self.t(k).detach().cpu().clone()


def protocol(G, tag, call, mine=None, partly=(), poison_ws=True, sized=True):
    """the protocol of the module docstring around one entry: call(ws, ws_bytes) -> return code. `mine`: the outputs the entry owns (all of
    them by default), `partly`: those of them it need not fill. poison_ws = False: the workspace carries an earlier call's state (CTC backward)
    -> {name: CPU tensor} of the first call"""
    mine = list(G.outs) if mine is None else list(mine)
    others = [k for k in G.outs if k not in mine]

    def run(ws, n):
        rc = call(ws, n)
        G.sync()
        return rc

    kept = {k: G.f[k].clone() for k in others}
    G.reset(mine)
    if poison_ws:
        G.ws_fill(NAN)
    rc = run(G.ws, G.need)
    assert rc == 0, "%s returned %d: %s" % (tag, rc, G.L.last_error())
    assert G.intact(), "%s: a canary next to a buffer was overwritten" % tag
    assert G.untouched(), "%s: an input changed" % tag
    assert all(same_bits(G.f[k], kept[k]) for k in others), "%s wrote to a buffer it does not own" % tag
    first = {k: G.f[k].clone() for k in mine}
    for k in mine:
        if k not in partly and G.dtype[k] == torch.float32:
            n = int((~torch.isfinite(first[k])).sum())
            assert n == 0, "%s: %d elements of %s are not finite (never written, or written from workspace contents)" % (tag, n, k)
    out = {k: G.get(k) for k in mine}
    G.reset(mine)
    if poison_ws:
        G.ws_fill(0.0)
    assert run(G.ws, G.need) == 0, tag
    differ = [k for k in mine if not same_bits(G.f[k], first[k])]
    assert not differ, "%s: the second call (workspace zero-filled) gives other bits in %s" % (tag, differ)
    assert G.intact() and G.untouched(), "%s: canaries / inputs after the second call" % tag
    if G.need and sized:
        for what, ws, n in (("one byte of workspace too few", G.ws, G.need - 1), ("no workspace", None, G.need)):
            G.reset(mine)
            rc = run(ws, n)
            assert rc == HWG_ERR_WORKSPACE, "%s with %s returned %d" % (tag, what, rc)
            assert not G.as_reset(mine), "%s with %s wrote to %s" % (tag, what, G.as_reset(mine))
            assert G.intact() and G.untouched(), "%s with %s: canaries / inputs" % (tag, what)
    return out


def refused(G, tag, call, code=HWG_ERR_ARG):
    """a call the host code turns down before any launch: its code, nothing written"""
    G.reset()
    rc = call()
    G.sync()
    assert rc == code, "%s returned %d" % (tag, rc)
    assert not G.as_reset(), "%s wrote to %s" % (tag, G.as_reset())
    assert G.intact() and G.untouched(), tag


def bits_differ(pairs):
    return [name for name, a, b in pairs if not same_bits(a.reshape(-1), b.reshape(-1))]
