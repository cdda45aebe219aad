"""torch.autograd wrappers around the hwg C-ABI kernels.

All activations handled here are NHWC fp32 CUDA(HIP) tensors ([N,H,W,C], C fastest). Parameters keep the
PyTorch layouts of the reference's state-dict (Conv [O,I,R,S], ConvTranspose [I,O,R,S], Linear [O,I]) so
released checkpoints load; the kernels read/write those layouts directly through strides.

Nothing in this module computes on the CPU or through ATen math kernels: every op is a call into
libhwg_hip.so on torch's current stream. torch is used for memory, autograd bookkeeping and views.
"""
import collections
import ctypes
import math
import os

import torch

from . import _lib as L


class Function(torch.autograd.Function):
    """torch.autograd.Function with `.apply` bound straight to the C++ entry point. torch's Python-level `Function.apply` first walks the
    arguments for functorch wrappers and checks for a setup_context override - 10-25 us per call on the host, several times what the
    forward of a small op costs here, for ~140 ops per training step. None of these ops is used under functorch transforms."""

    # how `backward` treats S gradient sets stacked along the batch axis (Tape.backward_sets): "loop" = called once per set on that set's
    # slice (ops whose backward reads saved per-sample state), "stacked" = called once on the stacked gradient (stateless in the batch),
    # "native" = the class implements backward_sets(ctx, S, targets, *stacked_grads) itself
    sets = "loop"

    @classmethod
    def apply(cls, *args):
        if TAPE is not None:
            return TAPE.record(cls, args)
        return super(torch.autograd.Function, cls).apply(*args)


# ---- explicit tape (a sub-network run outside autograd so that SEVERAL upstream gradients can go through it in one pass) ----------------
# The balanced GAN lessons send two or three different gradients through the generator, one backward pass each, on layers that fill a
# quarter of the chip at 8 lines. With the generator's forward recorded on a Tape its backward can take the S gradients stacked along the
# batch axis: data-gradient convolutions, blurs and resamplings run ONCE on S x N samples; ops that read saved per-sample state (AdaIN,
# weight gradients, the style MLP) run per set on slices, each set accumulating its parameter gradients into its own buffer (grad_set).
TAPE = None


class _TapeCtx:
    """the part of torch.autograd's ctx the Functions of this module use"""

    def __init__(self, needs):
        self.needs_input_grad = needs
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *a):
        pass

    def set_materialize_grads(self, v):
        pass


class SetGrad:
    """gradient of one taped tensor for S sets: `stacked` [S*N, ...] (sets along the batch axis) and / or `parts` (one tensor per set)"""

    __slots__ = ("stacked", "parts", "S")

    def __init__(self, S, stacked=None, parts=None):
        self.S, self.stacked, self.parts = S, stacked, parts

    def get_parts(self):
        if self.parts is None:
            n = self.stacked.shape[0] // self.S
            self.parts = [self.stacked[i * n:(i + 1) * n] for i in range(self.S)]
        return self.parts

    def get_stacked(self):
        if self.stacked is None:
            self.stacked = self.parts[0] if self.S == 1 else torch.cat([p.contiguous() for p in self.parts], dim=0)
        return self.stacked

    def add(self, other):
        a, b = self.get_parts(), other.get_parts()
        out = []
        for x, y in zip(a, b):
            z = torch.empty_like(x)
            L.call("hwg_axpby", x.contiguous(), 1.0, y.contiguous(), 1.0, z, x.numel(), _stream())
            out.append(z)
        return SetGrad(self.S, parts=out)


class Tape:
    def __init__(self):
        self.nodes = []          # (Function class | "alias", ctx, inputs (the original argument tuple), outputs tuple)
        self.live = {}           # id(tensor) -> tensor, for every tensor a gradient can arrive at (keeps the ids valid)
        self.by_mem = {}         # (address, elements) of the contiguous live tensors -> tensor (how reshapes of them are recognised)

    def watch(self, t):
        self._live(t)
        return t

    def _adopt_views(self, args):
        """torch-level reshapes of taped tensors (`y.view(rows, O)`, `.reshape(B, -1)`, also of results that are themselves views): autograd
        would track them; here a contiguous tensor that covers exactly the memory of a contiguous live tensor becomes an alias node. Any
        other view of a live tensor is an error."""
        for a in args:
            if not isinstance(a, torch.Tensor) or id(a) in self.live or a._base is None:
                continue
            base = self.by_mem.get((a.data_ptr(), a.numel())) if a.is_contiguous() else None
            if base is not None:
                self.live[id(a)] = a
                self.nodes.append(("alias", tuple(base.shape), (base,), (a,)))
            elif (a._base.data_ptr(), a._base.numel()) in self.by_mem:
                raise L.HwgError("taped forward: unsupported view of a taped tensor (shape %s of base %s)" % (tuple(a.shape), tuple(a._base.shape)))

    def _live(self, t):
        self.live[id(t)] = t
        if t.is_contiguous():
            self.by_mem.setdefault((t.data_ptr(), t.numel()), t)

    def record(self, cls, args):
        global TAPE
        self._adopt_views(args)
        needs = tuple(isinstance(a, torch.Tensor) and (id(a) in self.live or (a.requires_grad and a.is_leaf)) for a in args)
        ctx = _TapeCtx(needs)
        TAPE = None             # ops called from inside a forward are part of it, not nodes of their own
        try:
            out = cls.forward(ctx, *args)
        finally:
            TAPE = self
        if any(needs):
            outs = out if isinstance(out, tuple) else (out,)
            for o in outs:
                if isinstance(o, torch.Tensor):
                    self._live(o)
            self.nodes.append((cls, ctx, args, outs))
        return out

    def alias(self, new, old):
        """`new` is a reshape of the taped tensor `old` (same elements, same order)"""
        if id(old) in self.live:
            self._live(new)
            self.nodes.append(("alias", tuple(old.shape), (old,), (new,)))
        return new

    def backward_sets(self, out, grads, targets):
        """send S gradients of `out` (list of [N, ...] tensors) through the recorded ops in one pass. targets[s]: where set s accumulates its
        parameter gradients - None = the parameters' own .grad, else (flat buffer, touched mask) as produced by FlatParams.stash().
        -> {id(watched input): list of S gradient tensors}"""
        global GRAD_SET
        S = len(grads)
        g = {id(out): SetGrad(S, parts=[x.contiguous() for x in grads])}
        prev = GRAD_SET
        try:
            for cls, ctx, args, outs in reversed(self.nodes):
                gouts = [g.pop(id(o), None) if isinstance(o, torch.Tensor) else None for o in outs]
                if all(x is None for x in gouts):
                    continue
                if cls == "alias":      # ctx = the base tensor's shape; per set: the same elements in the base's shape
                    gin = [SetGrad(S, parts=[p_.contiguous().reshape(ctx) for p_ in gouts[0].get_parts()])]
                else:
                    for i, x in enumerate(gouts):      # a multi-output op with a missing output gradient: zeros, as autograd materialises them
                        if x is None and isinstance(outs[i], torch.Tensor):
                            z = torch.zeros((S * outs[i].shape[0],) + tuple(outs[i].shape[1:]), dtype=outs[i].dtype, device=outs[i].device)
                            gouts[i] = SetGrad(S, stacked=z)
                    gin = self._node_backward(cls, ctx, gouts, S, targets)
                for a, need, gi in zip(args, ctx.needs_input_grad if cls != "alias" else (True,), gin):
                    if gi is None or not need:
                        continue
                    if a.requires_grad and a.is_leaf and id(a) not in self.live:
                        # a parameter whose gradient came back as a tensor (not accumulated in place by the kernel): add it to its set's buffer
                        for s_, part in enumerate(gi.get_parts()):
                            GRAD_SET = targets[s_]
                            buf = _grad_buffer(a)
                            L.call("hwg_axpby", part.contiguous(), 1.0, buf, 1.0, buf, buf.numel(), _stream())
                        continue
                    k = id(a)
                    g[k] = gi if k not in g else g[k].add(gi)
        finally:
            GRAD_SET = prev
        return {k: v.get_parts() for k, v in g.items()}

    @staticmethod
    def _node_backward(cls, ctx, gouts, S, targets):
        global GRAD_SET
        mode = cls.sets if S > 1 else "loop"
        if mode == "native":
            res = cls.backward_sets(ctx, S, targets, *[x.get_stacked() for x in gouts])
            return [None if r is None else (r if isinstance(r, SetGrad) else SetGrad(S, stacked=r)) for r in res]
        if mode == "stacked":
            GRAD_SET = targets[0]
            res = cls.backward(ctx, *[x.get_stacked() for x in gouts])
            res = res if isinstance(res, tuple) else (res,)
            return [None if r is None else SetGrad(S, stacked=r) for r in res]
        per_set = []
        for s_ in range(S):
            GRAD_SET = targets[s_]
            res = cls.backward(ctx, *[x.get_parts()[s_] for x in gouts])
            per_set.append(res if isinstance(res, tuple) else (res,))
        out = []
        for i in range(len(per_set[0])):
            col = [r[i] for r in per_set]
            out.append(None if col[0] is None else SetGrad(S, parts=col))
        return out


# ---- debug guard for taped forwards (HWG_TAPE_CHECK=1) ---------------------------------------------------------------------------------
# A taped forward runs under no_grad and tracks only Function calls plus contiguous whole-memory reshapes of their results. Any OTHER
# torch-level op on a taped tensor (arithmetic, torch.cat, indexing, a norm in eval mode ...) would produce a tensor the tape does not
# know, and the gradient path through it would be dropped without an error. With the check on, every torch-level call made while a tape is
# recording is inspected: an argument that is (a view of) a taped tensor is only allowed in the shape / view / bookkeeping calls below.
TAPE_CHECK = bool(int(os.environ.get("HWG_TAPE_CHECK", "0") or 0))
_TAPE_SAFE = {"view", "reshape", "contiguous", "flatten", "size", "dim", "numel", "data_ptr", "is_contiguous", "stride", "detach", "requires_grad_",
              "__get__", "__len__", "__repr__", "storage_offset", "element_size", "untyped_storage", "is_floating_point", "get_device", "_is_view",
              "__set__", "__bool__", "is_leaf", "__format__", "__str__", "type", "nelement", "ndimension", "__hash__", "__reduce_ex__"}


class _TapeGuard(torch.overrides.TorchFunctionMode):
    def __torch_function__(self, func, types, args=(), kwargs=None):
        tape = TAPE
        if tape is not None:                       # (None inside an op's own forward: ops allocate and launch freely there)
            name = getattr(func, "__name__", str(func))
            if name not in _TAPE_SAFE:
                stack = list(args) + list((kwargs or {}).values())
                while stack:
                    a = stack.pop()
                    if isinstance(a, (list, tuple)):
                        stack.extend(a)
                    elif isinstance(a, torch.Tensor) and (id(a) in tape.live or (a._base is not None and id(a._base) in tape.live)):
                        raise L.HwgError("taped forward: torch-level op %r on a taped tensor (shape %s) - its result would be unknown to the tape and the "
                                         "gradient through it silently dropped; route it through an ops.Function" % (name, tuple(a.shape)))
        return func(*args, **(kwargs or {}))


class taping:
    """`with ops.taping(tape):` - Function.apply records on `tape` instead of autograd's graph (no_grad is the caller's business)"""

    def __init__(self, tape):
        self.tape, self.guard = tape, (_TapeGuard() if TAPE_CHECK else None)

    def __enter__(self):
        global TAPE
        TAPE = self.tape
        if self.guard is not None:
            self.guard.__enter__()
        return self.tape

    def __exit__(self, *exc):
        global TAPE
        if self.guard is not None:
            self.guard.__exit__(*exc)
        TAPE = None
        return False


ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
NORM_IN, NORM_GN, NORM_BN = 0, 1, 2


_raw_stream = torch._C._cuda_getCurrentRawStream if hasattr(torch._C, "_cuda_getCurrentRawStream") else None
_get_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    # raw hipStream_t of torch's current stream (the Python Stream object is ~20 us to build, torch.cuda.current_device() re-checks the lazy
    # initialisation on every call: ~1 us; the two C entry points together ~0.3 us - this runs ~430 times per training step)
    if _raw_stream is None or _get_device is None:       # a torch build without the private entry points: the public (slower) API
        return torch.cuda.current_stream().cuda_stream
    return _raw_stream(_get_device())


_copy_streams = {}


class AsyncFetch:
    """Device->host copy on a side stream: the producer's stream keeps running (and the host keeps enqueueing) while the bytes
    travel; `.get()` waits only for the copy. Replaces `.cpu()` / `.item()` where the value is needed later than it is produced."""

    def __init__(self, tensor):
        dev = tensor.device
        cs = _copy_streams.get(dev)
        if cs is None:
            cs = _copy_streams[dev] = torch.cuda.Stream(device=dev)
        self.src = tensor.detach()
        self.host = torch.empty(tensor.shape, dtype=tensor.dtype, pin_memory=True)
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(cs):
            cs.wait_event(ready)
            self.host.copy_(self.src, non_blocking=True)
            self.done = torch.cuda.Event()
            self.done.record()
        self.src.record_stream(cs)

    def get(self):
        self.done.synchronize()
        return self.host


def h2d(host, device, dtype=None):
    """Asynchronous host->device upload through pinned staging memory. A plain `.to(device)` of pageable memory blocks the host
    until every kernel queued before it has finished, which serialises the CPU against the GPU a dozen times per step."""
    t = torch.as_tensor(host)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.is_cuda:
        return t.to(device)
    pinned = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    pinned.copy_(t)
    return pinned.to(device, non_blocking=True)


_ws_cache = {}


def workspace(nbytes, device):
    """Shared scratch buffer (stream ordered, contents are dead once the call that used it returns)."""
    nbytes = int(nbytes)
    # one buffer per (device, stream): passes that run concurrently on different streams (the per-set style passes of the GAN trainer) must
    # not share scratch memory; torch's allocator ties the buffer to the stream that is current when it is created
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# ---- side stream for weight gradients -----------------------------------------------------------------------------------
# Nothing in the backward pass waits for a conv's weight gradient, only the optimizer side does. With SIDE_WGRAD on (the trainers
# switch it on and call join_side_stream() after every backward()), the MFMA weight-gradient kernels are enqueued on a second HIP
# stream: their workgroups fill the CUs that the data-gradient chain leaves idle (kernel tails, small elementwise launches).
# Per tensor the accumulation order is unchanged (all weight gradients run in order on the one side stream).
SIDE_WGRAD = False
_side_streams = {}
_side_dirty = set()


def _side_stream(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    hit = _side_streams.get(key)
    if hit is None:
        st = torch.cuda.Stream(device=device)
        hit = _side_streams[key] = (st, st.cuda_stream, key)
    return hit


def _side_workspace(nbytes, device, stream):
    key = ("side", device.index if device.index is not None else torch.cuda.current_device())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        buf.record_stream(stream)
        _ws_cache[key] = buf
    return buf


_side_hold = []      # operands of side-stream launches: kept alive until the join so that the allocator cannot hand their memory to a main-stream kernel


def join_side_stream():
    """make torch's current stream wait for every weight gradient enqueued on the side stream so far, then sum the weight-gradient partial
    images whose reduction was deferred (flush_deferred_reduce): after this call every parameter gradient is complete on the current stream"""
    for key in list(_side_dirty):
        L.call("hwg_stream_join", _side_streams[key][1], _stream())
    _side_dirty.clear()
    del _side_hold[:]
    if _defer["count"] or _sn_defer:
        flush_deferred_reduce()


# ---- deferred sum of the weight-gradient partial images -------------------------------------------------------------------
# A weight gradient leaves one partial image per pixel range in its workspace and sums them with a launch of its own: 65 launches of
# 5..25 us per training step, too small to stream at memory rate. With DEFER_REDUCE on (the trainers switch it on around their backward
# passes and call join_side_stream() after every backward()), a weight gradient's workspace comes out of a private arena instead of the
# shared scratch buffer, its sum is only queued (hwg_wgrad_defer_next), and flush_deferred_reduce() sums everything queued with one
# table-driven launch per 32 gradients. Bit-identical to the undeferred order (same schedule per gradient, several gradients of one tensor in
# queue order). Gradients are undefined between the backward call and the flush.
DEFER_REDUCE = False
_defer = {"count": 0, "offset": 0, "arena": {}, "launches": 0, "flushes": 0, "fallbacks": 0, "sn_launches": 0}
_sn_defer = []       # queued spectral-norm backward passes: (dW_sn, W_bar, u, v, sigma, destination, R, K), tensors held until the flush
_SN_BWD_REC = [("dWsn", "<u8"), ("Wbar", "<u8"), ("u", "<u8"), ("v", "<u8"), ("sigma", "<u8"), ("dst", "<u8"), ("R", "<i4"), ("K", "<i4"), ("acc", "<i4"), ("pad", "<i4")]
DEFER_ARENA_BYTES = int(os.environ.get("HWG_DEFER_ARENA_MB", "1536")) << 20


def _defer_workspace(nbytes, device):
    """`nbytes` of the arena that stays untouched until the next flush, or None when the arena is full (the caller then sums at once)"""
    key = device.index if device.index is not None else torch.cuda.current_device()
    arena = _defer["arena"].get(key)
    if arena is None:
        arena = _defer["arena"][key] = torch.empty(DEFER_ARENA_BYTES, dtype=torch.uint8, device=device)
        for st in _side_streams.values():
            arena.record_stream(st[0])
    off = _defer["offset"]
    need = (int(nbytes) + 255) & ~255
    if off + need > arena.numel():
        _defer["fallbacks"] += 1
        return None
    _defer["offset"] = off + need
    _defer["count"] += 1
    return arena[off: off + need]


DEFER_KEEP_ARENA = False     # passes on several streams in flight: a flush must not hand the arena's start to the next pass (reset after the join)


_FLUSH_LAUNCHES = None     # the flush's `int* launches` out-parameter: a module-lifetime host array (never a temporary: a call list that
                            # recorded the address of a temporary would write through a dangling pointer on every replay)


def flush_deferred_reduce():
    """sum every queued set of partial images on the current stream (call after the side stream has been joined)"""
    global _FLUSH_LAUNCHES
    import numpy as np
    if _FLUSH_LAUNCHES is None:
        _FLUSH_LAUNCHES = np.zeros(1, dtype=np.int32)
    n = _FLUSH_LAUNCHES
    n[0] = 0
    L.call("hwg_wgrad_defer_flush", _stream(), n.ctypes.data)
    _defer["launches"] += int(n[0]); _defer["flushes"] += 1
    _defer["count"] = 0
    if not DEFER_KEEP_ARENA:
        _defer["offset"] = 0
    if _sn_defer:          # queued spectral-norm backward passes (their dW_sn inputs are complete: summed eagerly, or by the launch above)
        # a launch adds every entry's result to its destination with a plain read-modify-write: two entries with the SAME destination (the
        # discriminator applied twice in one backward pass - a lesson with both 'disc' and 'gen') must not share a launch. The k-th
        # occurrence of a destination goes to pass k, passes run one after the other in queue order (as hwg_wgrad_defer_flush does for convs).
        passes, seen = [], {}
        for e in _sn_defer:
            k = seen.get(e[5].data_ptr(), 0)
            seen[e[5].data_ptr()] = k + 1
            if k == len(passes):
                passes.append([])
            passes[k].append(e)
        chunks = [pas[i: i + 16] for pas in passes for i in range(0, len(pas), 16)]
        for chunk in chunks:
            rec = np.zeros(len(chunk), dtype=_SN_BWD_REC)
            for k, (dwsn, w_bar, u, v, sigma, dst, R, K) in enumerate(chunk):
                rec[k] = (dwsn.data_ptr(), w_bar.data_ptr(), u.data_ptr(), v.data_ptr(), sigma.data_ptr(), dst.data_ptr(), R, K, 1, 0)
            ws = workspace(L.query("hwg_spectral_bwd_multi_workspace", len(chunk)), chunk[0][0].device)
            L.call("hwg_spectral_bwd_multi", rec.ctypes.data, len(chunk), ws, ws.numel(), _stream())
            _defer["sn_launches"] += 1
        del _sn_defer[:]


def reset_defer_arena():
    _defer["offset"] = 0


def _chk(t, name, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise L.HwgError("%s must live on the GPU (no CPU fallback exists)" % name)
    if t.dtype != dtype:
        raise L.HwgError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise L.HwgError("%s must be contiguous" % name)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


# Parameter gradients are accumulated by the kernels straight into `param.grad` (the trainer keeps those as views of one flat
# buffer) instead of being returned to autograd, which would allocate a temporary and launch an extra add kernel per tensor.
DIRECT_PARAM_GRADS = True


def _direct(p):
    return DIRECT_PARAM_GRADS and p is not None and p.is_leaf and p.requires_grad


# Gradient-set redirect: None = parameter gradients accumulate into param.grad (views of the trainer's flat buffer). Otherwise
# (buffer, touched mask) of a stashed gradient set (FlatParams.stash()): kernels accumulate into the SAME offsets of that buffer and the
# set's mask is marked - how the batched generator backward (Tape.backward_sets) and the per-set style-extractor passes put every set's
# gradients where the reference's sequential backward + clone-and-zero would have put them.
GRAD_SET = None
_set_views = {}


class grad_set:
    def __init__(self, target):
        self.target = target

    def __enter__(self):
        global GRAD_SET
        self.prev = GRAD_SET
        GRAD_SET = self.target

    def __exit__(self, *exc):
        global GRAD_SET
        GRAD_SET = self.prev


def _grad_buffer(p):
    """the buffer parameter gradients accumulate into (zero-initialised on first use)"""
    gs = GRAD_SET
    if gs is not None:
        info = getattr(p, "_hwg_flat", None)
        if info is None:
            raise L.HwgError("gradient-set redirect needs parameters that live in a FlatParams buffer")
        flat, k = info
        buf, mask = gs
        mask[k] = True
        key = (buf.data_ptr(), id(flat), k)
        v = _set_views.get(key)
        if v is None:
            off = int(flat.offsets[k])
            v = _set_views[key] = buf[off: off + int(flat.numel[k])].view_as(p)
        return v
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    touch = getattr(p, "_hwg_touch", None)
    if touch is not None:
        touch()
    return p.grad


# ----------------------------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------------------------
def _desc(N, H, W, C, K, R, S, stride, pad, dil, P, Q, transposed=0):
    d = L.ConvDesc()
    d.N, d.H, d.W, d.C, d.K, d.R, d.S = N, H, W, C, K, R, S
    d.stride_h, d.stride_w = stride
    d.pad_h, d.pad_w = pad
    d.dil_h, d.dil_w = dil
    d.P, d.Q = P, Q
    d.transposed = transposed
    return d


# Packed ([tap][K][C]) images of leaf parameters are cached until the parameter changes: `_version` catches torch-side writes
# (load_state_dict, copy_), WEIGHT_EPOCH[...] is bumped by the multi-tensor Adam kernel, which writes through raw pointers.
# After an optimizer step `repack_group` refreshes every cached image of that optimizer's parameters in ONE launch
# (hwg_conv_pack_weight_multi) instead of ~100 single-weight launches spread over the next step.
WEIGHT_EPOCH = {}
_pack_cache = {}          # key -> [version, epoch, packed tensor, weight, (A, B, Bpad, R, S, sa, sb, flip)]
_pack_tables = {}         # group -> (number of cache entries it was built for, device table, total blocks, entries)
PACK_PER_BLOCK = 1024
_PACK_DTYPE = None


def bump_weight_epoch(group):
    WEIGHT_EPOCH[group] = WEIGHT_EPOCH.get(group, 0) + 1


def _pack(weight, A, B, R, S, sa, sb, flip, Bpad=None, wino=False):
    """engine image of a weight: [tap][A][Bpad], or (wino) the Winograd-domain filters U = G g G^T as [Bpad/16][16][Apad][16]"""
    Bpad = B if Bpad is None else Bpad
    Apad = (A + 15) // 16 * 16 if wino else A
    if wino == 2:
        # F(3x3,2x2) image of a 4x4 stride-2 convolution's weight (hwg_wino_s2_pack_weight): A = the convolution's output channels, B = its input
        # channels, sa / sb their strides, flip = 1: the image of the data-gradient product ((a,b,c) block channels x K)
        Apad, Bpad = ((4 * B + 15) // 16 * 16, (A + 15) // 16 * 16) if flip else ((A + 15) // 16 * 16, (4 * B + 15) // 16 * 16)
    elif wino:
        Bpad = (B + 15) // 16 * 16
    pre = getattr(weight, "_hwg_prepack", None)
    if pre is not None:
        # a spectral-norm layer's W_bar / sigma: its images were written by the network's one scaled multi-pack launch (SpectralBank.update);
        # an image nobody asked for before is packed here, from the tensor itself, and joins the launch from the next forward pass on
        variant = (A, B, Bpad, R, S, sa, sb, int(flip), int(wino), Apad)
        img = pre.images.get(variant)
        if img is not None:
            return img
        pre.miss(variant, weight)
    key = hit = group = None
    # cached per PARAMETER only: under no_grad (taped forwards, the discriminator lessons' detached generator pass) every derived weight - the
    # fused-upsample 4x4 image, an equal-lr scaled copy - is a "leaf" too, and caching those kept one entry (the temporary and its packed image)
    # alive per forward pass for the rest of the run
    if isinstance(weight, torch.nn.Parameter):
        group = getattr(weight, "_hwg_group", None)
        epoch = WEIGHT_EPOCH.get(group, 0)
        key = (id(weight), weight.data_ptr(), A, B, Bpad, sa, sb, int(flip), int(wino))
        hit = _pack_cache.get(key)
        if hit is not None and hit[0] == weight._version and hit[1] == epoch:
            return hit[2]
    if key is not None and hit is not None:
        out = hit[2]
    elif wino:
        out = torch.empty((Bpad // 16, 16, Apad, 16), dtype=torch.float32, device=weight.device)
    else:
        out = torch.empty((R * S, A, Bpad), dtype=torch.float32, device=weight.device)
    if wino == 2:
        L.call("hwg_wino_s2_pack_weight", weight, out, A, B, sa, sb, int(flip), _stream())
    elif wino:
        L.call("hwg_wino_pack_weight", weight, out, A, B, sa, sb, S, 1, int(flip), _stream())
    else:
        L.call("hwg_conv_pack_weight", weight, out, A, B, Bpad, R, S, sa, sb, S, 1, int(flip), _stream())
    if key is not None:
        _pack_cache[key] = [weight._version, epoch, out, weight, (A, B, Bpad, R, S, sa, sb, int(flip), int(wino), Apad), group]
    return out


def repack_group(group):
    """refresh all cached packed images of the parameters of `group` (call right after bump_weight_epoch(group))"""
    global _PACK_DTYPE
    import numpy as np
    entries = [e for e in _pack_cache.values() if e[5] == group]
    if not entries:
        return
    tab = _pack_tables.get(group)
    if tab is None or tab[0] != len(entries):
        if _PACK_DTYPE is None:
            _PACK_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("A", "<i4"), ("B", "<i4"), ("Bpad", "<i4"), ("R", "<i4"), ("S", "<i4"), ("flip", "<i4"),
                                    ("sa", "<i8"), ("sb", "<i8"), ("sr", "<i8"), ("ss", "<i8"), ("total", "<i8"), ("first_block", "<i8"),
                                    ("mode", "<i4"), ("Apad", "<i4")])
        host = np.zeros(len(entries), dtype=_PACK_DTYPE)
        blocks = 0
        for i, e in enumerate(entries):
            A, B, Bpad, R, S, sa, sb, flip, mode, Apad = e[4]
            total = Apad * Bpad if mode else R * S * A * Bpad
            host[i] = (e[3].data_ptr(), e[2].data_ptr(), A, B, Bpad, R, S, flip, sa, sb, S, 1, total, blocks, mode, Apad)
            blocks += (total + PACK_PER_BLOCK - 1) // PACK_PER_BLOCK
        dev = h2d(torch.from_numpy(host.view(np.uint8)), entries[0][2].device)
        tab = _pack_tables[group] = (len(entries), dev, blocks, entries)
    L.call("hwg_conv_pack_weight_multi", tab[1], tab[0], tab[2], _stream())
    epoch = WEIGHT_EPOCH.get(group, 0)
    for e in tab[3]:
        if e[0] == e[3]._version:    # torch-side writes still force a private re-pack on next use
            e[1] = epoch


def _pad_channels(x, Cpad):
    N, H, W, C = x.shape
    out = torch.empty((N, H, W, Cpad), dtype=x.dtype, device=x.device)
    L.call("hwg_pad_channels", x, C, out, Cpad, N * H * W, _stream())      # copy + zero lanes in one launch (and visible to replay.py's call log)
    return out


# Per-launch timing of the MFMA conv kernels (bench.py's roofline measurement) is done inside the library (hwg_prof_*: HIP events
# recorded right around the launches). Here we only label the launches with their layer shape when a profile is running.
PROF_SHAPES = None     # None, or {shape tuple: tag}
SCOPE = None           # which network is running its forward ("G", "D", ...): convs remember it so that a profile can be split by network


class scope:
    """`with ops.scope("G"):` around a network's forward; nested scopes keep the outermost label"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global SCOPE
        self.prev = SCOPE
        if SCOPE is None:
            SCOPE = self.name

    def __exit__(self, *exc):
        global SCOPE
        SCOPE = self.prev


def prof_start(max_records=200000):
    global PROF_SHAPES
    PROF_SHAPES = {}
    L.call("hwg_prof_start", max_records)


def prof_enable(on):
    """pause / resume an open profile"""
    L.call("hwg_prof_enable", int(bool(on)))


def prof_stop():
    """-> list of (kind, shape, work, seconds); kind in conv_mfma_kernel / wgrad_mfma_kernel / conv_split_reduce / wgrad_reduce / direct kernels /
    wino_conv_kernel (the three Winograd forward / data-gradient kernels; work = direct-form FLOPs of the layer) / wino_wgrad_kernel"""
    global PROF_SHAPES
    import numpy as np
    cap = 200000
    kinds = np.zeros(cap, dtype=np.int32); tags = np.zeros(cap, dtype=np.int32)
    work = np.zeros(cap, dtype=np.float64); ms = np.zeros(cap, dtype=np.float32)
    n = L.query("hwg_prof_stop", kinds.ctypes.data, tags.ctypes.data, work.ctypes.data, ms.ctypes.data, cap)
    by_tag = {v: k for k, v in (PROF_SHAPES or {}).items()}
    PROF_SHAPES = None
    names = ("conv_mfma_kernel", "wgrad_mfma_kernel", "conv_split_reduce_kernel", "wgrad_reduce_kernel", "conv_direct_kernels", "wgrad_direct_kernels",
             "wino_conv_kernel", "wino_wgrad_kernel")
    return [(names[kinds[i]], by_tag.get(int(tags[i])), float(work[i]), float(ms[i]) * 1e-3) for i in range(n)]


def _prof_tag(shape):
    tag = PROF_SHAPES.get(shape)
    if tag is None:
        tag = PROF_SHAPES[shape] = len(PROF_SHAPES)
    L.call("hwg_prof_tag", tag)


_RUN_SCOPE = [None]     # scope of the conv op currently being executed (forward: SCOPE, backward: the scope saved at forward time)


_conv_plans = {}    # geometry -> (descriptor, workspace bytes, descriptor address): built (and the library's schedule queried) once per geometry
_CONV_ENTRY = ("hwg_conv_fwd", "hwg_wino_conv_fwd", "hwg_wino_s2_conv")      # entry families: direct, Winograd F(2x2,3x3), two-tap Winograd F(3x3,2x2)
_CONV_WORKSPACE = ("hwg_conv_fwd_workspace", "hwg_wino_conv_workspace", "hwg_wino_s2_workspace")


def static_host_ptrs():
    """addresses of the host-side descriptors that live as long as the plan caches (what a recorded call list may hold as literal host
    pointers - replay.py rejects every other host address: a temporary's address would dangle on replay); lowerings hold _conv_plans entries"""
    out = {int(p[2]) for p in _conv_plans.values()}
    out.update(int(p.d.ptr) for p in _wgrad_plans.values())
    return out


# One library product a layer's forward or data gradient is lowered to (integers and a descriptor only, never a tensor): entry family (index
# into _CONV_ENTRY), its _conv_plans entry, the channel count the contraction side is zero-padded to (or None), _pack's arguments (A, B, R, S,
# sa, sb, flip, Bpad, wino), the result's shape and, or None, the launch that follows as (entry, result shape, integers): hwg_col2im_taps
# folding a tap matrix back into the image, hwg_pad2d_fwd restoring rows the filter never met
_Product = collections.namedtuple("_Product", "wino plan cpad pack oshape post")


def _product(pack, cpad, N, H, W, C, K, R, S, stride, pad, dil, P, Q, transposed, post=None):
    wino = pack[8]
    key = (N, H, W, C, K, R, S, stride, pad, dil, P, Q, transposed, wino)
    plan = _conv_plans.get(key)
    if plan is None:
        d = _desc(N, H, W, C, K, R, S, stride, pad, dil, P, Q, transposed)
        plan = _conv_plans[key] = (d, L.query(_CONV_WORKSPACE[wino], d.ptr), d.ptr)
    return _Product(wino, plan, cpad, pack, (N, P, Q, K), post)


def _run_conv(prod, x, weight, bias):
    """execute a lowered product: pad, pack, launch, post step"""
    if prod.cpad is not None:
        x = _pad_channels(x, prod.cpad)
    wp = _pack(weight, *prod.pack)
    y = torch.empty(prod.oshape, dtype=torch.float32, device=x.device)
    d, need, dptr = prod.plan
    if PROF_SHAPES is not None:
        _prof_tag((d.N, d.H, d.W, d.C, d.K, d.R, d.S, (d.stride_h, d.stride_w), (d.pad_h, d.pad_w), (d.dil_h, d.dil_w), d.transposed, _RUN_SCOPE[0]))
    ws = workspace(need, x.device) if need else None
    L.call(_CONV_ENTRY[prod.wino], dptr, x, wp, bias, y, 0, ws, need, _stream())
    if prod.post is not None:
        entry, oshape, ints = prod.post
        t, y = y, torch.empty(oshape, dtype=torch.float32, device=x.device)
        L.call(entry, t, y, *ints, _stream())
    return y


# 3x3 / stride 1 / dilation 1 products with >= 16 output channels run as F(2x2,3x3) (csrc/conv_wino.hip); HWG_WINO=0 keeps them on the
# direct implicit-GEMM kernels (A/B timing and numerics comparisons)
WINOGRAD = bool(int(os.environ.get("HWG_WINO", "1") or 1))


_wino_choice = {}


TUNE_EPOCH = 0      # bumped by tuning_reload(): anything derived from the library's plans (recorded launch lists, replay.py) is keyed by it


def tuning_reload():
    """The library plans every geometry once and reads its tuning knobs (HWG_WINO, HWG_WINO_FORCE, HWG_CONV_FORCE, ...) at plan time; the
    per-geometry choices are cached here as well. Call this after changing such a variable in a running process."""
    global WINOGRAD, TUNE_EPOCH
    TUNE_EPOCH += 1
    WINOGRAD = bool(int(os.environ.get("HWG_WINO", "1") or 1))
    _wino_choice.clear(); _wino_wgrad_choice.clear(); _conv_plans.clear(); _wgrad_plans.clear(); _fwd_lowerings.clear(); _dgrad_lowerings.clear()
    L.call("hwg_tuning_reload")


class tuning:
    """`with ops.tuning(HWG_WINO="2", HWG_WINO_FORCE="6"):` - set tuning variables for a block (tests, sweeps) and restore them after"""

    def __init__(self, **env):
        self.env = {k: (None if v is None else str(v)) for k, v in env.items()}

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        tuning_reload()
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        tuning_reload()


def last_plan():
    """(engine, schedule id, split factor) of this thread's last convolution-family launch (engine: the profiler's kind codes - 0 direct
    MFMA conv, 1 MFMA weight gradient, 6 Winograd conv, 7 Winograd weight gradient)"""
    import numpy as np
    out = np.full(3, -1, dtype=np.int32)
    L.call("hwg_last_plan", out.ctypes.data)
    return tuple(int(v) for v in out)


def _wino_ok(N, H, W, C, K, R, S, stride, pad, dil, P, Q):
    """the library's cost models decide per product (cached per geometry): many tiles x few channels run as Winograd, few tiles x many
    channels (the 512-channel recogniser layers) stay on the direct kernels"""
    if not (WINOGRAD and R == 3 and S == 3 and stride == (1, 1) and dil == (1, 1) and C % 16 == 0 and K >= 16 and pad[0] >= 0 and pad[1] >= 0):
        return False
    key = (N, H, W, C, K, pad)
    hit = _wino_choice.get(key)
    if hit is None:
        d = _desc(N, H, W, C, K, 3, 3, (1, 1), pad, (1, 1), P, Q, 0)
        hit = _wino_choice[key] = bool(L.query("hwg_wino_preferred", d.ptr))
    return hit


def _wino_s2_ok(N, H, W, C, K, R, S, stride, pad, dil, P, Q, transposed):
    """4x4 stride-2 pad-0 layers (transposed = 1: their data gradient, described as the fractionally strided product) in the Winograd domain
    F(3x3,2x2) on the space-to-depth image (csrc/conv_wino.hip, hwg_wino_s2_*) - the library's cost models decide per geometry"""
    if not (WINOGRAD and R == 4 and S == 4 and stride == (2, 2) and pad == (0, 0) and dil == (1, 1) and C % 16 == 0):
        return False
    key = (N, H, W, C, K, "s2", transposed, P, Q)     # (P, Q: the data gradient of an odd-width input is not the F(3x3,2x2) geometry)
    hit = _wino_choice.get(key)
    if hit is None:
        d = _desc(N, H, W, C, K, 4, 4, (2, 2), (0, 0), (1, 1), P, Q, transposed)
        hit = _wino_choice[key] = bool(L.query("hwg_wino_s2_preferred", d.ptr))
    return hit


_wino_wgrad_choice = {}


def _wino_wgrad_ok(d):
    """weight gradient of a 3x3 stride-1 layer in the Winograd domain (conv_wino_wgrad.hip) - the library decides per geometry"""
    if not WINOGRAD or not ((d.R == 3 and d.S == 3) or (d.R == 4 and d.S == 4 and d.stride_h == 2 and d.stride_w == 2 and not d.transposed)):
        return False      # (4x4 stride 2 pad 0: the two-tap problem on the space-to-depth image, F(2x2 taps, 3x3 gradient tiles))
    key = (d.N, d.H, d.W, d.C, d.K, d.R, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w, d.P, d.Q)
    hit = _wino_wgrad_choice.get(key)
    if hit is None:
        hit = _wino_wgrad_choice[key] = bool(L.query("hwg_wino_wgrad_preferred", d.ptr))
    return hit


def _cpad(C, K, fractional=False):
    """channel count the contraction side must be zero-padded to: multiples of 16 for the MFMA path (always taken by the fractionally
    strided mode: conv-transpose with stride > 1, data gradient of a strided conv), multiples of 4 for the K <= 2 direct kernel,
    nothing for the single-channel direct kernel"""
    if fractional:
        return (C + 15) // 16 * 16
    if C == 1:
        return C
    if K <= 2:
        return (C + 3) // 4 * 4
    return (C + 15) // 16 * 16


def _taps(weight):
    d = weight.dim()
    if d == 4:
        return weight.shape[2], weight.shape[3]
    if d == 3:
        return 1, weight.shape[2]
    if d == 2:
        return 1, 1
    raise L.HwgError("conv weight must have 2, 3 or 4 dimensions")


_fwd_lowerings = {}      # (N, H, W, C, K, R, S, stride, padding, dilation, transposed, output_padding) -> (_Product, effective stride, P, Q)
_dgrad_lowerings = {}    # (dy's N, H, W, C, K, R, S, effective stride, padding, dilation, transposed, P, Q) -> _Product


def _lower_forward(N, H, W, C, K, R, S, stride, padding, dilation, transposed, output_padding):
    """the library product a layer's forward becomes -> (_Product, the stride backward sees, P, Q)"""
    sh, sw = stride; ph, pw = padding; dh, dw = dilation
    if not transposed:
        P = (H + 2 * ph - dh * (R - 1) - 1) // sh + 1
        Q = (W + 2 * pw - dw * (S - 1) - 1) // sw + 1
        Cp = _cpad(C, K)
        if Cp == C and _wino_s2_ok(N, H, W, C, K, R, S, stride, padding, dilation, P, Q, 0):
            return _product((K, C, 4, 4, C * 16, 16, 0, None, 2), None, N, H, W, C, K, 4, 4, (2, 2), (0, 0), (1, 1), P, Q, 0), stride, P, Q
        wino = int(_wino_ok(N, H, W, Cp, K, R, S, stride, padding, dilation, P, Q))
        return _product((K, C, R, S, C * R * S, R * S, 0, Cp, wino), Cp if Cp != C else None, N, H, W, Cp, K, R, S, stride, padding, dilation, P, Q, 0), stride, P, Q
    oph, opw = output_padding
    if H == 1 and sh == 1 and ph == 0 and dh == 1 and dw == 1 and R > 1 and oph == 0:
        # ONE input row (the generator's 1-D -> 2-D lift, ConvTranspose (4,3)): output row p takes tap row r = p and nothing else, so
        # the layer is its own stride-(R, sw) twin. Run as that fractionally strided layer every output row is a parity class with
        # its 1 x S taps; as a stride-1 layer it is a correlation over R x S taps of which R - 1 rows only ever meet padding
        # (4 x the multiplies: 62 -> 25 us at 8 lines, 325 -> 100 us at a generation batch of 64). Backward follows the returned stride.
        sh = R
        stride = (R, sw)
    P = (H - 1) * sh - 2 * ph + dh * (R - 1) + 1 + oph
    Q = (W - 1) * sw - 2 * pw + dw * (S - 1) + 1 + opw
    Cp = _cpad(C, K, fractional=(sh != 1 or sw != 1))
    cpad = Cp if Cp != C else None
    if sh == 1 and sw == 1:
        # stride-1 transposed conv == correlation with mirrored taps and padding dil*(R-1)-pad
        pad = (dh * (R - 1) - ph, dw * (S - 1) - pw)
        wino = int(_wino_ok(N, H, W, Cp, K, R, S, (1, 1), pad, dilation, P, Q))
        return _product((K, C, R, S, R * S, K * R * S, 1, Cp, wino), cpad, N, H, W, Cp, K, R, S, (1, 1), pad, dilation, P, Q, 0), stride, P, Q
    assert dh == 1 and dw == 1, "strided conv_transpose needs dilation 1"
    return _product((K, C, R, S, R * S, K * R * S, 0, Cp, 0), cpad, N, H, W, Cp, K, R, S, stride, padding, (1, 1), P, Q, 1), stride, P, Q


def _lower_dgrad(N, H, W, C, K, R, S, stride, padding, dilation, transposed, P, Q):
    """the library product a layer's data gradient becomes: a contraction over K (dy's channels) producing C channels; N is dy's batch"""
    sh, sw = stride; ph, pw = padding; dh, dw = dilation
    Kp = _cpad(K, C, fractional=(not transposed and (sh != 1 or sw != 1)))
    kpad = Kp if Kp != K else None
    if transposed:
        # gradient of a transposed conv is an ordinary (strided) correlation of dy
        wino = int(_wino_ok(N, P, Q, Kp, C, R, S, stride, padding, dilation, H, W))
        return _product((C, K, R, S, K * R * S, R * S, 0, Kp, wino), kpad, N, P, Q, Kp, C, R, S, stride, padding, dilation, H, W, 0)
    if C == 1 and sh == 1 and sw == 1 and K % 16 == 0 and 1 < R * S <= 64:
        # single-channel input (first layers): dx has one channel, so instead of a matrix-vector kernel the tap matrix
        # t[pixel][tap] = dy x W^T is formed by a 1x1 convolution on the matrix cores and folded back by col2im (379 -> ~40 us for
        # the discriminator's 7x7 in_conv at 8 x 64 x 512). The packed image is [1][taps][K]: element (tap, k) = w[k][0][tap]; K % 16 == 0
        # needs no padding
        return _product((R * S, K, 1, 1, 1, R * S, 0, None, 0), None, N, P, Q, K, R * S, 1, 1, (1, 1), (0, 0), (1, 1), P, Q, 0,
                        post=("hwg_col2im_taps", (N, H, W, 1), (N, H, W, P, Q, R, S, ph, pw, dh, dw)))
    if sh == 1 and sw == 1 and P == 1 and ph == 0 and dh == 1 and dw == 1 and R > 1 and Kp % 16 == 0 and C > 2:
        # ONE row of output gradients (the recogniser's last 3x3 layer: three rows in, one out): input row r receives tap row r
        # and nothing else - a fractionally strided layer with stride (R, 1) whose row classes have 1 x S taps each. As a stride-1
        # correlation with padding R - 1 two thirds of the multiplies meet padding (97 -> ~55 us at 8 x 1 x 126 x 512 -> 512).
        return _product((C, K, R, S, R * S, C * R * S, 0, Kp, 0), kpad, N, P, Q, Kp, C, R, S, (R, 1), (0, pw), (1, 1), H, W, 1)
    if sh == 1 and sw == 1:
        pad = (dh * (R - 1) - ph, dw * (S - 1) - pw)
        wino = int(_wino_ok(N, P, Q, Kp, C, R, S, (1, 1), pad, dilation, H, W))
        return _product((C, K, R, S, R * S, C * R * S, 1, Kp, wino), kpad, N, P, Q, Kp, C, R, S, (1, 1), pad, dilation, H, W, 0)
    if Kp == K and _wino_s2_ok(N, P, Q, K, C, R, S, stride, padding, dilation, H, W, 1):
        return _product((K, C, 4, 4, C * 16, 16, 1, None, 2), None, N, P, Q, K, C, 4, 4, (2, 2), (0, 0), (1, 1), H, W, 1)
    assert dh == 1 and dw == 1, "strided conv backward needs dilation 1"
    pack = (C, K, R, S, R * S, C * R * S, 0, Kp, 0)
    if P == 1 and ph == 0 and R > sh:
        # one output row (so R <= H < R + sh): the vertical stride never moves - stride R gives every input row its own class of 1 x S taps
        # where stride sh pairs each class with R / sh tap rows of which all but one meet nothing; the style extractor's last 4x4
        # stride-(2,1) layer.
        # (H > R: rows R.. of the input never met the filter - the style extractor's last block sees 5 rows and uses 4. They
        # get zeros; the R live rows run as the stride-R twin instead of sh-strided classes whose second block row is dead:
        # 4x1x254x256 -> 4x5x257x256: 81 -> ~50 us)
        dead = ("hwg_pad2d_fwd", (N, H, W, C), (N, R, W, C, 0, H - R, 0, 0, 0, 0.0)) if H > R else None
        return _product(pack, kpad, N, P, Q, Kp, C, R, S, (R, sw), padding, (1, 1), R, W, 1, post=dead)
    return _product(pack, kpad, N, P, Q, Kp, C, R, S, stride, padding, (1, 1), H, W, 1)


_wgrad_plans = {}


class _WgradPlan:
    """A layer's weight gradient as the library runs it (integers and a descriptor only, never a tensor): descriptor; engine 0 = Winograd
    F(3x3,2x2), 1 = MFMA kernel on channel-padded copies (Kq, Cq: the counts rounded up to multiples of 4, also in the descriptor), 2 = MFMA /
    direct kernel on the tensors as they are; need = workspace bytes of one launch; anchor_dy: dy is the kernel's anchor operand and x the
    gathered one (a transposed layer swaps them); S, sa, sb: tap columns and the gradient's channel strides in the parameter's layout;
    fuse_bias_ok: the bias gradient (column sums of dy) can ride along; tag: the launches' profile label, without the scope"""
    __slots__ = ("d", "engine", "need", "Kq", "Cq", "tiny_end", "tap_gemm", "anchor_dy", "S", "sa", "sb", "fuse_bias_ok", "tag", "_sets_ok", "_sets_ws")

    def sets_ok(self):
        """the S weight gradients of several gradient sets can run as ONE launch (asked once, when a grouped pass first meets the layer)"""
        if self._sets_ok is None:
            self._sets_ok = self.engine != 1 and not (self.engine == 0 and not self.anchor_dy) and not self.tiny_end and (
                self.engine == 0 or bool(L.query("hwg_conv_wgrad_sets_supported", self.d.ptr)))
        return self._sets_ok

    def sets_ws(self, S):
        if S not in self._sets_ws:
            self._sets_ws[S] = L.query("hwg_wino_wgrad_sets_workspace" if self.engine == 0 else "hwg_conv_wgrad_sets_workspace", self.d.ptr, S)
        return self._sets_ws[S]


def _make_wgrad_plan(N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, P, Q, transposed):
    p = _WgradPlan()
    d = _desc(N, P, Q, K, C, R, S, (sh, sw), (ph, pw), (dh, dw), H, W) if transposed else _desc(N, H, W, C, K, R, S, (sh, sw), (ph, pw), (dh, dw), P, Q)
    p.d, p.Kq, p.Cq = d, (d.K + 3) // 4 * 4, (d.C + 3) // 4 * 4
    # single-channel ends (C == 1 first layers, K <= 2 heads) have a direct kernel; on large images the MFMA kernel on a
    # 4-channel zero-padded copy is faster (measured 164 vs 390 us for the 7x7 first layer of D), so only small ones stay direct
    # (the direct kernel runs a K<=2 head as ONE workgroup: 166 us for the discriminator's 256->1 3x3 head at 304 pixels, so heads
    # with a wide gathered side go through the padded MFMA path as well; only narrow-and-small cases stay direct)
    p.tiny_end = ((d.C == 1 and d.K % 4 == 0 and d.K > 2) or (d.K <= 2 and d.C % 4 == 0 and d.C < 16)) and d.N * d.P * d.Q < 8192
    # single gathered channel (first layers): the library runs the taps as the GEMM's N dimension, no padding needed
    p.tap_gemm = d.C == 1 and d.K > 2 and d.K % 4 == 0 and R * S <= 64
    # engine 1: channel counts that are not multiples of 4 (RIMES: 78 classes -> 206/334-channel inputs, 78 outputs): the kernel runs on
    # zero-padded copies and the valid block of its result is kept
    p.engine = 0 if _wino_wgrad_ok(d) else 1 if (p.Kq != d.K or p.Cq != d.C) and not p.tiny_end and not p.tap_gemm else 2
    # The bias gradient rides along only when dy is the kernel's anchor operand (not transposed) and, on the MFMA engine, the MFMA path runs.
    # Engine 1 never fuses it, never defers its sum and never leaves the main stream.
    p.fuse_bias_ok = not transposed and (p.engine == 0 or (p.engine == 2 and not p.tiny_end and d.K > 2 and (d.C > 2 or p.tap_gemm)))
    if p.engine == 1:
        d.K, d.C = p.Kq, p.Cq
    p.need = L.query("hwg_wino_wgrad_workspace" if p.engine == 0 else "hwg_conv_wgrad_workspace", d.ptr)
    p.anchor_dy, p.S, p.sa, p.sb = not transposed, S, (K if transposed else C) * R * S, R * S
    p.tag = (d.N, d.H, d.W, d.C, d.K, R, S, (sh, sw), (ph, pw), (dh, dw), "wgrad")
    p._sets_ok, p._sets_ws = None, {}
    return p


def _wgrad_begin(ctx, dy):
    """what every weight-gradient path starts with -> (the layer's plan, anchor operand, gathered operand); descriptor, engine choice and
    workspace size are fixed per geometry: built once (the library's cost models run there)"""
    x, weight = ctx.saved_tensors
    _RUN_SCOPE[0] = ctx.scope
    stride, padding, dilation, transposed, P, Q = ctx.geom
    pkey = tuple(x.shape) + (dy.shape[3],) + _taps(weight) + stride + padding + dilation + (P, Q, transposed)
    plan = _wgrad_plans.get(pkey)
    if plan is None:
        plan = _wgrad_plans[pkey] = _make_wgrad_plan(*pkey)
    if PROF_SHAPES is not None:
        _prof_tag(plan.tag + (ctx.scope,))
    return (plan, dy, x) if plan.anchor_dy else (plan, x, dy)


def _fused_bias_dest(ctx, plan, device):
    """where the bias gradient that rides along with a weight-gradient launch goes -> (dbias, bacc, db): the buffer the kernel writes, whether
    it accumulates there, and what goes back to autograd (None: accumulated in place). (None, 0, None): nothing rides along - no bias
    gradient is wanted, or the launch cannot carry it and the caller sums dy's columns itself"""
    if not (ctx.has_bias and ctx.needs_input_grad[2] and plan.fuse_bias_ok):
        return None, 0, None
    bref = ctx.param_refs[1]
    if _direct(bref):
        return _grad_buffer(bref), 1, None
    db = torch.empty((plan.d.K,), dtype=torch.float32, device=device)
    return db, 0, db


def _bias_colsum(dy, bref):
    """the bias gradient as a launch of its own -> the gradient, or None where it was accumulated into the parameter's buffer"""
    cols = dy.view(-1, dy.shape[3])
    if not _direct(bref):
        return colsum(cols)
    colsum(cols, out=_grad_buffer(bref), accumulate=True)


def _wgrad_route(plan, nbytes, device, operands, direct, bias_ok, ask_arena, eager_ws):
    """Where one weight-gradient launch of engine 0 or 2 goes -> (stream, workspace); queues the deferred sum and forks the side stream.
    bias_ok: no bias gradient rides along, or it accumulates in place (a returned one is read right after the launch).
    ask_arena: the partial images go to a slice of the deferred-sum arena; with bias_ok their sum is only queued (hwg_wgrad_defer_next), else
    the slice serves as plain workspace. A full arena means workspace and an immediate sum. With SIDE_WGRAD the MFMA engine's launch for a
    parameter's own buffer goes to the side stream (dy and x are complete on the main stream when it forks; operands held until the join), the
    Winograd engine's never. eager_ws: the single-gradient path asks for the shared scratch buffer before it is known that the launch leaves
    the main stream (the order of scratch requests is part of recorded launch lists)."""
    st = _stream()
    arena = ws = _defer_workspace(nbytes, device) if ask_arena else None
    side = SIDE_WGRAD and direct and bias_ok and plan.engine == 2
    if ws is None and (eager_ws or not side):
        ws = workspace(nbytes, device)
    if side:
        s2, st2, skey = _side_stream(device)
        L.call("hwg_stream_fork", st, st2)
        if arena is None:
            ws = _side_workspace(nbytes, device, s2)
        st = st2
        _side_hold.append(operands)
        _side_dirty.add(skey)
    if arena is not None and bias_ok:
        L.call("hwg_wgrad_defer_next")
    return st, ws


class _Conv2d(Function):
    """y = conv2d(x, w) (+b) or conv_transpose2d(x, w) (+b); x NHWC."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dilation, transposed, output_padding):
        _chk(x, "conv input"); _chk(weight, "conv weight"); _chk(bias, "conv bias")
        ctx.scope = _RUN_SCOPE[0] = SCOPE
        N, H, W, C = x.shape
        # Linear [O,I] and Conv1d [O,I,S] parameters are used as they are (same memory as [O,I,1,S]); a .view() of the parameter would be a
        # non-leaf tensor, lose the packed-weight cache and the direct gradient accumulation and cost three extra ATen ops per backward
        R, S = _taps(weight)
        if not transposed:
            K = weight.shape[0]
            assert weight.shape[1] == C, "conv: weight expects %d input channels, got %d" % (weight.shape[1], C)
        else:
            K = weight.shape[1]
            assert weight.shape[0] == C, "conv_transpose: weight expects %d input channels, got %d" % (weight.shape[0], C)
        key = (N, H, W, C, K, R, S, stride, padding, dilation, transposed, output_padding)
        low = _fwd_lowerings.get(key)
        if low is None:
            low = _fwd_lowerings[key] = _lower_forward(*key)
        prod, stride, P, Q = low
        y = _run_conv(prod, x, weight, bias)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.param_refs = (weight, bias)
        ctx.geom = (stride, padding, dilation, transposed, P, Q)
        return y

    sets = "native"

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = _Conv2d._dgrad(ctx, dy) if ctx.needs_input_grad[0] else None
        dw_, db = _Conv2d._wgrad(ctx, dy)
        return dx, dw_, db, None, None, None, None, None

    @staticmethod
    def backward_sets(ctx, S, targets, dy):
        """S gradient sets stacked along the batch axis (Tape.backward_sets): ONE data-gradient launch over S x N samples (the generator's
        layers fill a quarter of the chip at 8 lines), one weight gradient per set (x is shared, every set accumulates into its own buffer)"""
        global GRAD_SET
        dy = dy.contiguous()
        dx = _Conv2d._dgrad(ctx, dy) if ctx.needs_input_grad[0] else None
        grouped = _Conv2d._wgrad_sets(ctx, dy, S, targets) if S > 1 else None
        if grouped is not None:
            dws, dbs = grouped
        else:
            n = dy.shape[0] // S
            dws, dbs = [], []
            for s_ in range(S):
                GRAD_SET = targets[s_]
                dw_, db = _Conv2d._wgrad(ctx, dy[s_ * n:(s_ + 1) * n])
                dws.append(dw_); dbs.append(db)
        return (dx, None if dws[0] is None else SetGrad(S, parts=dws), None if dbs[0] is None else SetGrad(S, parts=dbs), None, None, None, None, None)

    @staticmethod
    def _dgrad(ctx, dy):
        x, weight = ctx.saved_tensors
        _RUN_SCOPE[0] = ctx.scope
        # (dy's batch may be a multiple of x's: several gradient sets through the same layer)
        key = (dy.shape[0],) + tuple(x.shape[1:]) + (dy.shape[3],) + _taps(weight) + ctx.geom
        prod = _dgrad_lowerings.get(key)
        if prod is None:
            prod = _dgrad_lowerings[key] = _lower_dgrad(*key)
        return _run_conv(prod, dy, weight, None)

    @staticmethod
    def _wgrad(ctx, dy):
        """-> (dw, db) as tensors, or None where the kernel accumulated straight into the parameter's gradient buffer"""
        dw_ = db = dbias = None
        wref, bref = ctx.param_refs
        if ctx.needs_input_grad[1]:
            plan, u, v = _wgrad_begin(ctx, dy)
            direct = _direct(wref)
            dw_ = _grad_buffer(wref) if direct else torch.empty_like(ctx.saved_tensors[1])
            acc = 1 if direct else 0
            if plan.engine == 1:
                # the kernel runs on zero-padded copies (the plan's descriptor carries the padded counts)
                Kq, Cq, S, RS = plan.Kq, plan.Cq, plan.S, plan.sb
                dK, dC = u.shape[3], v.shape[3]
                up = _pad_channels(u, Kq) if Kq != dK else u
                vp = _pad_channels(v, Cq) if Cq != dC else v
                tmp = torch.empty((Kq, Cq, RS // S, S), dtype=torch.float32, device=dy.device)
                ws = workspace(plan.need, dy.device)
                L.call("hwg_conv_wgrad", plan.d.ptr, up, vp, tmp, Cq * RS, RS, S, 1, 0, None, 0, ws, ws.numel(), _stream())
                # the valid block of the padded result, added to (or copied into) the gradient through the C-ABI: row k of `tmp` holds Cq*R*S floats
                # of which the first dC*R*S belong to real channels (a torch-side add_ here was invisible to a recorded call list: every RIMES
                # geometry of the recogniser failed its replay self-check)
                L.call("hwg_copy_channels", tmp, Cq * RS, 0, dw_, dC * RS, 0, dC * RS, dK, 1, 0, acc, _stream())
            else:
                dbias, bacc, db = _fused_bias_dest(ctx, plan, dy.device)
                # the sum of the partial images may wait for the flush behind the backward pass where nothing reads the gradient earlier: a
                # parameter's buffer, or the dW_sn of a spectral-norm layer whose own backward is queued for the same flush (_SpectralScale).
                # The arena is asked before the bias is looked at.
                late = direct or getattr(wref, "_hwg_sn_defer", False)
                st, ws = _wgrad_route(plan, plan.need, dy.device, (u, v), direct, dbias is None or bacc == 1,
                                      ask_arena=bool(DEFER_REDUCE and late and plan.need), eager_ws=True)
                L.call("hwg_wino_wgrad" if plan.engine == 0 else "hwg_conv_wgrad", plan.d.ptr, u, v, dw_, plan.sa, plan.sb, plan.S, 1, acc, dbias, bacc,
                       ws, ws.numel(), st)
            if direct:
                dw_ = None
        if ctx.has_bias and ctx.needs_input_grad[2] and dbias is None:
            db = _bias_colsum(dy, bref)
        return dw_, db

    @staticmethod
    def _wgrad_sets(ctx, dy, S, targets):
        """the S weight gradients of this layer as ONE launch (hwg_conv_wgrad_sets / hwg_wino_wgrad_sets: the layer input is shared, every set
        has its own pixel ranges, partial images and destination buffer). -> (per-set dw list, per-set db list) with None where the kernels
        accumulated in place, or None when this layer has no grouped path (channel-padded copies, K <= 2 / C <= 2 direct kernels)"""
        global GRAD_SET
        import numpy as np
        if not ctx.needs_input_grad[1]:
            return None
        plan, u, v = _wgrad_begin(ctx, dy)
        if not plan.sets_ok():
            return None
        weight = ctx.saved_tensors[1]
        wref, bref = ctx.param_refs
        direct = _direct(wref)
        dws, dbs, dws_out, dbs_out, bacc = [], [], [], [], 0
        for s_ in range(S):
            GRAD_SET = targets[s_]
            dws.append(_grad_buffer(wref) if direct else torch.empty_like(weight))
            dws_out.append(None if direct else dws[-1])
            dbias, bacc, db = _fused_bias_dest(ctx, plan, dy.device)
            if dbias is not None:
                dbs.append(dbias); dbs_out.append(db)
        wptr = np.array([t.data_ptr() for t in dws], dtype=np.int64)
        btab = np.array([t.data_ptr() for t in dbs], dtype=np.int64)
        bptr = btab.ctypes.data if dbs else None
        total = plan.sets_ws(S)
        bias_ok = not dbs or bacc == 1
        # (here the bias is looked at first: the arena is only asked where the sum can wait, for a parameter's own buffer)
        st, ws = _wgrad_route(plan, total, dy.device, (u, v), direct, bias_ok, ask_arena=bool(DEFER_REDUCE and direct and bias_ok and total), eager_ws=False)
        if plan.engine == 0:
            L.call("hwg_wino_wgrad_sets", plan.d.ptr, u, v, S, wptr.ctypes.data, plan.sa, plan.sb, plan.S, 1, 1 if direct else 0, bptr, bacc, ws, ws.numel(), st)
        else:
            L.call("hwg_conv_wgrad_sets", plan.d.ptr, u, v, S, 0 if plan.anchor_dy else 1, wptr.ctypes.data, plan.sa, plan.sb, plan.S, 1, 1 if direct else 0, bptr, bacc,
                   ws, ws.numel(), st)
        if ctx.has_bias and ctx.needs_input_grad[2] and not dbs:
            n = dy.shape[0] // S
            for s_ in range(S):
                GRAD_SET = targets[s_]
                dbs_out.append(_bias_colsum(dy[s_ * n:(s_ + 1) * n], bref))
        if not dbs_out:
            dbs_out = [None] * S
        return dws_out, dbs_out


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1):
    return _Conv2d.apply(x, weight, bias, _pair(stride), _pair(padding), _pair(dilation), False, (0, 0))


def conv_transpose2d(x, weight, bias=None, stride=1, padding=0, output_padding=0, dilation=1):
    return _Conv2d.apply(x, weight, bias, _pair(stride), _pair(padding), _pair(dilation), True, _pair(output_padding))


def conv1d(x, weight, bias=None, stride=1, padding=0, dilation=1):
    """x [N,1,L,C]; weight in Conv1d layout [O,I,S]"""
    return conv2d(x, weight, bias, (1, stride), (0, padding), (1, dilation))


def linear(x, weight, bias=None):
    """x [rows, I] -> [rows, O]; weight [O, I]"""
    rows, I = x.shape
    y = conv2d(x.view(rows, 1, 1, I), weight, bias)
    return y.view(rows, weight.shape[0])


def colsum(x2d, out=None, accumulate=False):
    rows, C = x2d.shape
    if out is None:
        out = torch.empty((C,), dtype=torch.float32, device=x2d.device)
    need = L.query("hwg_colsum_workspace", rows, C)
    ws = workspace(need, x2d.device)
    L.call("hwg_colsum", x2d, rows, C, out, int(accumulate), ws, ws.numel(), _stream())
    return out


# ----------------------------------------------------------------------------------------------
# normalisation + activation
# ----------------------------------------------------------------------------------------------
def _affine_stamp(gamma, beta):
    """(version counters, optimizer epoch) of a norm's affine parameters: HipAdam writes through raw pointers behind torch's version
    counters and bumps WEIGHT_EPOCH of the parameter's group instead"""
    return tuple((p._version, WEIGHT_EPOCH.get(getattr(p, "_hwg_group", None), 0)) for p in (gamma, beta) if p is not None)


class _Norm(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, mode, groups, eps, mask, act, slope, running_mean, running_var, momentum):
        _chk(x, "norm input"); _chk(gamma, "norm weight"); _chk(beta, "norm bias"); _chk(mask, "channel mask")
        N, C = x.shape[0], x.shape[-1]
        HW = x.numel() // (N * C)
        y = torch.empty_like(x)
        mean = torch.empty((N, C), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        ws = workspace(L.query("hwg_norm_workspace", N, HW, C), x.device)
        L.call("hwg_norm_fwd", x, y, N, HW, C, mode, groups, eps, gamma, beta, 0, mask, act, slope, mean, rstd,
               running_mean, running_var, momentum, ws, ws.numel(), _stream())
        ctx.save_for_backward(x, y, gamma, mask, mean, rstd)
        ctx.cfg = (mode, groups, act, slope, N, HW, C, beta is not None)
        ctx.param_refs = (gamma, beta)
        # the backward pass recomputes relu / leaky-relu gates from x and the affine it reads THEN: remember which weights the forward saw
        ctx.wstamp = _affine_stamp(gamma, beta) if act in (ACT_RELU, ACT_LRELU) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, mask, mean, rstd = ctx.saved_tensors
        mode, groups, act, slope, N, HW, C, has_beta = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        gref, bref = ctx.param_refs
        if ctx.wstamp is not None and ctx.wstamp != _affine_stamp(gref, bref):
            raise L.HwgError("norm backward after its affine parameters changed (optimizer step / in-place write between forward and backward): the "
                             "activation gates are recomputed from x and the current affine and would be wrong; run backward before stepping")
        direct = (gamma is None or _direct(gref)) and (not has_beta or _direct(bref))
        if direct:
            dgamma = _grad_buffer(gref) if gamma is not None else None
            dbeta = _grad_buffer(bref) if has_beta else None
        else:
            dgamma = torch.empty((C,), dtype=torch.float32, device=x.device) if gamma is not None else None
            dbeta = torch.empty((C,), dtype=torch.float32, device=x.device) if has_beta else None
        ws = workspace(L.query("hwg_norm_workspace", N, HW, C), x.device)
        # beta: relu / leaky relu gates are recomputed from x and the forward call's affine instead of being read from y (csrc/norm_act.hip)
        L.call("hwg_norm_bwd", dy, x, y, dx, N, HW, C, mode, groups, gamma, bref if has_beta else None, 0, mask, act, slope, mean, rstd, dgamma, dbeta, 1 if direct else 0,
               ws, ws.numel(), _stream())
        if direct:
            dgamma = dbeta = None
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None


def group_norm(x, groups, gamma, beta, eps=1e-5, mask=None, act=ACT_NONE, slope=0.0):
    return _Norm.apply(x, gamma, beta, NORM_GN, groups, eps, mask, act, slope, None, None, 0.0)


def batch_norm_train(x, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, act=ACT_NONE, slope=0.0):
    return _Norm.apply(x, gamma, beta, NORM_BN, 1, eps, None, act, slope, running_mean, running_var, momentum)


def instance_norm(x, eps=1e-5):
    return _Norm.apply(x, None, None, NORM_IN, 1, eps, None, ACT_NONE, 0.0, None, None, 0.0)


class _AdaIN(Function):
    """(x, noise, noise_weight_orig, gamma, beta) -> gamma*IN(lrelu(x + w*noise)) + beta  (+ folded conv-bias gradient)"""

    @staticmethod
    def forward(ctx, x, noise, noise_w, gamma, beta, noise_scale, slope, eps):
        for t, n in ((x, "x"), (noise, "noise"), (noise_w, "noise weight"), (gamma, "gamma"), (beta, "beta")):
            _chk(t, "adain " + n)
        N, C = x.shape[0], x.shape[-1]
        HW = x.numel() // (N * C)
        u = torch.empty_like(x)
        y = torch.empty_like(x)
        mean = torch.empty((N, C), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        ws = workspace(L.query("hwg_norm_workspace", N, HW, C), x.device)
        L.call("hwg_adain_fwd", x, noise, noise_w, noise_scale, slope, gamma, beta, eps, u, y, mean, rstd, N, HW, C, ws, ws.numel(), _stream())
        ctx.save_for_backward(u, noise, gamma, mean, rstd)
        ctx.cfg = (noise_scale, slope, N, HW, C, noise_w.shape)
        ctx.param_refs = (noise_w,)
        return y

    @staticmethod
    def backward(ctx, dy):
        u, noise, gamma, mean, rstd = ctx.saved_tensors
        noise_scale, slope, N, HW, C, wshape = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty_like(u)
        dgamma = torch.empty((N, C), dtype=torch.float32, device=u.device)
        dbeta = torch.empty_like(dgamma)
        (nwref,) = ctx.param_refs
        direct = _direct(nwref)
        dnw = _grad_buffer(nwref) if direct else torch.empty((C,), dtype=torch.float32, device=u.device)
        need = L.query("hwg_norm_workspace", N, HW, C)
        ws = _defer_workspace(need, u.device) if (DEFER_REDUCE and direct) else None      # the noise-weight sum joins the pass's one deferred launch
        if ws is not None:
            L.call("hwg_wgrad_defer_next")
        else:
            ws = workspace(need, u.device)
        L.call("hwg_adain_bwd", dy, u, noise, noise_scale, slope, gamma, mean, rstd, dx, dgamma, dbeta, dnw, None, 1 if direct else 0, N, HW, C,
               ws, ws.numel(), _stream())
        return dx, None, (None if direct else dnw.view(wshape)), dgamma, dbeta, None, None, None

    sets = "native"

    @staticmethod
    def backward_sets(ctx, S, targets, dy):
        """S gradient sets stacked along the batch axis: the saved activations are shared, so the kernel runs once per set on that set's slice
        and writes its slice of the stacked results (no concatenation pass); the noise-weight gradient of set s goes to set s's buffer"""
        global GRAD_SET
        u, noise, gamma, mean, rstd = ctx.saved_tensors
        noise_scale, slope, N, HW, C, wshape = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty((S * N,) + tuple(u.shape[1:]), dtype=torch.float32, device=u.device)
        dgamma = torch.empty((S * N, C), dtype=torch.float32, device=u.device)
        dbeta = torch.empty_like(dgamma)
        (nwref,) = ctx.param_refs
        if not _direct(nwref):
            raise L.HwgError("batched AdaIN backward needs the noise weight's gradient buffer (a leaf parameter)")
        need = L.query("hwg_norm_workspace", N, HW, C)
        st = _stream()
        for s_ in range(S):
            GRAD_SET = targets[s_]
            dnw = _grad_buffer(nwref)
            sl = slice(s_ * N, (s_ + 1) * N)
            ws = _defer_workspace(need, u.device) if DEFER_REDUCE else None
            if ws is not None:
                L.call("hwg_wgrad_defer_next")
            else:
                ws = workspace(need, u.device)
            L.call("hwg_adain_bwd", dy[sl], u, noise, noise_scale, slope, gamma, mean, rstd, dx[sl], dgamma[sl], dbeta[sl], dnw, None, 1, N, HW, C,
                   ws, ws.numel(), st)
        return dx, None, None, dgamma, dbeta, None, None, None


class VirtualNoise:
    """a noise tensor that is never written: `shape` standard normals = what hwg_randn(seed, offset) would put into a tensor of that shape
    (rng.NoiseBlock hands these out in forward-only passes; adain_epilogue draws the values inside its kernel)"""

    __slots__ = ("seed", "offset", "shape")

    def __init__(self, seed, offset, shape):
        self.seed, self.offset, self.shape = int(seed), int(offset), tuple(shape)

    def materialise(self, device):
        out = torch.empty(self.shape, dtype=torch.float32, device=device)
        L.call("hwg_randn", out, out.numel(), self.seed, self.offset, _stream())
        return out


def adain_epilogue(x, noise, noise_w, gamma, beta, noise_scale, slope=0.2, eps=1e-5):
    if isinstance(noise, VirtualNoise):
        if TAPE is not None or (torch.is_grad_enabled() and any(t.requires_grad for t in (x, noise_w, gamma, beta))):
            noise = noise.materialise(x.device)          # (a backward pass will read the noise)
        else:
            for t, n in ((x, "x"), (noise_w, "noise weight"), (gamma, "gamma"), (beta, "beta")):
                _chk(t, "adain " + n)
            assert tuple(x.shape) == noise.shape
            N, C = x.shape[0], x.shape[-1]
            HW = x.numel() // (N * C)
            u = torch.empty_like(x)
            y = torch.empty_like(x)
            mean = torch.empty((N, C), dtype=torch.float32, device=x.device)
            rstd = torch.empty_like(mean)
            ws = workspace(L.query("hwg_norm_workspace", N, HW, C), x.device)
            L.call("hwg_adain_fwd_rng", x, noise.seed, noise.offset, noise_w, noise_scale, slope, gamma, beta, eps, u, y, mean, rstd, N, HW, C,
                   ws, ws.numel(), _stream())
            return y
    return _AdaIN.apply(x, noise, noise_w, gamma, beta, noise_scale, slope, eps)


class _BiasAct(Function):
    @staticmethod
    def forward(ctx, x, bias, mask, act, slope):
        _chk(x, "bias_act input"); _chk(bias, "bias"); _chk(mask, "channel mask")
        C = x.shape[-1]
        N = x.shape[0]
        rows = x.numel() // C
        HW = rows // N
        y = torch.empty_like(x)
        L.call("hwg_bias_act_fwd", x, bias, mask, y, rows, HW, C, act, slope, _stream())
        ctx.save_for_backward(y, mask)
        ctx.cfg = (act, slope, rows, HW, C, bias is not None)
        ctx.param_refs = (bias,)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, mask = ctx.saved_tensors
        act, slope, rows, HW, C, has_bias = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        L.call("hwg_bias_act_bwd", dy, y, mask, dx, rows, HW, C, act, slope, _stream())
        db = None
        if has_bias and ctx.needs_input_grad[1]:
            (bref,) = ctx.param_refs
            if _direct(bref):
                colsum(dx.view(rows, C), out=_grad_buffer(bref), accumulate=True)
            else:
                db = colsum(dx.view(rows, C))
        return dx, db, None, None, None


def bias_act(x, bias=None, mask=None, act=ACT_NONE, slope=0.0):
    return _BiasAct.apply(x, bias, mask, act, slope)


def relu(x):
    return _BiasAct.apply(x, None, None, ACT_RELU, 0.0)


def leaky_relu(x, slope):
    return _BiasAct.apply(x, None, None, ACT_LRELU, slope)


class _Tanh(Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x, "tanh input")
        y = torch.empty_like(x)
        L.call("hwg_tanh_fwd", x, y, x.numel(), _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        L.call("hwg_tanh_bwd", dy.contiguous(), y, dx, y.numel(), _stream())
        return dx


def tanh(x):
    return _Tanh.apply(x)


class _PixelNorm(Function):
    @staticmethod
    def forward(ctx, x, eps):
        _chk(x, "pixelnorm input")
        rows, C = x.shape
        y = torch.empty_like(x)
        L.call("hwg_pixelnorm_fwd", x, y, rows, C, eps, _stream())
        ctx.save_for_backward(x)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        L.call("hwg_pixelnorm_bwd", dy.contiguous(), x, dx, x.shape[0], x.shape[1], ctx.eps, _stream())
        return dx, None


def pixel_norm(x, eps=1e-8):
    return _PixelNorm.apply(x, eps)


# ----------------------------------------------------------------------------------------------
# pooling / resampling / padding / concat
# ----------------------------------------------------------------------------------------------
class _AvgPool(Function):
    sets = "stacked"

    @staticmethod
    def forward(ctx, x, kh, kw):
        _chk(x, "avgpool input")
        N, H, W, C = x.shape
        y = torch.empty((N, H // kh, W // kw, C), dtype=torch.float32, device=x.device)
        L.call("hwg_avgpool_fwd", x, y, N, H, W, C, kh, kw, _stream())
        ctx.cfg = (N, H, W, C, kh, kw)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C, kh, kw = ctx.cfg
        N = dy.shape[0]           # (several gradient sets stacked along the batch axis: Tape.backward_sets)
        dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
        L.call("hwg_avgpool_bwd", dy.contiguous(), dx, N, H, W, C, kh, kw, _stream())
        return dx, None, None


def avg_pool2d(x, kernel):
    kh, kw = _pair(kernel)
    return _AvgPool.apply(x, kh, kw)


class _ActAvgPool(Function):
    """avg_pool2d(act(mask * x)) as one kernel per direction (hwg_act_avgpool_*): bit-identical to bias_act + avg_pool2d, without writing and
    re-reading the full-resolution activation (forward) and its gradient (backward); the gate is recomputed from x"""

    @staticmethod
    def forward(ctx, x, mask, act, slope, kh, kw):
        _chk(x, "act_avgpool input"); _chk(mask, "channel mask")
        N, H, W, C = x.shape
        y = torch.empty((N, H // kh, W // kw, C), dtype=torch.float32, device=x.device)
        L.call("hwg_act_avgpool_fwd", x, mask, y, N, H, W, C, kh, kw, act, slope, _stream())
        ctx.save_for_backward(x, mask)
        ctx.cfg = (N, H, W, C, kh, kw, act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask = ctx.saved_tensors
        N, H, W, C, kh, kw, act, slope = ctx.cfg
        dx = torch.empty_like(x)
        L.call("hwg_act_avgpool_bwd", dy.contiguous(), x, mask, dx, N, H, W, C, kh, kw, act, slope, _stream())
        return dx, None, None, None, None, None


def act_avg_pool2d(x, kernel, mask=None, act=ACT_NONE, slope=0.0):
    """avg_pool2d(bias_act(x, None, mask, act, slope), kernel) in one pass"""
    kh, kw = _pair(kernel)
    return _ActAvgPool.apply(x, mask, act, slope, kh, kw)


class _MaxPool(Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding, relu):
        _chk(x, "maxpool input")
        N, H, W, C = x.shape
        kh, kw = kernel; sh, sw = stride; ph, pw = padding
        P = (H + 2 * ph - kh) // sh + 1
        Q = (W + 2 * pw - kw) // sw + 1
        y = torch.empty((N, P, Q, C), dtype=torch.float32, device=x.device)
        idx = torch.empty((N, P, Q, C), dtype=torch.int32, device=x.device)
        L.call("hwg_maxpool_relu_fwd" if relu else "hwg_maxpool_fwd", x, y, idx, N, H, W, C, kh, kw, sh, sw, ph, pw, P, Q, _stream())
        if relu:
            ctx.save_for_backward(idx, y)
        else:
            ctx.save_for_backward(idx)
        ctx.cfg = (N, H, W, C, kh, kw, sh, sw, ph, pw, P, Q, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C, kh, kw, sh, sw, ph, pw, P, Q, relu = ctx.cfg
        dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
        if relu:
            idx, y = ctx.saved_tensors
            L.call("hwg_maxpool_relu_bwd", dy.contiguous(), y, idx, dx, N, H, W, C, kh, kw, sh, sw, ph, pw, P, Q, _stream())
        else:
            (idx,) = ctx.saved_tensors
            L.call("hwg_maxpool_bwd", dy.contiguous(), idx, dx, N, H, W, C, kh, kw, sh, sw, ph, pw, P, Q, _stream())
        return dx, None, None, None, None


def max_pool2d(x, kernel, stride=None, padding=0, relu=False):
    """relu=True: relu(max_pool2d(x)) (== max_pool2d(relu(x)) exactly) with the ReLU riding along in the pooling kernels, both directions"""
    kernel = _pair(kernel)
    stride = kernel if stride is None else _pair(stride)
    return _MaxPool.apply(x, kernel, stride, _pair(padding), bool(relu))


class _Upsample(Function):
    sets = "stacked"

    @staticmethod
    def forward(ctx, x, fh, fw):
        _chk(x, "upsample input")
        N, H, W, C = x.shape
        y = torch.empty((N, H * fh, W * fw, C), dtype=torch.float32, device=x.device)
        L.call("hwg_upsample_nearest_fwd", x, y, N, H, W, C, fh, fw, _stream())
        ctx.cfg = (N, H, W, C, fh, fw)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C, fh, fw = ctx.cfg
        N = dy.shape[0]
        dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
        L.call("hwg_upsample_nearest_bwd", dy.contiguous(), dx, N, H, W, C, fh, fw, _stream())
        return dx, None, None


def upsample_nearest(x, scale):
    fh, fw = _pair(scale)
    return _Upsample.apply(x, fh, fw)


class _Blur(Function):
    sets = "stacked"

    @staticmethod
    def forward(ctx, x):
        _chk(x, "blur input")
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        L.call("hwg_blur3", x, y, N, H, W, C, _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        return _Blur.apply(dy.contiguous())  # symmetric kernel; differentiable again like the reference's BlurFunctionBackward


def blur3(x):
    return _Blur.apply(x)


class _Pad2d(Function):
    sets = "stacked"

    @staticmethod
    def forward(ctx, x, pt, pb, pl, pr, mode, value):
        _chk(x, "pad input")
        N, H, W, C = x.shape
        y = torch.empty((N, H + pt + pb, W + pl + pr, C), dtype=torch.float32, device=x.device)
        L.call("hwg_pad2d_fwd", x, y, N, H, W, C, pt, pb, pl, pr, mode, value, _stream())
        ctx.cfg = (N, H, W, C, pt, pb, pl, pr, mode)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C, pt, pb, pl, pr, mode = ctx.cfg
        N = dy.shape[0]
        dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
        L.call("hwg_pad2d_bwd", dy.contiguous(), dx, N, H, W, C, pt, pb, pl, pr, mode, _stream())
        return dx, None, None, None, None, None, None


def pad2d(x, left, right, top=0, bottom=0, mode="constant", value=0.0):
    if left == 0 and right == 0 and top == 0 and bottom == 0:
        return x
    return _Pad2d.apply(x, top, bottom, left, right, 1 if mode == "replicate" else 0, float(value))


class _CatChannels(Function):
    """concatenate along C; parts that are 2-D [N, c] are broadcast over the pixels of sample n"""
    sets = "stacked"

    @staticmethod
    def forward(ctx, ref_shape, *parts):
        N, H, W = ref_shape
        rows = N * H * W
        widths = [p.shape[-1] for p in parts]
        Ct = sum(widths)
        out = torch.empty((N, H, W, Ct), dtype=torch.float32, device=parts[0].device)
        off = 0
        st = _stream()
        for p, c in zip(parts, widths):
            _chk(p, "cat part")
            bcast = 1 if p.dim() == 2 else 0
            L.call("hwg_copy_channels", p, c, 0, out, Ct, off, c, rows, H * W, bcast, 0, st)
            off += c
        ctx.cfg = (N, H, W, widths, [p.dim() == 2 for p in parts])
        return out

    @staticmethod
    def backward(ctx, dy):
        N, H, W, widths, bc = ctx.cfg
        dy = dy.contiguous()
        N = dy.shape[0]
        Ct = sum(widths)
        rows = N * H * W
        grads = []
        off = 0
        st = _stream()
        for i, (c, b) in enumerate(zip(widths, bc)):
            if not ctx.needs_input_grad[1 + i]:
                grads.append(None)
            elif b:
                g = torch.empty((N, c), dtype=torch.float32, device=dy.device)
                L.call("hwg_reduce_rows", dy, Ct, off, g, c, N, H * W, 0, st)
                grads.append(g)
            else:
                g = torch.empty((N, H, W, c), dtype=torch.float32, device=dy.device)
                L.call("hwg_copy_channels", dy, Ct, off, g, c, 0, c, rows, H * W, 0, 0, st)
                grads.append(g)
            off += c
        return (None,) + tuple(grads)


def cat_channels(parts, spatial):
    """parts: list of [N,H,W,c] or [N,c] (broadcast) tensors; spatial = (N,H,W)"""
    return _CatChannels.apply(tuple(spatial), *parts)


def onehot_rows(label_LB, ncls):
    """label int32 [L,B] (device) -> float [B,1,L,ncls]"""
    Lr, B = label_LB.shape
    _chk(label_LB, "label", torch.int32)
    out = torch.empty((B, 1, Lr, ncls), dtype=torch.float32, device=label_LB.device)
    L.call("hwg_onehot", label_LB, out, Lr, B, ncls, ncls, 0, _stream())
    return out


def onehot_both(label_LB, ncls):
    """label int32 [L,B] (device) -> (time-major [L,B,ncls] with the NHWC rows [B,1,L,ncls] hanging on it as `_hwg_nhwc`), one launch: the
    consumers that read NHWC (generator, spacer) take the attached tensor instead of permuting the time-major one back"""
    Lr, B = label_LB.shape
    _chk(label_LB, "label", torch.int32)
    blc = torch.empty((B, 1, Lr, ncls), dtype=torch.float32, device=label_LB.device)
    lbc = torch.empty((Lr, B, ncls), dtype=torch.float32, device=label_LB.device)
    L.call("hwg_onehot_both", label_LB, blc, lbc, Lr, B, ncls, _stream())
    lbc._hwg_nhwc = blc
    return lbc


def nhwc_of(content_LBC):
    """the NHWC twin of a time-major tensor made by onehot_both (None for any other tensor, e.g. a slice of it)"""
    twin = getattr(content_LBC, "_hwg_nhwc", None)
    if twin is not None and content_LBC.dim() == 3 and twin.shape[0] == content_LBC.shape[1] and twin.shape[2] == content_LBC.shape[0]:
        return twin
    return None


def stretch_frames(T, scales):
    """host side of stretch_onehot: per scale s the (T_out, r, identity) F.interpolate(x [.., T], scale_factor=s, mode='linear') works with -
    T_out = floor(double(T) * s), r = float32(1 / s), identity = (T_out == T: torch copies its input then, whatever s is). A scale that
    leaves no step is a ValueError."""
    import math
    import numpy as np
    frames = []
    for s in scales:
        s = float(s)
        if not (s > 0.0 and math.isfinite(s)):
            raise ValueError("stretch_onehot: scale %r is not a positive finite number" % s)
        T_out = int(math.floor(float(T) * s))
        if T_out < 1:
            raise ValueError("stretch_onehot: scale %r leaves no step of a line of %d" % (s, T))
        frames.append((T_out, np.float32(1.0 / s), T_out == T))
    return frames


def stretch_onehot(label_TB, ncls, scales, out=None, offsets=None):
    """The stretch film's labels (csrc/stretch.hip): label int32 [T,B] (the aligned line, device or host) -> a list with one time-major
    tensor [T_out,B,ncls] per scale, the one-hot of the line re-sampled along time as F.interpolate(scale_factor=s, mode='linear') does
    on the CPU, bit for bit (stretch_frames); each carries its NHWC rows [B,1,T_out,ncls] as `_hwg_nhwc`, as onehot_both's result does.
    One launch fills all frames; the tensors are views into two ragged fp32 buffers, every frame starting at a multiple of 4 floats.
    The labels and the scales are validated here, before anything is uploaded or launched: a class outside [0, ncls) or a frame without
    steps is a ValueError. `out`: (blc, lbc), two contiguous 1-D fp32 device buffers to write into, with `offsets` = (offsets into blc,
    offsets into lbc): one multiple of 4 per frame, frames inside their buffer and apart from each other; nothing else of the buffers
    is written."""
    import numpy as np
    if not torch.is_tensor(label_TB) or label_TB.dim() != 2 or label_TB.dtype != torch.int32:
        raise L.HwgError("stretch_onehot: label must be an int32 [T,B] tensor")
    T, B = label_TB.shape
    ncls = int(ncls)
    if T < 1 or B < 1 or ncls < 1:
        raise L.HwgError("stretch_onehot: bad sizes T=%d B=%d ncls=%d" % (T, B, ncls))
    frames = stretch_frames(T, scales)
    F = len(frames)
    if F < 1:
        raise ValueError("stretch_onehot: no scales")
    host = label_TB.cpu().numpy()
    if ((host < 0) | (host >= ncls)).any():
        raise ValueError("stretch_onehot: labels must lie in [0, %d), got %d .. %d" % (ncls, host.min(), host.max()))
    sizes = np.asarray([B * f[0] * ncls for f in frames], dtype=np.int64)
    if out is None:
        if offsets is not None:
            raise L.HwgError("stretch_onehot: offsets without out")
        if not label_TB.is_cuda:
            raise L.HwgError("stretch_onehot: a host label needs `out` to name the device")
        off = np.zeros(F, dtype=np.int64)
        np.cumsum((sizes[:-1] + 3) // 4 * 4, out=off[1:])
        offs = (off, off)
        total = int(off[-1] + sizes[-1])
        bufs = (torch.empty((total,), dtype=torch.float32, device=label_TB.device), torch.empty((total,), dtype=torch.float32, device=label_TB.device))
    else:
        bufs = tuple(out)
        if len(bufs) != 2 or offsets is None or len(offsets) != 2:
            raise L.HwgError("stretch_onehot: out = (blc, lbc) goes with offsets = (offsets into blc, offsets into lbc)")
        offs = tuple(np.asarray(o, dtype=np.int64).reshape(-1) for o in offsets)
        for buf, off, name in zip(bufs, offs, ("blc", "lbc")):
            if not torch.is_tensor(buf) or not buf.is_cuda or buf.dtype != torch.float32 or buf.dim() != 1 or not buf.is_contiguous() or buf.data_ptr() % 16:
                raise L.HwgError("stretch_onehot: out %s must be a contiguous, 16-byte aligned 1-D fp32 device buffer" % name)
            if off.shape[0] != F or (off % 4 != 0).any() or (off < 0).any() or (off + sizes > buf.numel()).any():
                raise L.HwgError("stretch_onehot: %s offsets must be %d multiples of 4 with every frame inside the buffer, got %s" % (name, F, off.tolist()))
            order = np.argsort(off, kind="stable")
            if (off[order][1:] < (off + sizes)[order][:-1]).any():
                raise L.HwgError("stretch_onehot: %s frames overlap: offsets %s, sizes %s" % (name, off.tolist(), sizes.tolist()))
    dev = bufs[0].device
    table = np.zeros(F, dtype=np.dtype([("T_out", np.int32), ("r", np.float32), ("identity", np.int32), ("reserved", np.int32),
                                        ("off_blc", np.int64), ("off_lbc", np.int64)]))       # hwg_stretch_frame, 32 bytes
    table["T_out"] = [f[0] for f in frames]
    table["r"] = [f[1] for f in frames]
    table["identity"] = [f[2] for f in frames]
    table["off_blc"], table["off_lbc"] = offs
    table_d = h2d(torch.from_numpy(table.view(np.int64)), dev)          # (int64 words: the records hold 8-byte fields)
    label_d = label_TB.contiguous() if label_TB.is_cuda else h2d(label_TB.contiguous(), dev)
    L.call("hwg_stretch_onehot", label_d, T, B, ncls, table_d, F, max(f[0] for f in frames), bufs[0], bufs[0].numel(), bufs[1],
           bufs[1].numel(), _stream())
    result = []
    for k, (T_out, _, _) in enumerate(frames):
        lbc = bufs[1][int(offs[1][k]):int(offs[1][k]) + int(sizes[k])].view(T_out, B, ncls)
        lbc._hwg_nhwc = bufs[0][int(offs[0][k]):int(offs[0][k]) + int(sizes[k])].view(B, 1, T_out, ncls)
        result.append(lbc)
    return result


def permute4(x, dims, strides):
    out = torch.empty(tuple(dims), dtype=torch.float32, device=x.device)
    L.call("hwg_permute4", x, out, dims[0], dims[1], dims[2], dims[3], strides[0], strides[1], strides[2], strides[3], _stream())
    return out


class _ToNCHW(Function):
    """layout change at the module boundary (NHWC -> NCHW copy); only used for multi-channel boundary tensors"""
    sets = "stacked"

    @staticmethod
    def forward(ctx, x):
        N, H, W, C = x.shape
        return permute4(x, (N, C, H, W), (H * W * C, 1, W * C, C))

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W = dy.shape
        return permute4(dy.contiguous(), (N, H, W, C), (C * H * W, W, 1, H * W))


class _ToNHWC(Function):
    sets = "stacked"

    @staticmethod
    def forward(ctx, x):
        N, C, H, W = x.shape
        return permute4(x, (N, H, W, C), (C * H * W, W, 1, H * W))

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = dy.shape
        return permute4(dy.contiguous(), (N, C, H, W), (H * W * C, 1, W * C, C))


def to_nchw(x):
    if x.shape[3] == 1:
        y = x.reshape(x.shape[0], 1, x.shape[1], x.shape[2])
        return TAPE.alias(y, x) if TAPE is not None else y
    return _ToNCHW.apply(x)


def to_nhwc(x):
    if x.shape[1] == 1:
        y = x.reshape(x.shape[0], x.shape[2], x.shape[3], 1)
        return TAPE.alias(y, x) if TAPE is not None else y
    return _ToNHWC.apply(x.contiguous())


# ----------------------------------------------------------------------------------------------
# sequence ops
# ----------------------------------------------------------------------------------------------
class _LogSoftmaxTB(Function):
    """x [B,1,T,C] (NHWC) -> log-probs [T,B,C]"""

    @staticmethod
    def forward(ctx, x):
        _chk(x, "log_softmax input")
        B, _, T, C = x.shape
        y = torch.empty((T, B, C), dtype=torch.float32, device=x.device)
        L.call("hwg_log_softmax_fwd", x, y, B * T, C, B, T, 1, _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        T, B, C = y.shape
        dx = torch.empty((B, 1, T, C), dtype=torch.float32, device=y.device)
        L.call("hwg_log_softmax_bwd", dy.contiguous(), y, dx, B * T, C, B, T, 1, _stream())
        return dx


def log_softmax_tbc(x):
    return _LogSoftmaxTB.apply(x)


# The beta recursion of the CTC backward pass reads log_probs only, so the forward launch runs it beside alpha (hwg_ctc_fwd_beta) whenever a
# gradient will be asked for, and backward starts at the gradient kernel. False: beta in its own launch at the head of backward (same bits).
CTC_BETA_IN_FWD = True


class _CTC(Function):
    @staticmethod
    def forward(ctx, log_probs, targets, in_len, tg_len):
        _chk(log_probs, "ctc log_probs")
        for t, n in ((targets, "targets"), (in_len, "input lengths"), (tg_len, "target lengths")):
            _chk(t, "ctc " + n, torch.int32)
        T, B, C = log_probs.shape
        Lmax = targets.shape[1]
        nbytes = L.query("hwg_ctc_workspace", T, B, Lmax)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=log_probs.device)  # kept for backward
        loss = torch.empty((), dtype=torch.float32, device=log_probs.device)
        ctx.have_beta = CTC_BETA_IN_FWD and ctx.needs_input_grad[0]
        L.call("hwg_ctc_fwd_beta" if ctx.have_beta else "hwg_ctc_fwd", log_probs, targets, in_len, tg_len, T, B, C, Lmax, loss, ws, ws.numel(),
               _stream())
        ctx.save_for_backward(log_probs, targets, in_len, tg_len, ws)
        return loss

    @staticmethod
    def backward(ctx, gout):
        log_probs, targets, in_len, tg_len, ws = ctx.saved_tensors
        T, B, C = log_probs.shape
        grad = torch.empty_like(log_probs)
        L.call("hwg_ctc_bwd_grad" if ctx.have_beta else "hwg_ctc_bwd", log_probs, targets, in_len, tg_len, T, B, C, targets.shape[1],
               gout.contiguous(), grad, ws, ws.numel(), _stream())
        return grad, None, None, None


def ctc_loss(log_probs, targets, input_lengths, target_lengths):
    """F.ctc_loss(blank=0, reduction='mean') with an infinite result reported as 0 (model/loss.py:28-30).
    targets [B, Lmax]; lengths may be host tensors / lists (they are host data in the reference too)."""
    dev = log_probs.device
    targets = h2d(targets, dev, torch.int32).contiguous()
    il = h2d(torch.as_tensor(input_lengths, dtype=torch.int32), dev)
    tl = h2d(torch.as_tensor(target_lengths, dtype=torch.int32), dev)
    return _CTC.apply(log_probs.contiguous(), targets, il, tl)


class DTWPending:
    """alignment kernel already enqueued; `.result()` waits (side-stream copy) only for the path lengths"""

    def __init__(self, out, lens):
        self.out, self.lens = out, lens
        self.fetch = AsyncFetch(lens)

    def result(self):
        maxlen = int(self.fetch.get().max())
        return self.out[:maxlen].contiguous(), self.lens


def dtw_align_async(pred_TBC, label_LB):
    _chk(pred_TBC, "dtw pred")
    T, B, C = pred_TBC.shape
    label = h2d(label_LB, pred_TBC.device, torch.int32).contiguous()
    Lr = label.shape[0]
    out = torch.empty((T + 2 * Lr + 1, B), dtype=torch.int64, device=pred_TBC.device)
    lens = torch.empty((B,), dtype=torch.int32, device=pred_TBC.device)
    ws = torch.empty(L.query("hwg_dtw_workspace", T, B, Lr), dtype=torch.uint8, device=pred_TBC.device)   # private: outlives this call
    L.call("hwg_dtw_align", pred_TBC, label, T, B, C, Lr, out, lens, ws, ws.numel(), _stream())
    return DTWPending(out, lens)


def dtw_align(pred_TBC, label_LB):
    """correct_pred: returns (aligned int64 [maxlen,B], lens[B]); one D2H wait for the path length."""
    return dtw_align_async(pred_TBC, label_LB).result()


def gt_counts(index_spaced, label_LB):
    """run-length scan of an aligned label sequence -> (gt_counts [L,B,2], min pos)"""
    Tp, B = index_spaced.shape
    label = h2d(label_LB, index_spaced.device, torch.int32).contiguous()
    Lr = label.shape[0]
    gt = torch.zeros((Lr, B, 2), dtype=torch.float32, device=index_spaced.device)
    meta = h2d(torch.tensor([2 ** 31 - 1, 0], dtype=torch.int32), index_spaced.device)
    L.call("hwg_gt_counts", index_spaced.contiguous(), label, Tp, B, Lr, gt, meta[0:1], meta[1:2], _stream())
    return gt, meta


def argmax_rows(x2d):
    rows, C = x2d.shape
    out = torch.empty((rows,), dtype=torch.int32, device=x2d.device)
    L.call("hwg_argmax_rows", x2d, out, rows, C, _stream())
    return out


# ----------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------
LOSS_L1, LOSS_MSE, LOSS_MEAN, LOSS_HINGE_REAL, LOSS_HINGE_FAKE = 0, 1, 2, 3, 4


class _Loss(Function):
    @staticmethod
    def forward(ctx, a, b, mode, scale):
        _chk(a, "loss input"); _chk(b, "loss target")
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ws = workspace(L.query("hwg_loss_workspace"), a.device)
        L.call("hwg_loss_fwd", a, b, a.numel(), mode, scale, out, 0, ws, ws.numel(), _stream())
        ctx.save_for_backward(a, b)
        ctx.cfg = (mode, scale)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        mode, scale = ctx.cfg
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if (b is not None and ctx.needs_input_grad[1]) else None
        if da is None and db is None:
            return None, None, None, None
        L.call("hwg_loss_bwd", a, b, a.numel(), mode, scale, gout.contiguous(), da, db, 0, _stream())
        return da, db, None, None


def l1_loss(a, b):
    return _Loss.apply(a.contiguous(), b.contiguous(), LOSS_L1, 1.0)


def mse_loss(a, b):
    return _Loss.apply(a.contiguous(), b.contiguous(), LOSS_MSE, 1.0)


def mean_loss(a, mode=LOSS_MEAN, scale=1.0):
    return _Loss.apply(a.contiguous(), None, mode, scale)


class _MaskedL1(Function):
    @staticmethod
    def forward(ctx, recon, image, mask):
        B, _, H, W = recon.shape
        out = torch.empty((), dtype=torch.float32, device=recon.device)
        ws = workspace(L.query("hwg_loss_workspace"), recon.device)
        L.call("hwg_masked_l1_fwd", recon, image, mask, B * H, W, mask.shape[3], out, ws, ws.numel(), _stream())
        ctx.save_for_backward(recon, image, mask)
        return out

    @staticmethod
    def backward(ctx, gout):
        recon, image, mask = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        B, _, H, W = recon.shape
        dr = torch.empty_like(recon)
        L.call("hwg_masked_l1_bwd", recon, image, mask, B * H, W, mask.shape[3], gout.contiguous(), dr, _stream())
        return dr, None, None


def masked_l1_loss(recon, image, mask):
    """The foreground-only reconstruction loss (reference trainer :596-601): mean over all B*H*W elements of |recon * mask - image * mask|,
    each product rounded to fp32 like the reference's two multiplications. recon, image [B,1,H,W]; mask [B,1,H,Wm] with Wm <= W, columns
    >= Wm count as 0 (the reference pads the mask with zeros when it pads the image). A mask of ones gives the bits of l1_loss, value and
    gradient. The gradient goes to `recon` only: image and mask are data."""
    for t, name in ((recon, "masked_l1_loss recon"), (image, "masked_l1_loss image"), (mask, "masked_l1_loss mask")):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 1:
            raise L.HwgError("%s must be a [B,1,H,W] tensor" % name)
    recon, image, mask = recon.contiguous(), image.contiguous(), mask.contiguous()
    _chk(recon, "masked_l1_loss recon"); _chk(image, "masked_l1_loss image"); _chk(mask, "masked_l1_loss mask")
    if image.shape != recon.shape:
        raise L.HwgError("masked_l1_loss: recon %s and image %s differ in shape" % (tuple(recon.shape), tuple(image.shape)))
    if mask.shape[0] != recon.shape[0] or mask.shape[2] != recon.shape[2] or not (1 <= mask.shape[3] <= recon.shape[3]):
        raise L.HwgError("masked_l1_loss: mask %s does not fit the images %s (same lines and rows, 1 <= Wm <= W)" % (tuple(mask.shape), tuple(recon.shape)))
    if image.requires_grad or mask.requires_grad:
        raise L.HwgError("masked_l1_loss: image and mask are data, no gradient flows to them")
    return _MaskedL1.apply(recon, image, mask)


# ----------------------------------------------------------------------------------------------
# spectral norm
# ----------------------------------------------------------------------------------------------
class _SpectralScale(Function):
    """W_sn = W_bar / sigma with sigma = u^T W v treated as a function of W_bar (u, v constants) - discriminator_ap.py:31-32"""

    @staticmethod
    def forward(ctx, w_bar, u, v, sigma, inv_sigma, lazy):
        out = torch.empty_like(w_bar)
        if not lazy:          # lazy: every image the convolutions need comes from the bank's scaled multi-pack; the tensor itself is only a handle
            L.call("hwg_scale_by_ptr", w_bar, inv_sigma, out, w_bar.numel(), _stream())
        ctx.save_for_backward(w_bar, u, v, sigma)
        ctx.leaf = w_bar if isinstance(w_bar, torch.nn.Parameter) and w_bar.requires_grad else None
        return out

    @staticmethod
    def backward(ctx, dwsn):
        w_bar, u, v, sigma = ctx.saved_tensors
        R = w_bar.shape[0]
        K = w_bar.numel() // R
        ws = workspace(L.query("hwg_spectral_workspace", R, K), w_bar.device)
        if ctx.leaf is not None:
            # W_bar is a parameter: its gradient is added where parameter gradients live (the current set or the redirected one), like the
            # convolutions' - returning it would cost the autograd engine an add_ launch per layer and would not follow ops.grad_set
            dst = _grad_buffer(ctx.leaf)
            if DEFER_REDUCE:
                # nothing reads a parameter gradient before the join behind the backward pass: the layers of a network are queued and walk
                # backward together there, two launches instead of two per layer (flush_deferred_reduce -> hwg_spectral_bwd_multi)
                _sn_defer.append((dwsn.contiguous(), w_bar, u, v, sigma, dst, R, K))
                return None, None, None, None, None, None
            L.call("hwg_spectral_bwd", dwsn.contiguous(), w_bar, u, v, sigma, dst, R, K, 1, ws, ws.numel(), _stream())
            return None, None, None, None, None, None
        dwbar = torch.empty_like(w_bar)
        L.call("hwg_spectral_bwd", dwsn.contiguous(), w_bar, u, v, sigma, dwbar, R, K, 0, ws, ws.numel(), _stream())
        return dwbar, None, None, None, None, None


def spectral_normalize(w_bar, u, v, eps=1e-12):
    """one power iteration (u, v updated in place, like the reference does on every forward) and W/sigma"""
    R = w_bar.shape[0]
    K = w_bar.numel() // R
    sig = torch.empty((2,), dtype=torch.float32, device=w_bar.device)
    ws = workspace(L.query("hwg_spectral_workspace", R, K), w_bar.device)
    # the kernels that update u and v in place also write the snapshot this forward's backward pass will read (the reference clones them)
    un, vn = torch.empty_like(u), torch.empty_like(v)
    with torch.no_grad():
        L.call("hwg_spectral_update_to", w_bar.detach(), u, v, un, vn, R, K, eps, sig[0:1], sig[1:2], ws, ws.numel(), _stream())
    w = _SpectralScale.apply(w_bar, un, vn, sig[0:1], sig[1:2], False)
    w._hwg_sn_defer = isinstance(w_bar, torch.nn.Parameter) and w_bar.requires_grad
    return w


class _Prepack:
    """images of one spectral-norm layer's normalised weight for one forward pass (`images`: variant -> tensor), and what to do on a miss"""

    __slots__ = ("images", "bank", "layer", "w_bar", "inv_sigma", "materialised")

    def __init__(self, images, bank, layer, w_bar, inv_sigma, materialised):
        self.images, self.bank, self.layer, self.w_bar, self.inv_sigma, self.materialised = images, bank, layer, w_bar, inv_sigma, materialised

    def miss(self, variant, weight):
        self.bank.request(self.layer, variant)
        if not self.materialised:      # the handle has no values yet: W_bar / sigma into it now, the ordinary pack follows
            with torch.no_grad():
                L.call("hwg_scale_by_ptr", self.w_bar, self.inv_sigma, weight, weight.numel(), _stream())
            self.materialised = True


class SpectralBank:
    """The power iterations of all spectral-norm layers a network runs in one forward pass, as four launches (hwg_spectral_update_multi)
    instead of four per layer. Built once per (network, set of layers): the parameters' storage is persistent, only the snapshot buffer and
    the sigma outputs are fresh per forward."""

    def __init__(self, layers):
        import numpy as np
        self.layers = list(layers)                 # [(w_bar, u, v)] parameters
        rec = np.zeros(len(self.layers), dtype=np.dtype([("W", "<u8"), ("u", "<u8"), ("v", "<u8"), ("copy_off", "<i8"), ("ws_off", "<i8"), ("R", "<i4"), ("K", "<i4")]))
        off = 0
        self.spans = []
        for i, (w, u, v) in enumerate(self.layers):
            R = w.shape[0]
            K = w.numel() // R
            rec[i] = (w.data_ptr(), u.data_ptr(), v.data_ptr(), off, off, R, K)
            self.spans.append((off, R, K))
            off += (R + K + 3) // 4 * 4
        self.total = off
        self.max_R = max(R for _, R, _ in self.spans)
        self.max_K = max(K for _, _, K in self.spans)
        self.ptrs = [(w.data_ptr(), u.data_ptr(), v.data_ptr()) for w, u, v in self.layers]
        dev = self.layers[0][0].device
        self.table = h2d(torch.from_numpy(rec.view(np.uint8)), dev)
        self.ws = torch.empty(self.total, dtype=torch.float32, device=dev)
        # scaled multi-pack: the weight images the layers' convolutions asked for so far, (layer, variant) in request order
        self.requests = []
        self._ptab = None
        self.prepack = bool(int(os.environ.get("HWG_SN_PREPACK", "1") or 0))

    def request(self, layer, variant):
        if (layer, variant) not in self.requests:
            self.requests.append((layer, variant))
            self._ptab = None

    def _pack_table(self):
        import numpy as np
        if self._ptab is None:
            dt = np.dtype([("src", "<u8"), ("dst", "<u8"), ("A", "<i4"), ("B", "<i4"), ("Bpad", "<i4"), ("R", "<i4"), ("S", "<i4"), ("flip", "<i4"),
                           ("sa", "<i8"), ("sb", "<i8"), ("sr", "<i8"), ("ss", "<i8"), ("total", "<i8"), ("first_block", "<i8"),
                           ("mode", "<i4"), ("Apad", "<i4"), ("dst_off", "<i8"), ("scale_idx", "<i4"), ("pad", "<i4")])
            assert dt.itemsize == 112
            host = np.zeros(len(self.requests), dtype=dt)
            blocks = off = 0
            spans = []
            for i, (layer, (A, B, Bpad, R, S, sa, sb, flip, wino, Apad)) in enumerate(self.requests):
                total = Apad * Bpad if wino else R * S * A * Bpad
                host[i] = (self.layers[layer][0].data_ptr(), 0, A, B, Bpad, R, S, flip, sa, sb, S, 1, total, blocks, wino, Apad, off, 2 * layer + 1, 0)
                shape = (Bpad // 16, 16, Apad, 16) if wino else (R * S, A, Bpad)
                floats = 16 * Apad * Bpad if wino else total        # (Winograd: one thread per (a, b) pair writes its 16 positions)
                spans.append((off, floats, shape))
                blocks += (total + PACK_PER_BLOCK - 1) // PACK_PER_BLOCK
                off += (floats + 3) // 4 * 4
            self._ptab = (h2d(torch.from_numpy(host.view(np.uint8)), self.ws.device), blocks, off, spans)
        return self._ptab

    def valid(self):
        return all((w.data_ptr(), u.data_ptr(), v.data_ptr()) == p for (w, u, v), p in zip(self.layers, self.ptrs))

    def update(self, eps=1e-12):
        """-> per layer (u snapshot, v snapshot, sigma[0:1], sigma[1:2]) for `spectral_scale`"""
        dev = self.ws.device
        copies = torch.empty(self.total, dtype=torch.float32, device=dev)
        sig = torch.empty(2 * len(self.layers), dtype=torch.float32, device=dev)
        with torch.no_grad():
            L.call("hwg_spectral_update_multi", self.table, len(self.layers), self.max_R, self.max_K, eps, self.ws, copies, sig, _stream())
        images = [{} for _ in self.layers]
        if self.prepack and self.requests:
            tab, blocks, total, spans = self._pack_table()
            buf = torch.empty(total, dtype=torch.float32, device=dev)
            with torch.no_grad():
                L.call("hwg_conv_pack_weight_multi_scaled", tab, len(self.requests), blocks, buf, sig, _stream())
            for (layer, variant), (off, n, shape) in zip(self.requests, spans):
                images[layer][variant] = buf[off: off + n].view(shape)
        out = []
        for i, (off, R, K) in enumerate(self.spans):
            inv = sig[2 * i + 1: 2 * i + 2]
            pre = _Prepack(images[i], self, i, self.layers[i][0], inv, False) if self.prepack else None
            out.append((copies[off: off + R], copies[off + R: off + R + K], sig[2 * i: 2 * i + 1], inv, pre))
        return out


def spectral_scale(w_bar, fresh):
    """W / sigma from a SpectralBank.update() record (the power iteration already ran). With the bank's scaled multi-pack on, the returned
    tensor is a handle: the images the convolutions need were written by that launch and hang on the handle (`_hwg_prepack`); its own
    values are only computed if a convolution asks for an image the bank has not seen yet."""
    un, vn, sigma, inv_sigma, pre = fresh
    lazy = pre is not None and len(pre.images) > 0
    w = _SpectralScale.apply(w_bar, un, vn, sigma, inv_sigma, lazy)
    # read by _Conv2d._wgrad: with deferral on, this weight's gradient is consumed at the flush behind the backward pass (_SpectralScale.backward)
    w._hwg_sn_defer = isinstance(w_bar, torch.nn.Parameter) and w_bar.requires_grad
    if pre is not None:
        pre.materialised = not lazy
        w._hwg_prepack = pre
    return w


# ----------------------------------------------------------------------------------------------
# style extraction helpers
# ----------------------------------------------------------------------------------------------
class _GatherWindows(Function):
    @staticmethod
    def forward(ctx, x, idx_b, idx_pos, window):
        _chk(x, "window source")
        B, Wx, C = x.shape
        n = idx_b.numel()
        out = torch.empty((n, 1, 2 * window + 1, C), dtype=torch.float32, device=x.device)
        L.call("hwg_gather_windows", x, B, Wx, C, idx_b, idx_pos, n, window, out, _stream())
        ctx.save_for_backward(idx_b, idx_pos)
        ctx.cfg = (B, Wx, C, n, window)
        return out

    @staticmethod
    def backward(ctx, dy):
        idx_b, idx_pos = ctx.saved_tensors
        B, Wx, C, n, window = ctx.cfg
        dx = torch.empty((B, Wx, C), dtype=torch.float32, device=dy.device)
        win_of = torch.empty((B * Wx,), dtype=torch.int32, device=dy.device)
        L.call("hwg_scatter_windows", dy.contiguous(), B, Wx, C, idx_b, idx_pos, n, window, win_of, dx, _stream())
        return dx, None, None, None


def gather_windows(x_BWC, idx_b, idx_pos, window):
    """patches[i] = x[idx_b[i], idx_pos[i]-window : idx_pos[i]+window+1, :] (zero outside). PRECONDITION of the deterministic backward
    (hwg_scatter_windows inverts the window list instead of scattering with atomics): the centres (idx_b[i], idx_pos[i]) are unique - true for
    the caller (CharStyleEncoder: one arg-max class per column). HWG_DEBUG=1 checks it on the host."""
    if os.environ.get("HWG_DEBUG"):
        key = (idx_b.long() * x_BWC.shape[1] + idx_pos.long()).cpu()
        assert key.unique().numel() == key.numel(), "gather_windows: duplicate window centres (their gradients would be dropped)"
        assert int(idx_pos.min()) >= 0 and int(idx_pos.max()) < x_BWC.shape[1] and int(idx_b.min()) >= 0 and int(idx_b.max()) < x_BWC.shape[0]
    return _GatherWindows.apply(x_BWC, idx_b, idx_pos, window)


class _SegMean(Function):
    @staticmethod
    def forward(ctx, v, wgt, seg, B):
        n, C = v.shape
        out = torch.empty((B, C), dtype=torch.float32, device=v.device)
        wsum = torch.empty((B,), dtype=torch.float32, device=v.device)
        L.call("hwg_segment_weighted_mean", v, wgt, seg, n, C, B, out, wsum, _stream())
        ctx.save_for_backward(wgt, seg, wsum)
        ctx.cfg = (n, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        wgt, seg, wsum = ctx.saved_tensors
        n, C = ctx.cfg
        dv = torch.empty((n, C), dtype=torch.float32, device=dout.device)
        L.call("hwg_segment_weighted_mean_bwd", dout.contiguous(), wgt, seg, wsum, n, C, dv, _stream())
        return dv, None, None, None


def segment_weighted_mean(v, wgt, seg, B):
    return _SegMean.apply(v.contiguous(), wgt, seg, B)


def gather_scores(x_BWC, idx_b, idx_pos, idx_cls):
    n = idx_b.numel()
    out = torch.empty((n,), dtype=torch.float32, device=x_BWC.device)
    B, Wx, C = x_BWC.shape
    L.call("hwg_gather_scores", x_BWC, B, Wx, C, idx_b, idx_pos, idx_cls, n, out, _stream())
    return out


# ----------------------------------------------------------------------------------------------
# random numbers (device Philox; parity tests inject host-drawn tensors instead)
# ----------------------------------------------------------------------------------------------
class DeviceRNG:
    def __init__(self, seed=0):
        self.seed = int(seed)
        self.offset = 0
        self.text_offset = 0      # `insert_spaces` draws from its own Philox stream (seed + 1): the pipelined generation loop plans request
        # i+1 before it renders request i, and both orders must consume the noise stream and the text stream identically

    def randn(self, shape, device):
        out = torch.empty(shape, dtype=torch.float32, device=device)
        n = out.numel()
        L.call("hwg_randn", out, n, self.seed, self.offset, _stream())
        self.offset += (n + 3) // 4
        return out

    def insert_spaces_begin(self, counts, label, label_lengths, count_std, dup_std, count_duplicates):
        """device `insert_spaces`, first half: counts [L,B,2] float, label [L,B] int32, label_lengths [B] int32 (all on the GPU); draws the plan
        and starts the small device->host copy of the expanded lengths that will size the result"""
        Lc, B = label.shape
        dev = counts.device
        reps = torch.empty((B, 2 * Lc), dtype=torch.int32, device=dev)
        starts = torch.empty((B, Lc), dtype=torch.int32, device=dev)
        lens_max = torch.empty((B + 1,), dtype=torch.int32, device=dev)
        L.call("hwg_insert_spaces_plan", counts.contiguous(), label_lengths, Lc, B, float(count_std), float(dup_std), int(bool(count_duplicates)),
               self.seed + 1, self.text_offset, reps, starts, lens_max, _stream())
        self.text_offset += Lc * B
        return (label, label_lengths, reps, starts, AsyncFetch(lens_max))

    def insert_spaces_finish(self, plan):
        """-> (idx int32 [T,B] on the GPU, padded fractions)"""
        label, label_lengths, reps, starts, fetch = plan
        Lc, B = label.shape
        host = fetch.get().tolist()
        lens, max_count = host[:B], host[B]
        T = max(lens) + max_count
        idx = torch.zeros((T, B), dtype=torch.int32, device=label.device)
        L.call("hwg_insert_spaces_fill", label, label_lengths, reps, starts, Lc, B, T, idx, _stream())
        return idx, [(T - n) / T for n in lens]

    def dropmask(self, shape, p, device):
        out = torch.empty(shape, dtype=torch.float32, device=device)
        n = out.numel()
        L.call("hwg_dropmask", out, n, float(p), self.seed, self.offset, _stream())
        self.offset += (n + 3) // 4
        return out


    def dropmask_multi(self, counts, ps, device):
        """the feature-dropout masks of one network pass from ONE launch: counts[j] elements (multiples of 4) with drop probability ps[j], back
        to back in one buffer -> list of flat views; the values (and the stream position afterwards) are those of consecutive dropmask calls"""
        import numpy as np
        total = int(sum(counts))
        out = torch.empty((total,), dtype=torch.float32, device=device)
        ne = np.asarray(counts, dtype=np.int64); pp = np.asarray(ps, dtype=np.float32)
        L.call("hwg_dropmask_multi", out, len(counts), ne.ctypes.data, pp.ctypes.data, self.seed, self.offset, _stream())
        self.offset += total // 4
        views, off = [], 0
        for n in counts:
            views.append(out[off: off + n]); off += n
        return views


# ----------------------------------------------------------------------------------------------
# line augmentation of the recogniser pre-training: Tensmeyer brightness + mesh warp on the collated batch (csrc/augment.hip)
# ----------------------------------------------------------------------------------------------
AUG_STATS = 258          # per line: Otsu threshold, border level, LUT[256]
AUG_BRIGHT_SIGMA = 30.0  # utils/augmentation.py:24


def warp_lattice(h, w, interval=12):
    """control lattice of grid_distortion.warp_image (:25-41) -> (src_y [gy], src_x [gx]) fp64: intervals fitted to the image, np.mgrid
    with a float step (the same numpy expression as the reference, so the end points come out the same)"""
    import numpy as np
    w_ratio = max(1, round(w / float(interval)))
    h_ratio = max(1, round(h / float(interval)))
    wi, hi = w / w_ratio, h / h_ratio
    src = np.mgrid[0:h + hi:hi, 0:w + wi:wi]
    return src[0][:, 0].copy(), src[1][0, :].copy()


class LineMesh:
    """the control lattices of one batch of lines of height H: widths [B] valid columns per line, x_off [B] first valid column (0 unless
    the batch is centre padded), sigma (scalar or [B]) of the displacements, warp / bright [B] flags (the "low" variant skips either per
    line); lines of H <= 5 or w <= 5 are not warped (grid_distortion.py:12). disp: None = unit draws from the device generator, or per
    line (disp_y [gy, gx], disp_x [gy, gx]) explicit displacements (None for an unwarped line) - the teacher-forced path of the tests."""

    def __init__(self, H, widths, sigma=1.5, x_off=None, warp=None, bright=None, disp=None):
        import numpy as np
        self.H, self.widths = int(H), [int(w) for w in widths]
        B = len(self.widths)
        self.x_off = [0] * B if x_off is None else [int(v) for v in x_off]
        self.sigma = [float(s) for s in (np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B,)))]
        self.bright = [True] * B if bright is None else [bool(v) for v in bright]
        warp = [True] * B if warp is None else [bool(v) for v in warp]
        self.src = [warp_lattice(self.H, w) if (warp[b] and self.H > 5 and w > 5) else None for b, w in enumerate(self.widths)]
        self.GY = max([len(s[0]) for s in self.src if s is not None] or [0])
        self.GX = max([len(s[1]) for s in self.src if s is not None] or [0])
        self.disp = disp
        if disp is not None:
            for s, d in zip(self.src, disp):
                assert (s is None) or (d is not None and tuple(d[0].shape) == tuple(d[1].shape) == (len(s[0]), len(s[1]))), "displacements do not fit the lattice"

    def tables(self, explicit_fg_bg=None):
        """-> (lines_i int32 [B,4], lines_f float32 [B, 4+GY+GX], draws float32 [B, 2+2*GY*GX] or None when the draws are made on the device)"""
        import numpy as np
        B, GY, GX = len(self.widths), self.GY, self.GX
        explicit = explicit_fg_bg is not None
        assert explicit == (self.disp is not None), "explicit brightness draws and explicit displacements go together"
        li = np.zeros((B, 4), dtype=np.int32)
        lf = np.zeros((B, 4 + GY + GX), dtype=np.float32)
        dr = np.zeros((B, 2 + 2 * GY * GX), dtype=np.float32) if explicit else None
        for b in range(B):
            s = self.src[b]
            li[b] = (self.widths[b], 0 if s is None else len(s[0]), 0 if s is None else len(s[1]), self.x_off[b])
            if explicit:
                lf[b, :4] = 1.0
                if self.bright[b]:
                    dr[b, :2] = explicit_fg_bg[b]
            else:
                lf[b, :2] = AUG_BRIGHT_SIGMA if self.bright[b] else 0.0
                lf[b, 2:4] = self.sigma[b]
            if s is not None:
                gy, gx = len(s[0]), len(s[1])
                lf[b, 4:4 + gy] = s[0]
                lf[b, 4 + GY:4 + GY + gx] = s[1]
                if explicit:
                    dr[b, 2:2 + gy * gx] = np.asarray(self.disp[b][0]).reshape(-1)
                    dr[b, 2 + gy * gx:2 + 2 * gy * gx] = np.asarray(self.disp[b][1]).reshape(-1)
        return li, lf, dr


def augment_lines(image, mesh, fg_bg=None, want_map=False, rng=None):
    """Brightness + mesh warp of every line of the collated batch `image` [B,1,H,W] (device, fp32: 1 - level/128, padding -1) in two launches
    (hwg_augment_stats, hwg_augment_warp) -> a new tensor of the same shape. fg_bg None: the brightness shifts N(0, 30) and the
    displacements N(0, sigma) are unit draws of `rng` (a DeviceRNG; one hwg_randn launch, the stream offset advances); fg_bg [B,2]
    (host): explicit shifts, with the explicit displacements of `mesh.disp`. want_map: -> (y, map [B,2,H,W] = (map_y, map_x) in line
    coordinates, NaN outside the mesh, stats int32 [B,258] = (threshold, border level, LUT))."""
    B, C, H, W = image.shape
    assert C == 1 and H == mesh.H and B == len(mesh.widths) and image.is_cuda and image.dtype == torch.float32
    assert all(0 <= o and w >= 0 and o + w <= W for o, w in zip(mesh.x_off, mesh.widths)), "line extents outside the batch"
    image = image.contiguous()
    dev = image.device
    li, lf, dr = mesh.tables(fg_bg)
    if dr is None:
        if rng is None:
            raise L.HwgError("augment_lines: no explicit draws and no device generator")
        draws = rng.randn((B, 2 + 2 * mesh.GY * mesh.GX), dev)
    else:
        draws = h2d(dr, dev)
    li_d, lf_d = h2d(li, dev), h2d(lf, dev)
    stats = torch.empty((B, AUG_STATS), dtype=torch.int32, device=dev)
    y = torch.empty_like(image)
    map_out = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if want_map else None
    st = _stream()
    L.call("hwg_augment_stats", image, li_d, lf_d, lf.shape[1], draws, draws.shape[1], B, H, W, stats, st)
    L.call("hwg_augment_warp", image, li_d, lf_d, lf.shape[1], draws, draws.shape[1], stats, B, H, W, mesh.GY, mesh.GX, y, map_out, st)
    return (y, map_out, stats) if want_map else y


# ----------------------------------------------------------------------------------------------
# generated lines as 8-bit grey pictures, ragged (csrc/lines_out.hip)
# ----------------------------------------------------------------------------------------------
def lines_to_u8(img, widths, out=None, offsets=None):
    """The generator's image `img` [B,1,H,W] (device, fp32 in [-1, 1]) -> (pixels, offsets): `pixels` a uint8 1-D device tensor in which
    line b is the finished H x widths[b] grey picture pixels[offsets[b]:offsets[b + 1]] (the reference's ((1 - im) * 127.5).astype(uint8),
    cut to the line's own width), `offsets` a host int64 [B+1] array. `widths` is a host list / array: multiples of 4 in [4, W], validated
    here, before anything is uploaded or launched. `out`: a uint8 device buffer of at least offsets[B] bytes to write into; `offsets`
    [B+1] places the lines explicitly (multiples of 4; offsets[B] = the bytes in use) instead of back to back."""
    import numpy as np
    if img.dim() != 4 or img.shape[1] != 1 or not img.is_cuda or img.dtype != torch.float32:
        raise L.HwgError("lines_to_u8: img must be a [B,1,H,W] fp32 device tensor, got %s %s" % (tuple(img.shape), img.dtype))
    B, _, H, W = img.shape
    w = np.asarray(widths, dtype=np.int64).reshape(-1)
    if B < 1 or w.shape[0] != B:
        raise L.HwgError("lines_to_u8: %d widths for a batch of %d lines" % (w.shape[0], B))
    if W % 4:
        raise L.HwgError("lines_to_u8: image width %d is not a multiple of 4" % W)
    if ((w < 4) | (w > W) | (w % 4 != 0)).any():
        raise L.HwgError("lines_to_u8: widths must be multiples of 4 in [4, %d], got %s" % (W, w.tolist()))
    if offsets is None:
        offsets = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(H * w, out=offsets[1:])          # multiples of 4, as the kernel's 32-bit stores need
    else:
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.shape[0] != B + 1 or (offsets % 4 != 0).any() or (offsets[:B] < 0).any() or (offsets[:B] + H * w > offsets[B]).any():
            raise L.HwgError("lines_to_u8: offsets must be %d multiples of 4 with every line inside [0, offsets[B]), got %s" % (B + 1, offsets.tolist()))
    total = int(offsets[B])
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=img.device)
    elif not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < total:
        raise L.HwgError("lines_to_u8: out must be a contiguous uint8 device buffer of at least %d bytes" % total)
    table = np.empty(3 * B, dtype=np.int32)      # offsets [B] int64 first (8-byte aligned), then widths [B] int32: one upload
    table[:2 * B].view(np.int64)[:] = offsets[:B]
    table[2 * B:] = w
    table_d = h2d(table, img.device)
    L.call("hwg_lines_to_u8", img.contiguous(), B, H, W, table_d[2 * B:], table_d[:2 * B], out, _stream())
    return out[:total], offsets


def lines_from_u8(pixels, offsets, widths, select, real=None, out=None, height=64):
    """The inverse of lines_to_u8, mixed with a real batch: -> a collated fp32 device batch [B,1,H,W] whose row b is line select[b] = k >= 0
    of the ragged pool (`pixels` uint8 1-D device tensor, `offsets` / `widths` host arrays: line k is the H x widths[k] picture at
    pixels[offsets[k]:], the layout lines_to_u8 writes) as 1 - p / 128, padded with -1, or row r of `real` [Br,1,H,Wr] (device fp32, any
    Wr) for select[b] = -1 - r. H is real's, or `height` without one. W = max(Wr, selected widths) rounded up to a multiple of 4. One launch
    (hwg_lines_from_u8) writes every element. The host tables are validated here, before anything is uploaded or launched. `out`: a
    contiguous fp32 device buffer of at least B * H * W elements to write into (16-byte aligned); the returned tensor is a view of it."""
    import numpy as np
    if not torch.is_tensor(pixels) or not pixels.is_cuda or pixels.dtype != torch.uint8 or pixels.dim() != 1 or not pixels.is_contiguous():
        raise L.HwgError("lines_from_u8: pixels must be a contiguous 1-D uint8 device tensor")
    if pixels.data_ptr() % 4:
        raise L.HwgError("lines_from_u8: pixels must be 4-byte aligned")
    H, Br, Wr = int(height), 0, 0
    if real is not None:
        if real.dim() != 4 or real.shape[1] != 1 or not real.is_cuda or real.dtype != torch.float32 or real.shape[0] < 1 or real.shape[3] < 1:
            raise L.HwgError("lines_from_u8: real must be a [Br,1,H,Wr] fp32 device tensor, got %s %s" % (tuple(real.shape), real.dtype))
        real = real.contiguous()
        Br, _, H, Wr = real.shape
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    w = np.asarray(widths, dtype=np.int64).reshape(-1)
    sel = np.asarray(select, dtype=np.int64).reshape(-1)
    n, B = w.shape[0], sel.shape[0]
    if B < 1:
        raise L.HwgError("lines_from_u8: empty select")
    if off.shape[0] < n:
        raise L.HwgError("lines_from_u8: %d offsets for %d widths" % (off.shape[0], n))
    if ((sel >= n) | (sel < -Br)).any():
        raise L.HwgError("lines_from_u8: select entries must lie in [%d, %d), got %s" % (-Br, n, sel.tolist()))
    used = np.unique(sel[sel >= 0])               # only the selected lines are checked and uploaded: the pool may hold thousands
    uw, uo = w[used], off[used]
    if ((uw < 4) | (uw % 4 != 0)).any():
        raise L.HwgError("lines_from_u8: widths must be positive multiples of 4, got %s" % uw.tolist())
    if ((uo < 0) | (uo % 4 != 0) | (uo + H * uw > pixels.numel())).any():
        raise L.HwgError("lines_from_u8: offsets must be multiples of 4 with every line inside the %d bytes of pixels, got %s" % (pixels.numel(), uo.tolist()))
    W = -(-max(Wr, int(uw.max()) if used.size else 0) // 4) * 4
    if out is None:
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=pixels.device)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < B * H * W
          or out.data_ptr() % 16):
        raise L.HwgError("lines_from_u8: out must be a contiguous 16-byte aligned fp32 device buffer of at least %d elements" % (B * H * W))
    m = max(int(used.size), 1)
    table = np.zeros(3 * m + B, dtype=np.int32)   # offsets [m] int64 first (8-byte aligned), then widths [m] and select [B] int32: one upload
    table[:2 * m].view(np.int64)[:used.size] = uo
    table[2 * m:2 * m + used.size] = uw
    table[3 * m:] = np.where(sel >= 0, np.searchsorted(used, sel), sel)      # pool indices renumbered to the uploaded lines
    table_d = h2d(table, pixels.device)
    L.call("hwg_lines_from_u8", pixels, pixels.numel(), table_d[:2 * m], table_d[2 * m:3 * m], int(used.size), table_d[3 * m:], int(sel.min()),
           real, Br, Wr, B, H, W, out, _stream())
    return out.view(-1)[:B * H * W].view(B, 1, H, W)


# ----------------------------------------------------------------------------------------------
# line images of any height fitted to the recognisers' height, PIL's bytes (csrc/fit_lines.hip)
# ----------------------------------------------------------------------------------------------
FIT_MAX_IN_H, FIT_MAX_H, FIT_MAX_W, FIT_MAX_B = 1024, 1024, 1 << 20, 65535      # the limits hwg_fit_lines checks
fit_fallbacks = 0                                        # lines (or, for a batch beyond the limits, batches) fitted on the host (tests read it)
_fit_fallback_said = False


def _fit_said(why):
    global _fit_fallback_said
    if not _fit_fallback_said:
        _fit_fallback_said = True
        import sys
        print("fit_lines: %s; such lines are fitted on the host" % why, file=sys.stderr)


def fit_lines(images, height=64, W=None, out=None, device=None):
    """Grey line pictures of any height and width - a list of 2-D uint8 numpy arrays - resized to `height` rows and the width the loaders'
    `_resize` gives them (data.fit_tables.fitted_width), bicubic with PIL's bytes, mapped to 1 - p / 128 and collated padded with -1:
    -> (batch [B,1,H,W] fp32 device tensor, widths list). One upload of the pixels, one of the tables (per-line entries and the coefficient
    tables of data.fit_tables, one per distinct (in, out) pair of the batch), one launch (hwg_fit_lines). W: the batch width, a multiple of 4
    not below the widest fitted line (default: that width rounded up to a multiple of 4). `out`: a contiguous 16-byte aligned fp32 device
    buffer of at least B * H * W elements to write into. `device`: out's, else the current one. A picture beyond the kernel's limits
    (taller than FIT_MAX_IN_H, wider than FIT_MAX_W) is fitted on the host with `_resize` and goes through the launch as it is (both
    passes skipped); a batch beyond them (H, W, B) is fitted and collated on the host and uploaded. The values are the same; it is said
    once on stderr and counted in ops.fit_fallbacks."""
    import numpy as np
    from .data import fit_tables as FT
    from .data.author_hw_dataset import _resize
    global fit_fallbacks
    H = int(height)
    if H < 1:
        raise L.HwgError("fit_lines: line height %d" % H)
    images = list(images)
    if not images:
        raise L.HwgError("fit_lines: no images")
    for i, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 2 or im.shape[0] < 1 or im.shape[1] < 1:
            raise L.HwgError("fit_lines: image %d must be a non-empty 2-D uint8 numpy array, got %s %s" % (
                i, getattr(im, "shape", type(im)), getattr(im, "dtype", None)))
    B = len(images)
    widths = [FT.fitted_width(im.shape[0], im.shape[1], H) for im in images]
    Wmin = -(-max(widths) // 4) * 4
    if W is None:
        W = Wmin
    W = int(W)
    if W % 4 or W < max(widths):
        raise L.HwgError("fit_lines: batch width %d must be a multiple of 4 and at least the widest fitted line (%d)" % (W, max(widths)))
    if device is None:
        device = out.device if torch.is_tensor(out) else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=device)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < B * H * W
          or out.data_ptr() % 16):
        raise L.HwgError("fit_lines: out must be a contiguous 16-byte aligned fp32 device buffer of at least %d elements" % (B * H * W))
    batch = out.view(-1)[:B * H * W].view(B, 1, H, W)

    def on_host(im):
        fitted = im if im.shape[0] == H else _resize(im, float(H) / im.shape[0])
        assert fitted.shape[0] == H, (im.shape, fitted.shape)
        return np.ascontiguousarray(fitted)
    if H > FIT_MAX_H or W > FIT_MAX_W or B > FIT_MAX_B:
        fit_fallbacks += 1
        _fit_said("H=%d W=%d B=%d is beyond the kernel's limits (%d, %d, %d)" % (H, W, B, FIT_MAX_H, FIT_MAX_W, FIT_MAX_B))
        host = np.full((B, 1, H, W), -1.0, dtype=np.float32)
        for b, im in enumerate(images):
            fitted = on_host(im)
            host[b, 0, :, :fitted.shape[1]] = np.float32(1.0) - fitted.astype(np.float32) / np.float32(128.0)
        batch.copy_(h2d(host, device))
        return batch, widths
    for b, im in enumerate(images):
        if im.shape[0] > FIT_MAX_IN_H or im.shape[1] > FIT_MAX_W:
            fit_fallbacks += 1
            _fit_said("a picture of %d x %d is beyond the kernel's limits (%d rows, %d columns)" % (im.shape[0], im.shape[1], FIT_MAX_IN_H, FIT_MAX_W))
            images[b] = on_host(im)
            assert images[b].shape[1] == widths[b], (im.shape, images[b].shape, widths[b])
    # the tables: lines [B][10] int64 first, then one coefficient block per distinct (in, out) pair - one upload
    lines, coef = FT.batch_tables([im.shape for im in images], H, widths)
    n = lines.size * 2
    table = np.empty(n + coef.size, dtype=np.int32)
    table[:n] = lines.reshape(-1).view(np.int32)
    table[n:] = coef
    pixels = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])
    pixels_d = h2d(pixels, device)
    table_d = h2d(table, device)
    L.call("hwg_fit_lines", pixels_d, pixels.size, table_d, table_d[n:], coef.size, max(im.shape[0] for im in images), B, H, W,
           batch, _stream())
    return batch, widths


def fg_masks(pixels, offsets, widths, height=64, out=None, want_thresholds=False):
    """Foreground masks of a ragged pool of grey lines (csrc/fg_mask.hip; the reference's cv2 Otsu threshold, inversion and dilation with the
    9 x 9 ellipse, datasets/author_hw_dataset.py:216-219) in one launch -> a uint8 pool of the same layout, 255 = foreground, 0 = not.
    `pixels`: uint8 1-D device tensor; `offsets` [B+1] and `widths` [B] host arrays: line b is the row-major `height` x widths[b] picture at
    pixels[offsets[b]:], offsets[B] = the bytes in use. Any width >= 1 and any byte offset; height <= 64. The host tables are validated here,
    before anything is uploaded or launched. `out`: a uint8 device buffer of pixels' size to write into (only the lines' own bytes are
    written; without one the bytes between the lines are 0). want_thresholds: -> (masks, int32 [B] device tensor of the Otsu levels)."""
    import numpy as np
    if not torch.is_tensor(pixels) or not pixels.is_cuda or pixels.dtype != torch.uint8 or pixels.dim() != 1 or not pixels.is_contiguous():
        raise L.HwgError("fg_masks: pixels must be a contiguous 1-D uint8 device tensor")
    H = int(height)
    if not (1 <= H <= 64):
        raise L.HwgError("fg_masks: line height %d, need 1..64" % H)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    w = np.asarray(widths, dtype=np.int64).reshape(-1)
    B = w.shape[0]
    if B < 1 or off.shape[0] != B + 1:
        raise L.HwgError("fg_masks: %d offsets for %d widths, need one more" % (off.shape[0], B))
    if ((w < 1) | (H * w > (1 << 22))).any():
        raise L.HwgError("fg_masks: widths must lie in [1, %d], got %s" % ((1 << 22) // H, w.tolist()))
    end = off[:B] + H * w
    if (off[:B] < 0).any() or (end > off[B]).any() or off[B] > pixels.numel():
        raise L.HwgError("fg_masks: every line must lie inside [0, offsets[B]) and offsets[B] inside the %d bytes of pixels, got %s" % (pixels.numel(), off.tolist()))
    order = np.argsort(off[:B], kind="stable")
    if (end[order][:-1] > off[:B][order][1:]).any():
        raise L.HwgError("fg_masks: lines overlap, offsets %s widths %s" % (off.tolist(), w.tolist()))
    if out is None:
        out = torch.zeros_like(pixels)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
          or out.numel() < pixels.numel() or out.data_ptr() == pixels.data_ptr()):
        raise L.HwgError("fg_masks: out must be a contiguous 1-D uint8 device buffer of at least %d bytes, not pixels itself" % pixels.numel())
    table = np.empty(3 * B, dtype=np.int32)      # offsets [B] int64 first (8-byte aligned), then widths [B] int32: one upload
    table[:2 * B].view(np.int64)[:] = off[:B]
    table[2 * B:] = w
    table_d = h2d(table, pixels.device)
    thr = torch.empty((B,), dtype=torch.int32, device=pixels.device) if want_thresholds else None
    L.call("hwg_fg_masks", pixels, pixels.numel(), table_d[:2 * B], table_d[2 * B:], B, H, out, thr, _stream())
    return (out, thr) if want_thresholds else out


# ----------------------------------------------------------------------------------------------
# GAN batches from a device-resident line store (csrc/line_store.hip, data/line_store.py)
# ----------------------------------------------------------------------------------------------
class LinePool:
    """A ragged uint8 pool of fitted lines in GPU memory, the layout of fg_masks: `pixels` a contiguous 1-D uint8 device tensor, `offsets` /
    `widths` host arrays [n] - line k is the row-major `height` x widths[k] picture at pixels[offsets[k]:], any width >= 1 and any byte
    offset. `masks` (optional): a second pool of the same layout and size, bytes 0 / 255. Nothing is checked or uploaded here: store_batch
    validates the pool's tables on the host the first time it is handed the pool and keeps the device copies of the two tables with it."""

    def __init__(self, pixels, offsets, widths, height=64, masks=None):
        self.pixels, self.masks, self.height = pixels, masks, int(height)
        self.offsets, self.widths = offsets, widths
        self._tables = None
        self._stats = None                                     # store_line_stats: (thr, hist), computed once

    def __len__(self):
        return len(self.widths)

    def _prepare(self):
        import numpy as np
        if self._tables is not None:
            return self._tables
        px, H = self.pixels, self.height
        if not torch.is_tensor(px) or not px.is_cuda or px.dtype != torch.uint8 or px.dim() != 1 or not px.is_contiguous() or px.numel() < 1:
            raise L.HwgError("store_batch: the pool's pixels must be a contiguous non-empty 1-D uint8 device tensor")
        mk = self.masks
        if mk is not None and (not torch.is_tensor(mk) or mk.device != px.device or mk.dtype != torch.uint8 or mk.dim() != 1 or not mk.is_contiguous()
                               or mk.numel() != px.numel()):
            raise L.HwgError("store_batch: the mask pool must be a contiguous 1-D uint8 tensor on the pixels' device and of their size (%d bytes), got %s"
                             % (px.numel(), "%s %s %s" % (tuple(mk.shape), mk.dtype, mk.device) if torch.is_tensor(mk) else type(mk)))
        if H < 1:
            raise L.HwgError("store_batch: line height %d" % H)
        off = np.asarray(self.offsets, dtype=np.int64).reshape(-1)
        w = np.asarray(self.widths, dtype=np.int64).reshape(-1)
        n = w.shape[0]
        if n < 1 or n >= (1 << 31) or off.shape[0] < n:
            raise L.HwgError("store_batch: %d offsets for %d widths" % (off.shape[0], n))
        off = off[:n]
        if ((w < 1) | (w >= (1 << 31))).any():
            raise L.HwgError("store_batch: widths must be at least 1, got %s" % w[(w < 1) | (w >= (1 << 31))][:8].tolist())
        end = off + H * w
        if (off < 0).any() or (end > px.numel()).any():
            bad = np.nonzero((off < 0) | (end > px.numel()))[0][:8]
            raise L.HwgError("store_batch: every line must lie inside the %d bytes of pixels; lines %s do not" % (px.numel(), bad.tolist()))
        order = np.argsort(off, kind="stable")
        if (end[order][:-1] > off[order][1:]).any():
            bad = order[1:][end[order][:-1] > off[order][1:]][:8]
            raise L.HwgError("store_batch: lines overlap (lines %s begin inside another)" % bad.tolist())
        table = np.empty(3 * n, dtype=np.int32)      # offsets [n] int64 first (8-byte aligned), then widths [n] int32: one upload
        table[:2 * n].view(np.int64)[:] = off
        table[2 * n:] = w
        table_d = h2d(table, px.device)
        self._tables = (table_d[:2 * n], table_d[2 * n:], n)
        return self._tables


def store_batch(pool, rows, W=None, want_mask=False, out=None):
    """One collated GAN batch from a LinePool in one launch (hwg_store_batch): `rows` = [(line, out_w, strech, m)] per output row - line
    `line` of the pool stretched by `strech` and sheared by m = tan(skew) around the mid-line into `out_w` columns (the reference's
    affine_trans: cv2.warpAffine, bilinear, border blended in), as 1 - level / 128, padded with -1 to W columns -> fp32 [B,1,H,W] on the
    pool's device. W: default max(out_w); any positive integer, not rounded. want_mask: -> (image, fg_mask), the pool's masks through the
    same map (border 0, padded with 0). Everything is validated here on the host, before anything is uploaded or launched; then the row
    tables go up in one pinned buffer (one h2d) and one launch on the current stream writes every element. `out`: a contiguous 16-byte
    aligned fp32 device buffer of at least B*H*W rounded up to 4 elements to write into (with want_mask a pair of them); the returned
    tensors are views of it."""
    import numpy as np
    if not isinstance(pool, LinePool):
        raise L.HwgError("store_batch: pool must be an ops.LinePool, got %s" % type(pool))
    off_d, w_d, n = pool._prepare()
    H, dev = pool.height, pool.pixels.device
    if want_mask and pool.masks is None:
        raise L.HwgError("store_batch: want_mask, but the pool has no masks")
    try:
        r = np.asarray([tuple(x) for x in rows], dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise L.HwgError("store_batch: rows must be (line, out_w, strech, m) tuples: %s" % e)
    if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] != 4:
        raise L.HwgError("store_batch: rows must be a non-empty list of (line, out_w, strech, m), got shape %s" % (r.shape,))
    B = r.shape[0]
    line, ow, strech, m = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    if not (np.isfinite(line).all() and (line == np.floor(line)).all() and (line >= 0).all() and (line < n).all()):
        raise L.HwgError("store_batch: line indices must be integers in [0, %d), got %s" % (n, line.tolist()))
    if not (np.isfinite(ow).all() and (ow == np.floor(ow)).all() and (ow >= 0).all() and (ow < (1 << 31)).all()):
        raise L.HwgError("store_batch: out_w must be integers >= 0, got %s" % ow.tolist())
    if W is None:
        W = int(ow.max())
    W = int(W)
    if W < 1:
        raise L.HwgError("store_batch: batch width %d, need at least 1" % W)
    if (ow > W).any():
        raise L.HwgError("store_batch: out_w %s above the batch width %d" % (ow[ow > W].tolist(), W))
    if not (np.isfinite(strech).all() and (strech > 0).all()):
        raise L.HwgError("store_batch: strech must be finite and positive, got %s" % strech.tolist())
    if not np.isfinite(m).all():
        raise L.HwgError("store_batch: m (tan of the skew) must be finite, got %s" % m.tolist())
    total = B * H * W
    need = -(-total // 4) * 4
    if need >= (1 << 62):
        raise L.HwgError("store_batch: a batch of %d x %d x %d elements" % (B, H, W))
    outs = list(out) if isinstance(out, (tuple, list)) else [out] + ([None] if want_mask else [])
    if len(outs) != (2 if want_mask else 1):
        raise L.HwgError("store_batch: out must be %s" % ("a pair (image buffer, mask buffer)" if want_mask else "one buffer"))
    for i, o in enumerate(outs):
        if o is None:
            outs[i] = torch.empty((need,), dtype=torch.float32, device=dev)
        elif (not torch.is_tensor(o) or o.device != dev or o.dtype != torch.float32 or not o.is_contiguous() or o.numel() < need or o.data_ptr() % 16):
            raise L.HwgError("store_batch: out must be a contiguous 16-byte aligned fp32 buffer on the pool's device of at least %d elements "
                             "(B*H*W = %d rounded up to 4)" % (need, total))
    elems = min(o.numel() for o in outs)
    table = np.empty(6 * B, dtype=np.int32)      # strech [B], m [B] fp64 first (8-byte aligned), then line [B], out_w [B] int32: one upload
    table[:2 * B].view(np.float64)[:] = strech
    table[2 * B:4 * B].view(np.float64)[:] = m
    table[4 * B:5 * B] = line.astype(np.int64)
    table[5 * B:] = ow.astype(np.int64)
    t = h2d(table, dev)
    L.call("hwg_store_batch", pool.pixels, pool.masks if want_mask else None, pool.pixels.numel(), off_d, w_d, n, t[4 * B:5 * B], t[5 * B:],
           t[:2 * B], t[2 * B:4 * B], B, H, W, outs[0], outs[1] if want_mask else None, elems, _stream())
    res = [o.view(-1)[:total].view(B, 1, H, W) for o in outs]
    return (res[0], res[1]) if want_mask else res[0]


def store_line_stats(pool):
    """The per-line statistics of the brightness augmentation for a whole LinePool, once (hwg_store_line_stats, one launch, one workgroup
    per line) -> (thr int32 [n], hist int32 [n, 256]) on the pool's device, kept with the pool: the Otsu level of augment_lines' statistics
    and the 256-bin histogram depend on the stored bytes alone. The pool's tables are validated on the host first (LinePool._prepare, and
    height x width <= 2^22 for the exact sums)."""
    import numpy as np
    if not isinstance(pool, LinePool):
        raise L.HwgError("store_line_stats: pool must be an ops.LinePool, got %s" % type(pool))
    if pool._stats is not None:
        return pool._stats
    off_d, w_d, n = pool._prepare()
    H, dev = pool.height, pool.pixels.device
    w = np.asarray(pool.widths, dtype=np.int64).reshape(-1)[:n]
    if (H * w > (1 << 22)).any():
        raise L.HwgError("store_line_stats: lines of more than 2^22 pixels (height %d, widths %s) are too large for the exact Otsu sums"
                         % (H, w[H * w > (1 << 22)][:8].tolist()))
    thr = torch.empty((n,), dtype=torch.int32, device=dev)
    hist = torch.empty((n, 256), dtype=torch.int32, device=dev)
    L.call("hwg_store_line_stats", pool.pixels, pool.pixels.numel(), off_d, w_d, n, H, thr, hist, _stream())
    pool._stats = (thr, hist)
    return pool._stats


def store_warp_batch(pool, lines, mesh, W=None, fg_bg=None, want_map=False, rng=None, out=None):
    """One augmented recogniser batch from a LinePool in one launch (hwg_store_warp_batch): output row b shows line lines[b] of the pool,
    re-lit and warped over `mesh` (a LineMesh of the pool's height whose widths are those lines' widths; mesh.x_off places a line inside
    the row, columns outside it are -1) -> fp32 [B,1,H,W] on the pool's device, W default max(x_off + width). The result equals
    augment_lines on the same lines collated and uploaded, bit for bit; the draws are consumed as there: fg_bg None - unit draws of `rng`
    (a DeviceRNG: one hwg_randn launch of (B, 2 + 2 GY GX), the stream offset advances); fg_bg [B,2] (host) - explicit shifts with the
    explicit displacements of mesh.disp. want_map: -> (y, map [B,2,H,W]). Everything is validated here on the host before anything is
    uploaded or launched; the row tables go up in one pinned buffer. `out`: a contiguous fp32 buffer on the pool's device of at least
    B*H*W elements to write into; the returned tensor is a view of it."""
    import numpy as np
    if not isinstance(pool, LinePool):
        raise L.HwgError("store_warp_batch: pool must be an ops.LinePool, got %s" % type(pool))
    if not isinstance(mesh, LineMesh):
        raise L.HwgError("store_warp_batch: mesh must be an ops.LineMesh, got %s" % type(mesh))
    off_d, w_d, n = pool._prepare()
    thr, hist = store_line_stats(pool)
    H, dev = pool.height, pool.pixels.device
    try:
        k = np.asarray(lines, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise L.HwgError("store_warp_batch: lines must be pool line indices: %s" % e)
    B = k.shape[0]
    if B < 1 or B > 65535 or B != len(mesh.widths):
        raise L.HwgError("store_warp_batch: %d lines for a mesh of %d rows (1..65535 rows)" % (B, len(mesh.widths)))
    if not (np.isfinite(k).all() and (k == np.floor(k)).all() and (k >= 0).all() and (k < n).all()):
        raise L.HwgError("store_warp_batch: line indices must be integers in [0, %d), got %s" % (n, k.tolist()))
    k = k.astype(np.int64)
    if mesh.H != H:
        raise L.HwgError("store_warp_batch: a mesh for lines of height %d over a pool of height %d" % (mesh.H, H))
    mw, xo = np.asarray(mesh.widths, dtype=np.int64), np.asarray(mesh.x_off, dtype=np.int64)
    pw = np.asarray(pool.widths, dtype=np.int64).reshape(-1)[k]
    if (mw != pw).any():
        raise L.HwgError("store_warp_batch: the mesh's widths %s are not the widths %s of the pool's lines %s" % (mw.tolist(), pw.tolist(), k.tolist()))
    if W is None:
        W = int((xo + mw).max())
    W = int(W)
    if W < 1 or W >= (1 << 31):
        raise L.HwgError("store_warp_batch: batch width %d" % W)
    if (xo < 0).any() or (xo + mw > W).any():
        raise L.HwgError("store_warp_batch: line extents (x_off %s, widths %s) outside the batch width %d" % (xo.tolist(), mw.tolist(), W))
    if mesh.GY > 16:
        raise L.HwgError("store_warp_batch: a lattice of %d rows (at most 16: lines up to ~190 px high)" % mesh.GY)
    if (fg_bg is None) != (mesh.disp is None):
        raise L.HwgError("store_warp_batch: explicit brightness draws and explicit displacements go together")
    if fg_bg is not None:
        fg_bg = np.asarray(fg_bg, dtype=np.float64)
        if fg_bg.shape != (B, 2) or not np.isfinite(fg_bg).all():
            raise L.HwgError("store_warp_batch: fg_bg must be %d finite pairs, got shape %s" % (B, fg_bg.shape))
    elif rng is None:
        raise L.HwgError("store_warp_batch: no explicit draws and no device generator")
    total = B * H * W
    if out is None:
        out = torch.empty((total,), dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or out.device != dev or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < total:
        raise L.HwgError("store_warp_batch: out must be a contiguous fp32 buffer on the pool's device of at least %d elements" % total)
    li, lf, dr = mesh.tables(fg_bg)
    lfs, drs = lf.shape[1], 2 + 2 * mesh.GY * mesh.GX
    table = np.empty(B * (5 + lfs + (0 if dr is None else drs)), dtype=np.int32)      # line [B], lines_i [B,4], lines_f, draws: one upload
    table[:B] = k
    table[B:5 * B] = li.reshape(-1)
    table[5 * B:5 * B + B * lfs].view(np.float32)[:] = lf.reshape(-1)
    if dr is not None:
        table[5 * B + B * lfs:].view(np.float32)[:] = dr.reshape(-1)
    t = h2d(table, dev)
    draws = rng.randn((B, drs), dev) if dr is None else t[5 * B + B * lfs:]
    map_out = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if want_map else None
    L.call("hwg_store_warp_batch", pool.pixels, pool.pixels.numel(), off_d, w_d, n, thr, hist, t[:B], t[B:5 * B], t[5 * B:5 * B + B * lfs], lfs,
           draws, drs, B, H, W, mesh.GY, mesh.GX, out, map_out, out.numel(), _stream())
    y = out.view(-1)[:total].view(B, 1, H, W)
    return (y, map_out) if want_map else y


# ----------------------------------------------------------------------------------------------
# sample sheets of GAN training: a batch of lines as one 8-bit grey picture (csrc/sample_sheet.hip)
# ----------------------------------------------------------------------------------------------
def sample_sheet_shape(B, H, W, nrow=None):
    """(rows, columns, nrow) of the sheet torchvision's make_grid lays out for B images of H x W with padding 2; nrow=None: the
    reference's max(1, 2048 // W)"""
    nrow = max(1, 2048 // W) if nrow is None else int(nrow)
    if nrow < 1:
        raise L.HwgError("sample_sheet: nrow %d, need at least 1" % nrow)
    if B == 1:
        return H, W, nrow
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    return (H + 2) * ymaps + 2, (W + 2) * xmaps + 2, nrow


def sample_sheet(images, nrow=None, out=None):
    """`images` [B,1,H,W] (device, fp32) -> the uint8 device tensor [Hs, Ws] that the reference's save_image(1 - images, nrow=nrow,
    normalize=True) writes to disk: normalised to the batch's own range, tiled nrow to a row with a border of 2, quantised with + 0.5
    (hwg_sheet_minmax + hwg_sheet_compose: two launches on the current stream, nothing comes to the host). nrow=None: max(1, 2048 // W).
    `out`: a contiguous 4-byte aligned uint8 device buffer of at least Hs * Ws bytes rounded up to 4 to write into (every byte of the sheet
    is written; the returned tensor is a view of it)."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 1 or min(images.shape) < 1:
        raise L.HwgError("sample_sheet: images must be a [B,1,H,W] fp32 device tensor, got %s" % (tuple(images.shape) if torch.is_tensor(images) else type(images),))
    _chk(images, "sample_sheet: images")
    B, _, H, W = images.shape
    Hs, Ws, nrow = sample_sheet_shape(B, H, W, nrow)
    if Hs * Ws > (1 << 31) - 4:
        raise L.HwgError("sample_sheet: a sheet of %d x %d bytes does not fit int" % (Hs, Ws))
    need = -(-Hs * Ws // 4) * 4
    if out is None:
        out = torch.empty((need,), dtype=torch.uint8, device=images.device)
    else:
        _chk(out, "sample_sheet: out", torch.uint8)
        if out.numel() < need or out.data_ptr() % 4:
            raise L.HwgError("sample_sheet: out must be a 4-byte aligned uint8 device buffer of at least %d bytes (the %d x %d sheet rounded up "
                             "to 4), got %d" % (need, Hs, Ws, out.numel()))
    n = B * H * W
    parts = L.query("hwg_sheet_parts", n)
    partials = torch.empty((parts, 2), dtype=torch.float32, device=images.device)
    st = _stream()
    L.call("hwg_sheet_minmax", images, n, partials, parts, st)
    L.call("hwg_sheet_compose", images, B, H, W, nrow, partials, parts, out, out.numel(), st)
    return out.view(-1)[:Hs * Ws].view(Hs, Ws)


def row_means(rows2d, n_rows=None, out=None):
    """fp32 mean of each of the first n_rows rows of a contiguous device [N, n] tensor -> [n_rows] (hwg_sheet_row_means, one launch);
    `out`: a contiguous fp32 device tensor of at least n_rows elements to write into"""
    _chk(rows2d, "row_means: input")
    if rows2d.dim() != 2 or rows2d.shape[0] < 1 or rows2d.shape[1] < 1:
        raise L.HwgError("row_means: input must be [N, n], got %s" % (tuple(rows2d.shape),))
    n_rows = rows2d.shape[0] if n_rows is None else min(int(n_rows), rows2d.shape[0])
    if out is None:
        out = torch.empty((n_rows,), dtype=torch.float32, device=rows2d.device)
    else:
        _chk(out, "row_means: out")
        if out.numel() < n_rows:
            raise L.HwgError("row_means: out holds %d elements, %d rows asked for" % (out.numel(), n_rows))
    L.call("hwg_sheet_row_means", rows2d, rows2d.shape[1], n_rows, rows2d.shape[1], out, _stream())
    return out


# ----------------------------------------------------------------------------------------------
# evaluation pictures of new_eval.py: the real line above its reconstruction, framed, captioned (csrc/eval_pictures.hip)
# ----------------------------------------------------------------------------------------------
def eval_pairs_shape(H, Wi, Wr, strip):
    """(rows, columns) of one picture of eval_pairs: 2 H + 2 rows (+ the 50 rows of the caption strip), max(Wi, Wr) columns"""
    return 2 * int(H) + 2 + (L.query("hwg_eval_strip_rows") if strip else 0), max(int(Wi), int(Wr))


def eval_pairs(image, recon, captions=None, atlas=None, out=None):
    """`image` [B,1,H,Wi] and `recon` [B,1,H,Wr] (device, fp32) -> the uint8 device tensor [B, Hp, Wp, 3] of the reference's per-line
    evaluation pictures, RGB: the real line in a green frame above the reconstruction in a blue one, the narrower of the two centred.
    `captions`: per line a sequence of glyph codes (a host list / array, -1 ends a caption; rows may differ in length) drawn from `atlas`
    (uint8 device tensor [G, gh, gw]) into a strip of 50 rows below; None: no strip. Codes are checked on the host, before the one small
    upload and the one launch (hwg_eval_pairs) on the current stream. `out`: a contiguous 4-byte aligned uint8 device buffer of at least
    B * Hp * Wp * 3 bytes rounded up to 4 to write into (every byte is written; the returned tensor is a view of it)."""
    import numpy as np
    for t, name in ((image, "image"), (recon, "recon")):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 1 or min(t.shape) < 1:
            raise L.HwgError("eval_pairs: %s must be a [B,1,H,W] fp32 device tensor, got %s" % (name, tuple(t.shape) if torch.is_tensor(t) else type(t)))
        _chk(t, "eval_pairs: " + name)
    B, _, H, Wi = image.shape
    if recon.shape[0] != B or recon.shape[2] != H:
        raise L.HwgError("eval_pairs: image %s and recon %s differ in lines or height" % (tuple(image.shape), tuple(recon.shape)))
    Wr = recon.shape[3]
    strip = captions is not None
    Hp, Wp = eval_pairs_shape(H, Wi, Wr, strip)
    total = B * Hp * Wp * 3
    if total > (1 << 31) - 4:
        raise L.HwgError("eval_pairs: %d pictures of %d x %d x 3 bytes do not fit int" % (B, Hp, Wp))
    need = -(-total // 4) * 4
    codes_d, G, gh, gw, n_codes = None, 0, 0, 0, 0
    if strip:
        if not torch.is_tensor(atlas) or atlas.dim() != 3 or min(atlas.shape) < 1:
            raise L.HwgError("eval_pairs: captions need a glyph atlas, a uint8 device tensor [G, gh, gw]")
        _chk(atlas, "eval_pairs: atlas", torch.uint8)
        G, gh, gw = atlas.shape
        if gh > Hp - 2 * H - 2:
            raise L.HwgError("eval_pairs: glyphs of %d rows do not fit the strip of %d" % (gh, Hp - 2 * H - 2))
        if len(captions) != B:
            raise L.HwgError("eval_pairs: %d captions for %d lines" % (len(captions), B))
        n_codes = max(1, min(max(len(c) for c in captions), -(-Wp // gw)))        # cells beyond the picture are never drawn: not uploaded
        codes = np.full((B, n_codes), -1, dtype=np.int32)
        for b, c in enumerate(captions):
            c = np.asarray(c, dtype=np.int64).reshape(-1)
            end = np.flatnonzero(c < 0)
            c = c[:end[0]] if end.size else c                                      # -1 ends a caption: what follows it is not drawn
            if c.size and c.max() >= G:
                raise L.HwgError("eval_pairs: caption %d holds code %d, the atlas has %d glyphs" % (b, int(c.max()), G))
            c = c[:n_codes]
            codes[b, :c.size] = c
        codes_d = h2d(codes, image.device)
    if out is None:
        out = torch.empty((need,), dtype=torch.uint8, device=image.device)
    else:
        _chk(out, "eval_pairs: out", torch.uint8)
        if out.numel() < need or out.data_ptr() % 4:
            raise L.HwgError("eval_pairs: out must be a 4-byte aligned uint8 device buffer of at least %d bytes (%d pictures of %d x %d x 3 rounded "
                             "up to 4), got %d" % (need, B, Hp, Wp, out.numel()))
    L.call("hwg_eval_pairs", image, recon, B, H, Wi, Wr, atlas if strip else None, G, gh, gw, codes_d, n_codes, out, out.numel(), _stream())
    return out.view(-1)[:total].view(B, Hp, Wp, 3)


# ----------------------------------------------------------------------------------------------
# recognition error rates: arg-max, greedy CTC decode, CER / WER counts on the device (csrc/error_rate.hip)
# ----------------------------------------------------------------------------------------------
ER_MAX_T, ER_MAX_C, ER_MAX_REF = 8192, 1024, 2047       # the limits hwg_ctc_error_rates checks
error_rate_fallbacks = 0                                # batches that took the host path (tests read it)
_error_rate_fallback_said = False


class ErrorRatesPending:
    """kernels already enqueued; `.result()` -> (cer_list, wer_list, pred_strs) per line, waiting (side-stream copy) only for the one
    int32 buffer that holds the counts and the decoded ids. The divisions are string_utils.rates_from_counts': the host path's values,
    bit for bit."""

    def __init__(self, fetch, T, refs, idx_to_char, done=None):
        self.fetch, self.T, self.refs, self.idx_to_char, self.done = fetch, T, refs, idx_to_char, done

    def counts(self):
        """-> (stats int32 [B, 8], decoded int32 [B, T]) as the kernel left them; None for a batch that took the host path"""
        if self.fetch is None:
            return None
        host = self.fetch.get().numpy()
        B = len(self.refs)
        return host[:8 * B].reshape(B, 8), host[8 * B:].reshape(B, self.T)

    def result(self):
        if self.done is None:
            from .utils import string_utils
            stats, decoded = self.counts()
            stats = stats.tolist()
            cers, wers, strs = [], [], []
            for b, ref in enumerate(self.refs):
                n_dec, cdist, hyp_chars, wdist, hyp_words = stats[b][:5]
                ref_words = ref.count(string_utils.SPACE) + 1 if ref else 0
                cers.append(string_utils.rates_from_counts(cdist, len(ref), hyp_chars))
                wers.append(string_utils.rates_from_counts(wdist, ref_words, hyp_words))
                strs.append(string_utils.label2str_single(decoded[b, :n_dec].tolist(), self.idx_to_char, False))
            self.done = (cers, wers, strs)
        return self.done


def host_error_rates(pred, gt, idx_to_char, casesensitive=True):
    """the host path (HWWithStyleTrainer.getCER line by line) on a [T,B,C] numpy array -> (cer_list, wer_list, pred_strs)"""
    from .utils import string_utils
    cers, wers, strs = [], [], []
    for i, gt_line in enumerate(gt):
        ids, _ = string_utils.naive_decode(pred[:, i])
        s = string_utils.label2str_single(ids, idx_to_char, False)
        cers.append(string_utils.cer(gt_line, s, casesensitive))
        wers.append(string_utils.wer(gt_line, s, casesensitive))
        strs.append(s)
    return cers, wers, strs


def ctc_error_rates(pred, gt, idx_to_char, casesensitive=True):
    """Greedy CTC decode of the recogniser's output `pred` [T,B,C] (device, fp32) and CER / WER of every line against the texts `gt`, on the
    device: -> ErrorRatesPending. One upload (class table, reference offsets and code points), two launches, one asynchronous fetch. Where
    the device cannot give string_utils.cer / wer's values - a character set class_code_table refuses, or a size beyond the kernel's limits -
    the batch takes the host path: same values, said once on stderr."""
    from .utils import string_utils
    global error_rate_fallbacks, _error_rate_fallback_said
    if pred.dim() != 3 or not pred.is_cuda or pred.dtype != torch.float32:
        raise L.HwgError("ctc_error_rates: pred must be a [T,B,C] fp32 device tensor, got %s %s" % (tuple(pred.shape), pred.dtype))
    T, B, C = pred.shape
    if T < 1 or B < 1 or C < 2 or len(gt) != B:
        raise L.HwgError("ctc_error_rates: %d texts for pred %s" % (len(gt), tuple(pred.shape)))
    pred = pred.detach().contiguous()
    table = string_utils.class_code_table(idx_to_char, C, casesensitive)
    refs = [string_utils.normalise_ref(g, casesensitive) for g in gt]
    longest = max(len(r) for r in refs)
    if table is None or T > ER_MAX_T or C > ER_MAX_C or longest > ER_MAX_REF:
        error_rate_fallbacks += 1
        if not _error_rate_fallback_said:
            _error_rate_fallback_said = True
            import sys
            why = "the character set does not compare class by class" if table is None else \
                "T=%d C=%d longest reference %d is beyond the kernel's limits (%d, %d, %d)" % (T, C, longest, ER_MAX_T, ER_MAX_C, ER_MAX_REF)
            print("ctc_error_rates: %s; such batches are scored on the host" % why, file=sys.stderr)
        return ErrorRatesPending(None, T, refs, idx_to_char, done=host_error_rates(pred.cpu().numpy(), gt, idx_to_char, casesensitive))
    packed_d = _upload_refs(table, refs, pred.device)
    out = torch.empty((8 * B + B * T,), dtype=torch.int32, device=pred.device)
    L.call("hwg_ctc_error_rates", pred, T, B, C, packed_d, packed_d[C + B + 1:], packed_d[C:C + B + 1], longest, out, _stream())
    return ErrorRatesPending(AsyncFetch(out), T, refs, idx_to_char)


def _upload_refs(table, refs, device):
    """class table [C], reference offsets [B + 1] and the references' code points (at least one int) as one int32 upload"""
    import numpy as np
    C, B = len(table), len(refs)
    offsets = np.zeros(B + 1, dtype=np.int32)
    np.cumsum([len(r) for r in refs], out=offsets[1:])
    total = int(offsets[B])
    packed = np.empty(C + B + 1 + max(total, 1), dtype=np.int32)
    packed[:C] = table
    packed[C:C + B + 1] = offsets
    packed[C + B + 1:] = 0
    if total:
        packed[C + B + 1:C + B + 1 + total] = np.fromiter((c for r in refs for c in r), dtype=np.int32, count=total)
    return h2d(packed, device)


# ----------------------------------------------------------------------------------------------
# the same error rates over the CTC prefix beam search's text (csrc/ctc_beam.hip)
# ----------------------------------------------------------------------------------------------
CB_MAX_BEAM, CB_MAX_T, CB_MAX_C = 32, 2048, 1024         # the limits hwg_ctc_beam_error_rates checks (the reference limit is ER_MAX_REF)
beam_fallbacks = 0                                       # batches that took the host path (tests read it)
_beam_fallback_said = False


class BeamErrorRatesPending(ErrorRatesPending):
    """ErrorRatesPending of the beam text; `.scores()` -> fp32 numpy [B, beam]: the final totals, descending, -inf padded"""

    def __init__(self, fetch, T, refs, idx_to_char, beam, done=None, scores=None):
        ErrorRatesPending.__init__(self, fetch, T, refs, idx_to_char, done)
        self.beam, self._scores = beam, scores

    def _host(self):
        return self.fetch.get().numpy()[:len(self.refs) * (8 + self.T)]

    def counts(self):
        if self.fetch is None:
            return None
        host, B = self._host(), len(self.refs)
        return host[:8 * B].reshape(B, 8), host[8 * B:].reshape(B, self.T)

    def scores(self):
        if self._scores is None:
            import numpy as np
            B = len(self.refs)
            self._scores = self.fetch.get().numpy()[B * (8 + self.T):].view(np.float32).reshape(B, self.beam).copy()
        return self._scores


def host_beam_error_rates(pred, gt, idx_to_char, casesensitive=True, beam=16):
    """the host path of ctc_beam_error_rates on a [T,B,C] numpy array -> ((cer_list, wer_list, pred_strs), scores fp32 [B, beam])"""
    import numpy as np
    from .utils import string_utils
    cers, wers, strs = [], [], []
    scores = np.empty((len(gt), beam), dtype=np.float32)
    for i, gt_line in enumerate(gt):
        ids, _, totals = string_utils.prefix_beam_decode(pred[:, i], beam)
        s = string_utils.label2str_single(ids, idx_to_char, False)
        cers.append(string_utils.cer(gt_line, s, casesensitive))
        wers.append(string_utils.wer(gt_line, s, casesensitive))
        strs.append(s)
        scores[i] = totals
    return (cers, wers, strs), scores


def ctc_beam_error_rates(pred, gt, idx_to_char, casesensitive=True, beam=16):
    """CTC prefix beam search (width `beam`) over the recogniser's output `pred` [T,B,C] (device, fp32, read as log-probabilities as they
    stand) and CER / WER of every line's most probable text against `gt`, on the device: -> BeamErrorRatesPending. One upload, two
    launches, one asynchronous fetch (counts, decoded ids and scores in one buffer); the workspace comes from the caching allocator.
    Where the device cannot serve - a character set class_code_table refuses, or a size beyond the kernel's limits - the batch is decoded
    and scored on the host (string_utils.prefix_beam_decode, fp64), said once on stderr."""
    from .utils import string_utils
    global beam_fallbacks, _beam_fallback_said
    if not torch.is_tensor(pred) or pred.dim() != 3 or not pred.is_cuda or pred.dtype != torch.float32:
        raise L.HwgError("ctc_beam_error_rates: pred must be a [T,B,C] fp32 device tensor, got %s %s" % (
            tuple(pred.shape) if torch.is_tensor(pred) else type(pred), getattr(pred, "dtype", None)))
    T, B, C = pred.shape
    if T < 1 or B < 1 or C < 2 or len(gt) != B:
        raise L.HwgError("ctc_beam_error_rates: %d texts for pred %s" % (len(gt), tuple(pred.shape)))
    beam = int(beam)
    if beam < 1:
        raise L.HwgError("ctc_beam_error_rates: a beam of %d" % beam)
    pred = pred.detach().contiguous()
    table = string_utils.class_code_table(idx_to_char, C, casesensitive)
    refs = [string_utils.normalise_ref(g, casesensitive) for g in gt]
    longest = max(len(r) for r in refs)
    if table is None or beam > CB_MAX_BEAM or T > CB_MAX_T or C > CB_MAX_C or longest > ER_MAX_REF:
        beam_fallbacks += 1
        if not _beam_fallback_said:
            _beam_fallback_said = True
            import sys
            why = "the character set does not compare class by class" if table is None else \
                "beam=%d T=%d C=%d longest reference %d is beyond the kernel's limits (%d, %d, %d, %d)" % (
                    beam, T, C, longest, CB_MAX_BEAM, CB_MAX_T, CB_MAX_C, ER_MAX_REF)
            print("ctc_beam_error_rates: %s; such batches are decoded and scored on the host" % why, file=sys.stderr)
        done, scores = host_beam_error_rates(pred.cpu().numpy(), gt, idx_to_char, casesensitive, beam)
        return BeamErrorRatesPending(None, T, refs, idx_to_char, beam, done=done, scores=scores)
    packed_d = _upload_refs(table, refs, pred.device)
    out = torch.empty((8 * B + B * T + B * beam,), dtype=torch.int32, device=pred.device)      # the scores ride behind the ids: one fetch
    ws = torch.empty(L.query("hwg_ctc_beam_workspace", T, B, C, beam), dtype=torch.uint8, device=pred.device)
    L.call("hwg_ctc_beam_error_rates", pred, T, B, C, beam, packed_d, packed_d[C + B + 1:], packed_d[C:C + B + 1], longest, out,
           out[8 * B + B * T:], ws, ws.numel(), _stream())
    return BeamErrorRatesPending(AsyncFetch(out), T, refs, idx_to_char, beam)


# ----------------------------------------------------------------------------------------------
# writer retrieval over style vectors: rank of the nearest other line of the same writer (csrc/writer_id.hip)
# ----------------------------------------------------------------------------------------------
WID_L1, WID_L2 = 0, 1                                   # hwg_writer_first_rank's metric: sum |a - b|, sum (a - b)^2


def writer_first_rank(styles, author_ids, metric, out=None):
    """styles [N, D] fp32 and author_ids [N] int32 on the device -> (first_rank int32 [N], nearest_same fp32 [N]): per row the place, in the
    stable order of its distances to all rows, of the nearest entry of its writer that is not at place 0 (N where there is none) and the
    distance there (+inf where there is none). `out`: a (first_rank, nearest_same) pair to write into."""
    if not torch.is_tensor(styles) or styles.dim() != 2 or not styles.is_cuda or styles.dtype != torch.float32 or not styles.is_contiguous():
        raise L.HwgError("writer_first_rank: styles must be a contiguous [N, D] fp32 device tensor, got %s %s" % (
            tuple(styles.shape) if torch.is_tensor(styles) else type(styles), getattr(styles, "dtype", None)))
    N, D = styles.shape
    if not torch.is_tensor(author_ids) or tuple(author_ids.shape) != (N,) or author_ids.dtype != torch.int32 or \
            author_ids.device != styles.device or not author_ids.is_contiguous():
        raise L.HwgError("writer_first_rank: author_ids must be a contiguous [%d] int32 tensor on %s, got %s %s" % (
            N, styles.device, tuple(author_ids.shape) if torch.is_tensor(author_ids) else type(author_ids), getattr(author_ids, "dtype", None)))
    if metric not in (WID_L1, WID_L2):
        raise L.HwgError("writer_first_rank: metric must be 0 (L1) or 1 (squared L2), got %r" % (metric,))
    if out is None:
        first_rank = torch.empty((N,), dtype=torch.int32, device=styles.device)
        nearest_same = torch.empty((N,), dtype=torch.float32, device=styles.device)
    else:
        first_rank, nearest_same = out
        if tuple(first_rank.shape) != (N,) or first_rank.dtype != torch.int32 or not first_rank.is_contiguous() or \
                tuple(nearest_same.shape) != (N,) or nearest_same.dtype != torch.float32 or not nearest_same.is_contiguous() or \
                first_rank.device != styles.device or nearest_same.device != styles.device:
            raise L.HwgError("writer_first_rank: out must be contiguous (int32 [%d], fp32 [%d]) tensors on %s" % (N, N, styles.device))
    L.call("hwg_writer_first_rank", styles, author_ids, N, D, int(metric), first_rank, nearest_same, _stream())
    return first_rank, nearest_same


# ----------------------------------------------------------------------------------------------
# style-space map: exact k nearest rows and the layout epochs over the fuzzy graph (csrc/style_map.hip)
# ----------------------------------------------------------------------------------------------
KNN_MAX_K = 64


def knn_rows(styles, k, out=None):
    """styles [N, D] fp32 on the device -> (idx int32 [N, k], d2 fp32 [N, k]): per row the k nearest other rows, ascending by
    (squared L2 distance, column); the row itself is left out by index. `out`: an (idx, d2) pair to write into."""
    if not torch.is_tensor(styles) or styles.dim() != 2 or not styles.is_cuda or styles.dtype != torch.float32 or not styles.is_contiguous():
        raise L.HwgError("knn_rows: styles must be a contiguous [N, D] fp32 device tensor, got %s %s" % (
            tuple(styles.shape) if torch.is_tensor(styles) else type(styles), getattr(styles, "dtype", None)))
    N, D = styles.shape
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K or k > N - 1:
        raise L.HwgError("knn_rows: k must be an integer in 1..%d and at most N - 1 = %d, got %r" % (KNN_MAX_K, N - 1, k))
    if out is None:
        idx = torch.empty((N, k), dtype=torch.int32, device=styles.device)
        d2 = torch.empty((N, k), dtype=torch.float32, device=styles.device)
    else:
        idx, d2 = out
        if tuple(idx.shape) != (N, k) or idx.dtype != torch.int32 or not idx.is_contiguous() or tuple(d2.shape) != (N, k) or \
                d2.dtype != torch.float32 or not d2.is_contiguous() or idx.device != styles.device or d2.device != styles.device:
            raise L.HwgError("knn_rows: out must be contiguous (int32 [%d, %d], fp32 [%d, %d]) tensors on %s" % (N, k, N, k, styles.device))
    L.call("hwg_knn_rows", styles, N, D, k, idx, d2, _stream())
    return idx, d2


class UmapGraph:
    """a checked graph on the device: row_ptr int32 [N + 1], col int32 [E], period_q int32 [E]"""

    def __init__(self, row_ptr, col, period_q, n, e):
        self.row_ptr, self.col, self.period_q, self.n, self.e = row_ptr, col, period_q, n, e


def umap_graph(row_ptr, col, period_q, device):
    """host arrays of a CSR graph -> UmapGraph on `device`. Checked here, before the upload, because the kernel follows these numbers into
    memory: row_ptr [N + 1] starts at 0, never decreases and ends at E = len(col) >= 1; 0 <= col < N; period_q >= 1."""
    import numpy as np
    row_ptr, col, period_q = (np.asarray(x) for x in (row_ptr, col, period_q))
    for name, x in (("row_ptr", row_ptr), ("col", col), ("period_q", period_q)):
        if x.ndim != 1 or x.dtype.kind not in "iu":
            raise L.HwgError("umap_graph: %s must be a 1-D integer array, got %s %s" % (name, x.shape, x.dtype))
    n, e = row_ptr.shape[0] - 1, col.shape[0]
    if n < 1 or n > 1 << 20 or e < 1 or e >= 1 << 31 or period_q.shape[0] != e:
        raise L.HwgError("umap_graph: bad sizes N=%d (1..2^20) E=%d (1..2^31-1) with %d periods" % (n, e, period_q.shape[0]))
    if int(row_ptr[0]) != 0 or int(row_ptr[-1]) != e or (np.diff(row_ptr.astype(np.int64)) < 0).any():
        raise L.HwgError("umap_graph: row_ptr must rise from 0 to E=%d without a step down" % e)
    if int(col.min()) < 0 or int(col.max()) >= n:
        raise L.HwgError("umap_graph: col must lie in 0..%d, got %d..%d" % (n - 1, int(col.min()), int(col.max())))
    if int(period_q.min()) < 1 or int(period_q.max()) >= 1 << 31:
        raise L.HwgError("umap_graph: period_q must lie in 1..2^31-1, got %d..%d" % (int(period_q.min()), int(period_q.max())))
    up = [h2d(np.array(x, dtype=np.int32), device) for x in (row_ptr, col, period_q)]
    return UmapGraph(up[0], up[1], up[2], n, e)


def umap_layout(graph, y, n_epochs, a, b, neg, seed, epoch_begin=0, epoch_end=None, scratch=None):
    """the layout epochs epoch_begin + 1 .. epoch_end (default: n_epochs) of n_epochs over `graph` (umap_graph), in place in y fp32 [N, 2]
    on the device; `scratch`: a second [N, 2] buffer (allocated when None). One launch per epoch; returns y."""
    if not isinstance(graph, UmapGraph):
        raise L.HwgError("umap_layout: graph must come from ops.umap_graph, got %s" % type(graph))
    if not torch.is_tensor(y) or tuple(y.shape) != (graph.n, 2) or not y.is_cuda or y.dtype != torch.float32 or not y.is_contiguous() or \
            y.device != graph.col.device:
        raise L.HwgError("umap_layout: y must be a contiguous [%d, 2] fp32 tensor on %s, got %s %s" % (
            graph.n, graph.col.device, tuple(y.shape) if torch.is_tensor(y) else type(y), getattr(y, "dtype", None)))
    if scratch is None:
        scratch = torch.empty_like(y)
    elif not torch.is_tensor(scratch) or tuple(scratch.shape) != (graph.n, 2) or scratch.dtype != torch.float32 or \
            not scratch.is_contiguous() or scratch.device != y.device or scratch.data_ptr() == y.data_ptr():
        raise L.HwgError("umap_layout: scratch must be another contiguous [%d, 2] fp32 tensor on %s" % (graph.n, y.device))
    if epoch_end is None:
        epoch_end = n_epochs
    L.call("hwg_umap_layout", graph.row_ptr, graph.col, graph.period_q, graph.n, graph.e, y, scratch, int(epoch_begin), int(epoch_end),
           int(n_epochs), float(a), float(b), int(neg), int(seed) & (2 ** 64 - 1), _stream())
    return y


# ----------------------------------------------------------------------------------------------
# same-writer / different-writer distances over all pairs of style vectors (csrc/style_pairs.hip)
# ----------------------------------------------------------------------------------------------
SP_SAME_DIFFERENT, SP_WRITER_PAIRS = 0, 1               # hwg_style_pair_stats's mode: two cells, writers x writers cells
SP_MAX_WRITERS, SP_MAX_BINS = 4096, 256                 # mode 1's limit on the writers, the histogram's on the bins


def style_pair_stats(styles, writer, mode, edge2=None, out=None, workspace=None):
    """styles [N, D] fp32 and writer [N] int32 on the device, the rows ordered so that writer (values 0 .. A-1, A = writer[-1] + 1) never
    decreases -> (count int64, sum fp64, sumsq fp64, d2_range fp32 [2], hist int64 [2, bins] or None) over the pairs i < j: number of
    pairs, sum of the distances and sum of their squares per cell - mode 0: [2], the pairs of one writer and the pairs of two; mode 1:
    [A, A], one cell per pair of writers, mirrored -, the smallest and largest squared distance (+inf, -inf without a pair), and with
    edge2 (fp32 [bins + 1], ascending, squared edges; a device tensor or a host array) the histograms of the one-writer and of the
    two-writer pairs. `out`: the tuple of tensors to write into (hist last, only with edge2); `workspace`: a uint8 device tensor of at
    least hwg_style_pair_stats_workspace bytes (allocated when None). The order of writer is checked here, on a host copy."""
    import numpy as np
    if not torch.is_tensor(styles) or styles.dim() != 2 or styles.dtype != torch.float32 or not styles.is_contiguous() or \
            styles.shape[0] < 1 or styles.shape[1] < 1:
        raise L.HwgError("style_pair_stats: styles must be a contiguous [N, D] fp32 device tensor, got %s %s" % (
            tuple(styles.shape) if torch.is_tensor(styles) else type(styles), getattr(styles, "dtype", None)))
    N, D = styles.shape
    if not torch.is_tensor(writer) or tuple(writer.shape) != (N,) or writer.dtype != torch.int32 or writer.device != styles.device or \
            not writer.is_contiguous():
        raise L.HwgError("style_pair_stats: writer must be a contiguous [%d] int32 tensor on %s, got %s %s" % (
            N, styles.device, tuple(writer.shape) if torch.is_tensor(writer) else type(writer), getattr(writer, "dtype", None)))
    if mode not in (SP_SAME_DIFFERENT, SP_WRITER_PAIRS):
        raise L.HwgError("style_pair_stats: mode must be 0 (same / different) or 1 (writers x writers), got %r" % (mode,))
    w = writer.cpu().numpy()
    if int(w[0]) < 0 or (np.diff(w.astype(np.int64)) < 0).any():
        raise L.HwgError("style_pair_stats: writer must start at 0 or above and never decrease (sort the rows by writer first)")
    A = int(w[-1]) + 1
    if A > N:
        raise L.HwgError("style_pair_stats: writer ids reach %d with %d rows: number the writers 0 .. A-1" % (A - 1, N))
    if mode == SP_WRITER_PAIRS and A > SP_MAX_WRITERS:
        raise L.HwgError("style_pair_stats: %d writers, the writers x writers mode takes at most %d" % (A, SP_MAX_WRITERS))
    bins = 0
    if edge2 is not None:
        e = edge2.detach().cpu().numpy() if torch.is_tensor(edge2) else np.asarray(edge2)
        if e.ndim != 1 or e.dtype != np.float32 or not 1 <= e.shape[0] - 1 <= SP_MAX_BINS or np.isnan(e).any() or (np.diff(e) < 0).any():
            raise L.HwgError("style_pair_stats: edge2 must be fp32 [bins + 1] with 1 <= bins <= %d, ascending, without NaN, got %s %s" % (
                SP_MAX_BINS, e.shape, e.dtype))
        bins = e.shape[0] - 1
        if not torch.is_tensor(edge2) or edge2.device != styles.device or not edge2.is_contiguous():
            edge2 = h2d(np.ascontiguousarray(e), styles.device)
    if not styles.is_cuda:
        raise L.HwgError("style_pair_stats: styles must be on a GPU, got %s" % (styles.device,))
    cells = (2,) if mode == SP_SAME_DIFFERENT else (A, A)
    want = [(cells, torch.int64), (cells, torch.float64), (cells, torch.float64), ((2,), torch.float32)] + ([((2, bins), torch.int64)] if bins else [])
    if out is None:
        out = tuple(torch.empty(shape, dtype=dtype, device=styles.device) for shape, dtype in want)
    else:
        out = tuple(out)
        if len(out) != len(want) or any(not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or
                                        t.device != styles.device for t, (shape, dtype) in zip(out, want)):
            raise L.HwgError("style_pair_stats: out must be contiguous tensors on %s of %s" % (
                styles.device, ", ".join("%s %s" % (dtype, list(shape)) for shape, dtype in want)))
    need = int(L.query("hwg_style_pair_stats_workspace", N, A, int(mode)))
    if need == 0:
        raise L.HwgError("style_pair_stats: N=%d A=%d mode=%d is beyond what the kernel takes" % (N, A, mode))
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=styles.device)
    elif not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous() or \
            workspace.device != styles.device or workspace.numel() < need:
        raise L.HwgError("style_pair_stats: workspace must be a contiguous uint8 tensor of at least %d bytes on %s" % (need, styles.device))
    L.call("hwg_style_pair_stats", styles, writer, N, D, A, int(mode), edge2, bins, out[0], out[1], out[2], out[3], out[4] if bins else None,
           workspace, workspace.numel(), _stream())
    return out if bins else out + (None,)


# ----------------------------------------------------------------------------------------------
# frozen BatchNorm (eval) and the FusedUpsample weight transform
# ----------------------------------------------------------------------------------------------
def norm_apply_frozen(x, running_mean, running_var, eps, gamma, beta, act=ACT_NONE, slope=0.0):
    if torch.is_grad_enabled() and (x.requires_grad or (gamma is not None and gamma.requires_grad)):
        raise L.HwgError("eval-mode BatchNorm has no backward kernel; run it under torch.no_grad()")
    N, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * C)
    y = torch.empty_like(x)
    mean = torch.empty((N, C), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    L.call("hwg_norm_frozen_fwd", x, y, N, HW, C, running_mean, running_var, eps, gamma, beta, act, slope, mean, rstd, _stream())
    return y


class _FusedUpWeight(Function):
    """[A,B,3,3] -> [A,B,4,4]: the averaged-shift weight of the reference's FusedUpsample (model/pure_gen.py:268-276)"""

    @staticmethod
    def forward(ctx, w3, mult):
        _chk(w3, "fused upsample weight")
        A, B = w3.shape[0], w3.shape[1]
        w4 = torch.empty((A, B, 4, 4), dtype=torch.float32, device=w3.device)
        L.call("hwg_fused_upsample_weight_fwd", w3, w4, A * B, mult, _stream())
        ctx.cfg = (A, B, mult)
        ctx.param_refs = (w3,)
        return w4

    @staticmethod
    def backward(ctx, dw4):
        A, B, mult = ctx.cfg
        (wref,) = ctx.param_refs
        if _direct(wref):      # a parameter: added where parameter gradients live (the current set or the redirected one), no add launch behind it
            L.call("hwg_fused_upsample_weight_bwd_acc", dw4.contiguous(), _grad_buffer(wref), A * B, mult, _stream())
            return None, None
        dw3 = torch.empty((A, B, 3, 3), dtype=torch.float32, device=dw4.device)
        L.call("hwg_fused_upsample_weight_bwd", dw4.contiguous(), dw3, A * B, mult, _stream())
        return dw3, None


def fused_upsample_weight(w3, mult):
    return _FusedUpWeight.apply(w3, float(mult))


class _Scale(Function):
    """y = x * c with a python constant (EqualLR weight scaling, loss weights)"""

    @staticmethod
    def forward(ctx, x, c):
        y = torch.empty_like(x)
        L.call("hwg_axpby", x, float(c), None, 0.0, y, x.numel(), _stream())
        ctx.c = float(c)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = torch.empty_like(dy)
        L.call("hwg_axpby", dy.contiguous(), ctx.c, None, 0.0, dx, dy.numel(), _stream())
        return dx, None


def scale(x, c):
    if float(c) == 1.0:       # (the adversarial losses carry weight 1 in every shipped config: no launch, forward or backward)
        return x
    return _Scale.apply(x.contiguous(), c)


class _WeightedSum(Function):
    """(sum_i w_i x_i, [w_i x_i]) over 0-dim tensors in ONE launch per direction - the trainer's weighted loss accumulation, rounded like the
    chain of scale / add launches it replaces (every product and every partial sum in fp32, left to right; w == 1 multiplies nothing)"""

    @staticmethod
    def forward(ctx, weights, *xs):
        import numpy as np
        n = len(xs)
        xs = [x.contiguous() for x in xs]
        total = torch.empty((), dtype=torch.float32, device=xs[0].device)
        scaled = torch.empty((n,), dtype=torch.float32, device=xs[0].device)
        ptrs = np.array([x.data_ptr() for x in xs], dtype=np.int64)
        w = np.array(weights, dtype=np.float32)
        L.call("hwg_weighted_sum", ptrs.ctypes.data, w.ctypes.data, n, scaled, total, _stream())
        ctx.w = w
        ctx.mark_non_differentiable(scaled)
        return total, scaled

    @staticmethod
    def backward(ctx, g, _unused):
        n = len(ctx.w)
        out = torch.empty((n,), dtype=torch.float32, device=g.device)
        L.call("hwg_weighted_sum_bwd", g.contiguous(), ctx.w.ctypes.data, n, out, _stream())
        return (None,) + tuple(out[i].reshape(()) if ctx.needs_input_grad[1 + i] else None for i in range(n))


def weighted_sum(xs, weights):
    """-> (sum_i weights[i] * xs[i] as a 0-dim tensor, the n scaled terms as a [n] tensor (no gradient))"""
    return _WeightedSum.apply(tuple(float(w) for w in weights), *xs)


class _Add(Function):
    """z = a*x + b*y (residual adds, loss sums)"""

    @staticmethod
    def forward(ctx, x, y, a, b):
        z = torch.empty_like(x)
        L.call("hwg_axpby", x, float(a), y, float(b), z, x.numel(), _stream())
        ctx.ab = (float(a), float(b))
        return z

    @staticmethod
    def backward(ctx, dz):
        a, b = ctx.ab
        dz = dz.contiguous()
        dx = dz if a == 1.0 else scale(dz, a)
        dy = dz if b == 1.0 else scale(dz, b)
        return dx, dy, None, None


def add(x, y, a=1.0, b=1.0):
    assert x.shape == y.shape
    return _Add.apply(x.contiguous(), y.contiguous(), a, b)


class _SplitCols(Function):
    """x [rows, sum(widths)] -> tuple of contiguous [rows, w_i] column blocks"""

    @staticmethod
    def forward(ctx, x, *widths):
        _chk(x, "split input")
        rows, Ct = x.shape
        outs = []
        off = 0
        st = _stream()
        for w in widths:
            o = torch.empty((rows, w), dtype=torch.float32, device=x.device)
            L.call("hwg_copy_channels", x, Ct, off, o, w, 0, w, rows, 1, 0, 0, st)
            outs.append(o)
            off += w
        ctx.cfg = (rows, Ct, widths)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        rows, Ct, widths = ctx.cfg
        dx = torch.empty((rows, Ct), dtype=torch.float32, device=grads[0].device)
        off = 0
        st = _stream()
        for g, w in zip(grads, widths):
            L.call("hwg_copy_channels", g.contiguous(), w, 0, dx, Ct, off, w, rows, 1, 0, 0, st)
            off += w
        return (dx,) + (None,) * len(widths)


def split_cols(x, widths):
    assert sum(widths) == x.shape[1]
    return _SplitCols.apply(x.contiguous(), *widths)


class _ChannelAffine(Function):
    """y = x * scale[c] + shift[c] over the last dim"""

    @staticmethod
    def forward(ctx, x, scale_, shift):
        _chk(x, "channel_affine input"); _chk(scale_, "scale"); _chk(shift, "shift")
        C = x.shape[-1]
        y = torch.empty_like(x)
        L.call("hwg_channel_affine", x, scale_, shift, y, x.numel() // C, C, _stream())
        ctx.save_for_backward(x, scale_)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, scale_ = ctx.saved_tensors
        dy = dy.contiguous()
        C = x.shape[-1]
        rows = x.numel() // C
        st = _stream()
        dx = torch.empty_like(x)
        L.call("hwg_channel_affine", dy, scale_, None, dx, rows, C, st)
        prod = torch.empty_like(x)
        L.call("hwg_mul", dy, x, prod, x.numel(), st)
        ds = colsum(prod.view(rows, C))
        dm = colsum(dy.view(rows, C))
        return dx, ds, dm


def channel_affine(x, scale_, shift):
    return _ChannelAffine.apply(x.contiguous(), scale_.contiguous(), shift.contiguous())


class _Permute(Function):
    """contiguous copy of x.permute(perm) for tensors of rank <= 4 (one strided-gather kernel)"""

    @staticmethod
    def forward(ctx, x, perm):
        _chk(x, "permute input")
        nd = x.dim()
        assert nd <= 4 and sorted(perm) == list(range(nd))
        shape = list(x.shape)
        strides = [1] * nd
        for i in range(nd - 2, -1, -1):
            strides[i] = strides[i + 1] * shape[i + 1]
        odims = [shape[p] for p in perm]
        ostr = [strides[p] for p in perm]
        pad = 4 - nd
        out = permute4(x, [1] * pad + odims, [0] * pad + ostr).view(odims)
        ctx.perm = perm
        return out

    @staticmethod
    def backward(ctx, dy):
        perm = ctx.perm
        inv = [0] * len(perm)
        for i, p in enumerate(perm):
            inv[p] = i
        return _Permute.apply(dy.contiguous(), tuple(inv)), None


def permute(x, perm):
    return _Permute.apply(x.contiguous(), tuple(perm))


def permute_bl_to_lb(x):
    """[B,1,L,C] -> [L,B,C]"""
    B, _, Lr, C = x.shape
    return permute(x.view(B, Lr, C), (1, 0, 2))


def permute_lb_to_bl(x):
    """[L,B,C] -> [B,1,L,C]"""
    Lr, B, C = x.shape
    return permute(x, (1, 0, 2)).view(B, 1, Lr, C)


class _MulConst(Function):
    """y = x * m with m a constant tensor of the same shape (elementwise dropout masks)"""

    @staticmethod
    def forward(ctx, x, m):
        _chk(x, "mul input"); _chk(m, "mul mask")
        y = torch.empty_like(x)
        L.call("hwg_mul", x, m, y, x.numel(), _stream())
        ctx.save_for_backward(m)
        return y

    @staticmethod
    def backward(ctx, dy):
        (m,) = ctx.saved_tensors
        dx = torch.empty_like(m)
        L.call("hwg_mul", dy.contiguous(), m, dx, m.numel(), _stream())
        return dx, None


def mul_const(x, m):
    return _MulConst.apply(x.contiguous(), m)


class _RepeatRows(Function):
    """[n, C] -> [n*k, C], every row repeated k times consecutively (style per author -> per line)"""

    @staticmethod
    def forward(ctx, x, k):
        _chk(x, "repeat_rows input")
        n, C = x.shape
        out = torch.empty((n * k, C), dtype=torch.float32, device=x.device)
        L.call("hwg_copy_channels", x, C, 0, out, C, 0, C, n * k, k, 1, 0, _stream())
        ctx.cfg = (n, C, k)
        return out

    @staticmethod
    def backward(ctx, dy):
        n, C, k = ctx.cfg
        dx = torch.empty((n, C), dtype=torch.float32, device=dy.device)
        L.call("hwg_reduce_rows", dy.contiguous(), C, 0, dx, C, n, k, 0, _stream())
        return dx, None


def repeat_rows(x, k):
    return _RepeatRows.apply(x.contiguous(), int(k))


class _ZeroRowsFrom(Function):
    """y = x with x[pos:] = 0 along dim 0 (the in-place `counts[pos:] = 0` of trainer :697)"""

    @staticmethod
    def forward(ctx, x, pos):
        y = x.clone()
        y[pos:].zero_()
        ctx.pos = pos
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = dy.clone()
        dx[ctx.pos:].zero_()
        return dx, None


def zero_rows_from(x, pos):
    return _ZeroRowsFrom.apply(x, int(pos))


# ----------------------------------------------------------------------------------------------
# bank of linear layers sharing one input (generator AdaIN affines)
# ----------------------------------------------------------------------------------------------
class LinearBank:
    """Evaluates L `Linear(I, O_l)` modules on the same input in one launch (forward) / two launches (backward) through device pointer
    tables; the modules keep their own parameters. Each layer's output comes back split in `halves` contiguous [B, O_l/halves] tensors."""

    def __init__(self, linears, halves=2):
        import numpy as np
        self.linears = list(linears)
        self.halves = halves
        self.L = len(self.linears)
        self.I = self.linears[0].weight.shape[1]
        self.O = [int(m.weight.shape[0]) for m in self.linears]
        assert all(m.weight.shape[1] == self.I for m in self.linears) and all(o % halves == 0 for o in self.O)
        self.first = np.concatenate([[0], np.cumsum(self.O)]).astype(np.int32)
        self.total = int(self.first[-1])
        self._tab = None
        self._key = None
        self._gtab = None
        self._gkey = None

    def tables(self, device, B):
        import numpy as np
        key = (self.linears[0].weight.data_ptr(), str(device), B)
        if self._key != key:
            off = (self.first[:-1].astype(np.int64)) * B
            ints = h2d(np.concatenate([np.array(self.O, dtype=np.int32), self.first]), device)
            ptrs = h2d(np.concatenate([np.array([m.weight.data_ptr() for m in self.linears], dtype=np.int64),
                                       np.array([m.bias.data_ptr() for m in self.linears], dtype=np.int64), off]), device)
            L_ = self.L
            self._tab = (ints[:L_], ints[L_:], ptrs[:L_], ptrs[L_:2 * L_], ptrs[2 * L_:])
            self._key = key
        return self._tab

    def grad_tables(self, device):
        import numpy as np
        # (_grad_buffer also marks the tensors touched for the trainer's None-gradient bookkeeping; frozen parameters get a null entry)
        gw = [_grad_buffer(m.weight) if m.weight.requires_grad else None for m in self.linears]
        gb = [_grad_buffer(m.bias) if m.bias.requires_grad else None for m in self.linears]
        addr = [g.data_ptr() if g is not None else 0 for g in gw + gb]
        key = tuple(addr)
        if self._gkey is None:
            self._gkey = {}
        tab = self._gkey.get(key)           # (one table per destination: the parameters' own gradients, or a stashed set's buffer)
        if tab is None:
            ptrs = h2d(np.array(addr, dtype=np.int64), device)
            tab = self._gkey[key] = (ptrs[:self.L], ptrs[self.L:])
        return tab

    def params(self):
        return [m.weight for m in self.linears] + [m.bias for m in self.linears]

    def __call__(self, x):
        # the parameters are passed to the autograd function although the kernels reach them through pointer tables: autograd must see
        # inputs that require grad, or - when x itself does not (the sampled styles of the text-only "gen" lessons) - it would never call
        # backward and the parameters would silently get no gradient
        outs = _LinearBank.apply(x.contiguous(), self, *self.params())
        h = self.halves
        return [outs[l * h:(l + 1) * h] for l in range(self.L)]


class _LinearBank(Function):
    @staticmethod
    def forward(ctx, x, bank, *params):
        _chk(x, "linear bank input")
        B, I = x.shape
        assert I == bank.I
        O, first, wptr, bptr, off = bank.tables(x.device, B)
        y = torch.empty((bank.total * B,), dtype=torch.float32, device=x.device)
        L.call("hwg_linear_bank_fwd", x, wptr, bptr, O, first, off, bank.L, B, I, bank.halves, bank.total, y, _stream())
        outs = []
        for l in range(bank.L):
            C = bank.O[l] // bank.halves
            base = int(bank.first[l]) * B
            for h in range(bank.halves):
                outs.append(y[base + h * B * C: base + (h + 1) * B * C].view(B, C))
        ctx.save_for_backward(x)
        ctx.bank = bank
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        import numpy as np
        (x,) = ctx.saved_tensors
        bank = ctx.bank
        B, I = x.shape
        O, first, wptr, bptr, off = bank.tables(x.device, B)
        keep = [g.contiguous() if g is not None else None for g in grads]
        dyptr = h2d(np.array([g.data_ptr() if g is not None else 0 for g in keep], dtype=np.int64), x.device)
        gw, gb = bank.grad_tables(x.device)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        need = L.query("hwg_linear_bank_bwd_workspace", bank.total, B, I)
        ws = workspace(need, x.device)
        L.call("hwg_linear_bank_bwd", x, dyptr, wptr, gw, gb, O, first, bank.L, B, I, bank.halves, bank.total, dx, ws, ws.numel(), _stream())
        return (dx, None) + (None,) * (2 * bank.L)      # parameter gradients were accumulated in place (grad_tables)


class MLPChain:
    """L square Linear(D, D) modules each followed by LeakyReLU(slope), evaluated in one launch per direction (style embedding MLP)"""

    def __init__(self, linears, slope):
        self.linears = list(linears)
        self.slope = float(slope)
        self.L = len(self.linears)
        self.D = int(self.linears[0].weight.shape[0])
        assert all(tuple(m.weight.shape) == (self.D, self.D) for m in self.linears)
        self._key = self._tab = self._gkey = self._gtab = None

    def tables(self, device):
        import numpy as np
        key = (self.linears[0].weight.data_ptr(), str(device))
        if self._key != key:
            p = h2d(np.array([m.weight.data_ptr() for m in self.linears] + [m.bias.data_ptr() for m in self.linears], dtype=np.int64), device)
            self._tab = (p[:self.L], p[self.L:])
            self._key = key
        return self._tab

    def grad_tables(self, device):
        import numpy as np
        gw = [_grad_buffer(m.weight) if m.weight.requires_grad else None for m in self.linears]
        gb = [_grad_buffer(m.bias) if m.bias.requires_grad else None for m in self.linears]
        addr = [g.data_ptr() if g is not None else 0 for g in gw + gb]
        key = tuple(addr)
        if self._gkey is None:
            self._gkey = {}
        tab = self._gkey.get(key)
        if tab is None:
            p = h2d(np.array(addr, dtype=np.int64), device)
            tab = self._gkey[key] = (p[:self.L], p[self.L:])
        return tab

    def params(self):
        return [m.weight for m in self.linears] + [m.bias for m in self.linears]

    def __call__(self, x):
        return _MLPChain.apply(x.contiguous(), self, *self.params())    # (parameters passed for autograd's sake, see LinearBank.__call__)


MLP_CHAIN_SPLIT = bool(int(os.environ.get("HWG_MLP_SPLIT", "1") or 0))


class _MLPChain(Function):
    @staticmethod
    def forward(ctx, x, chain, *params):
        _chk(x, "mlp chain input")
        B, D = x.shape
        assert D == chain.D
        wptr, bptr = chain.tables(x.device)
        acts = torch.empty((chain.L + 1, B, D), dtype=torch.float32, device=x.device)
        L.call("hwg_mlp_chain_fwd", x, wptr, bptr, chain.L, B, D, chain.slope, acts, _stream())
        ctx.save_for_backward(acts)
        ctx.chain = chain
        return acts[chain.L]

    @staticmethod
    def backward(ctx, dout):
        (acts,) = ctx.saved_tensors
        chain = ctx.chain
        _, B, D = acts.shape
        wptr, _ = chain.tables(acts.device)
        gw, gb = chain.grad_tables(acts.device)
        dx = torch.empty((B, D), dtype=torch.float32, device=acts.device) if ctx.needs_input_grad[0] else None
        if MLP_CHAIN_SPLIT:      # chain of data gradients on one workgroup, then all parameter gradients in parallel (bit-identical, 69 -> ~25 us)
            need = L.query("hwg_mlp_chain_bwd_workspace", chain.L, B, D)
            ws = workspace(need, acts.device)
            L.call("hwg_mlp_chain_bwd_split", dout.contiguous(), acts, wptr, gw, gb, chain.L, B, D, chain.slope, dx, ws, ws.numel(), _stream())
        else:
            L.call("hwg_mlp_chain_bwd", dout.contiguous(), acts, wptr, gw, gb, chain.L, B, D, chain.slope, dx, _stream())
        return (dx, None) + (None,) * (2 * chain.L)


# ----------------------------------------------------------------------------------------------
# bidirectional LSTM (csrc/lstm.hip): the CRNN recogniser's recurrence
# ----------------------------------------------------------------------------------------------
_lstm_pack_cache = {}     # (id(w_f), id(w_r)) -> [stamp, [2][H][4H] transposed image, (w_f, w_r)]


def _weight_stamp(w):
    return (w.data_ptr(), w._version, WEIGHT_EPOCH.get(getattr(w, "_hwg_group", None), 0))


def _lstm_packed_whh(w_f, w_r):
    """the [2][H][4H] image of W_hh the backward kernel reads: written once per weight epoch for parameters (as _pack does for conv weights),
    per call for anything else"""
    H = w_f.shape[1]
    cacheable = isinstance(w_f, torch.nn.Parameter) and isinstance(w_r, torch.nn.Parameter)
    key = stamp = hit = None
    if cacheable:
        key, stamp = (id(w_f), id(w_r)), (_weight_stamp(w_f), _weight_stamp(w_r))
        hit = _lstm_pack_cache.get(key)
        if hit is not None and hit[0] == stamp:
            return hit[1]
    out = hit[1] if hit is not None else torch.empty((2, H, 4 * H), dtype=torch.float32, device=w_f.device)
    L.call("hwg_lstm_pack_whh", w_f, w_r, H, out, _stream())
    if cacheable:
        _lstm_pack_cache[key] = [stamp, out, (w_f, w_r)]
    return out


def _linear_wgrad(x2d, dy2d, weight):
    """dW [O, I] = dy2d^T x2d through the convolution weight-gradient path (one GEMM over all rows). -> the gradient as a tensor, or None where the
    kernel accumulated straight into the parameter's gradient buffer"""
    rows, I = x2d.shape
    ctx = _TapeCtx((False, True, False))
    ctx.saved_tensors = (x2d.view(rows, 1, 1, I), weight)
    ctx.scope = SCOPE
    ctx.has_bias = False
    ctx.param_refs = (weight, None)
    ctx.geom = ((1, 1), (0, 0), (1, 1), False, 1, 1)
    return _Conv2d._wgrad(ctx, dy2d.view(rows, 1, 1, dy2d.shape[1]))[0]


class _LSTMLayer(Function):
    """one bidirectional LSTM layer given its input projections: xp_f / xp_r [T,B,4H] (x W_ih^T + b_ih of the forward / reverse direction),
    W_hh [4H,H] and b_hh [4H] per direction -> y [T,B,2H]"""

    @staticmethod
    def forward(ctx, xp_f, xp_r, w_f, w_r, b_f, b_r, may_keep):
        for t_, n_ in ((xp_f, "lstm xproj"), (xp_r, "lstm xproj (reverse)"), (w_f, "lstm W_hh"), (w_r, "lstm W_hh (reverse)"), (b_f, "lstm b_hh"), (b_r, "lstm b_hh (reverse)")):
            _chk(t_, n_)
        T, B, G = xp_f.shape
        H = G // 4
        if tuple(w_f.shape) != (G, H) or tuple(w_r.shape) != (G, H) or b_f.numel() != G or b_r.numel() != G or tuple(xp_r.shape) != (T, B, G) or G != 4 * H:
            raise L.HwgError("lstm_layer: shapes do not fit (xproj %s / %s, W_hh %s / %s)" % (tuple(xp_f.shape), tuple(xp_r.shape), tuple(w_f.shape), tuple(w_r.shape)))
        dev = xp_f.device
        y = torch.empty((T, B, 2 * H), dtype=torch.float32, device=dev)
        # what the backward pass reads (gates, c, the h_prev rows) is written only when one can follow. `may_keep` is lstm_layer's answer to
        # "is a tape recording, or is autograd" - asked THERE, because inside a Function's forward grad mode is always off, and torch fills
        # needs_input_grad from requires_grad whatever the mode outside. Train and eval mode alike: the GAN lessons differentiate through a
        # recogniser either way. Otherwise - validation, any forward under no_grad - two ping-pong c buffers.
        keep = bool(may_keep) and any(ctx.needs_input_grad[:6])
        if keep:
            gates = torch.empty((2, T, B, G), dtype=torch.float32, device=dev)
            c = torch.empty((2, T, B, H), dtype=torch.float32, device=dev)
            hseq = torch.empty((2, T + 1, B, H), dtype=torch.float32, device=dev)
        else:
            gates = hseq = None
            c = workspace(2 * 2 * B * H * 4, dev)
        L.call("hwg_lstm_fwd", xp_f, xp_r, w_f, w_r, b_f, b_r, y, gates, c, hseq, T, B, H, int(keep), _stream())
        if keep:
            ctx.save_for_backward(gates, c, hseq, w_f, w_r)
            ctx.param_refs = (w_f, w_r, b_f, b_r)
        return y

    @staticmethod
    def backward(ctx, dy):
        gates, c, hseq, w_f, w_r = ctx.saved_tensors
        _, T, B, G = gates.shape
        H = G // 4
        dev = gates.device
        wt = _lstm_packed_whh(w_f, w_r)
        dgates = torch.empty_like(gates)
        ws = workspace(2 * 2 * B * H * 4, dev)
        L.call("hwg_lstm_bwd", dy.contiguous(), gates, c, wt, dgates, ws, T, B, H, _stream())
        need = ctx.needs_input_grad
        wf_ref, wr_ref, bf_ref, br_ref = ctx.param_refs
        out = [dgates[0] if need[0] else None, dgates[1] if need[1] else None, None, None, None, None, None]
        for d, (wref, bref) in enumerate(((wf_ref, bf_ref), (wr_ref, br_ref))):
            dg2 = dgates[d].view(T * B, G)
            if need[2 + d]:
                hprev = (hseq[0, :T] if d == 0 else hseq[1, 1:]).reshape(T * B, H)      # (contiguous row ranges: views)
                out[2 + d] = _linear_wgrad(hprev, dg2, wref)
            if need[4 + d]:
                if _direct(bref):
                    colsum(dg2, out=_grad_buffer(bref).view(-1), accumulate=True)
                else:
                    out[4 + d] = colsum(dg2).view(bref.shape)
        return tuple(out)


def _pair_of(v, what):
    if isinstance(v, torch.Tensor):
        if v.shape[0] != 2:
            raise L.HwgError("lstm_layer: %s must be a (forward, reverse) pair or a tensor stacked [2, ...]" % what)
        return v[0], v[1]
    a, b = v
    return a, b


def lstm_layer(xproj, w_hh, b_hh, training=False):
    """One bidirectional LSTM layer. Each of xproj, w_hh, b_hh is a (forward, reverse) pair - or one tensor stacked [2, ...] -: xproj [T,B,4H]
    per direction (the input projection x W_ih^T + b_ih, an ops.linear per direction, which owns dx and dW_ih), w_hh [4H,H], b_hh [4H].
    -> y [T,B,2H], forward direction in [..., :H]. The gates are kept for a backward pass exactly when one can follow (autograd is recording
    and an input requires grad, or a tape records the call); under no_grad the kernel keeps two ping-pong c buffers instead. `training` is not
    read: the layer computes the same thing in train and eval mode (the dropout between layers is ops.bilstm's business); the argument is
    kept only so that the call reads like its siblings."""
    xf, xr = _pair_of(xproj, "xproj")
    wf, wr = _pair_of(w_hh, "w_hh")
    bf, br = _pair_of(b_hh, "b_hh")
    # (the rule of adain_epilogue: a tape, or autograd recording with something to differentiate)
    may_keep = TAPE is not None or (torch.is_grad_enabled() and any(t.requires_grad for t in (xf, xr, wf, wr, bf, br)))
    return _LSTMLayer.apply(xf, xr, wf, wr, bf, br, may_keep)


def lstm_limits(H):
    """(unit slice, batch tile) of the LSTM kernels for hidden size H: H must be a multiple of the slice; wider batches run in tiles"""
    return int(L.query("hwg_lstm_unit_slice")), int(L.query("hwg_lstm_batch_tile", int(H)))


def bilstm(x_TBC, params, p_drop, training, masks=None):
    """Stacked bidirectional LSTM. x [T,B,I]; params: per layer ((w_ih_f, w_hh_f, b_ih_f, b_hh_f), (the same four of the reverse direction)).
    Per layer: ops.linear per direction -> lstm_layer -> (between layers, training with p_drop > 0 only) an elementwise dropout multiplier
    over [T,B,2H] holding 0 or 1/(1-p): rng.seq_mask, or `masks[layer]` when supplied. -> [T,B,2H]"""
    from . import rng
    T, B, _ = x_TBC.shape
    h = x_TBC
    for li, (pf, pr) in enumerate(params):
        rows = h.contiguous().view(T * B, h.shape[2])
        G = pf[0].shape[0]
        xf = linear(rows, pf[0], pf[2]).view(T, B, G)
        xr = linear(rows, pr[0], pr[2]).view(T, B, G)
        h = lstm_layer((xf, xr), (pf[1], pr[1]), (pf[3], pr[3]), training)
        if li + 1 < len(params):
            m = masks[li] if masks is not None else (rng.seq_mask(tuple(h.shape), p_drop, h.device) if (training and p_drop > 0) else None)
            if m is not None:
                h = mul_const(h, m)
    return h


# ----------------------------------------------------------------------------------------------
# cache maintenance
# ----------------------------------------------------------------------------------------------
def _cache_dicts():
    from . import replay
    return [_pack_cache, _pack_tables, _lstm_pack_cache, _set_views, replay._programs]


def cache_mark():
    """what the module-level caches hold now (packed weight images and their refresh tables, the LSTM's transposed W_hh images, gradient-set
    views, recorded replay programs): hand it to drop_caches(since=...) later to drop only what was added in between"""
    return [set(c.keys()) for c in _cache_dicts()]


def drop_caches(since=None):
    """Forget cached images / programs: all of them, or those added after `since` (a cache_mark()). The caches reference every parameter they
    have seen for the rest of the process - and through a parameter's flat-buffer attributes its trainer -; a process that builds models or
    trainers it is done with (tests, sweeps) calls this to let them go. Everything dropped is rebuilt on next use. -> entries dropped"""
    n = 0
    dicts = _cache_dicts()
    for c, keep in zip(dicts, since if since is not None else [()] * len(dicts)):
        for k in [k for k in c if k not in keep]:
            del c[k]
            n += 1
    return n

