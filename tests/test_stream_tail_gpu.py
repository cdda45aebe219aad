"""GPU: the data-movement kernels of a training step that were rescheduled without changing a bit of their results - the max-pool backward
kernels (window-major scatter for windows that do not overlap, row-decoded gather with vector loads for those that do), the multi-tensor
optimizer kernels (several workgroups per chunk) and the CTC beta recursion (run beside alpha in the forward launch).

Max-pool backward is a routing of dy: compared with torch.equal on the int32 view (the sign of a zero counts) against the backward of
torch.nn.functional.max_pool2d on the CPU. With relu=True the kernels' definition is dx = scatter(dy * [y > 0]), y the pooled output after
the ReLU: the reference gates dy the same way (one exact fp32 product) before torch's backward; a window whose maximum is NaN has y = 0.
The multi-tensor kernels write every element from that element alone: the same call through two chunk tables must give the same bits.
Adam is held to the per-element bounds of tests/test_optim_rng_fp64_gpu.py (adam_bounds of tests/_optim_rng_checks.py, restated here). The two CTC paths must agree bit
for bit and sit within the tolerance tests/test_ops_gpu.py::test_log_softmax_ctc holds ops.ctc_loss to against F.ctc_loss."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import optim_ref as R
from _fp64 import _f32

pytestmark = pytest.mark.gpu

E = 2.0 ** -24            # one fp32 rounding, relative
SLACK = 1.01


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- max-pool backward -----------------------------------------------------------------------------------------------------------------------
POOL_2X2 = ((2, 2), (2, 2), (0, 0))
POOL_OVERLAP = ((2, 2), (2, 1), (0, 1))
POOL_CASES = [
    # name, (N, H, W, C), pool
    ("2x2_uncovered_row_col", (2, 5, 7, 8), POOL_2X2),
    ("2x2_single_window", (1, 2, 2, 4), POOL_2X2),
    ("2x2_c6_v2", (2, 4, 6, 6), POOL_2X2),
    ("overlap_pad", (2, 4, 5, 8), POOL_OVERLAP),
    ("overlap_pad_one_column", (1, 2, 1, 4), POOL_OVERLAP),
    # more than one workgroup; an odd channel count (one channel per thread)
    ("2x2_blocks", (3, 9, 21, 36), POOL_2X2),
    ("2x2_c3_v1", (2, 5, 4, 3), POOL_2X2),
    ("overlap_blocks", (3, 6, 100, 12), POOL_OVERLAP),
]


def _pool_inputs(shape, pool, seed):
    """x in NHWC: small integers (exact ties in most windows), one NaN, one all-negative window; dy with -0.0 in a third of its elements"""
    N, H, W, C = shape
    (kh, kw), (sh, sw), (ph, pw) = pool
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, shape, generator=g).float()
    x[0, 0:min(kh, H), 0:min(kw, W), :] = -3.0                                             # a window that is all negative and all tied
    x[0, 0, 0, C - 1] = -1.0                                                               # (its last channel: a negative maximum)
    x[N - 1, H - 1, 0, 0] = float("nan")
    P = (H + 2 * ph - kh) // sh + 1
    Q = (W + 2 * pw - kw) // sw + 1
    dy = torch.randn((N, P, Q, C), generator=g)
    dy[torch.rand((N, P, Q, C), generator=g) < 0.33] = -0.0
    return x, dy


def _pool_reference(x, dy, pool, relu):
    kernel, stride, padding = pool
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(xr, kernel, stride, padding)
    gy = dy.permute(0, 3, 1, 2).contiguous()
    if relu:
        gy = gy * (torch.relu(y.detach()) > 0).float()
    y.backward(gy)
    return xr.grad.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_maxpool_bwd_routes_exactly(cuda, case, relu):
    from handwriting_line_generation_amd import ops
    name, shape, pool = case
    x, dy = _pool_inputs(shape, pool, seed=len(name) + 7 * shape[2])
    assert bool((_bits(dy) == _bits(torch.tensor(-0.0))).any()) and bool(torch.isnan(x).any())
    want = _pool_reference(x, dy, pool, relu)
    xg = x.to(cuda).requires_grad_(True)
    y = ops.max_pool2d(xg, *pool, relu=relu)
    y.backward(dy.to(cuda))
    got = xg.grad
    same = _bits(got) == _bits(want)
    assert bool(same.all()), "maxpool_bwd %s relu=%s: %d of %d elements differ, first at %s" % (
        name, relu, int((~same).sum()), same.numel(), (~same).nonzero()[0].tolist())
    assert not bool((_bits(got) == _bits(torch.tensor(-0.0))).any()), "a routed -0.0 gradient is 0 + (-0.0) = +0.0"


# ---- multi-tensor optimizer kernels -------------------------------------------------------------------------------------------------------------
MT_NUMEL = [1, 3, 4, 1027, 8, 37, 70001]        # 70001: more than one default chunk, and every piece of a cut chunk has work
MT_ABSENT, MT_CLIP_ONLY = 4, 5                  # pointer 0 in every table / gradient only (no parameter entry)
MT_CLIP = 2.0
MT_GUARD = 64
MT_SENTINEL = -123.0


class _MtList:
    def __init__(self, cuda, chunk):
        from handwriting_line_generation_amd import ops
        self.ops, self.cuda, self.chunk = ops, cuda, chunk
        numel = np.array(MT_NUMEL, dtype=np.int64)
        padded = (numel + 3) // 4 * 4
        self.offsets = MT_GUARD + np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        self.total = int(MT_GUARD + padded.sum() + MT_GUARD)
        self.nt = len(MT_NUMEL)
        ct, co = [], []
        for k in range(self.nt):
            for off in range(0, int(numel[k]), chunk):
                ct.append(k); co.append(off)
        self.nchunks = len(ct)
        self.geom = (ops.h2d(numel, cuda), ops.h2d(np.array(ct, dtype=np.int32), cuda), ops.h2d(np.array(co, dtype=np.int64), cuda), self.nchunks, chunk)
        self.present = np.array([k != MT_ABSENT for k in range(self.nt)])
        self.stepped = self.present & np.array([k != MT_CLIP_ONLY for k in range(self.nt)])

    def mask(self, tensors):
        m = np.zeros(self.total, dtype=bool)
        for k in range(self.nt):
            if tensors[k]:
                m[self.offsets[k]: self.offsets[k] + MT_NUMEL[k]] = True
        return m

    def ptrs(self, bufs, masks):
        rows = [(b.data_ptr() + self.offsets * 4) * m.astype(np.int64) for b, m in zip(bufs, masks)]
        return self.ops.h2d(np.stack(rows), self.cuda)


def _mt_chunks():
    from handwriting_line_generation_amd.trainer.flat_params import CHUNK
    return 4, CHUNK          # the smallest chunk the 16-byte paths allow, and the trainer's


def _mt_host_buffers(lay):
    g = torch.Generator().manual_seed(31)
    n = lay.total
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g)
    grad[torch.rand(n, generator=g) < 0.05] *= 40.0          # beyond +-clip
    m = 0.1 * torch.randn(n, generator=g)
    v = (0.1 * torch.randn(n, generator=g)) ** 2
    o = lay.offsets
    grad[o[3] + 5] = float("nan"); grad[o[3] + 6] = float("inf"); grad[o[3] + 1026] = -float("inf")      # stepped tensor, body and scalar tail
    grad[o[5] + 2] = float("nan"); grad[o[5] + 36] = float("inf")                                            # clip-only tensor
    grad[o[6] + 65536 + 4464] = 77.0; grad[o[6] + 70000] = -77.0
    live = torch.from_numpy(lay.mask(np.ones(lay.nt, dtype=bool)))
    for t in (p, grad, m, v):
        t[~live] = MT_SENTINEL
    return p, grad, m, v


def _adam_bounds(p0, g, m0, v0, ss, bc2, b1, b2, eps, ref):
    """tests/_optim_rng_checks.py::adam_bounds, restated: every operation one fp32 rounding, division and square root two"""
    pr, _, mr, vr = ref
    c1 = 1.0 - b1
    bm = SLACK * E * (2 * ((g - m0) * c1).abs() + mr.abs())
    bv = SLACK * 3.5 * E * vr
    denom = vr.sqrt() / bc2 + eps
    u = ss * mr / denom
    bp = SLACK * (E * pr.abs() + 9.75 * E * u.abs() + ss * bm / denom)
    return bm, bv, bp


def test_mt_kernels_same_bits_through_two_chunk_tables(cuda):
    from handwriting_line_generation_amd import _lib as L
    from handwriting_line_generation_amd import ops
    results = {}
    lays = {}
    b1, b2, eps = _f32(0.5), _f32(0.999), _f32(1e-8)
    ss32 = np.linspace(1e-4, 3e-4, len(MT_NUMEL)).astype(np.float32)
    bc32 = np.linspace(0.05, 1.0, len(MT_NUMEL)).astype(np.float32)
    for chunk in _mt_chunks():
        lay = lays[chunk] = _MtList(cuda, chunk)
        host = _mt_host_buffers(lay)
        st = ops._stream()
        out = {}
        # unary: zero, clamp, copy, stash (through the present tensors only), and the non-finite scan
        for op, nm in ((0, "zero"), (1, "clamp"), (3, "copy"), (4, "stash")):
            a, b = host[1].to(cuda), host[0].to(cuda)
            tab = lay.ptrs([a, b], [lay.present, lay.present])
            L.call("hwg_mt_unary", tab[0], tab[1] if op >= 3 else None, op, MT_CLIP, None, *lay.geom, st)
            out["unary_" + nm] = (a.cpu(), b.cpu())
        flag = torch.zeros(1, dtype=torch.int32, device=cuda)
        L.call("hwg_mt_unary", lay.ptrs([host[1].to(cuda)], [lay.present])[0], None, 2, 0.0, flag, *lay.geom, st)
        out["scan_flag"] = (flag.cpu(),)
        # axpy over two sets; the second set lacks tensor 3, the first has a zero coefficient on tensor 0
        dst, s0, s1 = host[1].to(cuda).nan_to_num(0.0, 1.0, -1.0), host[2].to(cuda), host[3].to(cuda)
        m1 = lay.present & np.array([k != 3 for k in range(lay.nt)])
        tab = lay.ptrs([dst, s0, s1], [lay.present, lay.present, m1])
        coef = np.stack([np.linspace(0.0, 1.5, lay.nt), np.linspace(-2.0, 2.0, lay.nt)]).astype(np.float32)
        L.call("hwg_mt_axpy_sets", tab[0], tab[1:], ops.h2d(coef, cuda), 2, lay.nt, *lay.geom, st)
        out["axpy_sets"] = (dst.cpu(),)
        # clip + Adam in one launch
        bufs = [t.to(cuda) for t in host]
        flag = torch.zeros(1, dtype=torch.int32, device=cuda)
        tab = lay.ptrs(bufs, [lay.stepped, lay.present, lay.stepped, lay.stepped])
        sc = ops.h2d(np.stack([ss32, bc32]), cuda)
        L.call("hwg_mt_clip_adam", tab[0], tab[1], tab[2], tab[3], sc[0], sc[1], b1, b2, eps, MT_CLIP, flag, *lay.geom, st)
        out["clip_adam"] = tuple(b.cpu() for b in bufs) + (flag.cpu(),)
        results[chunk] = (host, out)
    small, default = _mt_chunks()
    assert lays[default].nchunks == len(MT_NUMEL) + 1 and lays[small].nchunks > 17000
    (host, a), (_, b) = results[small], results[default]
    for key in a:
        for i, (ta, tb) in enumerate(zip(a[key], b[key])):
            assert torch.equal(_bits(ta), _bits(tb)), "%s: output %d differs between chunk %d and chunk %d" % (key, i, small, default)

    # what the results must be (one table is enough now)
    lay = lays[default]
    p, g, m, v = host
    live = torch.from_numpy(lay.mask(lay.present))
    act = torch.from_numpy(lay.mask(lay.stepped))
    clamped = torch.where(live, R.clamp(g, MT_CLIP), g)
    zero = torch.zeros(())
    assert torch.equal(_bits(b["unary_zero"][0]), _bits(torch.where(live, zero, g)))
    assert torch.equal(_bits(b["unary_clamp"][0]), _bits(clamped))
    assert torch.equal(_bits(b["unary_copy"][0]), _bits(g)) and torch.equal(_bits(b["unary_copy"][1]), _bits(torch.where(live, g, p)))
    assert torch.equal(_bits(b["unary_stash"][0]), _bits(torch.where(live, zero, g))) and torch.equal(_bits(b["unary_stash"][1]), _bits(torch.where(live, g, p)))
    assert int(b["scan_flag"][0]) == 1
    gp, gg, gm, gv, gflag = b["clip_adam"]
    # the gradient buffer: clamp(g) on every tensor with a gradient (NaN kept), every other bit as it was - unclipped elements, the absent
    # tensor, padding and guards included
    assert torch.equal(_bits(gg), _bits(clamped)), "clip_adam: gradient buffer"
    assert bool(torch.isnan(gg[lay.offsets[3] + 5])) and bool(torch.isnan(gg[lay.offsets[5] + 2]))
    for nm, got, was in (("p", gp, p), ("m", gm, m), ("v", gv, v)):
        assert torch.equal(_bits(got[~act]), _bits(was[~act])), "clip_adam: %s written outside the stepped tensors" % nm
    tensor_of = np.zeros(lay.total, dtype=np.int64)
    for k in range(lay.nt):
        tensor_of[lay.offsets[k]: lay.offsets[k] + MT_NUMEL[k]] = k
    ss, bc = torch.from_numpy(ss32.astype(np.float64)[tensor_of]), torch.from_numpy(bc32.astype(np.float64)[tensor_of])
    ref = R.adam_step(p, g, m, v, ss, bc, b1, b2, eps, MT_CLIP)
    bounds = _adam_bounds(p.double(), ref[1], m.double(), v.double(), ss, bc, b1, b2, eps, ref)
    finite = act & torch.isfinite(ref[0])
    assert int((act & ~finite).sum()) == 1, "the NaN gradient of the stepped tensor"
    assert bool(torch.isnan(gp[act & ~finite]).all()) and int(gflag) == 1, "a NaN gradient reaches the parameter and raises the flag"
    worst = []
    for nm, got, want, bound in (("m", gm, ref[2], bounds[0]), ("v", gv, ref[3], bounds[1]), ("p", gp, ref[0], bounds[2])):
        err = (got.double() - want).abs()[finite]
        ratio = err / bound[finite].clamp(min=1e-300)
        print("clip_adam %s: worst error / derived bound %.3f" % (nm, float(ratio.max())))
        worst.append((nm, float(ratio.max())))
    for nm, r in worst:
        assert r <= 1.0, "clip_adam: %s off by %.3f of its bound" % (nm, r)


# ---- CTC: beta beside alpha in the forward launch ---------------------------------------------------------------------------------------------
def test_ctc_one_launch_equals_two_launches(cuda, monkeypatch):
    from handwriting_line_generation_amd import ops
    T, B, C, Lmax = 7, 3, 5, 3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, B, C, generator=g)
    targets = torch.tensor([[1, 1, 1], [4, 1, 1], [2, 2, 3]])       # lengths 0, 1, 3; the last has a repeated label
    tl = torch.tensor([0, 1, 3])
    il = torch.tensor([7, 5, 7])
    xr = x.clone().requires_grad_(True)
    loss_r = F.ctc_loss(F.log_softmax(xr, dim=2), targets, il, tl)
    loss_r.backward()

    def run(one_launch):
        monkeypatch.setattr(ops, "CTC_BETA_IN_FWD", one_launch)
        xg = x.to(cuda).requires_grad_(True)
        lp = torch.log_softmax(xg, dim=2)
        lp.retain_grad()
        loss = ops.ctc_loss(lp, targets, il, tl)
        loss.backward()
        return loss.detach().cpu(), lp.grad.cpu(), xg.grad.cpu()

    one, two = run(True), run(False)
    for nm, a, b in zip(("loss", "d log-probs", "d logits"), one, two):
        assert torch.equal(_bits(a), _bits(b)), "ctc %s: the one-launch path differs from the two-launch path" % nm
    assert torch.equal(one[1][5:, 1], torch.zeros(2, C)), "zero gradient behind the input length"
    for nm, res in (("one launch", one), ("two launches", two)):
        for what, got, want, tol in (("loss", res[0], loss_r.detach(), 1e-4), ("d logits", res[2], xr.grad, 2e-4)):
            scale = max(float(want.abs().max()), 1e-6)
            err = float((got - want).abs().max())
            print("ctc %s %s: max err %.3e (scale %.3e)" % (nm, what, err, scale))
            assert err <= tol * scale + 1e-6, "ctc %s %s: max err %.3e (scale %.3e)" % (nm, what, err, scale)
