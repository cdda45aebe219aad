"""GPU: the multi-tensor optimizer kernels, the Philox kernels and insert_spaces (csrc/optim_rng.hip, csrc/philox.h) against the plain
restatements of oracle/optim_ref.py, through the C entry points (pointer tables as the trainer builds them) and, where the wrapper is the
thing under test, through FlatParams / HipAdam / ops.DeviceRNG. Case tables and the regimes they reach: oracle/optim_cases.py; the
restatements, the tables and their sensitivity to seeded flaws are checked on the CPU by tests/test_optim_rng_ref_cpu.py.

Every tensor list lives in one flat buffer with a guard band in front and behind and with every tensor padded to four floats; guard and
padding hold a sentinel, and every comparison of a whole buffer (torch.equal) covers them and the tensors whose pointer entry is 0.

Exact results are compared with torch.equal. Floating-point results are held per element to bounds derived from the arithmetic (DERIVED and
adam_bounds of tests/_optim_rng_checks.py); the only measured bound is hwg_randn's (fp32 logf / sincosf). One line per case is printed."""
import math

import numpy as np
import pytest
import torch

from oracle import optim_cases as OC
from oracle import optim_ref as R
from _fp64 import _f32, cpu_threads
from _optim_rng_checks import DERIVED, RANDN_ABS, RANDN_DERIVED, ULP, adam_bounds, fp32_beta_distance

pytestmark = pytest.mark.gpu


class DevList:
    def __init__(self, cuda, entry):
        from handwriting_line_generation_amd import ops
        self.ops, self.cuda, self.name = ops, cuda, entry[0]
        self.lay, self.present = OC.list_layout(entry)
        lay = self.lay
        self.numel = ops.h2d(lay.numel, cuda)
        self.ct = ops.h2d(lay.chunk_tensor, cuda)
        self.co = ops.h2d(lay.chunk_off, cuda)
        self.geom = (self.numel, self.ct, self.co, lay.nchunks, lay.chunk)

    def ptrs(self, bufs, masks=None):
        """device int64 [len(bufs)][nt]: the tensors' addresses in each buffer, 0 where the mask (default: the list's present mask) is off"""
        rows = []
        for i, b in enumerate(bufs):
            m = self.present if masks is None else masks[i]
            assert b.numel() == self.lay.total and b.dtype == torch.float32 and b.is_contiguous()
            rows.append((b.data_ptr() + self.lay.offsets * 4) * m.astype(np.int64))
        return self.ops.h2d(np.stack(rows), self.cuda)

    def st(self):
        return self.ops._stream()


def _where_mask(mask_np, new, old):
    return torch.where(torch.from_numpy(mask_np), new, old)


def _same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@pytest.fixture(scope="module", params=OC.LISTS, ids=[e[0] for e in OC.LISTS])
def dlist(request, cuda):
    return DevList(cuda, request.param)


# ---- unary ops ---------------------------------------------------------------------------------------------------------------------------------
def test_unary_zero_copy_stash_clamp_exact(cuda, dlist):
    from handwriting_line_generation_amd import _lib as L
    lay, present = dlist.lay, dlist.present
    live = lay.mask(present)
    x = lay.buffer("unary_x_" + dlist.name, 3.0)
    i = torch.arange(lay.total)
    inside = torch.from_numpy(lay.mask())
    x[inside & (i % 89 == 1)] = 2.0
    x[inside & (i % 83 == 2)] = -2.0
    y0 = lay.buffer("unary_y_" + dlist.name)
    y_present = present.copy()
    y_present[5] = False                                   # a destination that is absent where the source exists: nothing is written
    both = lay.mask(present & y_present)
    # op 0: zero
    a = x.to(cuda)
    L.call("hwg_mt_unary", dlist.ptrs([a])[0], None, 0, 0.0, None, *dlist.geom, dlist.st())
    assert torch.equal(a.cpu(), _where_mask(live, torch.zeros_like(x), x)), "zero"
    # op 3: copy
    a, b = x.to(cuda), y0.to(cuda)
    tab = dlist.ptrs([a, b], [present, y_present])
    L.call("hwg_mt_unary", tab[0], tab[1], 3, 0.0, None, *dlist.geom, dlist.st())
    assert torch.equal(a.cpu(), x) and torch.equal(b.cpu(), _where_mask(both, x, y0)), "copy"
    # op 4: stash (copy, then zero the source; the source is zeroed also where the destination is absent)
    a, b = x.to(cuda), y0.to(cuda)
    tab = dlist.ptrs([a, b], [present, y_present])
    L.call("hwg_mt_unary", tab[0], tab[1], 4, 0.0, None, *dlist.geom, dlist.st())
    assert torch.equal(b.cpu(), _where_mask(both, x, y0)) and torch.equal(a.cpu(), _where_mask(live, torch.zeros_like(x), x)), "stash"
    # op 1: clamp
    a = x.to(cuda)
    L.call("hwg_mt_unary", dlist.ptrs([a])[0], None, 1, 2.0, None, *dlist.geom, dlist.st())
    want = _where_mask(live, R.clamp(x, 2.0), x)
    assert torch.equal(a.cpu(), want), "clamp"
    print("\nunary %-22s zero, copy, stash, clamp exact over %d floats (%d clipped, %d at the bound), canaries and absent tensors untouched"
          % (dlist.name, int(live.sum()), int((want != x).sum()), int((x[torch.from_numpy(live)].abs() == 2.0).sum())))


SCAN_CASES = [
    # name, list, (tensor, element) of the bad value or None, its value, expected flag
    ("clean", 0, None, None, 0),
    ("body", 0, (23, 5), float("nan"), 1),                       # first 16-byte piece of the large tensor
    ("tail", 0, (12, 1202), float("inf"), 1),                    # 1203 = 300 pieces + 3: the scalar tail
    ("last_chunk", 0, (23, 199001), float("-inf"), 1),           # chunk 3 of 4
    ("last_element", 1, (22, 131074), float("nan"), 1),          # the scalar tail of the last (3-element) chunk of 131075 at chunk 4096
    ("misaligned", 2, (17, 6000), float("nan"), 1),
    ("absent_tensor", 1, (11, 100), float("nan"), 0),            # a tensor whose pointer entry is 0 is not read
    ("padding", 0, (12, 1203), float("nan"), 0),                 # the pad float behind a tensor is not part of it
]


@pytest.mark.parametrize("case", SCAN_CASES, ids=[c[0] for c in SCAN_CASES])
def test_nonfinite_scan_exact(cuda, case):
    from handwriting_line_generation_amd import _lib as L
    name, li, where, value, want = case
    dl = DevList(cuda, OC.LISTS[li])
    x = dl.lay.buffer("scan_" + name)
    if where is not None:
        x[int(dl.lay.offsets[where[0]]) + where[1]] = value
    a = x.to(cuda)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda)
    L.call("hwg_mt_unary", dl.ptrs([a])[0], None, 2, 0.0, flag, *dl.geom, dl.st())
    assert int(flag.item()) == want, "scan %s: flag %d" % (name, int(flag.item()))
    assert _same_bits(a, x)
    print("\nscan %-14s flag %d" % (name, want))


# ---- abs-sum, axpy -----------------------------------------------------------------------------------------------------------------------------
def _set_masks(dlist, nsets):
    """present masks of nsets source sets: set k lacks tensor (2 k + 1) % nt on top of the list's own absent ones"""
    masks = []
    for k in range(nsets):
        m = dlist.present.copy()
        if nsets > 1:
            m[(2 * k + 1) % dlist.lay.nt] = False
        masks.append(m)
    return masks


def test_abs_sum_vs_fp64_and_sets_bit_identical(cuda, dlist):
    from handwriting_line_generation_amd import _lib as L
    lay, nt = dlist.lay, dlist.lay.nt
    worst = 0.0
    for nsets in (1, 2, 8):
        host = [lay.buffer("abssum_%s_%d" % (dlist.name, k), 10.0 ** (k % 3 - 1)) for k in range(nsets)]
        bufs = [h.to(cuda) for h in host]
        masks = _set_masks(dlist, nsets)
        tab = dlist.ptrs(bufs, masks)
        single = torch.full((nsets, nt), -1.0, dtype=torch.float64, device=cuda)
        part = torch.empty(lay.nchunks, dtype=torch.float64, device=cuda)
        for k in range(nsets):
            L.call("hwg_mt_abs_sum", tab[k], dlist.numel, dlist.ct, dlist.co, lay.nchunks, lay.chunk, nt, part, single[k], dlist.st())
        sets = torch.full((nsets, nt), -1.0, dtype=torch.float64, device=cuda)
        part = torch.empty(nsets * lay.nchunks, dtype=torch.float64, device=cuda)
        L.call("hwg_mt_abs_sum_sets", tab, nsets, dlist.numel, dlist.ct, dlist.co, lay.nchunks, lay.chunk, nt, part, sets, dlist.st())
        assert torch.equal(sets, single), "abs_sum_sets %s: %d sets differ from the one-set launches" % (dlist.name, nsets)
        got = single.cpu()
        for k in range(nsets):
            assert _same_bits(bufs[k], host[k])
            for t, sl in enumerate(lay.slices()):
                if not masks[k][t]:
                    assert float(got[k, t]) == 0.0, "abs_sum %s: absent tensor %d of set %d: %r" % (dlist.name, t, k, float(got[k, t]))
                    continue
                want = R.abs_sum(host[k][sl])
                rel = abs(float(got[k, t]) - want) / want
                worst = max(worst, rel)
                assert rel <= DERIVED["abs_sum_rel"], "abs_sum %s set %d tensor %d (%d elements): rel %.3e" % (dlist.name, k, t, lay.sizes[t], rel)
    print("\nabs_sum %-22s worst rel error vs fp64 %.2e (bound %.2e); 1, 2, 8 sets bit-identical to one-set launches" % (dlist.name, worst, DERIVED["abs_sum_rel"]))


def test_axpy_vs_fp64_and_sets_bit_identical(cuda, dlist):
    from handwriting_line_generation_amd import _lib as L
    lay, nt, present = dlist.lay, dlist.lay.nt, dlist.present
    cpu_threads()
    dst0 = lay.buffer("axpy_dst_" + dlist.name)
    worst = 0.0
    for nsets in (1, 2, 8):
        g = OC.gen("axpy_coef_%s_%d" % (dlist.name, nsets))
        coef = (torch.randn(nsets, nt, generator=g) * 0.7).float()
        coef[:, 4] = 0.0                                              # a zero coefficient: dst is not touched by that set
        coef[0, 20] = 0.0
        host = [lay.buffer("axpy_src_%s_%d" % (dlist.name, k)) for k in range(nsets)]
        srcs = [h.to(cuda) for h in host]
        masks = _set_masks(dlist, nsets)
        dcoef = coef.to(cuda)
        # the chain of one-set launches
        d1 = dst0.to(cuda)
        tab = dlist.ptrs([d1] + srcs, [present] + masks)
        ref = dst0.double()
        for k in range(nsets):
            before = d1.cpu().double()
            L.call("hwg_mt_axpy", tab[0], tab[1 + k], dcoef[k], *dlist.geom, dlist.st())
            live = lay.mask(present & masks[k])
            ck = torch.zeros(lay.total, dtype=torch.float64)
            ck[torch.from_numpy(lay.mask())] = coef[k].double()[torch.from_numpy(lay.tensor_of()[lay.mask()])]
            term = _where_mask(live, ck * host[k].double(), torch.zeros_like(ck))
            want = before + term                                      # from the device's own state before this launch: one launch is compared
            got = d1.cpu()
            err = (got.double() - want).abs()
            bound = DERIVED["axpy_ulps"] * ULP * (want.abs() + term.abs())
            assert bool((err <= bound).all()), "axpy %s set %d: element %d off by %.3e (bound %.3e)" % (
                dlist.name, k, int((err - bound).argmax()), float(err.max()), float(bound[(err - bound).argmax()]))
            untouched = torch.from_numpy(~live) | (term == 0)
            assert torch.equal(got[untouched], before.float()[untouched])
            worst = max(worst, float((err / (ULP * (want.abs() + term.abs())).clamp(min=1e-300)).max()))
            ref = ref + term
        # all sets in one pass
        d2 = dst0.to(cuda)
        tab2 = dlist.ptrs([d2] + srcs, [present] + masks)
        L.call("hwg_mt_axpy_sets", tab2[0], tab2[1:], dcoef, nsets, nt, *dlist.geom, dlist.st())
        assert torch.equal(d2, d1), "axpy_sets %s: %d sets differ from the chain of one-set launches" % (dlist.name, nsets)
        for k in range(nsets):
            assert _same_bits(srcs[k], host[k])
    # coef = NULL: c = 1
    d3, s3 = dst0.to(cuda), host[0].to(cuda)
    tab = dlist.ptrs([d3, s3])
    L.call("hwg_mt_axpy", tab[0], tab[1], None, *dlist.geom, dlist.st())
    assert torch.equal(d3.cpu(), _where_mask(lay.mask(present), dst0 + host[0], dst0)), "axpy with no coefficients"
    with pytest.raises(L.HwgError):                                   # nine sets: refused by the host-side argument check, nothing is launched
        L.call("hwg_mt_axpy_sets", tab2[0], tab2[1:], dcoef, 9, nt, *dlist.geom, dlist.st())
    torch.cuda.synchronize()
    print("\naxpy %-22s worst error %.2f of ulp (|result| + |c src|) (bound %.1f); 1, 2, 8 sets bit-identical to the chain; 9 sets refused"
          % (dlist.name, worst, DERIVED["axpy_ulps"]))


@pytest.mark.parametrize("case", OC.BALANCE_CASES, ids=[c[0] for c in OC.BALANCE_CASES])
def test_balance_coef_vs_fp64(cuda, case):
    from handwriting_line_generation_amd import _lib as L
    from handwriting_line_generation_amd import ops
    name, nt, ns, kind = case
    sum_d, sum_r, numel, gp, rp, xs = OC.balance_inputs(case)
    want = R.balance_coef(sum_d, sum_r, numel, gp, rp, xs)
    coef = torch.full((ns, nt), 777.0, dtype=torch.float32, device=cuda)
    # the kernel only tests the pointer entries against 0
    L.call("hwg_mt_balance_coef", ops.h2d(sum_d, cuda), ops.h2d(sum_r, cuda), ops.h2d(numel, cuda), ops.h2d(gp.astype(np.int64) * 16, cuda),
           ops.h2d(rp.astype(np.int64) * 16, cuda), ops.h2d(xs, cuda), ns, nt, coef, ops._stream())
    got = coef.cpu().double().numpy()
    zero = want == 0
    assert np.array_equal(got[zero], np.zeros(int(zero.sum()))), "balance %s: a coefficient that must be exactly 0" % name
    rel = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]) if (~zero).any() else np.zeros(1)
    print("\nbalance %-10s %d coefficients, %d exactly 0, worst rel error vs fp64 %.2e (bound %.2e)" % (name, want.size, int(zero.sum()), rel.max(),
                                                                                                         DERIVED["coef_rel"]))
    assert rel.max() <= DERIVED["coef_rel"]
    if kind == "all_zero_grad":
        assert zero.all()


def test_balance_end_to_end_leaves_dst_untouched_where_coef_is_zero(cuda):
    """abs-sum-sets -> coefficients -> axpy-sets over a real list, as FlatParams.balance chains them: a gradient that is all zero takes the
    replacement mean, a stashed tensor that is all zero or absent leaves the gradient as it was"""
    from handwriting_line_generation_amd import _lib as L
    from handwriting_line_generation_amd import ops
    dl = DevList(cuda, OC.LISTS[1])
    lay, nt, ns = dl.lay, dl.lay.nt, 2
    sl = lay.slices()
    grad = lay.buffer("bal_grad", 0.01)
    stash = [lay.buffer("bal_stash_%d" % k, 0.1) for k in range(ns)]
    grad[sl[14]] = 0.0                      # an all-zero gradient (2048 elements)
    stash[0][sl[9]] = 0.0                   # an all-zero stashed tensor
    masks = [dl.present.copy(), dl.present.copy()]
    masks[1][16] = False                    # an absent stashed tensor
    xs = np.array([0.5, -1.5], dtype=np.float32)
    dg, ds = grad.to(cuda), [s.to(cuda) for s in stash]
    tab = dl.ptrs([dg] + ds, [dl.present] + masks)
    sums = torch.empty((ns + 1, nt), dtype=torch.float64, device=cuda)
    part = torch.empty((ns + 1) * lay.nchunks, dtype=torch.float64, device=cuda)
    coef = torch.empty((ns, nt), dtype=torch.float32, device=cuda)
    L.call("hwg_mt_abs_sum_sets", tab, ns + 1, dl.numel, dl.ct, dl.co, lay.nchunks, lay.chunk, nt, part, sums, dl.st())
    L.call("hwg_mt_balance_coef", sums[0], sums[1:], dl.numel, tab[0], tab[1:], ops.h2d(xs, cuda), ns, nt, coef, dl.st())
    L.call("hwg_mt_axpy_sets", tab[0], tab[1:], coef, ns, nt, *dl.geom, dl.st())
    sd = [R.abs_sum(grad[s]) if dl.present[t] else 0.0 for t, s in enumerate(sl)]
    sr = [[R.abs_sum(stash[k][s]) if masks[k][t] else 0.0 for t, s in enumerate(sl)] for k in range(ns)]
    want_c = R.balance_coef(sd, sr, lay.numel, dl.present, np.stack(masks), xs)
    got_c = coef.cpu().double().numpy()
    assert np.array_equal(got_c[want_c == 0], np.zeros(int((want_c == 0).sum())))
    assert want_c[0, 9] == 0 and want_c[1, 16] == 0 and want_c[0, 14] != 0 and want_c[1, 14] != 0
    nz = want_c != 0
    # the sums carry DERIVED["abs_sum_rel"] each on top of the coefficient's own roundings
    assert float((np.abs(got_c[nz] - want_c[nz]) / np.abs(want_c[nz])).max()) <= DERIVED["coef_rel"] + 3 * DERIVED["abs_sum_rel"]
    want = grad.double()
    for k in range(ns):
        for t, s in enumerate(sl):
            if want_c[k, t] != 0:
                want[s] += float(got_c[k, t]) * stash[k][s].double()
    got = dg.cpu()
    err = (got.double() - want).abs()
    scale = grad.double().abs() + sum(abs(float(np.abs(got_c[k]).max())) * stash[k].double().abs() for k in range(ns))
    assert bool((err <= ns * ULP * scale).all())
    for t in (9, 16):                                                    # one set contributes nothing there, the other does
        assert not torch.equal(got[sl[t]], grad[sl[t]])
    dead = torch.from_numpy(~lay.mask(dl.present))
    assert torch.equal(got[dead], grad[dead])
    print("\nbalance end to end: replacement mean coefficient %.4g / %.4g on the all-zero gradient, exact zeros for the all-zero and the absent stash"
          % (got_c[0, 14], got_c[1, 14]))


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------------
def _per_element(lay, per_tensor):
    t = lay.tensor_of()
    return torch.from_numpy(np.where(t >= 0, np.asarray(per_tensor, dtype=np.float64)[np.maximum(t, 0)], 1.0))


def _adam_call(dl, kernel, bufs, masks, sc, betas, clip, flag=None):
    from handwriting_line_generation_amd import _lib as L
    tab = dl.ptrs(bufs, masks)
    if kernel == "adam":
        L.call("hwg_mt_adam", tab[0], tab[1], tab[2], tab[3], sc[0], sc[1], betas[0], betas[1], OC.ADAM_EPS, clip, *dl.geom, dl.st())
    else:
        L.call("hwg_mt_clip_adam", tab[0], tab[1], tab[2], tab[3], sc[0], sc[1], betas[0], betas[1], OC.ADAM_EPS, clip, flag, *dl.geom, dl.st())


def _check_adam(label, got, host, ref, bounds, active, zero):
    """got / host: (p, g, m, v) after (CPU) / before; ref: fp64 (p, g, m, v); active: bool numpy [total]. -> worst error / bound per quantity"""
    act = torch.from_numpy(active)
    worst = []
    for nm, i, b in (("m", 2, bounds[0]), ("v", 3, bounds[1]), ("p", 0, bounds[2])):
        assert bool(torch.isfinite(got[i][act]).all()), "%s: non-finite %s" % (label, nm)
        err = (got[i].double() - ref[i]).abs()[act]
        ratio = err / b[act].clamp(min=1e-300)
        k = int(ratio.argmax())
        assert bool((err <= b[act]).all()), "%s: %s off by %.3e at active element %d, bound %.3e" % (label, nm, float(err[k]), k, float(b[act][k]))
        worst.append(float(ratio.max()))
        assert torch.equal(got[i][~act], host[i][~act]), "%s: %s written outside the stepped tensors" % (label, nm)
    z = act & zero
    assert torch.equal(got[0][z], host[0][z]) and not bool(got[2][z].any()) and not bool(got[3][z].any()), "%s: g = m = v = 0 must not move p" % label
    return worst


@pytest.mark.parametrize("ci", range(len(OC.ADAM_CASES)), ids=[c[0] for c in OC.ADAM_CASES])
def test_adam_kernels_vs_fp64(cuda, dlist, ci):
    """hwg_mt_adam without clip, the separate tail (clamp pass, then hwg_mt_adam), hwg_mt_adam with the clip fused and hwg_mt_clip_adam, from
    the same inputs: each against the fp64 step, and the three clipped paths bit for bit against each other"""
    from handwriting_line_generation_amd import _lib as L
    from handwriting_line_generation_amd import ops
    case = OC.ADAM_CASES[ci]
    name, betas, gs = case
    lay, present = dlist.lay, dlist.present
    cpu_threads()
    p, g, m, v, steps, zero = OC.adam_inputs(case, lay)
    host = (p, g, m, v)
    ss64, bc64 = R.adam_scalars(OC.ADAM_LR, betas[0], betas[1], steps)
    ss32, bc32 = ss64.astype(np.float32), bc64.astype(np.float32)
    sc = ops.h2d(np.stack([ss32, bc32]), cuda)
    ss, bc = _per_element(lay, ss32), _per_element(lay, bc32)
    b1, b2, eps = _f32(betas[0]), _f32(betas[1]), _f32(OC.ADAM_EPS)
    clip_only = present & np.array([(k + ci) % 6 == 3 for k in range(lay.nt)])
    stepped = present & ~clip_only
    label = "adam %s %s" % (dlist.name, name)
    lines = []

    def run(kernel, clip, pre_clamp=False, masks=None, flag=None):
        bufs = [t.to(cuda) for t in host]
        if pre_clamp:
            L.call("hwg_mt_unary", dlist.ptrs([bufs[1]])[0], None, 1, OC.ADAM_CLIP, None, *dlist.geom, dlist.st())
        _adam_call(dlist, kernel, bufs, masks, sc, betas, clip, flag)
        return [b.cpu() for b in bufs]

    def reference(clip, active):
        ref = R.adam_step(p, g, m, v, ss, bc, b1, b2, eps, clip)
        return ref, adam_bounds(p.double(), ref[1], m.double(), v.double(), ss, bc, b1, b2, eps, ref)

    # no clip
    act = lay.mask(present)
    got = run("adam", 0.0)
    ref, bounds = reference(0.0, act)
    w = _check_adam(label + " plain", got, host, ref, bounds, act, zero)
    assert torch.equal(got[1], g), label + ": the gradient is not written without a clip"
    lines.append("plain m %.2f v %.2f p %.2f" % tuple(w))
    # the clipped paths
    ref, bounds = reference(OC.ADAM_CLIP, act)
    clamped = R.clamp(g, OC.ADAM_CLIP)
    sep = run("adam", 0.0, pre_clamp=True)
    fused = run("adam", OC.ADAM_CLIP)
    for nm, got in (("separate", sep), ("fused clip", fused)):
        w = _check_adam(label + " " + nm, got, host, ref, bounds, act, zero)
        assert torch.equal(got[1], _where_mask(act, clamped, g)), "%s %s: the gradient buffer is not clamp(g)" % (label, nm)
        lines.append("%s m %.2f v %.2f p %.2f" % ((nm,) + tuple(w)))
    for i, nm in enumerate("pgmv"):
        assert torch.equal(sep[i], fused[i]), "%s: %s of the fused clip differs from clamp pass + step" % (label, nm)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda)
    one = run("clip_adam", OC.ADAM_CLIP, masks=[stepped, present, stepped, stepped], flag=flag)
    act1 = lay.mask(stepped)
    w = _check_adam(label + " clip_adam", one, host, ref, bounds, act1, zero)
    lines.append("clip_adam m %.2f v %.2f p %.2f" % tuple(w))
    assert torch.equal(one[1], _where_mask(act, clamped, g)), label + ": clip_adam must clip every tensor with a gradient, stepped or not"
    a1 = torch.from_numpy(act1)
    for i, nm in enumerate("pgmv"):
        assert torch.equal(one[i][a1], fused[i][a1]), "%s: %s of clip_adam differs from hwg_mt_adam with clip" % (label, nm)
    assert int(flag.item()) == 0
    print("\n%-44s worst error / derived bound: %s; clipped paths bit-identical; %d clip-only tensors" % (label, "; ".join(lines), int(clip_only.sum())))


def test_nan_gradient_reaches_the_parameter_and_raises_the_flag(cuda):
    """clip_grad_value_ keeps a NaN gradient (torch's clamp_), the step poisons the parameter, and the reference's NaN assert stops the run one
    stepping lesson later. Here: the clamp keeps NaN at every site, the parameter becomes NaN, the sticky flag rises. Infinities clip to the
    bound and harm nothing."""
    from handwriting_line_generation_amd import _lib as L
    from handwriting_line_generation_amd import ops
    dl = DevList(cuda, OC.LISTS[0])
    lay = dl.lay
    case = OC.ADAM_CASES[0]
    p, g, m, v, steps, zero = OC.adam_inputs(case, lay)
    ss64, bc64 = R.adam_scalars(OC.ADAM_LR, 0.5, 0.999, steps)
    sc = ops.h2d(np.stack([ss64.astype(np.float32), bc64.astype(np.float32)]), cuda)
    o = lay.offsets
    nan_body, nan_tail, nan_cliponly = int(o[23]) + 10, int(o[12]) + 1202, int(o[13]) + 3        # 200003: a 16-byte piece; 1203: the scalar tail
    inf_pos, inf_neg = int(o[17]) + 5, int(o[17]) + 6
    clip_only = np.zeros(lay.nt, dtype=bool)
    clip_only[13] = True
    stepped = dl.present & ~clip_only
    masks = [stepped, dl.present, stepped, stepped]
    for with_nan in (True, False):
        gg = g.clone()
        gg[inf_pos], gg[inf_neg] = float("inf"), float("-inf")
        nans = [nan_body, nan_tail, nan_cliponly] if with_nan else []
        for i in nans:
            gg[i] = float("nan")
        want_g = R.clamp(gg, OC.ADAM_CLIP)
        assert float(want_g[inf_pos]) == 2.0 and float(want_g[inf_neg]) == -2.0 and all(math.isnan(float(want_g[i])) for i in nans)
        want_g = _where_mask(lay.mask(), want_g, gg)
        # the clamp pass
        a = gg.to(cuda)
        L.call("hwg_mt_unary", dl.ptrs([a])[0], None, 1, OC.ADAM_CLIP, None, *dl.geom, dl.st())
        assert _same_bits(a, want_g), "clamp: NaN must stay NaN, infinities become the bound"
        # both Adam kernels
        for kernel in ("adam", "clip_adam"):
            bufs = [t.to(cuda) for t in (p, gg, m, v)]
            flag = torch.zeros(1, dtype=torch.int32, device=cuda)
            _adam_call(dl, kernel, bufs, masks if kernel == "clip_adam" else None, sc, (0.5, 0.999), OC.ADAM_CLIP, flag)
            pp, g_after = bufs[0].cpu(), bufs[1].cpu()
            assert _same_bits(g_after, want_g), "%s: gradient after the step" % kernel
            stepped_nans = [i for i in nans if kernel == "adam" or i != nan_cliponly]
            bad = torch.isnan(pp).nonzero().flatten().tolist()
            assert bad == sorted(stepped_nans), "%s: NaN parameters at %s, NaN gradients at %s" % (kernel, bad, sorted(stepped_nans))
            assert bool(torch.isfinite(pp[inf_pos])) and bool(torch.isfinite(pp[inf_neg]))
            if kernel == "clip_adam":
                assert int(flag.item()) == (1 if with_nan else 0), "clip_adam flag %d with%s NaN gradients" % (int(flag.item()), "" if with_nan else "out")
                if with_nan:
                    assert math.isnan(float(g_after[nan_cliponly])) and torch.equal(pp[lay.slices()[13]], p[lay.slices()[13]])
        print("\nnan/inf: %s: clamp, hwg_mt_adam and hwg_mt_clip_adam %s" % (
            "NaN in a piece, a tail and a clip-only tensor, +-inf" if with_nan else "+-inf only",
            "keep the NaN, poison the parameter, flag 1" if with_nan else "clip to +-2, parameters finite, flag 0"))


@pytest.mark.parametrize("clip", [None, OC.ADAM_CLIP], ids=["plain", "clip2"])
def test_hipadam_three_steps_vs_torch_adam_fp64(cuda, clip):
    """HipAdam over a FlatParams of the size table against torch.optim.Adam in fp64 on the CPU, restarted before every step from the GPU's own
    fp32 state (the steps are compared, not their drift); every step touches another subset of tensors, so the step counts diverge"""
    from handwriting_line_generation_amd.trainer.flat_params import FlatParams, HipAdam
    cpu_threads()
    g0 = OC.gen("hipadam_params")
    params = [torch.nn.Parameter(torch.randn(n, generator=g0).to(cuda)) for n in OC.SIZES]
    flat = FlatParams(params, {"main": params})
    opt = HipAdam(flat, "main", lr=OC.ADAM_LR, betas=OC.HIPADAM_BETAS, eps=OC.ADAM_EPS)
    b1, b2 = OC.HIPADAM_BETAS
    steps = np.zeros(len(params), dtype=np.int64)
    worst_ratio, worst_dist = 0.0, 0.0
    for it, rule in enumerate(OC.HIPADAM_STEPS):
        touched = np.array([bool(rule(k)) for k in range(len(params))])
        grads = [torch.randn(n, generator=OC.gen("hipadam_g_%d_%d" % (it, k))) * (3.0 if k % 4 == 0 else 0.05) for k, n in enumerate(OC.SIZES)]
        before = [(q.detach().cpu().clone(), opt.exp_avg[int(flat.offsets[k]):int(flat.offsets[k]) + n].cpu().clone(),
                   opt.exp_avg_sq[int(flat.offsets[k]):int(flat.offsets[k]) + n].cpu().clone()) for k, (q, n) in enumerate(zip(params, OC.SIZES))]
        # torch's Adam from that state
        cpu = [torch.nn.Parameter(b[0].double()) for b in before]
        ref_opt = torch.optim.Adam(cpu, lr=OC.ADAM_LR, betas=OC.HIPADAM_BETAS, eps=OC.ADAM_EPS)
        for k, q in enumerate(cpu):
            if steps[k]:
                ref_opt.state[q] = {"step": torch.tensor(float(steps[k])), "exp_avg": before[k][1].double().clone(), "exp_avg_sq": before[k][2].double().clone()}
            q.grad = grads[k].double() if touched[k] else None
        if clip is not None:
            torch.nn.utils.clip_grad_value_(cpu, clip)
        ref_opt.step()
        # the library's
        flat.touched[:] = touched
        for k, n in enumerate(OC.SIZES):
            if touched[k]:
                flat.flat_grad[int(flat.offsets[k]):int(flat.offsets[k]) + n].copy_(grads[k].to(cuda))
        opt.step(clip=clip)
        steps[touched] += 1
        ss64, bc64 = R.adam_scalars(OC.ADAM_LR, b1, b2, np.maximum(steps, 1))
        for k, n in enumerate(OC.SIZES):
            got_p = params[k].detach().cpu()
            got_m = opt.exp_avg[int(flat.offsets[k]):int(flat.offsets[k]) + n].cpu()
            got_v = opt.exp_avg_sq[int(flat.offsets[k]):int(flat.offsets[k]) + n].cpu()
            if not touched[k]:
                assert torch.equal(got_p, before[k][0]) and torch.equal(got_m, before[k][1]) and torch.equal(got_v, before[k][2])
                continue
            gk = grads[k].double() if clip is None else R.clamp(grads[k].double(), clip)
            ss, bc = float(np.float32(ss64[k])), float(np.float32(bc64[k]))
            p0, m0, v0 = (t.double() for t in before[k])
            contract = R.adam_step(p0, gk, m0, v0, ss, bc, _f32(b1), _f32(b2), _f32(OC.ADAM_EPS))
            bm, bv, bp = adam_bounds(p0, gk, m0, v0, ss, bc, _f32(b1), _f32(b2), _f32(OC.ADAM_EPS), contract)
            dm, dv, du = fp32_beta_distance(gk, m0, v0, ss, bc, b1, b2, OC.ADAM_EPS, contract)
            st = ref_opt.state[cpu[k]]
            for nm, got, want, bound in (("m", got_m, st["exp_avg"], bm + dm), ("v", got_v, st["exp_avg_sq"], bv + dv), ("p", got_p, cpu[k].detach(), bp + du)):
                err = (got.double() - want).abs()
                assert bool((err <= bound).all()), "HipAdam step %d tensor %d (%d): %s off torch's by %.3e, bound %.3e" % (
                    it, k, n, nm, float(err.max()), float(bound[err.argmax()]))
                if nm == "p":
                    worst_ratio = max(worst_ratio, float((err / bound.clamp(min=1e-300)).max()))
            upd_t = (cpu[k].detach() - p0).abs()
            dist = ((contract[0] - cpu[k].detach()).abs() / upd_t.clamp(min=1e-300))[upd_t > 1e-12]
            if dist.numel():
                worst_dist = max(worst_dist, float(dist.max()))
            if clip is not None:
                assert torch.equal(flat.flat_grad[int(flat.offsets[k]):int(flat.offsets[k]) + n].cpu(), R.clamp(grads[k], clip))
        sd = opt.state_dict()["state"]
        assert sorted(sd) == [k for k in range(len(params)) if steps[k]]
        for k in sd:
            assert float(sd[k]["step"]) == float(steps[k]) == float(ref_opt.state[cpu[k]]["step"]) if touched[k] else float(sd[k]["step"]) == float(steps[k])
    assert int(flat._flag.item()) == 0
    assert sorted(set(steps.tolist())) == [1, 2, 3]
    print("\nHipAdam %s: 3 steps, step counts 1..3 as torch's; worst |p - torch| / (derived bound + fp32-beta distance) %.2f; "
          "fp64 contract with fp32 betas vs exact-beta torch Adam: %.2e of the update" % ("plain" if clip is None else "clip 2", worst_ratio, worst_dist))


# ---- random numbers ----------------------------------------------------------------------------------------------------------------------------
RANDN_MEASURED = {}


@pytest.mark.parametrize("stream", OC.RNG_STREAMS, ids=[s[0] for s in OC.RNG_STREAMS])
def test_randn_vs_fp64_box_muller(cuda, stream):
    """UNMEASURED so far: RANDN_ABS (4 x the worst error on an MI355X) is not set; the derived RANDN_DERIVED holds meanwhile. The line this
    test prints per stream carries the worst error: four times the largest of the four is the bound to write into RANDN_ABS."""
    from handwriting_line_generation_amd import ops
    name, seed, offset = stream
    worst, where = 0.0, None
    for n in OC.RNG_SIZES:
        rng = ops.DeviceRNG(seed)
        rng.offset = offset
        got = rng.randn((n,), cuda)
        assert rng.offset == offset + R.stream_blocks(n), "DeviceRNG.offset after %d elements" % n
        err = float(np.abs(got.cpu().double().numpy() - R.randn(seed, offset, n)).max())
        if err > worst:
            worst, where = err, n
        if n <= 4097:
            # a second call continues at the next counter; elements past n are not written
            from handwriting_line_generation_amd import _lib as L
            out = torch.full((n + 8,), OC.SENTINEL, dtype=torch.float32, device=cuda)
            L.call("hwg_randn", out, n, seed, rng.offset, ops._stream())
            assert torch.equal(out[n:].cpu(), torch.full((8,), OC.SENTINEL)), "randn wrote past n = %d" % n
            err2 = float(np.abs(out[:n].cpu().double().numpy() - R.randn(seed, offset + R.stream_blocks(n), n)).max())
            worst = max(worst, err2)
    RANDN_MEASURED[name] = worst
    print("\nrandn %-10s seed %#x offset %#x: worst |error| vs fp64 Box-Muller %.3e (n = %d), bound %s" % (
        name, seed, offset, worst, where, "%.1e" % RANDN_ABS if RANDN_ABS is not None else "%.1e (derived; the 4 x measured one is unmeasured)" % RANDN_DERIVED))
    assert worst <= (RANDN_ABS if RANDN_ABS is not None else RANDN_DERIVED)


@pytest.mark.parametrize("p", OC.DROP_PS)
def test_dropmask_pattern_exact(cuda, p):
    from handwriting_line_generation_amd import ops
    name, seed, offset = OC.RNG_STREAMS[2]
    for n in OC.DROP_SIZES:
        rng = ops.DeviceRNG(seed)
        rng.offset = offset
        got = rng.dropmask((n,), p, cuda).cpu()
        assert rng.offset == offset + R.stream_blocks(n)
        keep, value = R.dropmask(seed, offset, n, p)
        keep = torch.from_numpy(keep)
        assert torch.equal(got != 0, keep), "dropmask p = %g n = %d: keep pattern" % (p, n)
        kept = got[keep].double()
        if kept.numel():
            assert float(kept.min()) == float(kept.max())
            ulp = float(np.spacing(np.float32(value)))
            assert abs(float(kept[0]) - value) <= DERIVED["drop_keep_ulps"] * ulp, "dropmask p = %g: kept value %r, 1 / (1 - p) = %r" % (p, float(kept[0]), value)
        if p == 0.0:
            assert bool(keep.all()) and float(kept[0]) == 1.0
    print("\ndropmask p = %-5g keep pattern exact (%d of %d kept at n = %d), kept value %r" % (p, int(keep.sum()), n, n, float(kept[0]) if kept.numel() else None))


@pytest.mark.parametrize("nseg", OC.DROP_MULTI)
def test_dropmask_multi_is_consecutive_dropmasks(cuda, nseg):
    from handwriting_line_generation_amd import ops
    name, seed, offset = OC.RNG_STREAMS[1]
    sizes, ps = OC.drop_multi_segments(nseg)
    a, b = ops.DeviceRNG(seed), ops.DeviceRNG(seed)
    a.offset = b.offset = offset
    views = a.dropmask_multi(sizes, ps, cuda)
    for view, n, p in zip(views, sizes, ps):
        assert torch.equal(view, b.dropmask((n,), p, cuda)), "dropmask_multi: segment of %d elements, p = %g" % (n, p)
    assert a.offset == b.offset == offset + sum(sizes) // 4
    print("\ndropmask_multi %2d segments (%d elements): equal to consecutive dropmask calls, stream position equal" % (nseg, sum(sizes)))


def test_dropmask_multi_refuses_bad_segments(cuda):
    from handwriting_line_generation_amd import _lib as L
    from handwriting_line_generation_amd import ops
    out = torch.full((4 * 17,), OC.SENTINEL, dtype=torch.float32, device=cuda)
    for sizes in ([4] * 17, [8, 6, 4]):
        ne, pp = np.asarray(sizes, dtype=np.int64), np.full(len(sizes), 0.5, dtype=np.float32)
        with pytest.raises(L.HwgError):
            L.call("hwg_dropmask_multi", out, len(sizes), ne.ctypes.data, pp.ctypes.data, 1, 0, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((4 * 17,), OC.SENTINEL))


# ---- insert_spaces -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OC.INSERT_CASES, ids=[c[0] for c in OC.INSERT_CASES])
def test_insert_spaces_vs_restatement(cuda, case):
    from handwriting_line_generation_amd import _lib as L
    from handwriting_line_generation_amd import ops
    name, Lc, B, lens, cs, ds, dup, kind, seed, offset, cut = case
    counts, label, lens_t = OC.insert_inputs(case)
    pre = R.insert_spaces_draws(counts.numpy(), lens, cs, ds, seed + 1, offset)           # DeviceRNG draws the text stream from seed + 1
    want_reps = R.insert_spaces_reps(pre, lens, dup)
    near = OC.insert_near_ties(pre, lens, dup) if (cs or ds) else np.zeros_like(want_reps, dtype=bool)
    # the window against the device's arithmetic: the measured error of an fp32 normal times the std, and the rounding of the fp32 sum
    # c + std z (below 8 in every case: half an ulp of 8)
    assert float(np.nanmax(np.abs(pre))) < 8 and (RANDN_ABS or RANDN_DERIVED) * max(cs, ds) + 4 * ULP <= OC.INSERT_NEAR_TIE / 10
    rng = ops.DeviceRNG(seed)
    rng.text_offset = offset
    plan = rng.insert_spaces_begin(counts.to(cuda), label.to(cuda), lens_t.to(cuda), cs, ds, dup)
    assert rng.text_offset == offset + Lc * B and rng.offset == 0
    reps = plan[2].cpu().numpy().astype(np.int64)
    starts = plan[3].cpu().numpy().astype(np.int64)
    live = np.zeros_like(near)
    for b in range(B):
        live[b, :2 * lens[b]] = True
    differ = (reps != want_reps) & live
    assert not bool((differ & ~near).any()), "insert_spaces %s: reps differ at %s" % (name, np.argwhere(differ & ~near)[:8].tolist())
    assert int(near.sum()) * 100 <= int(live.sum()), "insert_spaces %s: %d of %d elements near a tie" % (name, int(near.sum()), int(live.sum()))
    # from the device's own reps everything else is exact
    want_starts, want_lens = R.insert_spaces_layout(reps, lens, counts.numpy())
    for b in range(B):
        assert np.array_equal(starts[b, :lens[b]], want_starts[b, :lens[b]]), "insert_spaces %s: starts of line %d" % (name, b)
    lens_max = plan[4].get().numpy().astype(np.int64)
    assert np.array_equal(lens_max, want_lens), "insert_spaces %s: lens_max %s, expected %s" % (name, lens_max.tolist(), want_lens.tolist())
    idx, padded = rng.insert_spaces_finish(plan)
    T = int(want_lens[:B].max() + want_lens[B])
    assert tuple(idx.shape) == (T, B)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), R.insert_spaces_fill(label.numpy(), lens, reps, want_starts, T))
    spaced, want_padded = R.insert_spaces_spaced(label.numpy(), lens, reps, counts.numpy(), OC.INSERT_CLASSES)
    assert torch.equal(torch.nn.functional.one_hot(idx.cpu().long(), OC.INSERT_CLASSES).float(), spaced), "insert_spaces %s: one_hot(idx) is not the reference's layout" % name
    assert padded == want_padded
    note = ""
    if cut:
        # a T inside the last run of the longest line: the run is cut there, nothing is written behind the buffer
        b_long = int(want_lens[:B].argmax())
        Tc = int(want_lens[b_long]) - 1
        assert reps[b_long, 2 * lens[b_long] - 1] >= 2, "the case must end in a run of two or more"
        buf = torch.full(((Tc + 2) * B,), -5, dtype=torch.int32, device=cuda)
        buf[:Tc * B] = 0
        L.call("hwg_insert_spaces_fill", label.to(cuda), lens_t.to(cuda), plan[2], plan[3], Lc, B, Tc, buf, ops._stream())
        got = buf.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[:Tc * B].reshape(Tc, B), R.insert_spaces_fill(label.numpy(), lens, reps, want_starts, Tc))
        assert np.array_equal(got[Tc * B:], np.full(2 * B, -5)), "insert_spaces_fill wrote past T"
        note = "; T = %d cuts the last run, nothing written past it" % Tc
    if kind == "ties":
        assert set(np.unique(reps[live]).tolist()) == {0, 2}, "round half to even of 0.5 / 1.5 / 2.5"
    if kind == "negative":
        assert int(reps[live].sum()) == int(reps[0, 1]) > 0
    print("\ninsert_spaces %-10s L %d B %d: %d draws, %d left out as near a tie, %d differ there; starts, lens_max, idx, one-hot layout, padded exact%s"
          % (name, Lc, B, int(live.sum()), int(near.sum()), int(differ.sum()), note))
