"""GPU: the forward-type convolution products - hwg_conv_fwd (conv_mfma_kernel with its four tiles, both channel steps and the three modes,
conv_split_reduce_kernel, the C == 1 kernels conv_c1_rows / conv_c1_mfma / conv_c1 and the K <= 2 kernels conv_to1 / conv_to1_3x3),
hwg_wino_conv_fwd (every tile config, uniform split, balanced schedule with both reduce bodies), hwg_wino_s2_conv (forward and data gradient)
and the weight-image entries - against the fp64 direct form of oracle/conv_ref.py, through L.call on the C ABI (never through ops.conv2d),
every schedule forced through ops.tuning (case tables and the regimes they cover: oracle/conv_cases.py; the restatements, the tables and
their sensitivity to seeded flaws are checked on the CPU by tests/test_conv_ref_cpu.py). The buffers are those of tests/_guarded.py, the
references, the bounds and check() those of tests/_conv_checks.py. The weight-gradient families are held to the same protocol by tests/test_wgrad_fp64_gpu.py.

Every call runs on buffers carved out of one allocation with 64-float canaries before, between and after x, the weight image, the bias, y
and the workspace. The workspace has exactly the bytes the entry's *_workspace query returns and is filled with NaN before every call, y is
filled with NaN (overwrite) or a random y0 (accumulate). After the call: canaries intact, x / weight image / bias bit-identical, y finite,
hwg_last_plan() the forced schedule (the C == 1 and K <= 2 kernels note no plan: there the dispatch restated in oracle/conv_cases.py names the
kernel and last_plan must not move), a second call after re-poisoning gives the same bits, and a call with one byte of workspace too few
returns HWG_ERR_WORKSPACE and leaves y and the canaries alone.

Against fp64 there are two conditions and no other tolerance. Per element |err| <= (T + c) 2^-24 A; per tensor the relative L2 error is at most
YARDSTICK_FACTOR times that of the fp32 CPU restatement of the same algorithm (direct form for the direct engines, tile transforms for the
Winograd engines). A = |x| (*) |w| + |bias| + |y0| (Winograd: A_w, the same pipeline with every transform matrix and operand replaced by its
absolute value). T is the contraction length of the engine, c counts the further rounded operations on the longest path to an output element:

  engine                                  T                              c                                        measured on an MI355X
  conv_mfma_kernel modes 0 / 1 / 2,       taps (per parity class) x C    [bias] + [accumulate] + (pieces - 1)      e/b 0.18, L2 x2.9
  conv_split_reduce_kernel                                               (the accumulator chain's T products and
                                                                          T - 1 sums are the T)
  conv_c1_rows / c1_mfma / c1             taps                           [bias] + [accumulate]                     e/b 0.33, L2 x1.0
  conv_to1 / conv_to1_3x3                 taps x C                       [bias] + [accumulate] (the lane tree is   e/b 0.36, L2 x1.2
                                                                          part of the T - 1 sums)
  hwg_wino_conv_fwd, F(2x2,3x3)           C                              2 (input transform: one sum per 1-D       e/b 0.016 (impulses 0.12), L2 x1.04
                                                                          stage) + 4 (filter: two sums per stage,
                                                                          the halving is exact) + 4 (output: two
                                                                          sums per stage) + [bias] + [accumulate]
                                                                          + (pieces - 1)
  hwg_wino_s2_conv, F(3x3,2x2)            4 C forward, C data gradient   2 + 2 (filter: one sum per stage) + 4     e/b 0.010 (impulses 0.14), L2 x1.03
                                                                          + [bias] + [accumulate] + (pieces - 1)
  U = G g G^T images                      -                              4 (F(2x2,3x3)) / 2 (F(3x3,2x2)) times
                                                                          2^-24 |G||g||G^T|; copies and padding    e/b 0.49 / 0.90
                                                                          exact
(measured: worst |err| / bound, worst relative L2 / yardstick over the engine's cases; every case prints its own line.)"""
import numpy as np
import pytest
import torch

from oracle import conv_cases as CC
from oracle import conv_ref as R
from _conv_checks import check, reference, reference_of
from _fp64 import _ratio
from _guarded import HWG_ERR_ARG, HWG_ERR_WORKSPACE, carve, put, same_bits

pytestmark = pytest.mark.gpu


class Run:
    """one case on carved buffers: .call() poisons the workspace and y and launches, .y is the output view"""

    def __init__(self, c, dev, x, w, b, y0):
        from handwriting_line_generation_amd import _lib as L, ops
        self.c, self.L, self.ops, self.y0 = c, L, ops, y0
        N, H, W, C, K, Rr, S = c["shape"]
        self.entry, ws_query = CC.workspace_entry(c)
        self.d = ops._desc(N, H, W, C, K, Rr, S, c["stride"], c["pad"], c["dil"], c["P"], c["Q"], c["transposed"])
        self.need = int(L.query(ws_query, self.d.ptr))
        assert self.need % 4 == 0
        st = self.st = ops._stream()
        if c["engine"] == "wino":
            n_img = int(L.query("hwg_wino_weight_floats", K, C))
        elif c["engine"] == "s2":
            src, Kc, Cc, dgrad = CC.s2_source(c, w)
            n_img = int(L.query("hwg_wino_s2_weight_floats", Kc, Cc, dgrad))
        else:
            n_img = Rr * S * K * C
        (self.xd, self.wd, self.bd, self.yd, self.ws), self.intact = carve(dev, x.numel(), n_img, K, CC.out_numel(c), self.need // 4)
        put(self.xd, x)
        if c["engine"] == "wino":
            assert L.query("hwg_wino_supported", self.d.ptr) == 1, c["name"]
            src, sa, sb, flip = CC.wino_source(c, w)
            L.call("hwg_wino_pack_weight", src.to(dev), self.wd, K, C, sa, sb, 3, 1, flip, st)
        elif c["engine"] == "s2":
            assert L.query("hwg_wino_s2_supported", self.d.ptr) == 1, c["name"]
            L.call("hwg_wino_s2_pack_weight", src.to(dev), self.wd, Kc, Cc, Cc * 16, 16, dgrad, st)
        else:
            put(self.wd, w.reshape(Rr * S, K, C))
        if b is not None:
            put(self.bd, b)
        torch.cuda.synchronize()
        self.sent = [t.clone() for t in (self.xd, self.wd, self.bd)]
        self.y = self.yd.view(N, c["P"], c["Q"], K)

    def poison(self):
        self.ws.fill_(float("nan"))
        if self.y0 is None:
            self.yd.fill_(float("nan"))
        else:
            put(self.yd, self.y0)

    def call(self, short=0):
        """-> the entry's return code"""
        self.poison()
        c = self.c
        rc = self.L.query(self.entry, self.d.ptr, self.xd, self.wd, self.bd if c["bias"] else None, self.yd, int(c["acc"]),
                          self.ws if self.need else None, self.need - short, self.st)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all(same_bits(a, b) for a, b in zip((self.xd, self.wd, self.bd), self.sent))


def expected_plan(c):
    if c["engine"] == "mfma":
        return CC.mfma_plan(c)[0]
    if c["engine"] in ("wino", "s2"):
        return CC.wino_plan(c)[1]
    return None


def run_case(c, dev, x, w, b, y0):
    """the protocol of the module docstring; -> the output of the first call (CPU)"""
    from handwriting_line_generation_amd import ops
    name = c["name"]
    with ops.tuning(**c["env"]):
        r = Run(c, dev, x, w, b, y0)
        before = ops.last_plan()
        rc = r.call()
        assert rc == 0, "%s: %s returned %d: %s" % (name, r.entry, rc, r.L.last_error())
        assert r.intact(), "%s: a canary next to a buffer was overwritten" % name
        assert r.untouched(), "%s: x, the weight image or the bias changed" % name
        y1 = r.y.detach().cpu().clone()
        assert bool(torch.isfinite(y1).all()), "%s: %d non-finite output elements (a piece nobody wrote, or an element never written)" % (
            name, int((~torch.isfinite(y1)).sum()))
        want = expected_plan(c)
        if want is not None:
            assert ops.last_plan() == want, "%s ran %s, forced %s" % (name, ops.last_plan(), want)
        else:
            assert ops.last_plan() == before, "%s: a direct kernel's case moved last_plan to %s" % (name, ops.last_plan())
        assert r.call() == 0
        assert same_bits(r.y, y1), "%s: the second call gives other bits" % name
        if r.need:
            rc = r.call(short=1)
            assert rc == HWG_ERR_WORKSPACE, "%s: %d bytes of workspace for %d needed returned %d" % (name, r.need - 1, r.need, rc)
            want_y = torch.full_like(y1, float("nan")) if y0 is None else y0
            assert same_bits(r.y, want_y), "%s: the refused call wrote to y" % name
        assert r.intact() and r.untouched(), "%s: canaries / inputs after the repeated calls" % name
    return y1


@pytest.mark.parametrize("c", CC.RUN_CASES, ids=[c["name"] for c in CC.RUN_CASES])
def test_conv_forward_vs_fp64(cuda, c):
    ref, yard, bound = reference(c)
    y = run_case(c, cuda, *CC.inputs(c))
    check(c, y, ref, yard, bound)


def test_c1_refusal_writes_nothing(cuda):
    """K = 256 with 9x9 taps does not fit the 64 KB of LDS: an error, and neither y nor a canary is touched"""
    c = CC.REFUSED
    assert CC.c1_kernel(c) == "refused"
    r = Run(c, cuda, *CC.inputs(c))
    rc = r.call()
    assert rc == HWG_ERR_ARG, rc
    assert same_bits(r.y, torch.full(r.y.shape, float("nan"))) and r.intact() and r.untouched()


# ---- index-exact ---------------------------------------------------------------------------------------------------------------------------
INDEX = [CC.BY_NAME[n] for n in CC.INDEX_CASES]


@pytest.mark.parametrize("c", INDEX, ids=CC.INDEX_CASES)
def test_impulses(cuda, c):
    """x zero but for ones with disjoint output footprints, no bias, overwrite: every product is by 1 and every sum is with 0, so the direct
    engines give the fp32 weight itself; the Winograd engines are held to the bound with T = 1 (one non-zero product per contraction)"""
    c = dict(c, bias=False, acc=False)
    _, w, _, _ = CC.inputs(c)
    for k, sites in enumerate(CC.impulse_sites(c)):
        x = torch.zeros(c["shape"][:4])
        for _, s in sites:
            x[s] = 1.0
        y = run_case(c, cuda, x, w, None, None)
        want = R.conv_direct(x.double(), w.double(), CC.geom(c))
        if c["engine"] in ("wino", "s2"):
            _, yard, bound = reference_of(c, x, w, None, None, terms=1)
            check(c, y, want, yard, bound, " impulses %d" % k)
        else:
            ok = torch.equal(y, want.float())
            print("\nconv_fp64 %-34s %-5s impulses %d: %s" % (c["name"], c["engine"], k, "equal" if ok else "NOT EQUAL"))
            assert ok, "%s impulses %d: %d elements differ from the weight they must be" % (c["name"], k, int((y != want.float()).sum()))


NAN_CASES = [c for c in INDEX if not (c["transposed"] and c["engine"] == "mfma")]


@pytest.mark.parametrize("c", NAN_CASES, ids=[c["name"] for c in NAN_CASES])
def test_one_nan_in_x(cuda, c):
    """direct engines: the NaN set of y is the receptive footprint of the pixel times all K; Winograd engines: it contains the footprint and
    lies within the outputs of the tiles whose input patch holds the pixel"""
    from handwriting_line_generation_amd import ops
    c = dict(c, acc=False)
    x, w, b, _ = CC.inputs(c)
    N, H, W, C = x.shape
    site = (N - 1, H // 2, W // 3, C - 1)
    x[site] = float("nan")
    with ops.tuning(**c["env"]):
        r = Run(c, cuda, x, w, b, None)
        assert r.call() == 0 and r.intact()
        got = torch.isnan(r.y.detach().cpu())
    K = c["shape"][4]
    fp = CC.site_footprint(c, site)[..., None].expand(-1, -1, -1, K)
    if c["engine"] in ("wino", "s2"):
        sup = CC.wino_tile_footprint(c, site)[..., None].expand(-1, -1, -1, K)
        assert bool((got | ~fp).all()), "%s: %d elements of the footprint are not NaN" % (c["name"], int((fp & ~got).sum()))
        assert bool((sup | ~got).all()), "%s: %d NaN outside the tiles that read the pixel" % (c["name"], int((got & ~sup).sum()))
    else:
        assert torch.equal(got, fp), "%s: NaN set differs from the footprint in %d elements" % (c["name"], int((got != fp).sum()))


# ---- the pack entries -----------------------------------------------------------------------------------------------------------------------
def _pack_reference(kind, case):
    """(exact image or None, (fp64 image, bound) or None)"""
    if kind == 0:
        name, A, B, Bpad, R_, S_, layout, flip = case
        src, sa, sb, sr, ss = CC.pack_source(name, A, B, R_, S_, layout)
        return src, R.pack_image(src, A, B, Bpad, R_, S_, sa, sb, sr, ss, flip), None
    if kind == 1:
        name, A, B, layout, flip = case
        src, sa, sb, sr, ss = CC.pack_source(name, A, B, 3, 3, layout)
        return src, None, (R.wino_image(src.double(), A, B, sa, sb, sr, ss, flip), R.sum_bound(4, R.wino_image(src.double(), A, B, sa, sb, sr, ss, flip, absolute=True)))
    name, Kc, Cc, dgrad = case
    src = CC.pack_source(name, Kc, Cc, 4, 4, "ab")[0]
    return src, None, (R.wino_s2_image(src.double(), Kc, Cc, Cc * 16, 16, dgrad), R.sum_bound(2, R.wino_s2_image(src.double(), Kc, Cc, Cc * 16, 16, dgrad, absolute=True)))


def _pack_records():
    """(kind, case, L.call name, arguments after (src, dst), image floats, the 96-byte record's fields after (src, dst)) of every pack case"""
    out = []
    for case in CC.PACK_CASES:
        name, A, B, Bpad, R_, S_, layout, flip = case
        _, sa, sb, sr, ss = CC.pack_source(name, A, B, R_, S_, layout)
        out.append((0, case, "hwg_conv_pack_weight", (A, B, Bpad, R_, S_, sa, sb, sr, ss, flip), R_ * S_ * A * Bpad,
                    (A, B, Bpad, R_, S_, flip, sa, sb, sr, ss, R_ * S_ * A * Bpad, 0, A)))
    for case in CC.WINO_PACK_CASES:
        name, A, B, layout, flip = case
        _, sa, sb, sr, ss = CC.pack_source(name, A, B, 3, 3, layout)
        Ap, Bp = R.ceil16(A), R.ceil16(B)
        out.append((1, case, "hwg_wino_pack_weight", (A, B, sa, sb, sr, ss, flip), 16 * Ap * Bp, (A, B, Bp, 3, 3, flip, sa, sb, sr, ss, Ap * Bp, 1, Ap)))
    for case in CC.S2_PACK_CASES:
        name, Kc, Cc, dgrad = case
        Ap, Bp = (R.ceil16(4 * Cc), R.ceil16(Kc)) if dgrad else (R.ceil16(Kc), R.ceil16(4 * Cc))
        out.append((2, case, "hwg_wino_s2_pack_weight", (Kc, Cc, Cc * 16, 16, dgrad), 16 * Ap * Bp, (Kc, Cc, Bp, 4, 4, dgrad, Cc * 16, 16, 4, 1, Ap * Bp, 2, Ap)))
    return out


def test_pack_entries(cuda):
    """copies and promised zero padding exact, U = G g G^T to the derived bound; hwg_conv_pack_weight_multi (one table with every record,
    built the way ops.repack_group builds it) bit for bit the single-call entries"""
    from handwriting_line_generation_amd import _lib as L, ops
    st = ops._stream()
    recs = _pack_records()
    dt = np.dtype([("src", "<u8"), ("dst", "<u8"), ("A", "<i4"), ("B", "<i4"), ("Bpad", "<i4"), ("R", "<i4"), ("S", "<i4"), ("flip", "<i4"),
                   ("sa", "<i8"), ("sb", "<i8"), ("sr", "<i8"), ("ss", "<i8"), ("total", "<i8"), ("first_block", "<i8"), ("mode", "<i4"), ("Apad", "<i4")])
    assert dt.itemsize == 96
    host = np.zeros(len(recs), dtype=dt)
    views, intact = carve(cuda, *([r[4] for r in recs] * 2))
    single, multi = views[:len(recs)], views[len(recs):]
    srcs, blocks = [], 0
    for i, (kind, case, fn, args, n, fields) in enumerate(recs):
        src = _pack_reference(kind, case)[0].to(cuda)
        srcs.append(src)
        single[i].fill_(float("nan")); multi[i].fill_(float("nan"))
        L.call(fn, src, single[i], *args, st)
        A, B, Bpad, R_, S_, flip, sa, sb, sr, ss, total, mode, Apad = fields
        host[i] = (src.data_ptr(), multi[i].data_ptr(), A, B, Bpad, R_, S_, flip, sa, sb, sr, ss, total, blocks, mode, Apad)
        blocks += (total + ops.PACK_PER_BLOCK - 1) // ops.PACK_PER_BLOCK
    table = torch.from_numpy(host.view(np.uint8)).to(cuda)
    L.call("hwg_conv_pack_weight_multi", table, len(recs), blocks, st)
    torch.cuda.synchronize()
    assert intact(), "a pack entry wrote outside its image"
    for i, (kind, case, fn, args, n, fields) in enumerate(recs):
        _, exact, bounded = _pack_reference(kind, case)
        got = single[i].detach().cpu()
        assert same_bits(multi[i], got), "%s: hwg_conv_pack_weight_multi differs from %s" % (case[0], fn)
        if exact is not None:
            assert torch.equal(got, exact.reshape(-1)), "%s: the image is not the copy" % case[0]
            print("\nconv_fp64 pack %-28s equal" % case[0])
        else:
            ref, bound = bounded
            r = _ratio(got, ref.reshape(-1), bound.reshape(-1))
            print("\nconv_fp64 pack %-28s e/b %.3g" % (case[0], r))
            assert r <= 1.0, "%s: U is %.3g x its bound off (a non-zero in the padding counts as infinite)" % (case[0], r)
