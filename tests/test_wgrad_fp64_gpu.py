"""GPU: the weight-gradient products - hwg_conv_wgrad (wgrad_mfma_kernel with its 32x32, 64x64 and 128x128 tiles and the taps-as-N form,
wgrad_narrow_kernel<3,3> / <4,4>, wgrad_c1_rows_kernel, wgrad_c1_kernel, wgrad_direct_kernel<0> / <1> with its own reduce), hwg_wino_wgrad
(F(3x3 taps, 2x2 gradient tiles) and the space-to-depth form F(2x2 taps, 3x3 gradient tiles)), the reduce kernels (VEC4, SCALAR, LANES4, LANES32
and the eight ROWS variants), hwg_conv_wgrad_sets / hwg_wino_wgrad_sets and hwg_colsum - against the fp64 direct form of oracle/conv_ref.py,
through L.query on the C ABI (never through ops.conv2d), every schedule forced through ops.tuning (case tables, the regimes they cover and the
restated planners: oracle/wgrad_cases.py; the restatements, the tables and their sensitivity to seeded flaws are checked on the CPU by
tests/test_wgrad_ref_cpu.py). The buffers are those of tests/_guarded.py, the comparisons and the two conditions those of
tests/_conv_checks.py (check()) and tests/_wgrad_checks.py (the references and bounds).

Every call runs on buffers carved out of one allocation with 64-float canaries before, between and after u, v, every dw, every dbias and the
workspace. The workspace has exactly the bytes the entry's *_workspace query returns and is filled with NaN before every call; dw and dbias are
filled with NaN (overwrite) or a random dw0 / db0 (accumulate), the gaps a strided dw leaves hold the canary. After the call: return code 0,
canaries and gaps intact, u and v bit-identical, dw and dbias finite (a partial image nobody wrote is NaN), hwg_last_plan() the restated triple
(the direct kernel notes none: last_plan must not move), a second call after re-poisoning gives the same bits, and a call with one byte of
workspace too few returns HWG_ERR_WORKSPACE and leaves dw, dbias and the canaries alone.

Against fp64 there are two conditions and no other tolerance. Per element |err| <= (T + c) 2^-24 A; per tensor the relative L2 error is at most
YARDSTICK_FACTOR times that of the fp32 CPU restatement of the same algorithm (direct form; tile transforms for the Winograd entry).
A = |u| (*) |v| + |dw0| (Winograd: the same pipeline with every transform matrix and operand replaced by its absolute value). T is the number of
anchor pixels whose tap falls inside the image (per tap), c counts the further rounded operations on the longest path to an element (ranges =
partial images summed by the reduce; every reduce schedule adds a range's image at most ranges - 1 times on its longest path, adding 0 is exact):

  engine                             c for dw                                              c for the bias gradient (T = N P Q, A = sum |u| + |db0|)   measured on an MI355X (dw; bias)
  wgrad_mfma_kernel 128x128          (ranges - 1) + [accumulate]                            1 (fp64 sum, rounded once) + (ranges - 1) + [accumulate]    e/b 0.17, L2 x1.39; e/b 0.0022, L2 x0.57
  wgrad_mfma_kernel 64x64            1 (two pixel halves of a step, summed through LDS)     as above                                                    e/b 0.14, L2 x1.01; e/b 0.016, L2 x0.72
                                     + (ranges - 1) + [accumulate]
  wgrad_mfma_kernel taps-as-N        as 64x64                                               as above                                                    e/b 0.092, L2 x0.86; e/b 0.014, L2 x0.89
  wgrad_mfma_kernel 32x32            3 (four quarters) + (ranges - 1) + [accumulate]        as above                                                    e/b 0.065, L2 x0.95; e/b 0.0046, L2 x0.86
  wgrad_narrow_kernel                log2(8 / channel blocks) (the LDS tree over the        2 (lane shuffles) + the same tree + (ranges - 1) + [acc.]   e/b 1.6e-05, L2 x0.57; e/b 5.8e-06, L2 x1.22
                                     wavefronts of a block) + (ranges - 1) + [accumulate]
  wgrad_c1_rows_kernel               3 (four wavefronts) + (ranges - 1) + [accumulate]      1 (the two lane halves) + 3 + (ranges - 1) + [accumulate]   e/b 0.00011, L2 x0.16; e/b 2.6e-05, L2 x0.95
  wgrad_c1_kernel                    3 (four wavefronts) + (ranges - 1) + [accumulate]      3 + (ranges - 1) + [accumulate]                             e/b 7.6e-05, L2 x0.14; e/b 3.6e-05, L2 x1.33
  wgrad_direct_kernel                (pixel lanes - 1) + (blocks - 1) + [accumulate]        - (no fused bias gradient: hwg_colsum)                      e/b 0.010, L2 x1.02
  hwg_wino_wgrad 3x3                 2 (Z = A dY A^T: one sum per 1-D stage) + 2 (V = B^T   3 (four dy wavefronts; the sums inside a tile are part of   e/b 0.042 (impulses 0.098), L2 x1.00;
                                     d B: one per stage) + 4 (G^T dU G: two per stage, the   the T - 1) + (ranges - 1) + [accumulate]                    e/b 0.039, L2 x0.98
                                     halving is exact) + (ranges - 1) + [accumulate];
                                     T = tiles (N ceil(P/2) ceil(Q/2))
  hwg_wino_wgrad 4x4 stride 2        4 (Z: two sums per stage) + 2 + 4 + (ranges - 1) +      as above                                                    e/b 0.016 (impulses 0.083), L2 x1.02;
                                     [accumulate]; T = tiles (N ceil(P/3) ceil(Q/3))                                                                     e/b 0.0059, L2 x1.25
  hwg_colsum                         -                                                      chunks (fp64 sums, one rounding per chunk, chunks - 1 sums) e/b 0.22, L2 x1.16
                                                                                            + [accumulate]; T = rows
(measured: worst |err| / bound, worst relative L2 / yardstick over the engine's cases; every case prints its own line.)"""
import numpy as np
import pytest
import torch

from oracle import conv_ref as R
from oracle import wgrad_cases as WC
from _conv_checks import check
from _fp64 import _rel
from _guarded import CANARY, HWG_ERR_ARG, HWG_ERR_WORKSPACE, carve, put, same_bits
from _wgrad_checks import reference, reference_of

pytestmark = pytest.mark.gpu


# ---- one case on carved buffers --------------------------------------------------------------------------------------------------------------
class Run:
    """.call() poisons the workspace, every dw and every dbias and launches; .dw(s) / .db(s) are the results of set s (CPU, logical layout)"""

    def __init__(self, c, dev, u, v, dw0, db0, via_sets=False, n_ptrs=None, ws_floats=None):
        from handwriting_line_generation_amd import _lib as L, ops
        self.c, self.L, self.ops, self.dw0, self.db0 = c, L, ops, dw0, db0
        N, H, W, C, K, Rr, S = c["shape"]
        self.sets = sets = c["sets"]
        self.via_sets = via_sets or sets != 1
        wino = c["engine"] in ("wino", "s2") or c.get("wino", False)
        self.entry = ("hwg_wino_wgrad" if wino else "hwg_conv_wgrad") + ("_sets" if self.via_sets else "")
        self.d = ops._desc(N, H, W, C, K, Rr, S, c["stride"], c["pad"], c["dil"], c["P"], c["Q"], 0)
        if ws_floats is None:
            self.need = int(L.query(self.entry + "_workspace", self.d.ptr, sets) if self.via_sets else L.query(self.entry + "_workspace", self.d.ptr))
            assert self.need % 4 == 0
        else:
            self.need = 4 * ws_floats
        self.st = ops._stream()
        self.ndw, self.sa, self.sb, self.sr, self.ss = WC.dw_strides(c)
        self.idx = WC.dw_index(c).to(dev)
        n = max(sets, 1) if n_ptrs is None else n_ptrs
        views, self.intact = carve(dev, u.numel(), v.numel(), *([self.ndw] * n), *([K] * n), self.need // 4)
        self.ud, self.vd, self.dwd, self.dbd, self.ws = views[0], views[1], views[2:2 + n], views[2 + n:2 + 2 * n], views[-1]
        put(self.ud, u)
        put(self.vd, v)
        torch.cuda.synchronize()
        self.sent = [t.clone() for t in (self.ud, self.vd)]
        self.dw_ptrs = np.array([t.data_ptr() for t in self.dwd], dtype=np.int64)
        self.db_ptrs = np.array([t.data_ptr() for t in self.dbd], dtype=np.int64)
        self.gaps = torch.ones(self.ndw, dtype=torch.bool, device=dev)
        self.gaps[self.idx.reshape(-1)] = False

    def poison(self):
        self.ws.fill_(float("nan"))
        for s, (dw, db) in enumerate(zip(self.dwd, self.dbd)):
            dw.fill_(CANARY)
            fill = torch.full(self.idx.shape, float("nan"), device=dw.device) if self.dw0 is None or s >= len(self.dw0) else self.dw0[s].to(dw.device)
            dw[self.idx.reshape(-1)] = fill.reshape(-1)
            if self.db0 is None or s >= len(self.db0):
                db.fill_(float("nan"))
            else:
                put(db, self.db0[s])

    def call(self, short=0, sets=None, set_on_v=None):
        """-> the entry's return code"""
        self.poison()
        torch.cuda.synchronize()
        self.before = [t.clone() for t in list(self.dwd) + list(self.dbd)]
        c = self.c
        tail = (self.sa, self.sb, self.sr, self.ss, int(c["acc"]))
        ws = (self.ws if self.need else None, self.need - short, self.st)
        if not self.via_sets:
            rc = self.L.query(self.entry, self.d.ptr, self.ud, self.vd, self.dwd[0], *tail, self.dbd[0] if c["bias"] else None, int(c["bias_acc"]), *ws)
        else:
            sets = self.sets if sets is None else sets
            head = (self.d.ptr, self.ud, self.vd, sets) + (() if "wino" in self.entry else (c["set_on_v"] if set_on_v is None else set_on_v,))
            rc = self.L.query(self.entry, *head, self.dw_ptrs.ctypes.data, *tail, self.db_ptrs.ctypes.data if c["bias"] else None, int(c["bias_acc"]), *ws)
        torch.cuda.synchronize()
        return rc

    def dw(self, s):
        return self.dwd[s][self.idx].detach().cpu()

    def db(self, s):
        return self.dbd[s].detach().cpu().clone()

    def untouched(self):
        return all(same_bits(a, b) for a, b in zip((self.ud, self.vd), self.sent))

    def outputs_untouched(self):
        return all(same_bits(a, b) for a, b in zip(list(self.dwd) + list(self.dbd), self.before))

    def gaps_intact(self):
        return all(bool((dw[self.gaps] == CANARY).all()) for dw in self.dwd)


def run_case(c, dev, u, v, dw0, db0, via_sets=False):
    """the protocol of the module docstring; -> ([dw of set s], [dbias of set s or None]) of the first call (CPU)"""
    from handwriting_line_generation_amd import ops
    name = c["name"]
    with ops.tuning(**c["env"]):
        r = Run(c, dev, u, v, dw0, db0, via_sets)
        assert r.need == WC.plan(c)["ws"], "%s: %s_workspace says %d bytes, the restated plan %d" % (name, r.entry, r.need, WC.plan(c)["ws"])
        before = ops.last_plan()
        rc = r.call()
        assert rc == 0, "%s: %s returned %d: %s" % (name, r.entry, rc, r.L.last_error())
        assert r.intact(), "%s: a canary next to a buffer was overwritten" % name
        assert r.gaps_intact(), "%s: a gap between the strided elements of dw was written" % name
        assert r.untouched(), "%s: u or v changed" % name
        dws = [r.dw(s) for s in range(c["sets"])]
        dbs = [r.db(s) if c["bias"] else None for s in range(c["sets"])]
        for s in range(c["sets"]):
            assert bool(torch.isfinite(dws[s]).all()), "%s set %d: %d non-finite elements of dw (a partial image nobody wrote, or an element never written)" % (
                name, s, int((~torch.isfinite(dws[s])).sum()))
            assert dbs[s] is None or bool(torch.isfinite(dbs[s]).all()), "%s set %d: non-finite bias gradient" % (name, s)
            if not c["bias"]:
                assert same_bits(r.dbd[s], r.before[len(r.dwd) + s]), "%s: dbias written without a fused bias gradient" % name
        want = WC.plan(c)["last_plan"]
        if want is not None:
            assert ops.last_plan() == want, "%s ran %s, the restated plan says %s" % (name, ops.last_plan(), want)
        else:
            assert ops.last_plan() == before, "%s: the direct kernel moved last_plan to %s" % (name, ops.last_plan())
        assert r.call() == 0
        for s in range(c["sets"]):
            assert same_bits(r.dw(s), dws[s]) and (dbs[s] is None or same_bits(r.db(s), dbs[s])), "%s set %d: the second call gives other bits" % (name, s)
        rc = r.call(short=1)
        assert rc == HWG_ERR_WORKSPACE, "%s: %d bytes of workspace for %d needed returned %d" % (name, r.need - 1, r.need, rc)
        assert r.outputs_untouched(), "%s: the refused call wrote to dw or dbias" % name
        assert r.intact() and r.untouched(), "%s: canaries / inputs after the repeated calls" % name
    return dws, dbs


def check_case(c, dws, dbs, refs, tag=""):
    for s, (ref, yard, bound, rb, yb, bb) in enumerate(refs):
        t = tag + (" set %d" % s if c["sets"] > 1 else "")
        check(c, dws[s], ref, yard, bound, t)
        if rb is not None:
            check(c, dbs[s], rb, yb, bb, t + " bias")


@pytest.mark.parametrize("c", WC.CASES, ids=[c["name"] for c in WC.CASES])
def test_wgrad_vs_fp64(cuda, c):
    refs = reference(c)
    dws, dbs = run_case(c, cuda, *WC.inputs(c))
    check_case(c, dws, dbs, refs)


@pytest.mark.parametrize("name", WC.SETS1_CASES)
def test_one_set_is_the_single_gradient_entry(cuda, name):
    """sets = 1 through the *_sets entry: the bits of hwg_conv_wgrad / hwg_wino_wgrad"""
    c = WC.BY_NAME[name]
    inp = WC.inputs(c)
    dws, dbs = run_case(c, cuda, *inp)
    dws1, dbs1 = run_case(c, cuda, *inp, via_sets=True)
    assert same_bits(dws1[0], dws[0]), "%s: one set through the sets entry differs from the single-gradient entry" % name
    assert dbs[0] is None or same_bits(dbs1[0], dbs[0]), name


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def refusal_case(name, geo, opt):
    N, H, W, C, K, Rr, S = geo["shape"]
    stride, pad, dil = geo.get("stride", (1, 1)), geo.get("pad", (0, 0)), geo.get("dil", (1, 1))
    P, Q = R.out_size(H, W, Rr, S, stride, pad, dil)
    return dict(name=name, engine="wino" if opt.get("wino") else "mfma", shape=geo["shape"], stride=stride, pad=pad, dil=dil, P=P, Q=Q, env={}, tags=set(),
                acc=False, bias=bool(opt.get("bias")), bias_acc=False, layout="kc", sets=1, set_on_v=opt.get("set_on_v", 0), wino=bool(opt.get("wino")))


@pytest.mark.parametrize("name, geo, opt", WC.REFUSALS, ids=[r[0] for r in WC.REFUSALS])
def test_refusals_write_nothing(cuda, name, geo, opt):
    """HWG_ERR_ARG, and neither dw, dbias, the workspace nor a canary is touched"""
    c = refusal_case(name, geo, opt)
    g = torch.Generator().manual_seed(5)
    N, H, W, C, K, Rr, S = c["shape"]
    sets = opt.get("sets", 1)
    n = max(sets, 1)
    u, v = torch.randn(1 if c["set_on_v"] else n, N, c["P"], c["Q"], K, generator=g), torch.randn(n if c["set_on_v"] else 1, N, H, W, C, generator=g)
    r = Run(c, cuda, u, v, None, None, via_sets="sets" in opt, n_ptrs=n, ws_floats=1 << 16)
    rc = r.call(sets=sets)
    assert rc == HWG_ERR_ARG, "%s: returned %d" % (name, rc)
    assert r.outputs_untouched() and r.intact() and r.untouched(), "%s: the refused call wrote something" % name
    assert bool(torch.isnan(r.ws).all()), "%s: the refused call wrote to the workspace" % name


# ---- index-exact -----------------------------------------------------------------------------------------------------------------------------
INDEX = [WC.BY_NAME[n] for n in WC.INDEX_CASES]


@pytest.mark.parametrize("c", INDEX, ids=WC.INDEX_CASES)
def test_impulses(cuda, c):
    """u zero but for ones, at most one per channel k and pass (the first and last pixel of split ranges, the last pixel, the image corners),
    overwrite: every product is by 1 and every sum is with 0, so dw[tap, k, :] is the fp32 value v[gather(pixel of k, tap), :] itself, or 0 in
    the padding, and the bias gradient the count of ones; the Winograd kernels are held to the bound with T = 1 (the ones per channel)"""
    c = dict(c, acc=False, bias_acc=False)
    _, v, _, _ = WC.inputs(c)
    passes = WC.impulse_passes(c)
    for i in range(len(passes)):
        u = torch.cat([WC.impulse_u(c, passes[(i + s) % len(passes)]) for s in range(1 if c["set_on_v"] else c["sets"])])
        dws, dbs = run_case(c, cuda, u, v, None, None)
        if c["engine"] in ("wino", "s2"):
            refs = reference_of(c, u, v, None, None, T=1.0)
            check_case(c, dws, dbs, refs, " impulses %d" % i)
        for s in range(c["sets"]):
            us, vs = WC.operands(c, u, v, s)
            if c["engine"] not in ("wino", "s2"):
                want = R.wgrad_direct(us.double(), vs.double(), WC.geom(c)).float()
                ok = torch.equal(dws[s], want)
                print("\nwgrad_fp64 %-34s %-6s impulses %d set %d: %s" % (c["name"], c["engine"], i, s, "equal" if ok else "NOT EQUAL"))
                assert ok, "%s impulses %d set %d: %d elements differ from the v they must be" % (c["name"], i, s, int((dws[s] != want).sum()))
            if c["bias"]:
                assert torch.equal(dbs[s], us.reshape(-1, us.shape[-1]).sum(0)), "%s impulses %d: the bias gradient is not the count of ones" % (c["name"], i)


NAN_CASES = [c for c in INDEX if "large" not in c["tags"]]


@pytest.mark.parametrize("c", NAN_CASES, ids=[c["name"] for c in NAN_CASES])
def test_one_nan_in_v(cuda, c):
    """direct-type kernels: the NaN set of dw is {taps under which some anchor pixel gathers the site} x all K x the site's channel; Winograd: it
    contains that set and lies within the taps the site's tiles feed, in that channel. The bias gradient stays finite."""
    from handwriting_line_generation_amd import ops
    c = dict(c, acc=False, bias_acc=False)
    u, v, _, _ = WC.inputs(c)
    N, H, W, C, K, Rr, S = c["shape"]
    site = (N - 1, H // 2, W // 3, C - 1)
    v[(0,) + site] = float("nan")
    fp = torch.zeros(Rr, S, K, C, dtype=torch.bool)
    fp[..., C - 1] = WC.tap_hits(c, site)[:, :, None]
    sup = torch.zeros(Rr, S, K, C, dtype=torch.bool)
    sup[..., C - 1] = WC.wino_tap_reach(c, site)[:, :, None]
    assert bool(fp.any())
    with ops.tuning(**c["env"]):
        r = Run(c, cuda, u, v, None, None)
        assert r.call() == 0 and r.intact()
        for s in range(c["sets"]):
            got = torch.isnan(r.dw(s))
            if c["set_on_v"] and s > 0:
                assert not bool(got.any()), "%s set %d: NaN from another set's v" % (c["name"], s)
            elif c["engine"] in ("wino", "s2"):
                assert bool((got | ~fp).all()), "%s: %d elements of the footprint are not NaN" % (c["name"], int((fp & ~got).sum()))
                assert bool((sup | ~got).all()), "%s: %d NaN outside the taps and channel the site feeds" % (c["name"], int((got & ~sup).sum()))
            else:
                assert torch.equal(got, fp), "%s set %d: the NaN set differs from the footprint in %d elements" % (c["name"], s, int((got != fp).sum()))
            assert not c["bias"] or bool(torch.isfinite(r.db(s)).all()), "%s: a NaN in v reached the bias gradient" % c["name"]


# ---- hwg_colsum -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, C, acc", WC.COLSUM_CASES, ids=["%dx%d_acc%d" % t for t in WC.COLSUM_CASES])
def test_colsum_vs_fp64(cuda, rows, C, acc):
    from handwriting_line_generation_amd import _lib as L, ops
    x, out0 = WC.colsum_input(rows, C, acc)
    need = int(L.query("hwg_colsum_workspace", rows, C))
    assert need == WC.colsum_chunks(rows) * C * 4
    (xd, od, ws), intact = carve(cuda, x.numel(), C, need // 4)
    put(xd, x)
    st = ops._stream()

    def call(short=0):
        ws.fill_(float("nan"))
        od.fill_(float("nan")) if out0 is None else put(od, out0)
        rc = L.query("hwg_colsum", xd, rows, C, od, acc, ws, need - short, st)
        torch.cuda.synchronize()
        return rc
    assert call() == 0 and intact()
    got = od.detach().cpu().clone()
    assert bool(torch.isfinite(got).all()) and same_bits(xd, x.reshape(-1))
    assert call() == 0 and same_bits(od, got), "the second call gives other bits"
    assert call(short=1) == HWG_ERR_WORKSPACE and intact()
    assert same_bits(od, torch.full((C,), float("nan")) if out0 is None else out0), "the refused call wrote to out"
    ref = R.colsum(x.double(), None if out0 is None else out0.double())
    yard = _rel(R.colsum(x, out0), ref)
    bound = R.sum_bound(rows + WC.colsum_chunks(rows) + acc, R.colsum(x.double(), None if out0 is None else out0.double(), absolute=True))
    check(dict(name="colsum_%dx%d_acc%d" % (rows, C, acc), engine="colsum"), got, ref, yard, bound)
