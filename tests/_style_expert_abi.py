"""The builders of tests/test_style_expert_abi_fp64_gpu.py (not collected by pytest): per family of csrc/style_ops.hip and csrc/expert_bank.hip,
case of oracle/style_cases.py -> the Guarded operands (tests/_guarded.py), the device pointer tables and the call lambdas of every entry.

Pointer tables (wptr, bptr, gwptr, gbptr, dyptr, gptrs, ptrs) are int64 INPUTS of the Guarded object, filled after carving with the addresses
of other carved views: the weights, biases and gradient buffers they name are carved buffers themselves, so an over-run of expert e's buffer
lands in a canary, and a table must have its bits after every call. A null entry is 0. Buffers an entry ADDS to are outputs pre-filled with the
case's non-zero values; the ones a null entry freezes (or an absent expert owns) are left out of `mine`, so protocol() asserts them unchanged.

`lib(G)` gives the function that calls an entry by name on the buffers of G: L.query on the GPU; Fake(G).query on CPU tensors - the fp32
restatements of oracle/style_ref.py behind the entries' signatures, with the flaws tests/test_style_expert_abi_cpu.py seeds. Every call
lambda is call(ws, ws_bytes, **over): `over` replaces arguments by name (None = NULL), which is how the refusal lists are run.

Out-of-range centres. window_setup() / scores_setup() with margin = True carve x out of the middle of a slab with one line of finite,
non-zero margin before and behind it; window_rows() / scores_rows() with edge = True use indices one step outside only. With the kernel's guard removed a bad row would then read the margin (a non-zero value
where the contract says 0) or put a window index into the canary next to win_of: inside this one allocation, never a fault.
edge_footprint() is that arithmetic; the CPU test asserts it."""
import numpy as np
import torch

from oracle import style_cases as SC
from oracle import style_ref as R
from _fp64 import YARDSTICK_FACTOR, _a, _d, _f, _ratio_rows, _rel, cpu_threads, entry, report
from _guarded import GUARD, HWG_ERR_WORKSPACE, Guarded

F32, I32, I64 = torch.float32, torch.int32, torch.int64
ULP = 2.0 ** -23
MARGIN = -1.0                 # the slab's margin lines: exp(-1) and -1 are both far from the 0 a guarded read gives
LB_OCHUNK, MC_ROWS = SC.LB_OCHUNK, SC.MC_MAXB
_REF = {}


def _cached(key, fn):
    if key not in _REF:
        cpu_threads()
        _REF[key] = fn()
    return _REF[key]


# ---- holding outputs to the references ---------------------------------------------------------------------------------------------------
def _kind(name):
    """dW3 -> dW, y0_1 -> y: the outputs that differ in a layer / expert / half index share a column of the printed line"""
    return name.rstrip("0123456789._")


def held(entry_name, shape, ws_bytes, outs, refs, extra=()):
    """outs {name: tensor}, refs {name: (fp64 value, yardstick, per-element bound)} as tests/test_style_expert_fp64_gpu.py holds them: the
    derived bound per element, YARDSTICK_FACTOR x the fp32 yardstick in relative L2. One line through _fp64.report (of the outputs that differ
    in a trailing index the worst) -> what is over"""
    worst = {}
    for name, got in outs.items():
        want, yard, bound = refs[name]
        got = got.detach().cpu()
        assert got.dtype == F32 and got.numel() == want.numel(), (entry_name, name, tuple(got.shape), tuple(want.shape))
        got = got.reshape(want.shape)
        assert bound is not None or (yard is not None and yard > 0), "%s %s: nothing to hold the output to" % (entry_name, name)
        if bound is not None:
            k = _kind(name)
            worst[k] = max(worst.get(k, 0.0), _ratio_rows(got, want, bound))
        if yard is not None and yard > 0:
            k = _kind(name) + " yard"
            worst[k] = max(worst.get(k, 0.0), _rel(got, want) / (YARDSTICK_FACTOR * yard))
    return report(entry_name, shape, ws_bytes, list(worst.items()) + list(extra))


# ---- tables and calls ----------------------------------------------------------------------------------------------------------------------
def fill_table(G, name, views):
    """the int64 input `name` <- the addresses of the carved views (None: a null entry)"""
    G.set_input(name, torch.tensor([0 if v is None else v.data_ptr() for v in views], dtype=I64))


def _entry(q, name, args):
    """args: {parameter name: value} in the order of include/hwg.h -> call(ws, n, **over)"""
    def call(ws=None, ws_bytes=0, /, **over):
        a = dict(args)
        if "workspace" in a:
            a["workspace"], a["workspace_bytes"] = ws, ws_bytes
        assert set(over) <= set(a), (name, sorted(set(over) - set(a)))
        a.update(over)
        return q(name, *a.values())
    call.args = args
    return call


def refusals(call, optional=(), sizes=None):
    """[(what, over)]: every operand that must not be null as NULL, every size as 0 and -1"""
    out = []
    for k, v in call.args.items():
        if k in ("stream", "workspace", "workspace_bytes") or k in optional:
            continue
        if torch.is_tensor(v):
            out.append(("%s = NULL" % k, {k: None}))
        elif isinstance(v, int) and (sizes is None or k in sizes):
            out += [("%s = 0" % k, {k: 0}), ("%s = -1" % k, {k: -1})]
    return out


def _stream(G):
    return G.st if G._on_gpu else None


# ---- LinearBank ----------------------------------------------------------------------------------------------------------------------------
def bank_layout(O, B):
    first = [int(v) for v in np.concatenate([[0], np.cumsum(O)])]
    return first, [f * B for f in first[:-1]]


def bank_refs(case, bias=True, gbias=True):
    """tests/_style_expert_checks.bank_reference for a variant of a table case (cached there for the table's own): without forward biases,
    without a bias-gradient table"""
    name, B, I, O, halves, unused, frozen, xgrad, backward = case
    if bias and gbias and case in SC.BANK_CASES:
        import _style_expert_checks as K
        return K.bank_reference(case)

    def make():
        import _style_expert_checks as K
        fwd = R.linear_bank_fwd if bias else (lambda X, W, b, h: R.linear_bank_fwd(X, W, [torch.zeros_like(v) for v in b], h))
        ref, yard, absv = (K.bank_values(case, c, fwd=fwd) for c in (_d, _f, _a))
        Kn = lambda k: I + int(bias) if k[0] == "y" else sum(O) if k == "dx" else B + 1          # noqa: E731
        return {k: entry(v, yard[k], R.sum_bound(Kn(k), absv[k])) for k, v in ref.items() if gbias or not k.startswith("db")}
    return _cached(("bank", case[0], tuple(unused), tuple(sorted(frozen.items())), xgrad, bias, gbias), make)


def bank_forward(dev, lib, case, bias=True):
    name, B, I, O, halves = case[:5]
    x, Ws, bs, dys, gW, gb = SC.bank_inputs(case)
    L_ = len(O)
    first, off = bank_layout(O, B)
    ins = dict(x=x, O=torch.tensor(O, dtype=I32), first=torch.tensor(first, dtype=I32), off=torch.tensor(off, dtype=I64), wptr=torch.zeros(L_, dtype=I64))
    ins.update({"W%d" % l: Ws[l] for l in range(L_)})
    if bias:
        ins.update({"b%d" % l: bs[l] for l in range(L_)}, bptr=torch.zeros(L_, dtype=I64))
    G = Guarded(dev, ins, dict(y=((first[-1] * B,), F32)))
    t = G.t
    fill_table(G, "wptr", [t("W%d" % l) for l in range(L_)])
    if bias:
        fill_table(G, "bptr", [t("b%d" % l) for l in range(L_)])
    G.call = _entry(lib(G), "hwg_linear_bank_fwd", dict(
        x=t("x"), wptr=t("wptr"), bptr=t("bptr") if bias else None, O=t("O"), first_wave=t("first"), off=t("off"), L=L_, B=B, I=I, halves=halves,
        total_outputs=first[-1], y=t("y"), stream=_stream(G)))
    return G


def bank_parts(y, O, B, halves):
    """the flat y of hwg_linear_bank_fwd -> {"y<l>_<h>": [B, O_l / halves]}"""
    first, off = bank_layout(O, B)
    out = {}
    for l, o in enumerate(O):
        C = o // halves
        for h in range(halves):
            out["y%d_%d" % (l, h)] = y[off[l] + h * B * C:off[l] + (h + 1) * B * C].view(B, C)
    return out


def bank_backward(dev, lib, case, gbias=True):
    """-> Guarded with .call, .mine (what the tables let the entry add to, and dx) and .frozen (the buffers it must leave alone)"""
    name, B, I, O, halves, unused, frozen, xgrad, backward = case
    x, Ws, bs, dys, gW, gb = SC.bank_inputs(case)
    L_ = len(O)
    first, off = bank_layout(O, B)
    q0 = lib(None)
    need = int(q0("hwg_linear_bank_bwd_workspace", first[-1], B, I)) if xgrad else 0
    assert need == (((first[-1] + LB_OCHUNK - 1) // LB_OCHUNK) * B * I * 4 if xgrad else 0)
    ins = dict(x=x, O=torch.tensor(O, dtype=I32), first=torch.tensor(first, dtype=I32), wptr=torch.zeros(L_, dtype=I64),
               dyptr=torch.zeros(L_ * halves, dtype=I64), gwptr=torch.zeros(L_, dtype=I64))
    if gbias:
        ins["gbptr"] = torch.zeros(L_, dtype=I64)
    ins.update({"W%d" % l: Ws[l] for l in range(L_)})
    ins.update({"dy%d_%d" % (l, h): dys[l][h] for l in range(L_) for h in range(halves) if (l, h) not in unused})
    outs = {}
    for l in range(L_):
        outs["dW%d" % l], outs["db%d" % l] = gW[l], gb[l]
    if xgrad:
        outs["dx"] = ((B, I), F32)
    G = Guarded(dev, ins, outs, need)
    t = G.t
    fill_table(G, "wptr", [t("W%d" % l) for l in range(L_)])
    fill_table(G, "dyptr", [None if (l, h) in unused else t("dy%d_%d" % (l, h)) for l in range(L_) for h in range(halves)])
    fill_table(G, "gwptr", [None if l in frozen else t("dW%d" % l) for l in range(L_)])
    if gbias:
        fill_table(G, "gbptr", [None if frozen.get(l) == "all" else t("db%d" % l) for l in range(L_)])
    G.mine = ["dW%d" % l for l in range(L_) if l not in frozen] + (["db%d" % l for l in range(L_) if frozen.get(l) != "all"] if gbias else [])
    G.mine += ["dx"] if xgrad else []
    G.frozen = [k for k in outs if k not in G.mine]
    G.call = _entry(lib(G), "hwg_linear_bank_bwd", dict(
        x=t("x"), dyptr=t("dyptr"), wptr=t("wptr"), gwptr=t("gwptr"), gbptr=t("gbptr") if gbias else None, O=t("O"), first_wave=t("first"), L=L_, B=B,
        I=I, halves=halves, total_outputs=first[-1], dx=t("dx") if xgrad else None, workspace=None, workspace_bytes=0, stream=_stream(G)))
    return G


# ---- MLPChain ------------------------------------------------------------------------------------------------------------------------------
def chain_refs(case, gbias=True):
    """tests/_style_expert_checks.chain_reference after ONE backward pass (the wrapper-level test runs two in a row)"""
    def make():
        import _style_expert_checks as K
        x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
        (ref, acts), (yard, _) = K.chain_values(case, _d, passes=1), K.chain_values(case, _f, passes=1)
        hb = R.chain_fwd_bound(acts, [_d(w) for w in Ws], [_d(b) for b in bs])
        return {k: entry(v, yard[k], hb if k == "h" else None) for k, v in ref.items()}
    refs = _cached(("chain", case), make)
    return refs if gbias else {k: v for k, v in refs.items() if not k.startswith("db")}


def chain_forward(dev, lib, case):
    name, D, B, L_, frozen, backward = case
    x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
    ins = dict(x=x, wptr=torch.zeros(L_, dtype=I64), bptr=torch.zeros(L_, dtype=I64))
    ins.update({"W%d" % l: Ws[l] for l in range(L_)})
    ins.update({"b%d" % l: bs[l] for l in range(L_)})
    G = Guarded(dev, ins, dict(acts=((L_ + 1, B, D), F32)))
    t = G.t
    fill_table(G, "wptr", [t("W%d" % l) for l in range(L_)])
    fill_table(G, "bptr", [t("b%d" % l) for l in range(L_)])
    G.call = _entry(lib(G), "hwg_mlp_chain_fwd", dict(x=t("x"), wptr=t("wptr"), bptr=t("bptr"), L=L_, B=B, D=D, slope=SC.CHAIN_SLOPE, acts=t("acts"),
                                                      stream=_stream(G)))
    return G


def chain_backward(dev, lib, case, acts, dx=True, gbias=True, wfrozen=None):
    """-> Guarded with .single, .split (hwg_mlp_chain_bwd / _bwd_split on the same buffers; the workspace is the split entry's), .mine, .frozen.
    The case's frozen layer has null entries in both tables; `wfrozen`: a layer whose gwptr entry alone is null (its bias trains)"""
    name, D, B, L_, frozen, backward = case
    x, Ws, bs, dout, gW, gb = SC.chain_inputs(case)
    need = int(lib(None)("hwg_mlp_chain_bwd_workspace", L_, B, D))
    assert need == L_ * MC_ROWS * D * 4
    ins = dict(dout=dout, acts=acts, wptr=torch.zeros(L_, dtype=I64), gwptr=torch.zeros(L_, dtype=I64))
    if gbias:
        ins["gbptr"] = torch.zeros(L_, dtype=I64)
    ins.update({"W%d" % l: Ws[l] for l in range(L_)})
    outs = {}
    for l in range(L_):
        outs["dW%d" % l], outs["db%d" % l] = gW[l], gb[l]
    if dx:
        outs["dx"] = ((B, D), F32)
    G = Guarded(dev, ins, outs, need)
    t = G.t
    fill_table(G, "wptr", [t("W%d" % l) for l in range(L_)])
    fill_table(G, "gwptr", [None if l in (frozen, wfrozen) else t("dW%d" % l) for l in range(L_)])
    if gbias:
        fill_table(G, "gbptr", [None if l == frozen else t("db%d" % l) for l in range(L_)])
    G.mine = ["dW%d" % l for l in range(L_) if l not in (frozen, wfrozen)] + (["db%d" % l for l in range(L_) if l != frozen] if gbias else []) + (["dx"] if dx else [])
    G.frozen = [k for k in outs if k not in G.mine]
    common = dict(dout=t("dout"), acts=t("acts"), wptr=t("wptr"), gwptr=t("gwptr"), gbptr=t("gbptr") if gbias else None, L=L_, B=B, D=D,
                  slope=SC.CHAIN_SLOPE, dx=t("dx") if dx else None)
    G.single = _entry(lib(G), "hwg_mlp_chain_bwd", dict(common, stream=_stream(G)))
    G.split = _entry(lib(G), "hwg_mlp_chain_bwd_split", dict(common, workspace=None, workspace_bytes=0, stream=_stream(G)))
    return G


# ---- grouped Conv1d --------------------------------------------------------------------------------------------------------------------------
def conv_plan(cls, R_):
    """the run and tile tables of model/expert_bank.make_plan / plan_tiles on the host (int32 numpy)"""
    from handwriting_line_generation_amd.model import expert_bank
    change = np.nonzero(np.diff(cls))[0] + 1
    starts = np.concatenate([[0], change, [cls.size]]).astype(np.int32)
    seg_eid = cls[starts[:-1]].astype(np.int32)
    tseg, trow, _ = expert_bank._tiles_host(starts, R_, expert_bank.TILE_ROWS)
    wseg, wrow, wrun = expert_bank._tiles_host(starts, R_, expert_bank.WGRAD_TILE_ROWS)
    return dict(seg_start=starts, seg_eid=seg_eid, tseg=tseg, trow=trow, wseg=wseg, wrow=wrow, wrun=wrun, tile_rows=expert_bank.WGRAD_TILE_ROWS)


def conv_refs(case):
    """tests/_style_expert_checks.conv_reference; a variant of a table case (bias tables dropped) is formed the same way under its own key"""
    import _style_expert_checks as K
    if case in SC.CONV_CASES:
        return K.conv_reference(case)

    def make():
        name, Cin, Cout, S, R_, plan, bias = case
        ref, yard, absv = K.conv_values(case, _d), K.conv_values(case, _f), K.conv_values(case, _a)
        rows = {e: n * R_ for e, n in SC.PLANS[plan][R_].items()}
        Kn = {"y": Cin * S + int(bias), "dx": Cout * S}
        return {k: entry(v, yard[k], R.sum_bound(Kn[k] if k in Kn else rows[int(k[2:])] + 1, absv[k])) for k, v in ref.items()}
    return _cached(("conv", case), make)


def conv_setup(dev, lib, case):
    """one Guarded for the three entries -> .fwd, .dgrad, .wgrad, .present (expert ids), .mine_wgrad"""
    name, Cin, Cout, S, R_, plan_name, bias = case
    x, dy, Ws, bs, gW, gb = SC.conv_inputs(case)
    cls = SC.plan_cls(plan_name, R_)
    p = conv_plan(cls, R_)
    n, nt, wnt, G_ = int(cls.size), int(p["tseg"].size), int(p["wseg"].size), int(p["seg_eid"].size)
    need = int(lib(None)("hwg_grouped_conv1d_wgrad_workspace", wnt, Cin, Cout, S))
    assert need == wnt * (Cout * Cin * S + Cout) * 4
    ins = dict(x=x, dy=dy, wptr=torch.zeros(SC.E, dtype=I64), gwptr=torch.zeros(SC.E, dtype=I64))
    ins.update({k: torch.from_numpy(p[k]) for k in ("seg_start", "seg_eid", "tseg", "trow", "wseg", "wrow", "wrun")})
    ins.update({"W%d" % e: Ws[e] for e in range(SC.E)})
    if bias:
        ins.update({"b%d" % e: bs[e] for e in range(SC.E)}, bptr=torch.zeros(SC.E, dtype=I64), gbptr=torch.zeros(SC.E, dtype=I64))
    outs = dict(y=((n, R_, Cout), F32), dx=((n, R_, Cin), F32))
    for e in range(SC.E):
        outs["dW%d" % e], outs["db%d" % e] = gW[e], gb[e]
    G = Guarded(dev, ins, outs, need)
    t = G.t
    fill_table(G, "wptr", [t("W%d" % e) for e in range(SC.E)])
    fill_table(G, "gwptr", [t("dW%d" % e) for e in range(SC.E)])
    if bias:
        fill_table(G, "bptr", [t("b%d" % e) for e in range(SC.E)])
        fill_table(G, "gbptr", [t("db%d" % e) for e in range(SC.E)])
    G.present = sorted(SC.PLANS[plan_name][R_])
    G.mine_wgrad = ["dW%d" % e for e in G.present] + (["db%d" % e for e in G.present] if bias else [])
    q, st = lib(G), _stream(G)
    tiles = dict(seg_start=t("seg_start"), seg_eid=t("seg_eid"), tile_seg=t("tseg"), tile_row0=t("trow"), ntiles=nt)
    geom = dict(R=R_, Cin=Cin, Cout=Cout, S=S, pad=S // 2)
    G.fwd = _entry(q, "hwg_grouped_conv1d_fwd", dict(dict(x=t("x")), **tiles, wptr=t("wptr"), bptr=t("bptr") if bias else None, y=t("y"), **geom, stream=st))
    G.dgrad = _entry(q, "hwg_grouped_conv1d_dgrad", dict(dict(dy=t("dy")), **tiles, wptr=t("wptr"), dx=t("dx"), **geom, stream=st))
    G.wgrad = _entry(q, "hwg_grouped_conv1d_wgrad", dict(
        dy=t("dy"), x=t("x"), seg_start=t("seg_start"), seg_eid=t("seg_eid"), G=G_, tile_seg=t("wseg"), tile_row0=t("wrow"), run_tile0=t("wrun"), ntiles=wnt,
        tile_rows=p["tile_rows"], gwptr=t("gwptr"), gbptr=t("gbptr") if bias else None, **geom, workspace=None, workspace_bytes=0, stream=st))
    return G


def accumulate_setup(dev, lib, C):
    """hwg_gather_rows_ptr (-> .gather on its own Guarded .Gg) and hwg_segment_accumulate_ptr (.call) over SC.ACCUMULATE_RUNS"""
    import _style_expert_checks as K
    cls, rows, pre, refs = K.accumulate_reference(C)
    p = conv_plan(cls, 1)
    n, G_ = int(cls.size), int(p["seg_eid"].size)
    ins = dict(eid=torch.from_numpy(cls.astype(np.int32)), ptrs=torch.zeros(SC.E, dtype=I64))
    ins.update({"src%d" % e: pre[e] for e in range(SC.E)})
    Gg = Guarded(dev, ins, dict(out=((n, C), F32)))
    fill_table(Gg, "ptrs", [Gg.t("src%d" % e) for e in range(SC.E)])
    Gg.call = _entry(lib(Gg), "hwg_gather_rows_ptr", dict(ptrs=Gg.t("ptrs"), eid=Gg.t("eid"), out=Gg.t("out"), n=n, C=C, stream=_stream(Gg)))
    ins = dict(rows=rows, seg_start=torch.from_numpy(p["seg_start"]), seg_eid=torch.from_numpy(p["seg_eid"]), gptrs=torch.zeros(SC.E, dtype=I64))
    G = Guarded(dev, ins, {"g%d" % e: pre[e] for e in range(SC.E)})
    fill_table(G, "gptrs", [G.t("g%d" % e) for e in range(SC.E)])
    G.mine = ["g%d" % e for e in sorted(SC.ACCUMULATE_RUNS)]
    G.call = _entry(lib(G), "hwg_segment_accumulate_ptr", dict(rows=G.t("rows"), seg_start=G.t("seg_start"), seg_eid=G.t("seg_eid"), G=G_, gptrs=G.t("gptrs"),
                                                               C=C, stream=_stream(G)))
    G.Gg, G.want_rows, G.refs = Gg, pre[torch.from_numpy(cls)], refs
    return G


# ---- windows, scores -----------------------------------------------------------------------------------------------------------------------
def _slab(x, margin):
    """x [B, ...] -> the slab the Guarded object holds (one line of MARGIN before and behind x when `margin`), and the view of x inside it"""
    if not margin:
        return x, (lambda s: s)
    pad = torch.full_like(x[:1], MARGIN)
    return torch.cat([pad, x, pad]), (lambda s: s[1:-1])


def window_setup(dev, lib, case, ib, ip, dp, margin=False):
    """hwg_gather_windows (.gather on .Gg) and hwg_scatter_windows (.call; win_of: an owned int32 scratch output of B * Wx elements)"""
    name, B, Wx, C, w = case
    x = SC.window_inputs(case)[0]
    n = int(ib.numel())
    slab, inner = _slab(x, margin)
    Gg = Guarded(dev, dict(x=slab, ib=ib, ip=ip), dict(patches=((n, 2 * w + 1, C), F32)))
    Gg.call = _entry(lib(Gg), "hwg_gather_windows", dict(x=inner(Gg.t("x")), B=B, Wx=Wx, C=C, idx_b=Gg.t("ib"), idx_pos=Gg.t("ip"), n=n, window=w,
                                                         patches=Gg.t("patches"), stream=_stream(Gg)))
    G = Guarded(dev, dict(dp=dp, ib=ib, ip=ip), dict(win_of=((B * Wx,), I32), dx=((B, Wx, C), F32)))
    G.call = _entry(lib(G), "hwg_scatter_windows", dict(dpatches=G.t("dp"), B=B, Wx=Wx, C=C, idx_b=G.t("ib"), idx_pos=G.t("ip"), n=n, window=w,
                                                        win_of=G.t("win_of"), dx=G.t("dx"), stream=_stream(G)))
    G.Gg = Gg
    return G


def window_rows(case, edge=False):
    """the centres of SC.window_inputs that lie inside the tensor (-> idx_b, idx_pos, d patches, None); with `edge`, centres ONE STEP outside
    are put between them: idx_b in {-1, B}, idx_pos in {-1, Wx} (-> ..., the mask of the good rows)"""
    name, B, Wx, C, w = case
    x, ib, ip, dp, n_in = SC.window_inputs(case)
    inside = (ib >= 0) & (ib < B) & (ip >= 0) & (ip < Wx)
    ib, ip, dp = ib[inside], ip[inside], dp[inside]
    assert int(ib.numel()) == n_in
    if not edge:
        return ib, ip, dp, None
    bad = [(-1, 0), (B, Wx - 1), (0, -1), (B - 1, Wx), (-1, Wx // 2), (B, 1)]
    g = SC.gen("win_edge_" + name)
    at = sorted(torch.randperm(n_in + 1, generator=g)[:len(bad)].tolist())         # before which good row each bad one goes (the last: behind them all)
    rows, good = [], []
    k = 0
    for i in range(n_in + 1):
        while k < len(bad) and at[k] == i:
            rows.append(bad[k] + (torch.randn(2 * w + 1, C, generator=g) + 3.0,))
            good.append(False)
            k += 1
        if i < n_in:
            rows.append((int(ib[i]), int(ip[i]), dp[i]))
            good.append(True)
    return (torch.tensor([r[0] for r in rows], dtype=I32), torch.tensor([r[1] for r in rows], dtype=I32), torch.stack([r[2] for r in rows]),
            torch.tensor(good))


def edge_footprint(B, Wx, C, w, ib, ip, good):
    """what the bad rows would touch with the centre clause of the kernels' guards REMOVED (the position clause kept) -> (lowest, highest
    float offset from x[0][0][0] read by gather_windows_kernel; lowest, highest int offset from win_of[0] written by window_index_kernel)"""
    xs, ws = [], []
    for b, p, ok in zip(ib.tolist(), ip.tolist(), good.tolist()):
        if ok:
            continue
        ws.append(b * Wx + p)
        for pos in range(p - w, p + w + 1):
            if 0 <= pos < Wx:
                xs += [(b * Wx + pos) * C, (b * Wx + pos) * C + C - 1]
    return min(xs), max(xs), min(ws), max(ws)


SCORES_EDGE = (2, 5, 12)           # B, Wx, C: Wx * C = 60 floats, under the 64 of a canary


def scores_rows(edge):
    """-> x, idx_b, idx_pos, idx_cls[, good]: SC.scores_inputs, or the small tensor with rows one step outside in each index put between good ones"""
    if not edge:
        return SC.scores_inputs()
    B, Wx, C = SCORES_EDGE
    g = SC.gen("scores_edge")
    x = -20.0 * torch.rand(B, Wx, C, generator=g)
    rows = [(int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, Wx, (1,), generator=g)), int(torch.randint(0, C, (1,), generator=g)), True)
            for _ in range(14)] + [(0, 0, 0, True), (B - 1, Wx - 1, C - 1, True)]
    bad = [(-1, 0, 0), (B, Wx - 1, C - 1), (1, -1, 3), (0, Wx, 3), (1, 2, -1), (0, 2, C), (B - 1, Wx - 1, C), (0, 0, -1)]
    for i, r in enumerate(bad):
        rows.insert(2 * i + 1, r + (False,))
    cols = [torch.tensor([r[i] for r in rows], dtype=I32) for i in range(3)]
    return x, cols[0], cols[1], cols[2], torch.tensor([r[3] for r in rows])


def scores_setup(dev, lib, x, ib, ip, ic, margin=False):
    B, Wx, C = x.shape
    n = int(ib.numel())
    slab, inner = _slab(x, margin)
    G = Guarded(dev, dict(x=slab, ib=ib, ip=ip, ic=ic), dict(out=((n,), F32)))
    G.call = _entry(lib(G), "hwg_gather_scores", dict(x=inner(G.t("x")), B=B, Wx=Wx, C=C, idx_b=G.t("ib"), idx_pos=G.t("ip"), idx_cls=G.t("ic"), n=n,
                                                      out=G.t("out"), stream=_stream(G)))
    return G


def edge_rows_hold(tag, with_bad, without_bad, good, sums=()):
    """the contract of the out-of-range rows: a bad row of a gathered output is +0 in every element, the good rows have the bits of the call
    without the bad rows; an output that is a sum over the rows (`sums`) has the bits of that call"""
    from _guarded import same_bits
    for k, a in with_bad.items():
        b = without_bad[k]
        if k in sums:
            assert same_bits(a, b), "%s: the rows outside the tensor changed %s" % (tag, k)
            continue
        assert not bool(a[~good].reshape(-1).view(I32).any()), "%s: a row outside the tensor gave a non-zero %s" % (tag, k)
        assert same_bits(a[good], b), "%s: the rows inside the tensor differ from the call without the bad rows in %s" % (tag, k)


# ---- segment mean ----------------------------------------------------------------------------------------------------------------------------
def seg_setup(dev, lib, case):
    """hwg_segment_weighted_mean on a Guarded with .call; .backward(wsum) -> the Guarded of hwg_segment_weighted_mean_bwd"""
    name, n, B, C, kind = case
    v, wgt, seg, dout = SC.seg_inputs(case)
    G = Guarded(dev, dict(v=v, wgt=wgt, seg=seg), dict(out=((B, C), F32), wsum=((B,), F32)))
    G.call = _entry(lib(G), "hwg_segment_weighted_mean", dict(v=G.t("v"), wgt=G.t("wgt"), seg=G.t("seg"), n=n, C=C, B=B, out=G.t("out"), wsum=G.t("wsum"),
                                                              stream=_stream(G)))

    def backward(wsum):
        Gb = Guarded(dev, dict(dout=dout, wgt=wgt, seg=seg, wsum=wsum), dict(dv=((n, C), F32)))
        Gb.call = _entry(lib(Gb), "hwg_segment_weighted_mean_bwd", dict(dout=Gb.t("dout"), wgt=Gb.t("wgt"), seg=Gb.t("seg"), wsum=Gb.t("wsum"), n=n, C=C,
                                                                       dv=Gb.t("dv"), stream=_stream(Gb)))
        return Gb
    G.backward = backward
    return G


# ---- the entries on CPU tensors ------------------------------------------------------------------------------------------------------------
class Fake:
    """the entries of the two families as fp32 restatements (oracle/style_ref.py) on the carved CPU views of one Guarded object, behind the
    signatures of include/hwg.h. Pointer tables are resolved to the carved views whose address they hold. `flaw` seeds one misbehaviour:
      adds_then_refuses     hwg_linear_bank_bwd adds dW / db and only then checks the workspace (the order the entry had)
      reduce_reads_unwritten  its data-gradient pass leaves the last workspace chunk unwritten, the reduce pass sums every chunk
      frozen_changes        it adds to the weight-gradient buffer of a layer whose table entry is null
      past_end              hwg_grouped_conv1d_wgrad stores one element behind the first present expert's weight-gradient buffer
      no_centre_guard       hwg_gather_windows / hwg_scatter_windows / hwg_gather_scores without the centre clause of their guards"""

    def __init__(self, G, flaw=None):
        self.G, self.flaw = G, flaw

    def query(self, name, *args):
        return getattr(self, name)(*args)

    def at(self, addr):
        for k, v in self.G.f.items():
            if v.numel() and v.data_ptr() == addr:
                return self.G.t(k)
        raise AssertionError("a table entry names no carved buffer")

    def table(self, tab, n=None):
        return [self.at(a) if a else None for a in tab.view(I64).reshape(-1)[:n].tolist()]

    @staticmethod
    def beyond(view, offset):
        """the element `offset` elements from view's first one, wherever in the allocation that is (what a kernel's address arithmetic reaches)"""
        return view.as_strided((1,), (1,), view.storage_offset() + offset)

    # workspace sizes
    @staticmethod
    def hwg_linear_bank_bwd_workspace(total, B, I):
        return (max(total, 1) + LB_OCHUNK - 1) // LB_OCHUNK * max(B, 0) * max(I, 0) * 4

    @staticmethod
    def hwg_mlp_chain_bwd_workspace(L_, B, D):
        return max(L_, 0) * MC_ROWS * max(D, 0) * 4

    @staticmethod
    def hwg_grouped_conv1d_wgrad_workspace(ntiles, Cin, Cout, S):
        return max(ntiles, 0) * (Cout * Cin * S + Cout) * 4

    # windows, scores, segment mean
    def hwg_gather_windows(self, x, B, Wx, C, ib, ip, n, w, patches, st):
        if self.flaw != "no_centre_guard":
            patches.copy_(R.gather_windows(x.reshape(B, Wx, C), ib, ip, w))
            return 0
        for k in range(n):
            for j in range(2 * w + 1):
                pos = int(ip[k]) - w + j
                for c in range(C):
                    patches[k, j, c] = self.beyond(x, ((int(ib[k]) * Wx + pos) * C + c))[0] if 0 <= pos < Wx else 0.0
        return 0

    def hwg_scatter_windows(self, dp, B, Wx, C, ib, ip, n, w, win_of, dx, st):
        win_of.fill_(-1)
        for k in range(n):
            b, p = int(ib[k]), int(ip[k])
            if self.flaw == "no_centre_guard" or (0 <= b < B and 0 <= p < Wx):
                cell = self.beyond(win_of, b * Wx + p)
                cell.copy_(torch.maximum(cell, torch.tensor([k], dtype=I32)))
        dx.copy_(R.scatter_windows(dp, ib, ip, w, B, Wx))
        return 0

    def hwg_gather_scores(self, x, B, Wx, C, ib, ip, ic, n, out, st):
        for k in range(n):
            b, p, c = int(ib[k]), int(ip[k]), int(ic[k])
            ok = 0 <= b < B and 0 <= p < Wx and 0 <= c < C
            out[k] = torch.exp(self.beyond(x, (b * Wx + p) * C + c))[0] if ok or self.flaw == "no_centre_guard" else 0.0
        return 0

    def hwg_segment_weighted_mean(self, v, wgt, seg, n, C, B, out, wsum, st):
        o, ws = R.segment_mean(v, wgt, seg, B)
        out.copy_(o)
        wsum.copy_(ws)
        return 0

    def hwg_segment_weighted_mean_bwd(self, dout, wgt, seg, wsum, n, C, dv, st):
        dv.copy_(R.segment_mean_bwd(dout, wgt, seg, wsum))
        return 0

    # LinearBank
    def hwg_linear_bank_fwd(self, x, wptr, bptr, O, first, off, L_, B, I, halves, total, y, st):
        Ws = self.table(wptr, L_)
        bs = self.table(bptr, L_) if bptr is not None else [torch.zeros(W.shape[0]) for W in Ws]
        parts = R.linear_bank_fwd(x, Ws, bs, halves)
        for l in range(L_):
            C = int(O[l]) // halves
            for h in range(halves):
                o = int(off[l]) + h * B * C
                y[o:o + B * C] = parts[l][h].reshape(-1)
        return 0

    def hwg_linear_bank_bwd(self, x, dyptr, wptr, gwptr, gbptr, O, first, L_, B, I, halves, total, dx, ws, nbytes, st):
        short = dx is not None and (ws is None or nbytes < self.hwg_linear_bank_bwd_workspace(total, B, I))
        if short and self.flaw != "adds_then_refuses":
            return HWG_ERR_WORKSPACE
        Ws, gw = self.table(wptr, L_), self.table(gwptr, L_)
        gb = self.table(gbptr, L_) if gbptr is not None else [None] * L_
        flat = self.table(dyptr, L_ * halves)
        dys = [flat[l * halves:(l + 1) * halves] for l in range(L_)]
        _, dWs, dbs = R.linear_bank_bwd(x, Ws, dys, halves)
        for l in range(L_):
            if gw[l] is not None:
                gw[l].add_(dWs[l])
            elif self.flaw == "frozen_changes":
                self.G.t("dW%d" % l).add_(dWs[l])
            if gb[l] is not None:
                gb[l].add_(dbs[l])
        if short:
            return HWG_ERR_WORKSPACE
        if dx is not None:
            dy, Wc = R._bank_dy(x, Ws, dys, halves), torch.cat(Ws, 0)
            nch = (total + LB_OCHUNK - 1) // LB_OCHUNK
            part = ws.view(F32)[:nch * B * I].view(nch, B, I)
            for c in range(nch - (self.flaw == "reduce_reads_unwritten")):
                part[c] = dy[:, c * LB_OCHUNK:(c + 1) * LB_OCHUNK] @ Wc[c * LB_OCHUNK:(c + 1) * LB_OCHUNK]
            dx.copy_(part.sum(0))
        return 0

    # MLPChain
    def hwg_mlp_chain_fwd(self, x, wptr, bptr, L_, B, D, slope, acts, st):
        acts.copy_(torch.stack(R.mlp_chain_fwd(x, self.table(wptr, L_), self.table(bptr, L_), slope)))
        return 0

    def hwg_mlp_chain_bwd(self, dout, acts, wptr, gwptr, gbptr, L_, B, D, slope, dx, st):
        d, dWs, dbs = R.mlp_chain_bwd(dout, list(acts), self.table(wptr, L_), slope)
        gw = self.table(gwptr, L_)
        gb = self.table(gbptr, L_) if gbptr is not None else [None] * L_
        for l in range(L_):
            if gw[l] is not None:
                gw[l].add_(dWs[l])
            if gb[l] is not None:
                gb[l].add_(dbs[l])
        if dx is not None:
            dx.copy_(d)
        return 0

    def hwg_mlp_chain_bwd_split(self, dout, acts, wptr, gwptr, gbptr, L_, B, D, slope, dx, ws, nbytes, st):
        if ws is None or nbytes < self.hwg_mlp_chain_bwd_workspace(L_, B, D):
            return HWG_ERR_WORKSPACE
        ws.fill_(0.5)
        return self.hwg_mlp_chain_bwd(dout, acts, wptr, gwptr, gbptr, L_, B, D, slope, dx, st)

    # grouped Conv1d
    @staticmethod
    def _cls(seg_start, seg_eid):
        return np.repeat(seg_eid.numpy().astype(np.int64), np.diff(seg_start.numpy()))

    def hwg_grouped_conv1d_fwd(self, x, seg_start, seg_eid, tile_seg, tile_row0, ntiles, wptr, bptr, y, R_, Cin, Cout, S, pad, st):
        y.copy_(R.grouped_conv_fwd(x, self._cls(seg_start, seg_eid), self.table(wptr), self.table(bptr) if bptr is not None else None, S))
        return 0

    def hwg_grouped_conv1d_dgrad(self, dy, seg_start, seg_eid, tile_seg, tile_row0, ntiles, wptr, dx, R_, Cin, Cout, S, pad, st):
        dx.copy_(R.grouped_conv_dgrad(dy, self._cls(seg_start, seg_eid), self.table(wptr), S))
        return 0

    def hwg_grouped_conv1d_wgrad(self, dy, x, seg_start, seg_eid, G_, tile_seg, tile_row0, run_tile0, ntiles, tile_rows, gwptr, gbptr, R_, Cin, Cout, S,
                                 pad, ws, nbytes, st):
        if ws is None or nbytes < self.hwg_grouped_conv1d_wgrad_workspace(ntiles, Cin, Cout, S):
            return HWG_ERR_WORKSPACE
        ws.fill_(0.5)
        gw = self.table(gwptr)
        gb = self.table(gbptr) if gbptr is not None else None
        for e, (dW, db) in R.grouped_conv_wgrad(dy, x, self._cls(seg_start, seg_eid), S).items():
            gw[e].add_(dW)
            if gb is not None:
                gb[e].add_(db)
        if self.flaw == "past_end":
            e = int(seg_eid[0])
            self.beyond(gw[e].reshape(-1), gw[e].numel()).fill_(1.0)
        return 0

    def hwg_gather_rows_ptr(self, ptrs, eid, out, n, C, st):
        out.copy_(torch.stack(self.table(ptrs))[eid.long()])
        return 0

    def hwg_segment_accumulate_ptr(self, rows, seg_start, seg_eid, G_, gptrs, C, st):
        dst = self.table(gptrs)
        for e, s in R.segment_accumulate(rows, self._cls(seg_start, seg_eid)).items():
            dst[e].add_(s)
        return 0


def fake_lib(flaw=None):
    return lambda G: Fake(G, flaw).query
