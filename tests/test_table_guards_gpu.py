"""GPU: the in-kernel guards of the entries that read their geometry from device-resident tables - hwg_fg_masks, hwg_store_batch,
hwg_store_line_stats, hwg_store_warp_batch, hwg_lines_from_u8, hwg_stretch_onehot - and the clamps of hwg_lines_to_u8, hwg_augment_stats and
hwg_augment_warp, called at the C ABI through L.query with tables that ops would have refused on the host. Every other test of these files
goes through ops.* and never reaches this code. The protocol (operands carved out of one allocation with canaries, poisoned outputs, inputs
bit-identical afterwards, a second call with the same bits, refusals that write nothing) is that of tests/_guarded.py, as in
tests/test_norm_abi_fp64_gpu.py and tests/test_seq_loss_abi_fp64_gpu.py. Case tables, the slabs and the numpy models: oracle/table_cases.py, checked on
the CPU by tests/test_table_guards_cpu.py - in particular that no bad row names memory outside this file's one allocation even with its
guard removed: a guard that is wrong shows here as a wrong byte, never as a fault. The offsets that overflow (2^62 and above) are in the CPU
file only.

Per case: one call on a batch mixing good and bad rows; return code 0; the good rows bit-equal to the existing restatement
(tests/_line_store_ref.store_batch, tests/_fg_mask_ref, tests/_stretch_ref, numpy for the 8-bit pair and the unwarped rows of the warp
store) and to the same call with the bad rows made good; the bad rows exactly as include/hwg.h documents them:
  hwg_store_batch        row all -1 in out, all 0 in out_mask         hwg_store_line_stats   thr -1, 256 zeros
  hwg_store_warp_batch   row all -1, NaN in the map                   hwg_lines_from_u8      row all -1
  hwg_fg_masks           threshold -1, EVERY byte of out keeps its pre-fill - the region the bad entry names included
  hwg_stretch_onehot     the frame's region in both buffers is still NaN; identity = 1 with T_out != T is an ordinary frame
  hwg_lines_to_u8, hwg_augment_stats / _warp   what the clamped table gives, bit for bit, nothing outside it written
Also: hwg_fg_masks across the seams of its 1024-column chunks (widths 1020 .. 2052, H 64 and 5), and every HWG_REQUIRE of the entries that
only ops ever called, directly: HWG_ERR_ARG, outputs still poisoned, canaries intact.

Integers and bit-exact fp32 / fp64 throughout: no tolerance. Every case prints one line (entry, shape, bad rows / all rows, differing
elements), kept in profiles/table_guards.txt."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import table_cases as TC
from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fg_mask_ref as FG  # noqa: E402
import _line_store_ref as LS  # noqa: E402
import _stretch_ref as ST  # noqa: E402
from _guarded import Guarded, protocol, refused  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
M = TC.MARGIN


def _lib():
    from handwriting_line_generation_amd import _lib as L
    return L


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _bits(a):
    a = np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a)
    return a.reshape(-1).view(np.uint8)


def _diff(got, want):
    """elements whose bits differ"""
    got = got.numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.size == want.size and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    return int((_bits(got).reshape(got.size, -1) != _bits(want).reshape(want.size, -1)).any(axis=1).sum())


def _line(entry, shape, c, rows, differing):
    print("\nguard %-22s %-30s bad %d/%d  differing %d" % (entry, shape, len(c["bad"]), rows, differing))


def _pool_inputs(p, tables=None):
    off, w = (p.off_phys, p.w_phys) if tables is None else tables
    return dict(pixels=_t(p.slab), offsets=_t(np.array(off, dtype=np.int64)), widths=_t(np.array(w, dtype=np.int32)))


def _pool_ptrs(G):
    """the addresses the entry is handed: MARGIN bytes / one table entry into what the allocation holds"""
    return G.t("pixels")[M:], G.t("offsets")[1:], G.t("widths")[1:]


def _made_good(p):
    """the tables with every bad entry replaced by line 0's"""
    off = [p.off[0] if k in p.bad else o for k, o in enumerate(p.off)]
    w = [p.w[0] if k in p.bad else v for k, v in enumerate(p.w)]
    return [p.tail_off] + off + [p.tail_off] * 2, [TC.TAIL_W] + w + [TC.TAIL_W] * 2


# ---- hwg_fg_masks: bad entries, and the chunk seams ----------------------------------------------------------------------------------------------------
def _fg_run(cuda, c, tables=None):
    L, p, H = _lib(), c["pool"], c["H"]
    G = Guarded(cuda, _pool_inputs(p, tables), dict(out=torch.full((p.phys_bytes,), TC.MASK_POISON, dtype=U8), thr=((p.n_lines,), I32)))
    pix, off, wid = _pool_ptrs(G)
    out = G.t("out")[M:]
    return protocol(G, c["name"], lambda ws, n: L.query("hwg_fg_masks", pix, p.pixel_bytes, off, wid, p.n_lines, H, out, G.f["thr"], G.st))


@pytest.mark.parametrize("H", TC.MASK_HEIGHTS)
def test_fg_masks_bad_entries_touch_nothing(cuda, H):
    c = TC.fg_case(H)
    p = c["pool"]
    got = _fg_run(cuda, c)
    want_out, want_thr, _ = TC.model_pool_lines(c, FG)
    d = _diff(got["out"], want_out) + _diff(got["thr"], want_thr)
    _line("hwg_fg_masks", "H%d widths %s" % (H, p.w), c, p.n_lines, d)
    for k in c["bad"]:
        assert int(got["thr"][k]) == -1, "%s: threshold of the bad entry %d (%s)" % (c["name"], k, c["bad"][k]["why"])
    pre = np.full(p.phys_bytes, TC.MASK_POISON, dtype=np.uint8)
    for k in range(p.n_good):
        m, t = FG.fg_mask(p.lines[k])
        a = M + p.off[k]
        assert np.array_equal(got["out"].numpy()[a:a + m.size], m.reshape(-1)) and int(got["thr"][k]) == t, "%s: line %d" % (c["name"], k)
        pre[a:a + m.size] = got["out"].numpy()[a:a + m.size]
    assert np.array_equal(got["out"].numpy(), pre), "%s: a byte of out outside the good lines lost its pre-fill" % c["name"]
    assert d == 0
    good = _fg_run(cuda, c, _made_good(p))
    for k in range(p.n_good):
        a = M + p.off[k]
        assert np.array_equal(good["out"].numpy()[a:a + H * p.w[k]], got["out"].numpy()[a:a + H * p.w[k]]) and int(good["thr"][k]) == int(got["thr"][k])


@pytest.mark.parametrize("H", TC.SEAM_HEIGHTS)
def test_fg_masks_across_the_chunk_seams(cuda, H):
    c = TC.seam_case(H)
    p = c["pool"]
    got = _fg_run(cuda, c)
    want_out, want_thr, _ = TC.model_pool_lines(c, FG)
    per_line = [_diff(got["out"][M + o:M + o + l.size], FG.fg_mask(l)[0].reshape(-1)) for o, l in zip(p.off, p.lines)]
    d = _diff(got["out"], want_out) + _diff(got["thr"], want_thr)
    _line("hwg_fg_masks seam", "H%d widths %s" % (H, list(TC.SEAM_WIDTHS)), c, p.n_lines, d)
    assert per_line == [0] * len(per_line), "%s: differing mask bytes per line %s" % (c["name"], per_line)
    assert d == 0


# ---- hwg_store_line_stats ----------------------------------------------------------------------------------------------------------------------------------
def _stats_run(cuda, c, tables=None):
    L, p = _lib(), c["pool"]
    G = Guarded(cuda, _pool_inputs(p, tables), dict(thr=((p.n_lines,), I32), hist=((p.n_lines, 256), I32)))
    pix, off, wid = _pool_ptrs(G)
    return protocol(G, c["name"], lambda ws, n: L.query("hwg_store_line_stats", pix, p.pixel_bytes, off, wid, p.n_lines, c["H"], G.f["thr"], G.f["hist"], G.st))


@pytest.mark.parametrize("H", TC.HEIGHTS)
def test_store_line_stats_bad_entries_read_nothing(cuda, H):
    c = TC.stats_case(H)
    p = c["pool"]
    got = _stats_run(cuda, c)
    _, want_thr, want_hist = TC.model_pool_lines(c, FG, want_masks=False)
    d = _diff(got["thr"], want_thr) + _diff(got["hist"], want_hist)
    _line("hwg_store_line_stats", "H%d widths %s" % (H, p.w), c, p.n_lines, d)
    for k in c["bad"]:
        assert int(got["thr"][k]) == -1 and not got["hist"][k].any(), "%s: bad entry %d (%s)" % (c["name"], k, c["bad"][k]["why"])
    for k in range(p.n_good):
        assert int(got["thr"][k]) == FG.threshold(p.lines[k]) and np.array_equal(got["hist"][k].numpy(), np.bincount(p.lines[k].reshape(-1), minlength=256))
    assert d == 0
    good = _stats_run(cuda, c, _made_good(p))
    g = list(range(p.n_good))
    assert _diff(good["thr"][g], got["thr"][g].numpy()) == 0 and _diff(good["hist"][g], got["hist"][g].numpy()) == 0


# ---- hwg_store_batch ---------------------------------------------------------------------------------------------------------------------------------------
def _store_run(cuda, c, rows, mask_slab):
    L, p, H, W = _lib(), c["pool"], c["H"], c["W"]
    B = len(rows)
    words = (B * H * W + 3) // 4
    ins = _pool_inputs(p)
    ins.update(line=_t(np.array([r[0] for r in rows], dtype=np.int32)), out_w=_t(np.array([r[1] for r in rows], dtype=np.int32)),
               strech=_t(np.array([r[2] for r in rows], dtype=np.float64)), m=_t(np.array([r[3] for r in rows], dtype=np.float64)))
    outs = dict(out=((4 * words,), F32))
    if mask_slab is not None:
        ins["masks"] = _t(mask_slab)
        outs["out_mask"] = ((4 * words,), F32)
    G = Guarded(cuda, ins, outs)
    pix, off, wid = _pool_ptrs(G)
    msk = G.t("masks")[M:] if mask_slab is not None else None
    om = G.f["out_mask"] if mask_slab is not None else None
    f = G.f
    return protocol(G, c["name"], lambda ws, n: L.query("hwg_store_batch", pix, msk, p.pixel_bytes, off, wid, p.n_lines, f["line"], f["out_w"], f["strech"],
                                                          f["m"], B, H, W, f["out"], om, 4 * words, G.st))


@pytest.mark.parametrize("masks", (False, True), ids=("lines", "lines_masks"))
@pytest.mark.parametrize("which", TC.STORE_BATCHES)
@pytest.mark.parametrize("H", TC.HEIGHTS)
def test_store_batch_bad_rows_become_padding(cuda, H, which, masks):
    c = TC.store_case(H, which, masks)
    p, W, rows = c["pool"], c["W"], c["rows"]
    B, n = len(rows), len(rows) * H * W
    line_masks = [FG.fg_mask(l)[0] for l in p.lines]
    ms = p.mask_slab(lambda l: FG.fg_mask(l)[0]) if masks else None
    got = _store_run(cuda, c, rows, ms)
    want, want_m = TC.model_store_batch(c, LS, ms)
    out = got["out"].numpy()
    d = _diff(out[:n], want.reshape(-1)) + int((out[n:] != -1).sum())
    if masks:
        om = got["out_mask"].numpy()
        d += _diff(om[:n], want_m.reshape(-1)) + int((_bits(om[n:]) != 0).sum())
    _line("hwg_store_batch" + (" + masks" if masks else ""), "%s H%d W%d B%d" % (which, H, W, B), c, B, d)
    good = [b for b in range(B) if b not in c["bad"]]
    ref = LS.store_batch(p.lines, [rows[b] for b in good], W, line_masks if masks else None)
    out4 = out[:n].reshape(B, 1, H, W)
    assert _diff(out4[good], ref[0] if masks else ref) == 0, "%s: the good rows against tests/_line_store_ref.store_batch" % c["name"]
    for b in c["bad"]:
        assert (out4[b] == -1).all(), "%s: row %d (%s) is not padding" % (c["name"], b, c["bad"][b]["why"])
    if masks:
        om4 = om[:n].reshape(B, 1, H, W)
        assert _diff(om4[good], ref[1]) == 0
        for b in c["bad"]:
            assert not _bits(om4[b]).any(), "%s: mask row %d (%s) is not +0" % (c["name"], b, c["bad"][b]["why"])
    assert d == 0
    fixed = _store_run(cuda, c, [rows[0] if b in c["bad"] else r for b, r in enumerate(rows)], ms)
    assert _diff(fixed["out"].numpy()[:n].reshape(B, 1, H, W)[good], out4[good]) == 0
    if masks:
        assert _diff(fixed["out_mask"].numpy()[:n].reshape(B, 1, H, W)[good], om4[good]) == 0


# ---- hwg_store_warp_batch ------------------------------------------------------------------------------------------------------------------------------------
def _warp_run(cuda, c, rows):
    L, p, H, W = _lib(), c["pool"], c["H"], c["W"]
    B = len(rows)
    _, thr, hist = TC.model_pool_lines(c, FG, want_masks=False)
    ins = _pool_inputs(p)
    ins.update(thr=_t(np.concatenate([[0], thr, [0, 0]]).astype(np.int32)),
               hist=_t(np.concatenate([np.zeros((1, 256)), hist, np.zeros((2, 256))]).astype(np.int32)),
               line=_t(np.array([r[0] for r in rows], dtype=np.int32)),
               lines_i=_t(np.array([[r[1], 0, 0, r[2]] for r in rows], dtype=np.int32)),
               lines_f=torch.ones(B, 4), draws=torch.zeros(B, 2))
    G = Guarded(cuda, ins, dict(out=((B, 1, H, W), F32), map=((B, 2, H, W), F32)))
    pix, off, wid = _pool_ptrs(G)
    f = G.f
    thr_p, hist_p = G.t("thr")[1:], G.t("hist")[1:]
    return protocol(G, c["name"], lambda ws, n: L.query("hwg_store_warp_batch", pix, p.pixel_bytes, off, wid, p.n_lines, thr_p, hist_p, f["line"], f["lines_i"],
                                                          f["lines_f"], 4, f["draws"], 2, B, H, W, 0, 0, f["out"], f["map"], B * H * W, G.st), partly=("map",))


@pytest.mark.parametrize("H", TC.HEIGHTS)
def test_store_warp_batch_bad_rows_become_padding(cuda, H):
    c = TC.warp_case(H)
    p, W, rows = c["pool"], c["W"], c["rows"]
    B = len(rows)
    got = _warp_run(cuda, c, rows)
    want, want_map = TC.model_store_warp(c)
    d = _diff(got["out"], want) + _diff(got["map"], want_map)
    _line("hwg_store_warp_batch", "H%d W%d B%d unwarped" % (H, W, B), c, B, d)
    good = [b for b in range(B) if b not in c["bad"]]
    # numpy: 1 - byte / 128 at [x_off, x_off + w), -1 elsewhere - what tests/_line_store_warp_ref.collate states for H = 64 (that helper
    # is fixed to its module's H = 64 and cannot serve H = 7, so the two lines are restated here for both heights)
    for b in good:
        k, w, xo = rows[b]
        ref = np.full((H, W), -1.0, dtype=np.float32)
        ref[:, xo:xo + w] = np.float32(1.0) - p.lines[k].astype(np.float32) / np.float32(128.0)
        assert _diff(got["out"][b, 0], ref) == 0, "%s: good row %d" % (c["name"], b)
    for b in c["bad"]:
        assert (got["out"][b] == -1).all() and torch.isnan(got["map"][b]).all(), "%s: row %d (%s)" % (c["name"], b, c["bad"][b]["why"])
    assert d == 0
    fixed = _warp_run(cuda, c, [rows[0] if b in c["bad"] else r for b, r in enumerate(rows)])
    assert _diff(fixed["out"][good], got["out"][good].numpy()) == 0 and _diff(fixed["map"][good], got["map"][good].numpy()) == 0


# ---- hwg_lines_from_u8 -----------------------------------------------------------------------------------------------------------------------------------------
def _from_u8_run(cuda, c, select):
    L, p, H, W = _lib(), c["pool"], c["H"], c["W"]
    B = len(select)
    ins = _pool_inputs(p)
    ins["select"] = _t(np.array(select, dtype=np.int32))
    if c["real"] is not None:
        ins["real"] = _t(c["real"])
    G = Guarded(cuda, ins, dict(out=((B, 1, H, W), F32)))
    pix, off, wid = _pool_ptrs(G)
    f = G.f
    real = f["real"] if c["real"] is not None else None
    return protocol(G, c["name"], lambda ws, n: L.query("hwg_lines_from_u8", pix, p.pixel_bytes, off, wid, p.n_lines, f["select"], c["min_select"], real,
                                                          TC.BR, TC.WR, B, H, W, f["out"], G.st))


@pytest.mark.parametrize("real", (False, True), ids=("pool", "pool_real"))
@pytest.mark.parametrize("H", TC.HEIGHTS)
def test_lines_from_u8_bad_rows_become_padding(cuda, H, real):
    c = TC.from_u8_case(H, real)
    p, W, select = c["pool"], c["W"], c["select"]
    B = len(select)
    got = _from_u8_run(cuda, c, select)
    d = _diff(got["out"], TC.model_from_u8(c))
    _line("hwg_lines_from_u8" + (" + real" if real else ""), "H%d W%d B%d" % (H, W, B), c, B, d)
    good = [b for b in range(B) if b not in c["bad"]]
    for b in good:
        ref = np.full((H, W), -1.0, dtype=np.float32)
        if select[b] >= 0:
            l = p.lines[select[b]]
            ref[:, :l.shape[1]] = np.float32(1.0) - l.astype(np.float32) / np.float32(128.0)
        else:
            ref[:, :TC.WR] = c["real"][-1 - select[b], 0]
        assert _diff(got["out"][b, 0], ref) == 0, "%s: good row %d" % (c["name"], b)
    for b in c["bad"]:
        assert (got["out"][b] == -1).all(), "%s: row %d (%s) is not padding" % (c["name"], b, c["bad"][b]["why"])
    assert d == 0
    fixed = _from_u8_run(cuda, c, [select[0] if b in c["bad"] else s for b, s in enumerate(select)])
    assert _diff(fixed["out"][good], got["out"][good].numpy()) == 0


# ---- hwg_stretch_onehot ----------------------------------------------------------------------------------------------------------------------------------------
FRAME = np.dtype([("T_out", np.int32), ("r", np.float32), ("identity", np.int32), ("reserved", np.int32), ("off_blc", np.int64), ("off_lbc", np.int64)])


def _stretch_run(cuda, c, frames):
    L = _lib()
    table = np.zeros(len(frames), dtype=FRAME)
    for k in ("T_out", "r", "identity", "off_blc", "off_lbc"):
        table[k] = [f[k] for f in frames]
    G = Guarded(cuda, dict(label=_t(c["label"]), frames=_t(table.view(np.int64))), dict(blc=((c["phys"],), F32), lbc=((c["phys"],), F32)))
    f = G.f
    blc, lbc = f["blc"][TC.MARGIN_F:], f["lbc"][TC.MARGIN_F:]
    return protocol(G, c["name"], lambda ws, n: L.query("hwg_stretch_onehot", f["label"], TC.ST_T, TC.ST_B, TC.ST_NCLS, f["frames"], len(frames), TC.ST_MAX,
                                                          blc, c["elems"], lbc, c["elems"], G.st), partly=("blc", "lbc"))


def test_stretch_onehot_bad_frames_write_nothing(cuda):
    c = TC.stretch_case()
    frames = c["frames"]
    got = _stretch_run(cuda, c, frames)
    want_blc, want_lbc = TC.model_stretch(c, ST)
    d = _diff(got["blc"], want_blc) + _diff(got["lbc"], want_lbc)
    _line("hwg_stretch_onehot", "T%d B%d ncls%d F%d max_T_out %d" % (TC.ST_T, TC.ST_B, TC.ST_NCLS, len(frames), TC.ST_MAX), c, len(frames), d)
    blc, lbc = got["blc"].numpy()[TC.MARGIN_F:], got["lbc"].numpy()[TC.MARGIN_F:]
    good = [i for i in range(len(frames)) if i not in c["bad"]]
    for i in good:          # frame `identity_frame` among them: identity = 1 with T_out != T is an ordinary frame
        f = frames[i]
        ref = ST.stretch(c["label"][:TC.ST_T], TC.ST_NCLS, f["s"])
        assert _diff(lbc[f["off_lbc"]:f["off_lbc"] + f["n"]], ref.reshape(-1)) == 0, "frame %d, time major" % i
        assert _diff(blc[f["off_blc"]:f["off_blc"] + f["n"]], ref.transpose(1, 0, 2).reshape(-1)) == 0, "frame %d, NHWC rows" % i
    for i in c["bad"]:
        lo, hi = frames[i]["region"]
        assert np.isnan(blc[lo:hi]).all() and np.isnan(lbc[lo:hi]).all(), "frame %d (%s) wrote into a buffer" % (i, c["bad"][i]["why"])
    assert d == 0
    fixed = [dict(f, T_out=frames[1]["T_out"], r=frames[1]["r"], identity=0, off_blc=f["region"][0], off_lbc=f["region"][0]) if i in c["bad"] else f
             for i, f in enumerate(frames)]
    again = _stretch_run(cuda, c, fixed)
    for i in good:
        f = frames[i]
        for name, key in (("blc", "off_blc"), ("lbc", "off_lbc")):
            a = TC.MARGIN_F + f[key]
            assert _diff(again[name][a:a + f["n"]], got[name].numpy()[a:a + f["n"]]) == 0


# ---- the clamps: hwg_lines_to_u8, hwg_augment_stats / hwg_augment_warp -------------------------------------------------------------------------------------------
def _to_u8_run(cuda, c, widths):
    L, H, W = _lib(), c["H"], c["W"]
    size = M + c["out_bytes"] + TC.TAIL
    G = Guarded(cuda, dict(img=_t(c["img"]), widths=_t(np.array(widths, dtype=np.int32)), offsets=_t(np.array(c["offsets"], dtype=np.int64))),
                dict(out=torch.full((size,), TC.MASK_POISON, dtype=U8)))
    f = G.f
    out = G.t("out")[M:]
    return protocol(G, c["name"], lambda ws, n: L.query("hwg_lines_to_u8", f["img"], len(widths), H, W, f["widths"], f["offsets"], out, G.st))


@pytest.mark.parametrize("H", TC.HEIGHTS)
def test_lines_to_u8_clamps_a_bad_width(cuda, H):
    c = TC.to_u8_case(H)
    got = _to_u8_run(cuda, c, c["widths"])
    d = _diff(got["out"], TC.model_to_u8(c))
    _line("hwg_lines_to_u8", "H%d W%d widths %s" % (H, c["W"], c["widths"]), c, len(c["widths"]), d)
    clamped = _to_u8_run(cuda, c, [TC.clamp_width_u8(w, c["W"]) for w in c["widths"]])
    assert _diff(clamped["out"], got["out"].numpy()) == 0, "%s: not what the clamped table gives" % c["name"]
    assert d == 0


def _augment_run(cuda, c, table):
    L, H, W = _lib(), c["H"], c["W"]
    B = len(table)
    x = TC.augment_image(c)
    ins = dict(x=_t(x), lines_i=_t(np.array([[w, 0, 0, xo] for w, xo in table], dtype=np.int32)), lines_f=torch.ones(B, 4), draws=torch.zeros(B, 2))
    G = Guarded(cuda, ins, dict(stats=((B, 258), I32)))
    f = G.f
    stats = protocol(G, c["name"] + " stats", lambda ws, n: L.query("hwg_augment_stats", f["x"], f["lines_i"], f["lines_f"], 4, f["draws"], 2, B, H, W, f["stats"], G.st))["stats"]
    G2 = Guarded(cuda, dict(ins, stats=stats), dict(y=((B, 1, H, W), F32), map=((B, 2, H, W), F32)))
    h = G2.f
    got = protocol(G2, c["name"] + " warp", lambda ws, n: L.query("hwg_augment_warp", h["x"], h["lines_i"], h["lines_f"], 4, h["draws"], 2, h["stats"], B, H, W, 0, 0,
                                                                  h["y"], h["map"], G2.st), partly=("map",))
    return x, stats, got["y"], got["map"]


@pytest.mark.parametrize("H", TC.HEIGHTS)
def test_augment_entries_clamp_a_bad_width_or_x_off(cuda, H):
    c = TC.augment_clamp_case(H)
    W, B = c["W"], len(c["stated"])
    x, stats, y, mp = _augment_run(cuda, c, c["stated"])
    _, stats_c, y_c, mp_c = _augment_run(cuda, c, c["clamped"])
    d = _diff(stats, stats_c.numpy()) + _diff(y, y_c.numpy()) + _diff(mp, mp_c.numpy())
    # numpy: brightness off and no lattice - the LUT is the identity, y is x, the map is (y, x - x_off) on the line and NaN elsewhere
    want_map = np.full((B, 2, H, W), np.nan, dtype=np.float32)
    for b, (w, xo) in enumerate(c["clamped"]):
        want_map[b, 0, :, xo:xo + w] = np.arange(H, dtype=np.float32)[:, None]
        want_map[b, 1, :, xo:xo + w] = np.arange(w, dtype=np.float32)[None, :]
        assert int(stats[b, 0]) == (FG.threshold(c["lines"][b][:, :w]) if w > 0 else 0), "row %d: threshold" % b
    thr, border, want_y = TC.model_augment(c, FG)
    d += _diff(y, x) + _diff(y, want_y) + _diff(mp, want_map) + int((stats[:, 2:].numpy() != np.arange(256)).sum())
    d += _diff(stats[:, 0], thr) + _diff(stats[:, 1], border)
    _line("hwg_augment_stats/_warp", "H%d W%d (w, x_off) %s" % (H, W, c["stated"]), c, B, d)
    assert d == 0


# ---- every HWG_REQUIRE of the entries that only ops ever called ------------------------------------------------------------------------------------------------------
def _refuse_all(G, entry, order, base, cases):
    L = _lib()
    for why, change in cases:
        args = dict(base, **change)
        refused(G, "%s refusing %s" % (entry, why), lambda: L.query(entry, *([args[k] for k in order] + [G.st])))
    print("\nguard %-22s %d refusals: HWG_ERR_ARG, nothing written" % (entry, len(cases)))


def _addr(t, plus):
    return t.data_ptr() + plus


def _nulls(names):
    return [("no " + k, {k: None}) for k in names]


BIG = 2 ** 31 - 1


def test_host_refusals_of_the_pool_entries(cuda):
    G = Guarded(cuda, dict(pixels=torch.full((64,), 200, dtype=U8), masks=torch.zeros(64, dtype=U8), offsets=torch.zeros(4, dtype=I64),
                           widths=torch.full((4,), 4, dtype=I32), line=torch.zeros(4, dtype=I32), out_w=torch.full((4,), 4, dtype=I32),
                           strech=torch.ones(4, dtype=F64), m=torch.zeros(4, dtype=F64), thr_in=torch.zeros(4, dtype=I32), hist_in=torch.zeros(4 * 256, dtype=I32),
                           lines_i=torch.zeros(16, dtype=I32), lines_f=torch.ones(64), draws=torch.zeros(64)),
                dict(out_u8=((64,), U8), thr=((4,), I32), hist=((4 * 256,), I32), out=((64,), F32), out_mask=((64,), F32), map=((128,), F32)))
    f = G.f
    base = dict(pixels=f["pixels"], pb=64, offsets=f["offsets"], widths=f["widths"], B=2, H=4, out=f["out_u8"], thr=f["thr"])
    _refuse_all(G, "hwg_fg_masks", ["pixels", "pb", "offsets", "widths", "B", "H", "out", "thr"], base,
                _nulls(["pixels", "offsets", "widths", "out"]) + [("out = pixels", {"out": f["pixels"]}), ("B = 0", {"B": 0}), ("pixel_bytes = 0", {"pb": 0}),
                                                                   ("H = 0", {"H": 0}), ("H = 65", {"H": 65})])
    base = dict(pixels=f["pixels"], pb=64, offsets=f["offsets"], widths=f["widths"], n=2, H=4, thr=f["thr"], hist=f["hist"])
    _refuse_all(G, "hwg_store_line_stats", ["pixels", "pb", "offsets", "widths", "n", "H", "thr", "hist"], base,
                _nulls(["pixels", "offsets", "widths", "thr", "hist"]) + [("n_lines = 0", {"n": 0}), ("pixel_bytes = 0", {"pb": 0}), ("H = 0", {"H": 0}),
                                                                          ("offsets off by 4 bytes", {"offsets": _addr(f["offsets"], 4)})] +
                [("%s off by 2 bytes" % k, {k: _addr(f[k], 2)}) for k in ("widths", "thr", "hist")])
    order = ["pixels", "masks", "pb", "offsets", "widths", "n", "line", "out_w", "strech", "m", "B", "H", "W", "out", "out_mask", "elems"]
    base = dict(pixels=f["pixels"], masks=f["masks"], pb=64, offsets=f["offsets"], widths=f["widths"], n=2, line=f["line"], out_w=f["out_w"], strech=f["strech"],
                m=f["m"], B=2, H=4, W=4, out=f["out"], out_mask=f["out_mask"], elems=32)
    _refuse_all(G, "hwg_store_batch", order, base,
                _nulls(["pixels", "offsets", "widths", "line", "out_w", "strech", "m", "out"]) +
                [("masks without out_mask", {"out_mask": None}), ("out_mask without masks", {"masks": None}), ("B = 0", {"B": 0}), ("H = 0", {"H": 0}),
                 ("W = 0", {"W": 0}), ("n_lines = 0", {"n": 0}), ("pixel_bytes = 0", {"pb": 0}), ("out off by 4 bytes", {"out": _addr(f["out"], 4)}),
                 ("out_mask off by 4 bytes", {"out_mask": _addr(f["out_mask"], 4)})] +
                [("%s off by 4 bytes" % k, {k: _addr(f[k], 4)}) for k in ("offsets", "strech", "m")] +
                [("%s off by 2 bytes" % k, {k: _addr(f[k], 2)}) for k in ("widths", "line", "out_w")] +
                [("B*H*W beyond 64 bits", {"B": BIG, "H": BIG, "W": BIG}), ("out_elems one short", {"elems": 31}),
                 ("more elements than one launch covers", {"B": 2 ** 21, "H": 2 ** 10, "W": 2 ** 11, "elems": 2 ** 42})])
    order = ["pixels", "pb", "offsets", "widths", "n", "thr", "hist", "line", "lines_i", "lines_f", "lfs", "draws", "drs", "B", "H", "W", "GY", "GX", "out", "map", "elems"]
    base = dict(pixels=f["pixels"], pb=64, offsets=f["offsets"], widths=f["widths"], n=2, thr=f["thr_in"], hist=f["hist_in"], line=f["line"], lines_i=f["lines_i"],
                lines_f=f["lines_f"], lfs=8, draws=f["draws"], drs=10, B=2, H=4, W=4, GY=2, GX=2, out=f["out"], map=f["map"], elems=32)
    _refuse_all(G, "hwg_store_warp_batch", order, base,
                _nulls(["pixels", "offsets", "widths", "thr", "hist", "line", "lines_i", "lines_f", "draws", "out"]) +
                [("B = 0", {"B": 0}), ("H = 0", {"H": 0}), ("W = 0", {"W": 0}), ("n_lines = 0", {"n": 0}), ("pixel_bytes = 0", {"pb": 0}),
                 ("B = 65536", {"B": 65536, "elems": 65536 * 4 * 4}),          # (out_elems stated large enough: only `B <= 65535` refuses it)
                 ("GY = -1", {"GY": -1}), ("GX = -1", {"GX": -1}), ("GY = 17", {"GY": 17}), ("lf_stride 7 for a 2 x 2 lattice", {"lfs": 7}),
                 ("draw_stride 9 for a 2 x 2 lattice", {"drs": 9}), ("offsets off by 4 bytes", {"offsets": _addr(f["offsets"], 4)})] +
                [("%s off by 2 bytes" % k, {k: _addr(f[s], 2)}) for k, s in (("widths", "widths"), ("thr", "thr_in"), ("hist", "hist_in"), ("line", "line"),
                                                                             ("lines_i", "lines_i"), ("lines_f", "lines_f"), ("draws", "draws"), ("out", "out"), ("map", "map"))] +
                [("B*H*W beyond 64 bits", {"B": 65535, "H": BIG, "W": BIG}), ("out_elems one short", {"elems": 31})])


def test_host_refusals_of_stretch_and_augment(cuda):
    G = Guarded(cuda, dict(label=torch.zeros(16, dtype=I32), frames=torch.zeros(8, dtype=I64), x=torch.zeros(64), lines_i=torch.zeros(16, dtype=I32),
                           lines_f=torch.ones(64), draws=torch.zeros(64), stats_in=torch.zeros(2 * 258, dtype=I32)),
                dict(blc=((64,), F32), lbc=((64,), F32), stats=((2 * 258,), I32), y=((64,), F32), map=((128,), F32)))
    f = G.f
    order = ["label", "T", "B", "ncls", "frames", "F", "maxT", "blc", "be", "lbc", "le"]
    base = dict(label=f["label"], T=4, B=2, ncls=3, frames=f["frames"], F=2, maxT=4, blc=f["blc"], be=64, lbc=f["lbc"], le=64)
    _refuse_all(G, "hwg_stretch_onehot", order, base,
                _nulls(["label", "frames", "blc", "lbc"]) +
                [("T = 0", {"T": 0}), ("B = 0", {"B": 0}), ("ncls = 0", {"ncls": 0}), ("max_T_out = 0", {"maxT": 0}), ("F = 0", {"F": 0}), ("F = 65536", {"F": 65536}),
                 ("T * B = 2^32", {"T": 2 ** 22, "B": 2 ** 10}), ("T = 2^23", {"T": 2 ** 23, "B": 1}), ("a frame of 2^31 elements", {"B": 2 ** 10, "maxT": 2 ** 11, "ncls": 2 ** 10}),
                 ("blc_elems = 0", {"be": 0}), ("lbc_elems = 0", {"le": 0}), ("out_blc off by 4 bytes", {"blc": _addr(f["blc"], 4)}),
                 ("out_lbc off by 4 bytes", {"lbc": _addr(f["lbc"], 4)}), ("frames off by 4 bytes", {"frames": _addr(f["frames"], 4)}),
                 ("label off by 2 bytes", {"label": _addr(f["label"], 2)})])
    order = ["x", "lines_i", "lines_f", "lfs", "draws", "drs", "B", "H", "W", "stats"]
    base = dict(x=f["x"], lines_i=f["lines_i"], lines_f=f["lines_f"], lfs=4, draws=f["draws"], drs=2, B=2, H=4, W=8, stats=f["stats"])
    _refuse_all(G, "hwg_augment_stats", order, base,
                _nulls(["x", "lines_i", "lines_f", "draws", "stats"]) +
                [("B = 0", {"B": 0}), ("H = 0", {"H": 0}), ("W = 0", {"W": 0}), ("lf_stride = 3", {"lfs": 3}), ("draw_stride = 1", {"drs": 1}),
                 ("a line of more than 2^22 pixels", {"H": 2 ** 11 + 1, "W": 2 ** 11})])
    order = ["x", "lines_i", "lines_f", "lfs", "draws", "drs", "stats", "B", "H", "W", "GY", "GX", "y", "map"]
    base = dict(x=f["x"], lines_i=f["lines_i"], lines_f=f["lines_f"], lfs=8, draws=f["draws"], drs=10, stats=f["stats_in"], B=2, H=4, W=8, GY=2, GX=2, y=f["y"], map=f["map"])
    _refuse_all(G, "hwg_augment_warp", order, base,
                _nulls(["x", "lines_i", "lines_f", "draws", "stats", "y"]) +
                [("y = x", {"y": f["x"]}), ("B = 0", {"B": 0}), ("H = 0", {"H": 0}), ("W = 0", {"W": 0}), ("GY = -1", {"GY": -1}), ("GX = -1", {"GX": -1}),
                 ("GY = 17", {"GY": 17}), ("lf_stride 7 for a 2 x 2 lattice", {"lfs": 7}), ("draw_stride 9 for a 2 x 2 lattice", {"drs": 9}), ("B = 65536", {"B": 65536})])
