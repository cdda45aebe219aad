"""Case tables for the in-kernel guards of the entries that read their geometry from device-resident tables (hwg_fg_masks, hwg_store_batch,
hwg_store_line_stats, hwg_store_warp_batch, hwg_lines_from_u8, hwg_stretch_onehot) and for the clamps of hwg_lines_to_u8 - the second line
of defence behind the host validation in ops, stated in include/hwg.h and written once in csrc/table_guard.h. Checked on the CPU by
tests/test_table_guards_cpu.py, run on the GPU at the C ABI by tests/test_table_guards_gpu.py.

PREDICATES, restated in Python's unbounded integers (no sum can wrap here):
  line_clauses(off, w, H, pixel_bytes)   the row-major H x w picture at byte off lies inside the pool
  block_clauses(off, n, elems)           the block of n >= 0 elements at element off lies inside the buffer, off a multiple of 4
A guard is the conjunction of its named clauses; `drop` names the one clause a seeded flaw leaves out.

SAFETY OF THE GPU FILE. A guard that is wrong must show as a wrong byte, never as a GPU fault. Every pool and buffer is therefore a SLAB that
physically holds more than the call states: MARGIN bytes (MARGIN_F floats) in front of the address the entry is handed, the stated
pixel_bytes / elems, then TAIL bytes (TAIL_F floats) behind them; the tables physically hold one entry in front of and two behind the
stated n_lines, and these surplus entries name a poison line INSIDE the stated pool - such an entry fails no clause but the index check in
front of it, so a kernel without that check shows the poison; the label and the real batch hold rows behind the stated T / Br. "Behind the
pool", a negative offset of a few bytes, line index -1 or n_lines therefore all name memory of the same allocation. What lies there is POISON: level 3 in a pixel pool (the lines hold
levels >= 10), 0x5A in a mask pool (masks hold 0 / 255), class POISON_CLASS in the surplus label rows, POISON_REAL in the surplus real row -
a kernel that reads through a bad entry shows it. Every bad row carries `touch`: the byte ranges (relative to the address the entry is
handed, per operand) a kernel would touch with that row's guard removed; footprints() checks them against the slab. Offsets of 2^62 and
above appear only in the CPU test of the predicates: nothing on a GPU may ever be pointed there.

A bad row is {"why": text, "clause": the one guard clause that fails for it, "touch": {operand: (first, behind)}, "inert": bool}. `inert`:
removing the clause changes no byte (the kernel's loops run zero times through such an entry: out_w = -1, T_out = 0): the row is still run
and must come out as documented, but no deletion of that clause can be seen in memory - said here rather than claimed.

The models (model_*) restate each entry in numpy ON THE SLAB, reading whatever bytes an entry names; with drop = a clause they are the
kernel with that clause deleted. Arithmetic comes from the tests' restatements (tests/_fg_mask_ref.py, tests/_line_store_ref.py,
tests/_stretch_ref.py), handed in by the caller. Test infrastructure, not product code."""
import math

import numpy as np

MARGIN, TAIL = 16, 320            # bytes of slab in front of / behind what a call states (16: the handed address keeps its alignment)
MARGIN_F, TAIL_F = 16, 16         # floats, for the stretch buffers
POISON, MASK_POISON = 3, 0x5A
POISON_CLASS, POISON_REAL = 4, 7.0
TAIL_W = 4                        # width of the all-poison "line" the surplus table entries name: it lies INSIDE the stated pool
INK, PAPER = 20, 230


# ---- the predicates ----------------------------------------------------------------------------------------------------------------------------------
def line_clauses(off, w, H, pixel_bytes):
    off, w, H, pixel_bytes = int(off), int(w), int(H), int(pixel_bytes)
    # (H is a launch parameter, not table data: every entry point refuses H < 1 on the host, so no row of a table can fail that clause)
    return {"H>=1": H >= 1, "w>=1": w >= 1, "off>=0": off >= 0, "end<=pixel_bytes": off + H * w <= pixel_bytes}


def line_in_pool(off, w, H, pixel_bytes, drop=None):
    return all(v for k, v in line_clauses(off, w, H, pixel_bytes).items() if k != drop)


def block_clauses(off, n, elems):
    off, n, elems = int(off), int(n), int(elems)
    # (n is a product of unsigned sizes in the one kernel that calls it: no frame of a table can fail that clause)
    return {"n>=0": n >= 0, "off>=0": off >= 0, "off%4==0": off % 4 == 0, "end<=elems": off + n <= elems}


def block_in_buffer(off, n, elems, drop=None):
    return all(v for k, v in block_clauses(off, n, elems).items() if k != drop)


def only_failing(clauses):
    """the name of the one clause that fails, None when none or several do"""
    bad = [k for k, v in clauses.items() if not v]
    return bad[0] if len(bad) == 1 else None


# the grid of the CPU test of the predicates (pb: the stated pool size)
def predicate_grid(pb):
    offs = [-2 ** 63, -1, 0, 1, pb - 1, pb, pb + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 62, 2 ** 63 - 4, 2 ** 63 - 1]
    return [(o, w, H, pb) for o in offs for w in (-4, 0, 1, 4, 2 ** 31 - 1) for H in (1, 64)] + [(0, 4, H, pb) for H in (0, -1, -2 ** 31)]


# ---- pools ---------------------------------------------------------------------------------------------------------------------------------------------
def text_line(rs, H, w):
    """light noisy paper (190 .. 255) with dark strokes (10 .. 109): no level below 10, so POISON is no level of a line"""
    img = rs.randint(190, 256, size=(H, w))
    for _ in range(max(w // 8, 1)):
        x, y = int(rs.randint(0, w)), int(rs.randint(0, H))
        img[y:y + int(rs.randint(1, 9)), x:x + int(rs.randint(1, 6))] = rs.randint(10, 110)
    return img.astype(np.uint8)


class Pool:
    """good lines at offsets that are multiples of `align` with poison between them, then the table entries of `bad` ((kind, w): "end+1" a
    line that ends `align` byte(s) behind pixel_bytes, "off-3" / "off+2" an offset of -3 / a good offset + 2, "w" width w at a good line's
    offset, "off=pb+1"). .off / .w: the stated tables (n_lines entries); .off_phys / .w_phys: what the buffers hold, one entry in front and
    two behind, all naming the poison line at .tail_off (inside the stated pool); .slab: the bytes, MARGIN in front of offset 0. masks: a second slab of the same
    layout (0 / 255 from `mask_of`, MASK_POISON elsewhere)."""

    def __init__(self, H, widths, seed, align=1, bad=(), lines=None):
        rs = np.random.RandomState(seed)
        self.H, self.align = H, align
        self.lines = [text_line(rs, H, w) for w in widths] if lines is None else lines
        self.off, pos = [], 0
        for k, l in enumerate(self.lines):
            pos += (1 + k % 3) if align == 1 else align
            pos = (pos + align - 1) // align * align
            self.off.append(pos)
            pos += l.size
        # the poison line the surplus table entries name: INSIDE the stated pool (an entry that fails no clause but the index check it sits
        # behind), at a multiple of 4, TAIL_W wide, every byte POISON
        self.tail_off = (pos + (1 if align == 1 else align) + 3) // 4 * 4
        pos = self.tail_off + H * TAIL_W
        self.pixel_bytes = pos + (2 if align == 1 else align)
        self.w = [l.shape[1] for l in self.lines]
        self.n_good = len(self.lines)
        self.bad = {}
        for kind, w in bad:
            if kind == "end+1":
                off = self.pixel_bytes - H * w + align
            elif kind == "off-3":
                off = -3
            elif kind == "off+2":
                off = self.off[0] + 2
            elif kind == "off=pb+1":
                off = self.pixel_bytes + 1
            else:
                assert kind == "w"
                off = self.off[0]
            self.bad[len(self.off)] = kind
            self.off.append(off)
            self.w.append(w)
        self.n_lines = len(self.off)
        assert self.tail_off % 4 == 0 and self.tail_off + H * TAIL_W <= self.pixel_bytes
        self.off_phys = [self.tail_off] + self.off + [self.tail_off] * 2
        self.w_phys = [TAIL_W] + self.w + [TAIL_W] * 2
        self.phys_bytes = (MARGIN + self.pixel_bytes + TAIL + 3) // 4 * 4
        self.slab = np.full(self.phys_bytes, POISON, dtype=np.uint8)
        for o, l in zip(self.off, self.lines):
            self.slab[MARGIN + o:MARGIN + o + l.size] = l.reshape(-1)

    def mask_slab(self, mask_of):
        s = np.full(self.phys_bytes, MASK_POISON, dtype=np.uint8)
        for o, l in zip(self.off, self.lines):
            s[MARGIN + o:MARGIN + o + l.size] = mask_of(l).reshape(-1)
        return s

    def entry(self, k):
        """(off, w) of table index k as a kernel without its index check finds it"""
        return self.off_phys[k + 1], self.w_phys[k + 1]

    def clauses(self, k):
        return line_clauses(self.off[k], self.w[k], self.H, self.pixel_bytes)

    def read(self, off, w, slab=None):
        slab = self.slab if slab is None else slab
        a = MARGIN + off
        assert 0 <= a and a + self.H * w <= slab.size, "a model read outside the slab"
        return slab[a:a + self.H * w].reshape(self.H, w)

    def touch(self, k):
        off, w = self.entry(k)
        return (off, off + self.H * max(w, 0))


def _bad(why, clause, touch, inert=False):
    return {"why": why, "clause": clause, "touch": touch, "inert": inert}


HEIGHTS = (7, 64)
MASK_HEIGHTS = (1, 7, 16, 64)
W_BATCH = 70          # width of the collated outputs: above the widest line, no multiple of 4


# ---- hwg_fg_masks, hwg_store_line_stats ----------------------------------------------------------------------------------------------------------------
def fg_case(H):
    p = Pool(H, [1, 5, 64, 65], 100 + H, bad=[("w", 0), ("w", -4), ("off-3", 5), ("end+1", 5)])
    rows = {4: _bad("w = 0", "w>=1", {}), 5: _bad("w = -4", "w>=1", {}),
            6: _bad("off = -3", "off>=0", {"pixels": p.touch(6), "out": p.touch(6)}),
            7: _bad("line ends 1 byte behind pixel_bytes", "end<=pixel_bytes", {"pixels": p.touch(7), "out": p.touch(7)})}
    return {"name": "fg_masks H%d" % H, "H": H, "pool": p, "bad": rows}


def stats_case(H):
    p = Pool(H, [3, 64, 65, 5], 200 + H, bad=[("w", 0), ("off-3", 4), ("off=pb+1", 1), ("end+1", 63)])
    rows = {4: _bad("w = 0", "w>=1", {}), 5: _bad("off = -3", "off>=0", {"pixels": p.touch(5)}),
            6: _bad("off = pixel_bytes + 1", "end<=pixel_bytes", {"pixels": p.touch(6)}),
            7: _bad("line ends 1 byte behind pixel_bytes", "end<=pixel_bytes", {"pixels": p.touch(7)})}
    return {"name": "store_line_stats H%d" % H, "H": H, "pool": p, "bad": rows}


def model_pool_lines(c, FG, drop=None, want_masks=True):
    """hwg_fg_masks / hwg_store_line_stats on the slab -> (out slab (pre-fill MASK_POISON), thr [n], hist [n, 256])"""
    p, H = c["pool"], c["H"]
    out = np.full(p.phys_bytes, MASK_POISON, dtype=np.uint8)
    thr, hist = np.full(p.n_lines, -1, dtype=np.int32), np.zeros((p.n_lines, 256), dtype=np.int32)
    for k in range(p.n_lines):
        off, w = p.off[k], p.w[k]
        if not line_in_pool(off, w, H, p.pixel_bytes, drop):
            continue
        if w < 1:                       # the loops over the line run zero times: an empty histogram, level 0
            thr[k] = 0
            continue
        line = p.read(off, w)
        hist[k] = np.bincount(line.reshape(-1), minlength=256)
        if want_masks:
            m, thr[k] = FG.fg_mask(line)
            out[MARGIN + off:MARGIN + off + H * w] = m.reshape(-1)
        else:
            thr[k] = FG.threshold(line)
    return out, thr, hist


# ---- hwg_fg_masks across the seams of its 1024-column chunks ------------------------------------------------------------------------------------------------
SEAM_WIDTHS = (1020, 1023, 1024, 1025, 1028, 1029, 2049, 2052)
SEAM_HEIGHTS = (64, 5)


def seam_line(H, w):
    """ink in columns 1019 .. 1029 and 2043 .. 2052 on rows 0 and H - 1, single pixels at x = 1020, 1023, 1024, 1027 on the middle row"""
    l = np.full((H, w), PAPER, dtype=np.uint8)
    for y in (0, H - 1):
        l[y, 1019:min(1030, w)] = INK
        l[y, 2043:min(2053, w)] = INK
    for x in (1020, 1023, 1024, 1027):
        if x < w:
            l[H // 2, x] = INK
    return l


def seam_case(H):
    p = Pool(H, None, 0, lines=[seam_line(H, w) for w in SEAM_WIDTHS])
    return {"name": "fg_masks seam H%d" % H, "H": H, "pool": p, "bad": {}}


# ---- hwg_store_batch -------------------------------------------------------------------------------------------------------------------------------------------
def _store_rows(p, which):
    """[(line, out_w, strech, m)], {row: bad}"""
    n, W, inf, nan = p.n_lines, W_BATCH, float("inf"), float("nan")
    g = [(0, 9, 1.3, 0.1), (1, W, 0.9, -0.2), (2, 64, 1.0, 0.0), (3, 61, 1.1, 0.3)]
    px = lambda k: {"pixels": p.touch(k), "masks": p.touch(k)}                      # noqa: E731
    if which == "lines":
        rows = [g[0], (-1, 8, 1.0, 0.0), g[1], (n, 8, 1.0, 0.0), (n + 1, 8, 1.0, 0.0), (4, 9, 1.0, 0.0), (5, 9, 1.0, 0.0), (6, 9, 1.0, 0.0)]
        bad = {1: _bad("line = -1", "line>=0", px(-1)), 3: _bad("line = n_lines", "line<n_lines", px(n)),
               4: _bad("line = n_lines + 1", "line<n_lines", px(n + 1)),
               5: _bad("line ends 1 byte behind pixel_bytes", "end<=pixel_bytes", px(4)), 6: _bad("off = -3", "off>=0", px(5)),
               7: _bad("w = 0", "w>=1", {})}
    elif which == "warp":
        rows = [g[2], (0, -1, 1.0, 0.0), (1, W + 1, 1.0, 0.0), (2, 40, 0.0, 0.1), (2, 40, -1.0, 0.1), (2, 40, inf, 0.1), (2, 40, nan, 0.1), g[3]]
        bad = {1: _bad("out_w = -1", "out_w>=0", {}, inert=True), 2: _bad("out_w = W + 1", "out_w<=W", px(1)),
               3: _bad("strech = 0", "strech>0", px(2)), 4: _bad("strech = -1", "strech>0", px(2)),
               5: _bad("strech = +inf", "strech finite", px(2)),
               # NaN fails `strech > 0` and `strech finite` at once: no deletion of ONE clause lets it through, in the kernel as here
               6: _bad("strech = NaN", None, px(2), inert=True)}
    else:
        rows = [g[1], (3, 50, 1.0, inf), (3, 50, 1.0, -inf), (3, 50, 1.0, nan), g[0]]
        bad = {1: _bad("m = +inf", "m finite", px(3)), 2: _bad("m = -inf", "m finite", px(3)), 3: _bad("m = NaN", "m finite", px(3))}
    return rows, bad


STORE_BATCHES = ("lines", "warp", "shear")


def store_case(H, which, masks):
    p = Pool(H, [5, 63, 64, 65], 300 + H, bad=[("end+1", 5), ("off-3", 5), ("w", 0)])
    rows, bad = _store_rows(p, which)
    return {"name": "store_batch %s%s H%d" % (which, " + masks" if masks else "", H), "H": H, "W": W_BATCH, "pool": p, "rows": rows, "bad": bad,
            "masks": masks}


def store_row_clauses(c, b):
    p = c["pool"]
    k, ow, s, m = c["rows"][b]
    cl = {"line>=0": k >= 0, "line<n_lines": k < p.n_lines}
    off, w = p.entry(k)          # (for an index outside the table: the surplus entry a kernel without its index check would find)
    cl.update(line_clauses(off, w, c["H"], p.pixel_bytes))
    cl.update({"out_w>=0": ow >= 0, "out_w<=W": ow <= c["W"], "strech>0": s > 0.0, "strech finite": abs(s) < math.inf, "m finite": abs(m) < math.inf})
    return cl


def model_store_batch(c, LS, mask_slab=None, drop=None):
    """-> (out [B,1,H,W] float32, out_mask or None). A row let through by a dropped clause is evaluated as the kernel would: the table entry
    it names (surplus entries included), out_w columns of the W there are; where the arithmetic is not finite (strech = 0, inf, NaN) the
    levels are numpy's, not necessarily the kernel's - no level at all gives the padding value -1, which is all the seeded flaws need."""
    p, H, W = c["pool"], c["H"], c["W"]
    B = len(c["rows"])
    out = np.full((B, 1, H, W), -1.0, dtype=np.float32)
    om = np.zeros((B, 1, H, W), dtype=np.float32) if mask_slab is not None else None
    for b, (k, ow, s, m) in enumerate(c["rows"]):
        if not all(v for n, v in store_row_clauses(c, b).items() if n != drop):
            continue
        off, w = p.entry(k)
        ow = min(ow, W)
        if ow <= 0:
            continue
        if w < 1:                       # every tap is the border: level 255, mask 0
            out[b, 0, :, :ow] = np.float32(1.0) - np.float32(255.0) / np.float32(128.0)
            continue
        with np.errstate(all="ignore"):
            out[b, 0, :, :ow] = LS.warp_line(p.read(off, w), ow, s, m)
            if om is not None:
                om[b, 0, :, :ow] = LS.warp_mask(p.read(off, w, mask_slab), ow, s, m)
    return out, om


# ---- hwg_store_warp_batch ----------------------------------------------------------------------------------------------------------------------------------------
def warp_case(H):
    """unwarped rows with the brightness off (lattice 0 x 0, scales 1, draws 0: the LUT is the identity): the guards sit in front of both paths,
    and this one has an exact restatement in two lines - 1 - byte / 128 at [x_off, x_off + w), the map (y, x - x_off), NaN / -1 elsewhere"""
    p = Pool(H, [5, 63, 64, 65], 400 + H, bad=[("end+1", 6)])
    n, W = p.n_lines, W_BATCH
    # (line, w stated in lines_i, x_off)
    rows = [(0, 5, 0), (-1, TAIL_W, 0), (n, TAIL_W, 0), (1, 64, 0), (2, 64, -1), (3, 65, W + 1 - 65), (4, 6, 0), (3, 65, 5)]
    px = lambda k: {"pixels": p.touch(k)}                      # noqa: E731
    bad = {1: _bad("line = -1", "line>=0", px(-1)), 2: _bad("line = n_lines", "line<n_lines", px(n)),
           3: _bad("lines_i[b][0] != widths[line]", "w==widths[line]", px(1)), 4: _bad("x_off = -1", "x_off>=0", px(2)),
           5: _bad("x_off + w = W + 1", "x_off+w<=W", px(3)), 6: _bad("line ends 1 byte behind pixel_bytes", "end<=pixel_bytes", px(4))}
    return {"name": "store_warp_batch H%d" % H, "H": H, "W": W, "pool": p, "rows": rows, "bad": bad}


def warp_row_clauses(c, b):
    p = c["pool"]
    k, wi, xo = c["rows"][b]
    cl = {"line>=0": k >= 0, "line<n_lines": k < p.n_lines}
    off, w = p.entry(k)          # (for an index outside the table: the surplus entry a kernel without its index check would find)
    cl.update(line_clauses(off, w, c["H"], p.pixel_bytes))
    cl.update({"w==widths[line]": wi == w, "x_off>=0": xo >= 0, "x_off+w<=W": xo + w <= c["W"]})
    return cl


def model_store_warp(c, drop=None):
    """-> (out [B,1,H,W], map [B,2,H,W]); a row let through shows the columns of its line that fall inside [0, W)"""
    p, H, W = c["pool"], c["H"], c["W"]
    B = len(c["rows"])
    out = np.full((B, 1, H, W), -1.0, dtype=np.float32)
    mp = np.full((B, 2, H, W), np.nan, dtype=np.float32)
    for b, (k, wi, xo) in enumerate(c["rows"]):
        if not all(v for n, v in warp_row_clauses(c, b).items() if n != drop):
            continue
        off, w = p.entry(k)
        line = p.read(off, w)
        for x in range(max(xo, 0), min(xo + w, W)):
            out[b, 0, :, x] = np.float32(1.0) - line[:, x - xo].astype(np.float32) / np.float32(128.0)
            mp[b, 0, :, x] = np.arange(H, dtype=np.float32)
            mp[b, 1, :, x] = np.float32(x - xo)
    return out, mp


# ---- hwg_lines_from_u8 ---------------------------------------------------------------------------------------------------------------------------------------------
W_U8 = 68
BR, WR = 2, 5


def from_u8_case(H, real):
    p = Pool(H, [64, 4, 64], 500 + H, align=4, bad=[("w", 6), ("w", W_U8 + 4), ("off+2", 4), ("end+1", 4)])
    n = p.n_lines
    px = lambda k, extra=0: {"pixels": (p.entry(k)[0], p.touch(k)[1] + extra)}                      # noqa: E731
    if not real:
        select = [0, n, 3, 4, 5, 6, 1, 2]
        bad = {1: _bad("k = n_lines", "k<n_lines", px(n)), 2: _bad("width 6", "w%4==0", px(3, 2)), 3: _bad("width W + 4", "w<=W", px(4)),
               4: _bad("offset 2 (mod 4)", "off%4==0", px(5)), 5: _bad("line ends behind pixel_bytes", "end<=pixel_bytes", px(6))}
    else:
        select = [0, -1, -1 - BR, -2, 1]
        bad = {2: _bad("r = Br", "r<Br", {"real": (BR * H * WR * 4, (BR + 1) * H * WR * 4)})}
    rs = np.random.RandomState(550 + H)
    realv = np.concatenate([rs.uniform(-1, 1, size=(BR, 1, H, WR)), np.full((1, 1, H, WR), POISON_REAL)]).astype(np.float32)
    return {"name": "lines_from_u8 %sH%d" % ("+ real " if real else "", H), "H": H, "W": W_U8, "pool": p, "select": select, "bad": bad,
            "real": realv if real else None, "min_select": -BR if real else 0}


def from_u8_row_clauses(c, b):
    p, s = c["pool"], c["select"][b]
    if s < 0:
        return {"r<Br": -1 - s < BR}
    cl = {"k<n_lines": s < p.n_lines}
    off, w = p.entry(s)          # (for k >= n_lines: the surplus entry a kernel without its index check would find)
    cl.update(line_clauses(off, w, c["H"], p.pixel_bytes))
    cl.update({"w<=W": w <= c["W"], "w%4==0": w % 4 == 0, "off%4==0": off % 4 == 0})
    return cl


def model_from_u8(c, drop=None):
    p, H, W = c["pool"], c["H"], c["W"]
    out = np.full((len(c["select"]), 1, H, W), -1.0, dtype=np.float32)
    for b, s in enumerate(c["select"]):
        if not all(v for n, v in from_u8_row_clauses(c, b).items() if n != drop):
            continue
        if s < 0:
            out[b, 0, :, :WR] = c["real"][-1 - s, 0]
            continue
        off, w = p.entry(s)
        for y in range(H):
            for col in range(0, min(w, W), 4):                      # one 32-bit word per lane, whatever the row stride is
                a = MARGIN + off + y * w + col
                out[b, 0, y, col:col + 4] = np.float32(1.0) - p.slab[a:a + 4].astype(np.float32) / np.float32(128.0)
    return out


# ---- hwg_stretch_onehot --------------------------------------------------------------------------------------------------------------------------------------------
ST_T, ST_B, ST_NCLS, ST_MAX = 9, 2, 5, 11
ST_SURPLUS = 4          # label rows behind T, class POISON_CLASS


def stretch_case():
    """frames (s, T_out, identity flag) laid out one behind the other in both buffers, every frame (the bad ones too) with a region of its
    own; the stated sizes are 1 (mod 4) so that the frame that ends 1 float behind lbc_elems still starts at a multiple of 4"""
    T, B, C = ST_T, ST_B, ST_NCLS
    rs = np.random.RandomState(77)
    label = np.concatenate([rs.randint(0, POISON_CLASS, size=(T, B)), np.full((ST_SURPLUS, B), POISON_CLASS)]).astype(np.int32)
    spec = [(1.0, None, None), (1.3, None, None), (1.3, 0, 0), (12.0 / 9.0 + 1e-9, None, None), (1.3, None, None), (1.3, None, None),
            (1.3, None, None), (1.3, None, 1), (0.8, None, None)]
    frames, pos = [], 0
    for s, t_forced, ident in spec:
        T_out = int(math.floor(float(T) * s)) if t_forced is None else t_forced
        n = B * T_out * C
        region = max((n + 3) // 4 * 4, 112)          # (room for a frame of max_T_out steps: the GPU test also runs the table with the bad frames made good)
        frames.append({"s": s, "T_out": T_out, "r": np.float32(1.0 / s), "identity": int(T_out == T) if ident is None else ident,
                       "off_blc": pos, "off_lbc": pos, "n": n, "region": (pos, pos + region)})
        pos += region
    elems = pos + 1
    n13 = frames[4]["n"]
    frames[4]["off_blc"] = frames[4]["off_blc"] + 2
    frames[5]["off_lbc"] = elems - n13 + 1
    frames[6]["off_blc"] = -4
    assert frames[3]["T_out"] == ST_MAX + 1 and frames[5]["off_lbc"] % 4 == 0 and frames[1]["T_out"] == ST_MAX
    both = lambda f: {k: (4 * f["off_" + k], 4 * (f["off_" + k] + f["n"])) for k in ("blc", "lbc")}                      # noqa: E731
    bad = {2: _bad("T_out = 0", "T_out>=1", {}, inert=True), 3: _bad("T_out = max_T_out + 1", "T_out<=max_T_out", both(frames[3])),
           4: _bad("off_blc = 2 (mod 4)", "blc off%4==0", both(frames[4])),
           5: _bad("off_lbc ends 1 float behind lbc_elems", "lbc end<=elems", both(frames[5])),
           6: _bad("off_blc = -4", "blc off>=0", both(frames[6]))}
    # frame 7 is not a bad frame: identity = 1 with T_out != T is an ordinary frame; with the `T_out == T` conjunct deleted it reads label rows >= T
    return {"name": "stretch_onehot", "label": label, "frames": frames, "bad": bad, "elems": elems, "phys": MARGIN_F + elems + TAIL_F + 3,
            "identity_frame": 7, "label_touch": (0, 4 * B * frames[7]["T_out"])}


def stretch_frame_clauses(c, i):
    f = c["frames"][i]
    cl = {"T_out>=1": f["T_out"] >= 1, "T_out<=max_T_out": f["T_out"] <= ST_MAX}
    for key in ("blc", "lbc"):
        cl.update({key + " " + k: v for k, v in block_clauses(f["off_" + key], f["n"], c["elems"]).items()})
    return cl


def model_stretch(c, ST, drop=None):
    """-> (blc slab, lbc slab) float32 with NaN where nothing is written; drop = "identity": the `T_out == T` conjunct of the identity flag"""
    T, B, C = ST_T, ST_B, ST_NCLS
    blc = np.full(c["phys"], np.nan, dtype=np.float32)
    lbc = np.full(c["phys"], np.nan, dtype=np.float32)
    for i, f in enumerate(c["frames"]):
        if not all(v for n, v in stretch_frame_clauses(c, i).items() if n != drop) or f["n"] == 0:
            continue
        if f["identity"] and (f["T_out"] == T or drop == "identity"):
            lab = c["label"][:f["T_out"]]
            v = (lab[:, :, None] == np.arange(C)).astype(np.float32)
        else:
            v = ST.stretch(c["label"][:T], C, f["s"])
        assert v.shape == (f["T_out"], B, C)
        a, b = MARGIN_F + f["off_lbc"], MARGIN_F + f["off_blc"]
        lbc[a:a + f["n"]] = v.reshape(-1)
        blc[b:b + f["n"]] = v.transpose(1, 0, 2).reshape(-1)
    return blc, lbc


# ---- hwg_lines_to_u8, hwg_augment_stats / hwg_augment_warp: widths and x_off are CLAMPED, the row is not refused ------------------------------------------------
W_CLAMP = 64


def clamp_width_u8(w, W):
    return min(w, W) & ~3


def clamp_augment(w, x_off, W):
    """-> (w, x_off) as augment.hip reads a lines_i entry"""
    x_off = max(x_off, 0)
    return max(min(w, W - x_off), 0), x_off


def to_u8_case(H):
    """widths W + 4, W + 1, 6, 0, -4 between two good rows; every row has a region of its own in `out`, sized for the UNCLAMPED width (a
    kernel without the clamp stays inside it) and rounded up to 4; the last row is good: a row of width W + 4 read without the clamp ends
    in the next image's first row"""
    W = W_CLAMP
    widths = [8, W + 4, W + 1, 6, 0, -4, W]
    rs = np.random.RandomState(600 + H)
    img = rs.uniform(-1, 1, size=(len(widths), 1, H, W)).astype(np.float32)
    offs, pos = [], 4
    for w in widths:
        offs.append(pos)
        pos += (H * max(w, 4) + 3) // 4 * 4 + 4
    bad = {}
    for b, why, clause in ((1, "w = W + 4", "w<=W"), (2, "w = W + 1", "w<=W and w%4==0"), (3, "w = 6", "w%4==0"), (4, "w = 0", None), (5, "w = -4", None)):
        w = widths[b]
        bad[b] = _bad(why, clause, {"img": (4 * b * H * W, 4 * (b * H * W + (H - 1) * W + max(w, 0) + 3)), "out": (offs[b], offs[b] + H * max(w, 0) + 4)},
                      inert=clause is None)
    return {"name": "lines_to_u8 H%d" % H, "H": H, "W": W, "img": img, "widths": widths, "offsets": offs, "out_bytes": pos, "bad": bad}


def model_to_u8(c, drop=None):
    """-> out slab (MARGIN in front, pre-fill MASK_POISON). drop: "w<=W" (no min) or "w%4==0" (no & ~3)"""
    H, W = c["H"], c["W"]
    out = np.full(MARGIN + c["out_bytes"] + TAIL, MASK_POISON, dtype=np.uint8)
    flat = c["img"].reshape(-1)
    for b, (w, off) in enumerate(zip(c["widths"], c["offsets"])):
        if drop != "w<=W":
            w = min(w, W)
        if drop != "w%4==0":
            w &= ~3
        for y in range(H):
            for col in range(0, min(w, W), 4):
                v = flat[(b * H + y) * W + col:(b * H + y) * W + col + 4]
                a = MARGIN + off + y * w + col
                out[a:a + 4] = ((np.float32(1.0) - v) * np.float32(127.5)).astype(np.uint8)
    return out


def augment_clamp_case(H):
    """(w, x_off) per row as stated -> what the clamp makes of it; images: levels at [x_off', x_off' + w'), -1 elsewhere. The first and the
    last row (w = 0: an image of padding) are what the clamp leaves alone: a row read without the clamp begins one float in front of its image (x_off = -1) or runs up to 5 floats past its
    last image row, and both stay inside x. The first column of every line is ink: the floats a row of width W + 1 or W + 4 would take
    from the start of the next image row move the border level by more than a rounding."""
    W = W_CLAMP
    stated = [(20, 3), (W + 4, 0), (W + 1, 0), (6, 0), (-4, 0), (30, -1), (W - 10 + 5, 10), (0, 0)]
    clamped = [clamp_augment(w, x, W) for w, x in stated]
    rs = np.random.RandomState(700 + H)
    lines = [text_line(rs, H, max(w, 1)) for w, _ in clamped]
    for l in lines:
        l[:, 0] = 10
    bad = {}
    for b, (w, xo) in enumerate(stated):
        if stated[b] != clamped[b]:
            first = b * H * W + min(xo, 0)
            behind = b * H * W + (H - 1) * W + xo + max(w, 0)
            # w <= 0: the loops run zero times and N <= 0 gives level 0, as for w' = 0
            bad[b] = _bad("w = %d, x_off = %d" % stated[b], "clamp", {"x": (4 * first, 4 * max(behind, first))}, inert=w <= 0)
    return {"name": "augment H%d" % H, "H": H, "W": W, "stated": stated, "clamped": clamped, "lines": lines, "bad": bad}


def augment_image(c):
    """x [B,1,H,W] float32: 1 - level / 128 at the clamped extents, -1 elsewhere"""
    H, W = c["H"], c["W"]
    x = np.full((len(c["stated"]), 1, H, W), -1.0, dtype=np.float32)
    for b, ((w, xo), l) in enumerate(zip(c["clamped"], c["lines"])):
        if w > 0:
            x[b, 0, :, xo:xo + w] = np.float32(1.0) - l[:, :w].astype(np.float32) / np.float32(128.0)
    return x


def model_augment(c, FG, clamp=True):
    """hwg_augment_stats + hwg_augment_warp with the brightness off and no lattice (the LUT is the identity) -> (thr [B], border level [B],
    y [B,1,H,W]); clamp = False: both entries without the clamp of (w, x_off), reading the floats of x the stated extent names"""
    H, W = c["H"], c["W"]
    x = augment_image(c)
    flat = x.reshape(-1)
    B = len(c["stated"])
    thr, border = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    y = np.full_like(x, -1.0)
    for b, (w, xo) in enumerate(c["clamped"] if clamp else c["stated"]):
        if w < 1:
            continue
        idx = (b * H + np.arange(H))[:, None] * W + xo + np.arange(w)[None, :]
        assert idx.min() >= 0 and idx.max() < flat.size, "a model read outside x"
        level = np.clip(np.rint((np.float32(1.0) - flat[idx]) * np.float32(128.0)), 0, 255).astype(np.uint8)         # padding (-1) counts as level 255
        thr[b] = FG.threshold(level)
        border[b] = min(max(int(np.rint(float(level.astype(np.int64).sum()) / float(H * w))), 0), 255)
        for X in range(max(xo, 0), min(xo + w, W)):          # column X of the batch shows x[b, :, X] itself
            y[b, 0, :, X] = np.float32(1.0) - level[:, X - xo].astype(np.float32) / np.float32(128.0)
    return thr, border, y


# ---- what the CPU test walks ----------------------------------------------------------------------------------------------------------------------------------------
def all_cases():
    cases = [fg_case(H) for H in MASK_HEIGHTS] + [stats_case(H) for H in HEIGHTS]
    cases += [store_case(H, which, masks) for H in HEIGHTS for which in STORE_BATCHES for masks in (False, True)]
    cases += [warp_case(H) for H in HEIGHTS] + [from_u8_case(H, real) for H in HEIGHTS for real in (False, True)]
    cases += [stretch_case()] + [to_u8_case(H) for H in HEIGHTS] + [augment_clamp_case(H) for H in HEIGHTS]
    return cases


def slab_ranges(c):
    """{operand: (first, behind)}: the bytes the GPU test's allocation physically holds per operand, relative to the address the entry is handed"""
    if "pool" in c:
        p = c["pool"]
        r = {k: (-MARGIN, p.phys_bytes - MARGIN) for k in ("pixels", "masks", "out")}
        if c.get("real") is not None:
            r["real"] = (0, c["real"].nbytes)
        return r
    if "frames" in c:
        return {k: (-4 * MARGIN_F, 4 * (c["phys"] - MARGIN_F)) for k in ("blc", "lbc")}
    if "img" in c:
        return {"img": (0, c["img"].nbytes), "out": (-MARGIN, c["out_bytes"] + TAIL)}
    return {"x": (0, 4 * len(c["stated"]) * c["H"] * c["W"])}


def footprints(c):
    """[(row, operand, touched, held)] for every bad row whose unguarded footprint leaves the slab (must be empty)"""
    held, out = slab_ranges(c), []
    for row, bad in c["bad"].items():
        for operand, (a, b) in bad["touch"].items():
            lo, hi = held[operand]
            if not (lo <= a and b <= hi):
                out.append((row, operand, (a, b), (lo, hi)))
    return out
