"""GPU: the LSTM kernels of csrc/lstm.hip - hwg_lstm_fwd (lstm_fwd_step_kernel<1 | 2 | 4 | 8 | 16>), hwg_lstm_bwd (lstm_bwd_step_kernel<...>) and
hwg_lstm_pack_whh - against the numpy fp64 reference tests/_lstm_ref.py, through L.query on the C ABI (never through ops, but for one test
at the end), at every template instance, every kind of partly filled k-slice and every batch tile (case table, the regimes each case covers,
the impulse inputs and the fp32 restatement of the summation order: oracle/lstm_cases.py; the restatement, the table and the sensitivity of
these checks to seeded flaws are checked on the CPU by tests/test_lstm_ref_cpu.py). The buffers and the protocol are those of
tests/_guarded.py (Dev wraps a Guarded without a workspace), the conditions those of tests/_lstm_checks.py.

Every call runs on buffers carved out of one allocation with 64-float canaries before, between and after every operand and every output; y,
gates, c, hseq, dgates, dc_ws, the packed W_hh and the non-training ping-pong are filled with NaN before the call. After the call: return code
0, canaries intact, every input bit-identical, every element the header says is written finite (hseq: all [2][T+1][B][H], the two zero rows
exactly +0), every output the call does not own still NaN, and a second call after re-poisoning gives the same bits.

Per step, at any T. Step t of a direction is recomputed in fp64 from the DEVICE's own h_{t-1} (the neighbouring row of y, which must equal the
hseq row bit for bit) and c_{t-1}, the backward step from the device's own dgates of the step before and its own dc f (dc_ws, while the slot
still holds it): a step's check is independent of every other step and no bound grows with T. u = 2^-24, nj = ceil(H/64); every bound is
multiplied by 1 + 2^-16 for the second-order terms.

  tensor               bound on |device - fp64|                                                                          measured on an MI355X (worst |err| / bound)
  gates[t]             L (n + 2) u A + e_act; n = 4 nj + 4 (the lane's chain of 4 nj fmaf, four butterfly sums), + 2 for      0.62 (H 516, B 63)
                       (xproj + b_hh) + sum; A = |xproj| + |b_hh| + sum_k |W_hh||h|; L = 1/4 (sigmoid) or 1 (tanh), the
                       activation's Lipschitz constant; e_act = 2 u: sigmoid and tanh within 2 ulp of the exact function
                       of their fp32 argument, values <= 1 (the figure of tests/test_lstm_gpu.py; 1 / (1 + expf(-x)) with
                       expf within 1 ulp and a correctly rounded sum and quotient stays within it). First step of a
                       direction: the sum is +0, the pre-activation ONE rounded sum: L u A + e_act.
  c[t]                 3 u (|f c_prev| + |i g|), from the device's gates[t] and c[t-1]: two products and a sum            0.64 (H 768, B 43)
  y[t]                 u |o| (2 + |tanh c| + 2 u), from the device's gates[t] and c[t]: tanhf within 2 ulp, one product   0.71 (H 1024, B 16)
  dgates[t], dc f      with E_dh = e_rec + u (|dy| + |dh_rec|), e_rec = (16 nj + 4) u sum |dgates[t+-1]||W_hh| (the four gate   0.60 (dgates; H 516, B 30), 0.49 (dc_ws; H 64, B 65)
                       blocks in one chain; 0 at the backward's first step, where dh = dy exactly),
                       E_s = 6 u for s = 1 - tanhf(c)^2 (2 u twice through the square, its rounding, the subtraction),
                       E_dc = E_dcn + |o| s E_dh + |dh o| E_s + 2 u |dh o s| + u |dc| (E_dcn = 0 where dc_ws still holds the
                       device's dc f of the step before, else that step's own bound on dc f):
                         i: |g i (1-i)| E_dc + 4 u |.|   (three products and the subtraction 1 - i)
                         f: |c_prev f (1-f)| E_dc + 4 u |.|
                         g: |i (1-g^2)| E_dc + u |dc i| + 2 u |.|   (1 - g g: a product and a subtraction, <= u in all)
                         o: |tanh(c) o (1-o)| E_dh + 2 u |dh o (1-o)| + 4 u |.|
                         dc f: |f| E_dc + u |.|
End to end, T = 6, one case per H, backward from the device's own forward: y and dgates against _lstm_ref with the project's second condition
alone - relative L2 error at most YARDSTICK_FACTOR times that of the fp32 restatement on the same case.               measured: y x0.94 (H 4), dgates x0.90 (every H) of the yardstick
(measured: worst over all cases; every case prints its own line, kept in profiles/lstm_fp64.txt.)"""
import numpy as np
import pytest
import torch

from oracle import lstm_cases as LC
from _fp64 import YARDSTICK_FACTOR
from _gpu_tidy import leave_nothing_behind  # noqa: F401  (module-scoped, autouse)
from _guarded import HWG_ERR_ARG, Guarded, protocol, refused
from _lstm_checks import (FWD_OUT, bits, check_backward_impulse, check_backward_steps, check_e2e, check_forward_impulse,
                          check_forward_steps)
from _lstm_layer import check_against_yardstick, ref_layer, run_layer, torch_layer

pytestmark = pytest.mark.gpu


# ---- one case on carved buffers ------------------------------------------------------------------------------------------------------------------
INPUTS = ("xp_f", "xp_r", "w_f", "w_r", "b_f", "b_r", "dy", "gates_in", "c_in")
EVAL_OUT, BWD_OUT = ("y", "pp"), ("dgates", "dc_ws")
OUTPUTS = ("y", "gates", "c", "hseq", "pp", "whh_t", "dgates", "dc_ws")


class Dev:
    """one case on a Guarded without a workspace (.G): the shapes and the argument marshalling of the three entries. gates_in / c_in are
    inputs; gates / c are outputs that bwd(own_forward=True) reads - the protocol holds them unchanged there, as outputs the call does not own"""

    def __init__(self, dev, x, state=None):
        T, B, G = x["xp"][0].shape
        H = G // 4
        self.T, self.B, self.H = T, B, H
        self.shape = dict(xp_f=(T, B, G), xp_r=(T, B, G), w_f=(G, H), w_r=(G, H), b_f=(G,), b_r=(G,), dy=(T, B, 2 * H), gates_in=(2, T, B, G), c_in=(2, T, B, H),
                          y=(T, B, 2 * H), gates=(2, T, B, G), c=(2, T, B, H), hseq=(2, T + 1, B, H), pp=(2, 2, B, H), whh_t=(2, H, G), dgates=(2, T, B, G),
                          dc_ws=(2, 2, B, H))
        gates_in, c_in = state if state is not None else (np.zeros(self.shape["gates_in"], np.float32), np.zeros(self.shape["c_in"], np.float32))
        ins = {k: torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(self.shape[k])
               for k, a in zip(INPUTS, (x["xp"][0], x["xp"][1], x["w"][0], x["w"][1], x["b"][0], x["b"][1], x["dy"], gates_in, c_in))}
        self.G = Guarded(dev, ins, {k: (self.shape[k], torch.float32) for k in OUTPUTS})
        self.v, self.L, self.st = self.G.f, self.G.L, self.G.st

    def run(self, tag, call, mine, partly=()):
        """`call` under the protocol -> {name: array} of the outputs it owns"""
        return {k: t.numpy() for k, t in protocol(self.G, tag, lambda ws, n: call(), mine=mine, partly=partly).items()}

    def get(self, k):
        return self.G.get(k).numpy()

    def fwd(self, training=1, **over):
        a = dict(xp_f=self.v["xp_f"], xp_r=self.v["xp_r"], w_f=self.v["w_f"], w_r=self.v["w_r"], b_f=self.v["b_f"], b_r=self.v["b_r"], y=self.v["y"],
                 gates=self.v["gates"] if training else None, c=self.v["c"] if training else self.v["pp"], hseq=self.v["hseq"] if training else None,
                 T=self.T, B=self.B, H=self.H)
        a.update(over)
        return self.L.query("hwg_lstm_fwd", a["xp_f"], a["xp_r"], a["w_f"], a["w_r"], a["b_f"], a["b_r"], a["y"], a["gates"], a["c"], a["hseq"], a["T"], a["B"], a["H"],
                            training, self.st)

    def bwd(self, own_forward=False, **over):
        a = dict(dy=self.v["dy"], gates=self.v["gates" if own_forward else "gates_in"], c=self.v["c" if own_forward else "c_in"], whh_t=self.v["whh_t"],
                 dgates=self.v["dgates"], dc_ws=self.v["dc_ws"], T=self.T, B=self.B, H=self.H)
        a.update(over)
        return self.L.query("hwg_lstm_bwd", a["dy"], a["gates"], a["c"], a["whh_t"], a["dgates"], a["dc_ws"], a["T"], a["B"], a["H"], self.st)

    def pack(self, **over):
        a = dict(w_f=self.v["w_f"], w_r=self.v["w_r"], H=self.H, whh_t=self.v["whh_t"])
        a.update(over)
        return self.L.query("hwg_lstm_pack_whh", a["w_f"], a["w_r"], a["H"], a["whh_t"], self.st)


def run_forward(D, tag, training=1):
    return D.run(tag + " hwg_lstm_fwd", lambda: D.fwd(training), FWD_OUT if training else EVAL_OUT)


def run_backward(D, tag, own_forward=False):
    """packs W_hh (checked exactly: whh_t[d][k][r] == w_d[r][k]) and runs hwg_lstm_bwd; at T = 1 only slot 0 of dc_ws is written"""
    wt = D.run(tag + " hwg_lstm_pack_whh", D.pack, ("whh_t",))["whh_t"]
    for d, k in enumerate(("w_f", "w_r")):
        assert (bits(wt[d]) == bits(D.get(k).T)).all(), "%s: the packed W_hh of direction %d is not the transpose" % (tag, d)
    out = D.run(tag + " hwg_lstm_bwd", lambda: D.bwd(own_forward), BWD_OUT, partly=("dc_ws",) if D.T == 1 else ())
    if D.T == 1:
        assert np.isfinite(out["dc_ws"][0]).all() and np.isnan(out["dc_ws"][1]).all(), "%s: at T = 1 exactly slot 0 of dc_ws is written" % tag
    return out


def _report(c, parts):
    H = c["H"]
    print("\nlstm_fp64 %-22s NJ %-2d nj %-2d chunk %-2d tiles %-10s %s" % (c["name"], LC.instance(H), LC.nj(H), LC.chunk(H),
                                                                       "+".join(str(nb) for _, nb in LC.tiles(H, c["B"])), "  ".join(parts)))


@pytest.mark.parametrize("c", LC.STEP_CASES, ids=[c["name"] for c in LC.STEP_CASES])
def test_every_step_against_fp64_from_the_devices_own_state(cuda, c):
    x = LC.inputs(c)
    state = LC.valid_state(x)
    D = Dev(cuda, x, state)
    fr, bad = check_forward_steps(x, run_forward(D, c["name"]))
    br = check_backward_steps(x["dy"], state[0], state[1], x["w"], run_backward(D, c["name"]))
    fr.update(br)
    _report(c, ["e/b %s %.3g" % (k, v) for k, v in fr.items()])
    bad += ["%s: |err| is %.3g x the derived bound" % (k, v) for k, v in fr.items() if not v <= 1.0]
    assert not bad, "%s: %s" % (c["name"], "; ".join(bad))


@pytest.mark.parametrize("c", LC.E2E_CASES, ids=[c["name"] for c in LC.E2E_CASES])
def test_six_steps_end_to_end_against_the_fp32_yardstick(cuda, c):
    x = LC.inputs(c)
    D = Dev(cuda, x)
    f = run_forward(D, c["name"])
    b = run_backward(D, c["name"], own_forward=True)
    ratios, line = check_e2e(c, f["y"], b["dgates"])
    _report(c, [line])
    assert all(v <= 1.0 for v in ratios.values()), "%s: relative L2 over %g x the fp32 yardstick: %s" % (c["name"], YARDSTICK_FACTOR, line)


@pytest.mark.parametrize("H", LC.IMPULSE_H)
def test_impulses(cuda, H):
    x, hot, col = LC.forward_impulse(H)
    D = Dev(cuda, x)
    out = run_forward(D, "impulse H%d" % H)
    bad = check_forward_impulse(H, hot, col, out)
    r, more = check_forward_steps(x, out)
    bad += more + ["%s: |err| is %.3g x the derived bound" % (k, v) for k, v in r.items() if not v <= 1.0]
    for rot in range(4):
        (dy, gates, cs, w), hot, blk = LC.backward_impulse(H, rot)
        xb = dict(xp=x["xp"], w=w, b=x["b"], dy=dy)
        D = Dev(cuda, xb, (gates, cs))
        bad += ["rot %d %s" % (rot, m) for m in check_backward_impulse(H, hot, blk, w, run_backward(D, "impulse H%d rot %d" % (H, rot)))]
    print("\nlstm_fp64 impulse H%d NJ %d: %d lines, %d mismatches" % (H, LC.instance(H), len(hot), len(bad)))
    assert not bad, "H %d: %s" % (H, "; ".join(bad))


# ---- exact properties at the batch tiles below 32 --------------------------------------------------------------------------------------------------
EXACT_H = (68, 768, 1024)


def _both(cuda, x, tag, training=1):
    """forward, then backward from the device's own forward: -> the outputs of both"""
    D = Dev(cuda, x)
    out = run_forward(D, tag, training)
    out.update(run_backward(D, tag, own_forward=True))
    return out


@pytest.mark.parametrize("H", EXACT_H)
def test_a_line_of_a_three_tile_batch_equals_the_line_run_alone(cuda, H):
    c = LC.chunk(H)
    B, T = 2 * c + 1, 3
    x = LC.make_case(T, B, H, seed=60 + H)
    full = _both(cuda, x, "rows H%d" % H)
    for row in sorted({0, 15, 16, c - 1, c, 2 * c}):
        one = dict(xp=[a[:, row:row + 1].copy() for a in x["xp"]], w=x["w"], b=x["b"], dy=x["dy"][:, row:row + 1].copy())
        alone = _both(cuda, one, "row %d alone H%d" % (row, H))
        for k in ("y", "gates", "c", "hseq", "dgates"):
            a, f = (alone[k], full[k][:, row:row + 1]) if k == "y" else (alone[k], full[k][:, :, row:row + 1])
            assert (bits(a) == bits(f)).all(), "H %d row %d: %s differs from the line run alone" % (H, row, k)


@pytest.mark.parametrize("H,T", [(68, 3), (768, 2), (1024, 3)])
def test_the_non_training_call_writes_y_and_the_ping_pong_only(cuda, H, T):
    B = 2 * LC.chunk(H) + 1
    x = LC.make_case(T, B, H, seed=70 + H)
    D = Dev(cuda, x)
    train = run_forward(D, "training H%d" % H)
    D.G.reset()
    ev = run_forward(D, "eval H%d" % H, training=0)          # (the protocol: every other output still NaN, canaries, inputs)
    assert (bits(ev["y"]) == bits(train["y"])).all()
    slot = (T - 1) & 1
    assert (bits(ev["pp"][slot, 0]) == bits(train["c"][0, T - 1])).all() and (bits(ev["pp"][slot, 1]) == bits(train["c"][1, 0])).all()


@pytest.mark.parametrize("H", EXACT_H)
def test_reverse_direction_equals_forward_on_the_flipped_sequence(cuda, H):
    B, T = LC.chunk(H) + 1, 3
    x = LC.make_case(T, B, H, seed=80 + H)
    a = _both(cuda, x, "flip a H%d" % H)
    f = dict(xp=[x["xp"][1][::-1].copy(), x["xp"][0][::-1].copy()], w=x["w"][::-1], b=x["b"][::-1],
             dy=np.concatenate([x["dy"][::-1, :, H:], x["dy"][::-1, :, :H]], axis=2).copy())
    b = _both(cuda, f, "flip b H%d" % H)
    assert (bits(a["y"][:, :, H:]) == bits(b["y"][::-1, :, :H])).all() and (bits(a["y"][:, :, :H]) == bits(b["y"][::-1, :, H:])).all()
    for k in ("gates", "c", "dgates"):
        assert (bits(a[k][1]) == bits(b[k][0][::-1])).all() and (bits(a[k][0]) == bits(b[k][1][::-1])).all(), k


@pytest.mark.parametrize("H", [4, 68, 132, 1024])
def test_pack_whh_is_the_exact_transpose(cuda, H):
    """68 and 132 are no multiples of the kernel's 32 x 32 tile; nothing is written outside [2][H][4H] (canaries) or to any other buffer"""
    x = LC.make_case(1, 1, H, seed=90 + H)
    D = Dev(cuda, x)
    wt = D.run("pack H%d" % H, D.pack, ("whh_t",))["whh_t"]
    for d in range(2):
        assert (bits(wt[d]) == bits(x["w"][d].T)).all(), d


# ---- refusals and queries ----------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_return_the_argument_error_and_write_nothing(cuda):
    x = LC.make_case(2, 3, 8, seed=1)
    D = Dev(cuda, x)
    v = D.v
    off = lambda k: v[k][1:]                                  # the same buffer, 4 bytes further on
    calls = [("fwd H 6", lambda: D.fwd(H=6)), ("fwd H 1028", lambda: D.fwd(H=1028)), ("fwd T 0", lambda: D.fwd(T=0)), ("fwd B 0", lambda: D.fwd(B=0)),
             ("fwd T B 4H = 2^31", lambda: D.fwd(T=1 << 19, B=1, H=1024)), ("fwd T B 4H > 2^31", lambda: D.fwd(T=3, B=1 << 20, H=512)),
             ("fwd training without gates", lambda: D.fwd(gates=None)), ("fwd training without hseq", lambda: D.fwd(hseq=None)),
             ("fwd y off by 4 bytes", lambda: D.fwd(y=off("y"))), ("fwd W_hh off by 4 bytes", lambda: D.fwd(w_f=off("w_f"))),
             ("fwd W_hh (reverse) off by 4 bytes", lambda: D.fwd(w_r=off("w_r"))),
             ("bwd H 6", lambda: D.bwd(H=6)), ("bwd H 1028", lambda: D.bwd(H=1028)), ("bwd T 0", lambda: D.bwd(T=0)), ("bwd B 0", lambda: D.bwd(B=0)),
             ("bwd T B 4H = 2^31", lambda: D.bwd(T=1 << 19, B=1, H=1024)),
             ("bwd dgates off by 4 bytes", lambda: D.bwd(dgates=off("dgates"))), ("bwd whh_t off by 4 bytes", lambda: D.bwd(whh_t=off("whh_t"))),
             ("pack H 0", lambda: D.pack(H=0)), ("pack H 1028", lambda: D.pack(H=1028)), ("pack without whh_t", lambda: D.pack(whh_t=None))]
    calls += [("fwd without %s" % k, (lambda k=k: D.fwd(**{k: None}))) for k in ("xp_f", "xp_r", "w_f", "w_r", "b_f", "b_r", "y", "c")]
    calls += [("bwd without %s" % k, (lambda k=k: D.bwd(**{k: None}))) for k in ("dy", "gates", "c", "whh_t", "dgates", "dc_ws")]
    calls += [("pack without %s" % k, (lambda k=k: D.pack(**{k: None}))) for k in ("w_f", "w_r")]
    for what, call in calls:
        refused(D.G, what, call, HWG_ERR_ARG)
    # (and the same buffers do serve an accepted call)
    assert D.fwd() == 0 and D.pack() == 0 and D.bwd(own_forward=True) == 0
    torch.cuda.synchronize()
    assert D.G.intact()


def test_limit_queries(cuda):
    from handwriting_line_generation_amd import _lib as L
    assert L.query("hwg_lstm_unit_slice") == LC.UNITS == 4
    want = {1: 32, 4: 32, 512: 32, 516: 31, 768: 21, 1024: 16, 1025: 0, 0: 0}
    assert {H: L.query("hwg_lstm_batch_tile", H) for H in want} == want
    assert all(LC.chunk(H) == want[H] for H in want if 1 <= H <= 1024)


# ---- through ops at the new tilings: dW_hh (the convolution weight-gradient path) and db_hh (colsum) at widths they have not seen ------------------
@pytest.mark.parametrize("H,B,T", [(768, 22, 3), (1024, 17, 2)])
def test_ops_lstm_layer_at_the_narrow_batch_tiles(cuda, H, B, T):
    c = LC.make_case(T, B, H, seed=H + 10 * B + 1000 * T)
    bad = check_against_yardstick("layer H%d B%d T%d" % (H, B, T), run_layer(c, cuda), ref_layer(c), torch_layer(c))
    assert not bad, bad
