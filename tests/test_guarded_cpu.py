"""CPU: the guarded-buffer harness of tests/_guarded.py catches what it claims to catch. Guarded / protocol / refused run on CPU tensors with
fake "entries" - Python callables that write into the carved views as a kernel would. One well-behaved entry passes; every seeded
misbehaviour makes protocol() or refused() raise an AssertionError whose message names the condition. The two return codes the harness
compares against are held to the enum of include/hwg.h."""
import os
import re

import pytest
import torch

from _guarded import GUARD, HWG_ERR_ARG, HWG_ERR_WORKSPACE, Guarded, carve, protocol, refused

N, WS = 300, 128          # floats of x / y / z, floats of workspace
CPU = torch.device("cpu")


def _guarded():
    g = torch.Generator().manual_seed(5)
    return Guarded(CPU, dict(x=torch.randn(N, generator=g), k=torch.arange(6, dtype=torch.int64)),
                   dict(y=((N,), torch.float32), acc=torch.randn(N, generator=g), z=((3, 100), torch.float32)), 4 * WS)


def entry(G, flaw=None):
    """y = 2 x + 1 and acc += x, through a workspace it first fills itself; z is not its output. `flaw` seeds one misbehaviour."""
    f = G.f

    def call(ws, n):
        if flaw == "rc":
            return -2
        if ws is None or (n < 4 * WS and flaw != "short_ws_accepted"):
            return HWG_ERR_WORKSPACE
        if flaw != "reads_ws":
            ws.fill_(1.0)
        f["y"].copy_(f["x"] * 2 + ws[0])
        f["acc"].add_(f["x"])
        if flaw == "before":
            f["y"].as_strided((1,), (1,), f["y"].storage_offset() - 1).fill_(3.0)
        if flaw == "after":
            f["acc"].as_strided((1,), (1,), f["acc"].storage_offset() + N).fill_(3.0)
        if flaw == "input":
            f["x"][7] += 1.0
        if flaw == "not_mine":
            f["z"][5] = 0.0
        if flaw == "unwritten":
            f["y"][N - 1] = float("nan")
        return 0
    return call


def test_carve_keeps_a_guard_around_every_view():
    views, intact = carve(CPU, 5, 0, 130)
    base = views[0].storage_offset()
    assert base == GUARD and [v.numel() for v in views] == [5, 0, 130] and intact()
    assert all(b.storage_offset() - (a.storage_offset() + a.numel()) >= GUARD for a, b in zip(views, views[1:]))
    assert all(v.storage_offset() % 64 == 0 for v in views)
    for v in views:
        v.fill_(1.0)
    assert intact()


def test_a_well_behaved_entry_passes():
    G = _guarded()
    sent = G.get("x")
    acc0 = G.get("acc")
    out = protocol(G, "good", entry(G), mine=("y", "acc"))
    assert torch.equal(out["y"], sent * 2 + 1) and torch.equal(out["acc"], acc0 + sent) and set(out) == {"y", "acc"}
    assert G.as_reset(("z",)) == [] and G.intact() and G.untouched()


@pytest.mark.parametrize("flaw,message", [
    ("before", "a canary next to a buffer was overwritten"),
    ("after", "a canary next to a buffer was overwritten"),
    ("input", "an input changed"),
    ("not_mine", "wrote to a buffer it does not own"),
    ("unwritten", "1 elements of y are not finite (never written, or written from workspace contents)"),
    ("reads_ws", "are not finite (never written, or written from workspace contents)"),
    ("short_ws_accepted", "with one byte of workspace too few returned 0"),
])
def test_protocol_names_the_condition_a_flawed_entry_breaks(flaw, message):
    G = _guarded()
    with pytest.raises(AssertionError) as e:
        protocol(G, "flawed", entry(G, flaw), mine=("y", "acc"))
    assert message in str(e.value), str(e.value)


def test_protocol_reports_a_nonzero_return_code():
    """(the message carries hwg_last_error(): the library is resolved here, on first use)"""
    G = _guarded()
    with pytest.raises(AssertionError) as e:
        protocol(G, "flawed", entry(G, "rc"), mine=("y", "acc"))
    assert "flawed returned -2: " in str(e.value)


def test_protocol_notices_an_output_that_depends_on_finite_workspace_contents():
    """an entry that reads the workspace it was handed, with the first fill made finite: the zero-filled second call gives other bits"""
    G = _guarded()
    plain = entry(G, "reads_ws")
    calls = []

    def call(ws, n):
        if ws is not None and n == 4 * WS and not calls:
            ws.fill_(1.0)          # (stands for an earlier kernel's leftovers: finite, so that only the second call can tell)
        calls.append(n)
        return plain(ws, n)
    with pytest.raises(AssertionError) as e:
        protocol(G, "flawed", call, mine=("y", "acc"))
    assert "the second call (workspace zero-filled) gives other bits in ['y']" in str(e.value)


def test_refused_wants_the_code_and_nothing_written():
    G = _guarded()
    refused(G, "refusal", lambda: HWG_ERR_ARG)
    refused(G, "refusal", lambda: HWG_ERR_WORKSPACE, code=HWG_ERR_WORKSPACE)
    with pytest.raises(AssertionError) as e:
        refused(G, "accepted", lambda: 0)
    assert "accepted returned 0" in str(e.value)

    def writes_one():
        G.f["z"][299] = 1.0
        return HWG_ERR_ARG
    with pytest.raises(AssertionError) as e:
        refused(G, "refusal", writes_one)
    assert "refusal wrote to ['z']" in str(e.value)

    def writes_prefilled():
        G.f["acc"][0] += 1.0
        return HWG_ERR_ARG
    with pytest.raises(AssertionError) as e:
        refused(G, "refusal", writes_prefilled)
    assert "refusal wrote to ['acc']" in str(e.value)


def test_error_codes_are_those_of_the_header():
    from handwriting_line_generation_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    codes = {k: int(v) for k, v in re.findall(r"\b(HWG_ERR_\w+)\s*=\s*(-?\d+)", text)}
    assert codes["HWG_ERR_ARG"] == HWG_ERR_ARG and codes["HWG_ERR_WORKSPACE"] == HWG_ERR_WORKSPACE
    assert os.path.basename(_lib.HEADER_PATH) == "hwg.h" and "hwg_last_error" in _lib.parse_header()
