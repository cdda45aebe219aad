"""The convolution family's dispatch, checked without a GPU: with the launch seam faked, forward, autograd backward and Tape.backward_sets of
every test geometry run on CPU tensors and must issue exactly the C-ABI calls of tests/golden/conv_dispatch.json.xz - same entry points,
descriptors, scalars, tensor shapes, streams and scratch requests, in the same order (tools/gen_golden_conv_dispatch.py holds the recorder
and wrote the file)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_golden_conv_dispatch", os.path.join(ROOT, "tools", "gen_golden_conv_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv_dispatch_matches_the_recorded_call_lists(monkeypatch):
    from handwriting_line_generation_amd import _lib as L, ops
    G = _generator()
    with open(G.GOLDEN, "rb") as f:
        want = G.loads(f.read())
    names = [c[:2] for c in G.cases()]
    assert len(set(names)) == len(names), "case names must be unique"
    with monkeypatch.context() as m:
        got = G.record_all(ops, L, m.setattr)
    assert L.call.__module__ == L.__name__ and not ops._pack_cache and not ops._side_dirty and not ops._side_hold      # nothing stays patched
    assert sorted(got) == sorted(want)
    bad = []
    for key in want:
        a, b = got[key], want[key]
        if a != b:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            bad.append("%s: record %d\n   got  %s\n   want %s" % (key, i, a[i] if i < len(a) else "(end)", b[i] if i < len(b) else "(end)"))
    assert not bad, "%d of %d traces differ:\n%s" % (len(bad), len(want), "\n".join(bad[:12]))
    # every branch of the lowering is in the file
    seen = {r[0] for t in want.values() for r in t}
    assert {"hwg_conv_fwd", "hwg_wino_conv_fwd", "hwg_wino_s2_conv", "hwg_conv_pack_weight", "hwg_wino_pack_weight", "hwg_wino_s2_pack_weight",
            "hwg_conv_wgrad", "hwg_wino_wgrad", "hwg_conv_wgrad_sets", "hwg_wino_wgrad_sets", "hwg_col2im_taps", "hwg_pad2d_fwd", "hwg_pad_channels",
            "hwg_copy_channels", "hwg_colsum", "hwg_stream_fork", "hwg_wgrad_defer_next", "workspace", "defer_workspace", "side_workspace"} <= seen
