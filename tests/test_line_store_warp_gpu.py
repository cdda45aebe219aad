"""GPU: the warp mode of the device-resident line store - hwg_store_line_stats / hwg_store_warp_batch (csrc/store_warp.hip) and
StoreLoader(variant=...) - against the path it replaces: ops.augment_lines on the same lines collated and uploaded, and
DeviceAugment(ShardedLoader(...)). tests/_augment_ref.py ties that path to fp64 (tests/test_augment_gpu.py); the store's path shares its
source (csrc/augment_warp.h) and adds no arithmetic, so every comparison here is bit equality, padding included."""
import os
import pickle
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as R  # noqa: E402
import _line_store_warp_ref as S  # noqa: E402

H = S.H
W = 341                                         # no multiple of 4 or 64
ROWS = [6, 2, 0, 5, 3, 1, 4, 5]                 # pool lines in non-pool order, line 5 (130 px) twice
WARP = [True, True, True, False, True, True, True, True]          # row 3: warp off
BRIGHT = [True, False, True, True, True, True, True, True]        # row 1: brightness off


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def pool(cuda):
    lines = S.pool_lines()
    assert [l.shape[1] for l in lines] == list(S.POOL_WIDTHS)
    p = S.make_pool(lines, cuda)
    assert {int(o) % 4 for o in p.offsets} == {0, 1, 2, 3}         # arbitrary byte offsets (see make_pool: the widths alone give none at H = 64)
    return lines, p


def _forced(lines, rows=ROWS, warp=WARP, bright=BRIGHT, centred=False, seed=77):
    """-> (mesh, fg_bg, x_off): explicit draws for the rows; the same draw for a row wherever it stands (keyed by its position in ROWS)"""
    from handwriting_line_generation_amd import ops
    widths = [lines[k].shape[1] for k in rows]
    x_off = [(W - w) // 2 if centred else 0 for w in widths]
    fg_bg, disp = [], []
    for b, w in enumerate(widths):
        rs = np.random.RandomState(seed + b)
        fg_bg.append(rs.normal(0, 30, size=2))
        d = S.draws(rs, w)
        disp.append(d if warp[b] else None)
    mesh = ops.LineMesh(H, widths, x_off=x_off, warp=warp, bright=bright, disp=disp)
    return mesh, np.asarray(fg_bg), x_off


def _both(cuda, lines, pool, rows, mesh, fg_bg, x_off, width=W):
    from handwriting_line_generation_amd import ops
    old = ops.augment_lines(S.collate([lines[k] for k in rows], width, x_off).to(cuda), mesh, fg_bg=fg_bg, want_map=True)
    new = ops.store_warp_batch(pool, rows, mesh, width, fg_bg=fg_bg, want_map=True)
    torch.cuda.synchronize()
    return old, new


def test_statistics_once_per_pool(cuda, pool):
    from handwriting_line_generation_amd import ops
    lines, p = pool
    thr, hist = ops.store_line_stats(p)
    assert ops.store_line_stats(p)[0] is thr                    # computed once, kept with the pool
    assert thr.dtype == torch.int32 and hist.dtype == torch.int32 and tuple(thr.shape) == (len(lines),) and tuple(hist.shape) == (len(lines), 256)
    thr, hist = thr.cpu().numpy(), hist.cpu().numpy()
    for k, l in enumerate(lines):
        want = np.bincount(l.reshape(-1), minlength=256)
        margin = R.split_margin(want)
        assert margin > 1e-9, (k, margin)                       # fp64 summation order cannot decide the threshold
        assert int(thr[k]) == R.stats(l, 0.0, 0.0)[0] and np.array_equal(hist[k], want), (k, int(thr[k]), R.stats(l, 0.0, 0.0)[0])


@pytest.mark.parametrize("centred", [False, True])
def test_teacher_forced_batch_equals_augment_lines_bit_for_bit(cuda, pool, centred):
    lines, p = pool
    mesh, fg_bg, x_off = _forced(lines, centred=centred)
    assert mesh.src[3] is None and mesh.src[2] is None and mesh.src[0] is not None            # warp off; 5 px: never warped
    if centred:
        assert any(o % 2 for o in x_off) and all(o > 0 for o in x_off)
    (y, mp, st), (y2, mp2) = _both(cuda, lines, p, ROWS, mesh, fg_bg, x_off)
    assert y2.shape == y.shape == (len(ROWS), 1, H, W) and mp2.shape == mp.shape
    assert torch.equal(_bits(y), _bits(y2))                       # every element, padding included
    assert torch.equal(_bits(mp), _bits(mp2))                     # NaN patterns too
    y, st = y.cpu().numpy(), st.cpu().numpy()
    x = S.collate([lines[k] for k in ROWS], W, x_off).numpy()
    for b, k in enumerate(ROWS):
        w, o = lines[k].shape[1], x_off[b]
        assert (y[b, 0, :, :o] == -1).all() and (y[b, 0, :, o + w:] == -1).all() and (y[b, 0, :, o:o + w] != -1).all()
        t, lut, m = R.stats(lines[k], *(fg_bg[b] if BRIGHT[b] else (0.0, 0.0)))
        assert int(st[b, 0]) == t and int(st[b, 1]) == m and np.array_equal(st[b, 2:], lut)       # what the old path's statistics launch found
        if not WARP[b] or w <= 5:                                 # the LUT alone, as observable through the output
            assert np.array_equal((1.0 - y[b, 0, :, o:o + w].astype(np.float64)) * 128.0, lut[lines[k]].astype(np.float64))
    assert not np.array_equal(y[0], x[0]) and not np.array_equal(y[1], x[1])      # re-lit and warped; warped only
    assert np.array_equal(st[1, 2:], np.arange(256))              # brightness off: the identity LUT


def test_golden_case_w150(cuda):
    from handwriting_line_generation_amd import ops
    g = np.load(os.path.join(ROOT, "tests", "golden", "warp_maps.npz"))
    img, src, dst = g["w150/image"].astype(np.int64), g["w150/source"], g["w150/destination"]
    gy, gx = (int(v) for v in g["w150/grid"])
    d = (dst - src).reshape(gy, gx, 2)
    mesh = ops.LineMesh(H, [img.shape[1]], disp=[(d[:, :, 0], d[:, :, 1])])
    fg_bg = np.array([[17.25, -23.5]])
    p = S.make_pool([img], cuda)
    (y, mp, _), (y2, mp2) = _both(cuda, [img], p, [0], mesh, fg_bg, None, width=img.shape[1])
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(mp), _bits(mp2))
    assert bool(torch.isfinite(mp2).any()) and not torch.equal(y2.cpu(), S.collate([img], img.shape[1]))


def test_device_draws(cuda, pool):
    from handwriting_line_generation_amd import ops
    lines, p = pool
    widths = [lines[k].shape[1] for k in ROWS]
    x_off = [(W - w) // 2 for w in widths]
    x = S.collate([lines[k] for k in ROWS], W, x_off).to(cuda)
    mesh = ops.LineMesh(H, widths, sigma=0.7, x_off=x_off, warp=WARP, bright=BRIGHT)

    def draw(seed, offset, new):
        g = ops.DeviceRNG(seed)
        g.offset = offset
        out = ops.store_warp_batch(p, ROWS, mesh, W, rng=g) if new else ops.augment_lines(x, mesh, rng=g)
        assert g.offset == offset + (len(ROWS) * (2 + 2 * mesh.GY * mesh.GX) + 3) // 4
        return out, g.offset
    (a, oa), (b, ob), (c, _) = draw(1000003 * 7, 40, False), draw(1000003 * 7, 40, True), draw(1000003 * 7, 41, True)
    torch.cuda.synchronize()
    assert oa == ob and torch.equal(_bits(a), _bits(b)) and not torch.equal(b, c)
    assert not torch.equal(b, x)


def test_batch_independence_and_determinism(cuda, pool):
    from handwriting_line_generation_amd import ops
    lines, p = pool
    mesh, fg_bg, x_off = _forced(lines, centred=True)
    y = ops.store_warp_batch(p, ROWS, mesh, W, fg_bg=fg_bg)
    again = ops.store_warp_batch(p, ROWS, mesh, W, fg_bg=fg_bg)
    perm = [5, 0, 7, 2, 4, 1, 3, 6]
    pmesh = ops.LineMesh(H, [mesh.widths[i] for i in perm], x_off=[x_off[i] for i in perm], warp=[WARP[i] for i in perm],
                         bright=[BRIGHT[i] for i in perm], disp=[mesh.disp[i] for i in perm])
    py = ops.store_warp_batch(p, [ROWS[i] for i in perm], pmesh, W, fg_bg=fg_bg[perm])
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(again))
    assert torch.equal(_bits(py), _bits(y[perm]))
    # into a caller's buffer that held something else: every element is written
    buf = torch.full((len(ROWS) * H * W + 5,), 7.0, device=cuda)
    into = ops.store_warp_batch(p, ROWS, mesh, W, fg_bg=fg_bg, out=buf)
    torch.cuda.synchronize()
    assert into.data_ptr() == buf.data_ptr() and torch.equal(_bits(into), _bits(y)) and bool((buf[-5:] == 7.0).all())


def test_bad_tables_are_refused_on_the_host(cuda, pool):
    from handwriting_line_generation_amd import _lib as L, ops
    lines, p = pool
    mesh, fg_bg, x_off = _forced(lines)
    for kw, word in [(dict(lines=[7] + ROWS[1:]), "line indices"), (dict(lines=ROWS[:-1]), "rows"), (dict(lines=[0] + ROWS[1:]), "widths"),
                     (dict(W=332), "outside the batch width"), (dict(fg_bg=None), "go together"), (dict(fg_bg=fg_bg[:-1]), "finite pairs"),
                     (dict(out=torch.empty(10, device=cuda)), "out must be")]:
        args = dict(lines=ROWS, W=W, fg_bg=fg_bg)
        args.update(kw)
        with pytest.raises(L.HwgError) as e:
            ops.store_warp_batch(p, args["lines"], mesh, args["W"], fg_bg=args["fg_bg"], out=args.get("out"))
        assert word in str(e.value), (kw, str(e.value))


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    d = tmp_path_factory.mktemp("warp_store_dirs")
    out = {}
    for which in ("iam", "rimes"):
        out[which] = str(d / which)
        S.fabricate(which, out[which])
    return out


LOADER_CASES = {"hw_true": ("iam", dict()), "hw_low_warp": ("iam", dict(augmentation="low warp")), "hw_center": ("iam", dict(center_pad=True)),
                "rimes_warp": ("rimes", dict())}


def _seed(mode):
    from handwriting_line_generation_amd import rng
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    rng.set_mode(mode, seed=3)


def _after():
    from handwriting_line_generation_amd import rng
    return (random.random(), float(np.random.random()), float(torch.rand(())), rng.device_rng().offset if rng.mode() == "device" else None)


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("case", sorted(LOADER_CASES))
def test_store_loader_epoch_equals_device_augment_over_sharded_loader(cuda, dirs, tmp_path, case, mode):
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.device_augment import DeviceAugment
    from handwriting_line_generation_amd.data.line_store import StoreLoader
    which, keys = LOADER_CASES[case]
    try:
        cfg = S.hwr_config(which, dirs[which], tmp_path, **keys)
        if case == "hw_true":
            assert cfg["data_loader"]["augmentation"] is True and cfg["data_loader"]["data_set_name"] == "HWDataset"      # as shipped
        if case == "rimes_warp":
            assert cfg["data_loader"]["augmentation"] == "warp" and cfg["data_loader"]["data_set_name"] == "AuthorRIMESLinesDataset"
        _seed(mode)
        old, _ = D.getDataLoader(cfg, "train")
        want = [dict(inst, image=inst["image"].cpu()) for inst in old]
        after_old = _after()
        cfg["data_loader"]["device_store"] = "warp"
        _seed(mode)
        new, vnew = D.getDataLoader(cfg, "train")
        assert isinstance(old, DeviceAugment) and isinstance(new, StoreLoader) and isinstance(vnew, StoreLoader)      # validation inherits the key
        assert new.variant == old.variant == ("low" if case == "hw_low_warp" else "full") and new.dataset.augmentation is None
        got = [dict(inst, image=inst["image"].cpu()) for inst in new]
        after_new = _after()
        assert len(got) == len(want) == len(old) == len(new) >= 2
        for g, w in zip(got, want):
            assert g["image"].dtype == torch.float32 and g["image"].shape == w["image"].shape
            assert torch.equal(_bits(g["image"]), _bits(w["image"]))
            for key in ("label", "label_lengths"):
                assert g[key].dtype == w[key].dtype and torch.equal(g[key], w[key]), key
            for key in ("gt", "name", "author"):
                assert g[key] == w[key], key
            assert set(g) - set(w) == {"line_extents"} and set(w) <= set(g)
        assert after_new == after_old                           # every generator stands where the old path leaves it
        if case == "hw_center":
            assert any(o > 0 for g in got for o in g["line_extents"][0])
    finally:
        rng.set_mode("device")


def _train(cfg, cls, n):
    from handwriting_line_generation_amd import model as M, rng
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.model import loss as loss_fns
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    rng.set_mode("device", seed=3)
    loader, vloader = D.getDataLoader(cfg, "train")
    model = M.HWWithStyle(cfg["model"])
    losses = {k: getattr(loss_fns, v) for k, v in cfg["loss"].items()}
    trainer = cls(model, losses, [], None, cfg, loader, vloader, None)
    logs = [trainer._train_iteration(it) for it in range(n)]
    torch.cuda.synchronize()
    return trainer, loader, logs, {k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items()}


def test_trainer_with_the_store_equals_the_trainer_without_it(cuda, dirs, tmp_path):
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.data.line_store import StoreLoader
    from handwriting_line_generation_amd.trainer import HWWithStyleTrainer
    try:
        cfg = S.hwr_config("iam", dirs["iam"], tmp_path)
        _, _, want_logs, want = _train(cfg, HWWithStyleTrainer, 3)
        cfg = S.hwr_config("iam", dirs["iam"], tmp_path, device_store="warp", device_store_cache=str(tmp_path / "pool"))
        _, loader, got_logs, got = _train(cfg, HWWithStyleTrainer, 3)
        assert isinstance(loader, StoreLoader) and os.listdir(str(tmp_path / "pool"))
        assert len(got_logs) == 3 and all(np.isfinite(v) for log in got_logs for v in log.values()) and "recogLoss" in got_logs[0]
        assert got_logs == want_logs, (got_logs, want_logs)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    finally:
        rng.set_mode("device")


def test_synth_trainer_runs_behind_the_store(cuda, dirs, tmp_path):
    """HWRWithSynthTrainer with the store on: the real rows arrive augmented from the store and pass the mixed batch's augmentation unchanged"""
    from _reference_checkpoint import unpack

    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.logger import load_checkpoint
    from handwriting_line_generation_amd.trainer import HWRWithSynthTrainer
    try:
        ck = load_checkpoint(unpack("gan", tmp_path))
        ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
        ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
        gen = str(tmp_path / "spread.pth")
        torch.save(ck, gen)
        styles = str(tmp_path / "train_styles_")
        with open(styles + "25000.pkl", "wb") as f:
            pickle.dump({"authors": ["000", "000", "017"], "styles": torch.randn(3, 128, generator=torch.Generator().manual_seed(1)).numpy()}, f)
        text = str(tmp_path / "text.txt")
        open(text, "w").write("the quick brown fox\njumps over\na line of text\nhello world\nshort\n")
        cfg = S.hwr_config("synth", dirs["iam"], tmp_path, device_store="warp")
        cfg["data_loader"]["batch_size"] = cfg["validation"]["batch_size"] = 2
        cfg["trainer"]["synth"] = dict(checkpoint=gen, styles=styles, text_data=text, per_batch=2, pool=4, gen_batch=3, seed=11, max_len=8, max_width=None,
                                       spacing_noise=False)
        assert cfg["data_loader"]["augmentation"] is True
        seen = []
        plain = HWRWithSynthTrainer.mix

        class Spy(HWRWithSynthTrainer):
            def mix(self, instance):
                out = plain(self, instance)
                seen.append((instance["image"], out["image"]))
                return out
        trainer, _, logs, _ = _train(cfg, Spy, 1)
        assert trainer._store_variant == "full" and trainer._augment is None
        assert len(logs) == 1 and all(np.isfinite(v) for v in logs[0].values()) and "recogLoss" in logs[0]
        real, mixed = seen[0]
        assert real.is_cuda and mixed.is_cuda and mixed.shape[0] == real.shape[0] + 2 and mixed.shape[3] >= real.shape[3]
        assert torch.equal(mixed[:real.shape[0], :, :, :real.shape[3]], real) and bool((mixed[:real.shape[0], :, :, real.shape[3]:] == -1).all())
        k = (1.0 - mixed[real.shape[0]:][mixed[real.shape[0]:] != -1].double()) * 128.0
        assert torch.equal(k, k.round()) and float(k.min()) >= 0 and float(k.max()) <= 255
    finally:
        rng.set_mode("device")
