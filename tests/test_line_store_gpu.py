"""GPU: the device-resident line store - hwg_store_batch (csrc/line_store.hip) through ops.store_batch against the fp64 restatement
tests/_line_store_ref.py, BIT FOR BIT (fp64 without contraction leaves nothing to round differently: a difference is a bug in one of the
two); guard elements around the outputs and guard bytes around and between the pool's lines; the host refusals in front of the launch;
StoreLoader against ShardedLoader on fabricated IAM / RIMES directories; HWWithStyleTrainer fed by it."""
import json
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _line_store_ref as R  # noqa: E402
from _gpu_tidy import leave_nothing_behind, scrub  # noqa: E402,F401  (leave_nothing_behind: module-scoped, autouse)

GOLD = os.path.join(ROOT, "tests", "golden")
CFGS = {"iam": "cf_IAMslant_noMask_charSpecSingleAppend_GANMedMT_autoAEMoPrcp2tightNewCTCUseGen_balB_hCF0.75_sMG.json",
        "rimes": "cf_RIMESLinesslant_noMask_charSpecSingleAppend_GANMedMT_autoAEMoPrcp2tightNewCTCUseGen_balB_hCF0.75_sMG.json"}
GUARD = 7                                   # the byte around and between the pool's lines
WIDTHS64 = (1, 3, 4, 5, 63, 64, 65, 257)
WIDTHS7 = (5, 1, 66, 4)
PI4 = math.pi / 4


def _host_pool(H, widths, binary, seed):
    """-> (buffer uint8 with guard bytes, offsets, lines, masks-buffer, masks): lines at odd byte offsets, 0 and 255 at the line ends"""
    rs = np.random.RandomState(seed)
    lines, masks, offsets, at = [], [], [], 13
    for w in widths:
        img = (rs.randint(0, 2, (H, w)) * 255 if binary else rs.randint(0, 256, (H, w))).astype(np.uint8)
        img[::2, 0], img[1::2, 0], img[::2, -1], img[1::2, -1] = 0, 255, 255, 0
        lines.append(img)
        masks.append((rs.randint(0, 2, (H, w)) * 255).astype(np.uint8))
        at += 1 - (at % 2)                  # odd offsets
        offsets.append(at)
        at += H * w + 5
    buf = np.full(at + 11, GUARD, dtype=np.uint8)
    mbuf = np.full(at + 11, GUARD, dtype=np.uint8)
    for off, img, mk in zip(offsets, lines, masks):
        buf[off:off + img.size] = img.reshape(-1)
        mbuf[off:off + mk.size] = mk.reshape(-1)
    return buf, np.array(offsets, dtype=np.int64), lines, mbuf, masks


@pytest.fixture(scope="module")
def pools(cuda):
    """host pools and their references' inputs, built once and left unchanged"""
    from handwriting_line_generation_amd import ops
    out = {}
    for name, H, widths, binary in (("h64", 64, WIDTHS64, False), ("h7", 7, WIDTHS7, False), ("h64_binary", 64, WIDTHS64, True)):
        buf, offsets, lines, mbuf, masks = _host_pool(H, widths, binary, len(name))
        pool = ops.LinePool(torch.from_numpy(buf).to(cuda), offsets, widths, height=H, masks=torch.from_numpy(mbuf).to(cuda))
        out[name] = (pool, lines, masks, buf, mbuf)
    return out


def _rows(lines, picks, W_max=None):
    """picks: [(line, strech or None = W_max / width, skew)] -> [(line, out_w, strech, m)]"""
    rows = []
    for k, s, skew in picks:
        w = lines[k].shape[1]
        s = W_max / w if s is None else s
        rows.append((k, int(w * s), s, math.tan(skew)))
    return rows


# (name, pool, picks, W: None = max(out_w) / "+n" = that plus n, W_max for strech = None)
CASES = [
    ("rest_five_lines", "h64", [(k, 1.0, 0.0) for k in range(5)], None, None),                             # W = 63
    ("rest_wide", "h64", [(7, 1.0, 0.0), (5, 1.0, 0.0), (0, 1.0, 0.0)], None, None),                       # W = 257
    ("one_row_w1", "h64", [(0, 1.0, 0.0)], None, None),                                                    # W = 1: B*H*W = 64
    ("one_row_w1_h7", "h7", [(1, 1.4, PI4)], None, None),                                                  # B*H*W = 7: surplus element
    ("shear_mixed", "h64", [(7, 0.6, PI4), (7, 1.4, -PI4), (4, 1.0, 1e-3), (6, 1.4, 1e-3), (1, 0.6, -PI4)], None, None),   # W = 359
    ("shear_mult4", "h64", [(5, 1.0, PI4), (5, 1.0, -PI4), (2, 1.4, 0.0)], None, None),                    # W = 64
    ("two_rows_repeated", "h64", [(6, 1.4, -PI4), (6, 0.6, 1e-3)], None, None),                            # W = 91
    ("shear_padded", "h64", [(3, 1.4, PI4), (4, 0.6, -PI4), (3, 1.4, PI4), (2, 0.6, 1e-3)], "+9", None),   # W above every out_w
    ("clamp_strech", "h64", [(6, None, PI4), (4, None, -PI4), (7, None, 1e-3)], None, 300),                # strech = W_max / width
    ("narrow_to_zero", "h64", [(0, 0.6, PI4), (1, 0.6, 0.0), (2, 1.4, -PI4)], None, None),                 # out_w = 0 and 1
    ("h7_mixed", "h7", [(0, 1.4, PI4), (2, 0.6, -PI4), (3, 1.0, 1e-3), (2, None, 0.0), (1, 1.0, 0.0)], None, 91),
    ("binary_guards", "h64_binary", [(7, 1.4, PI4), (3, 0.6, -PI4), (0, 1.4, 1e-3), (5, 1.0, 0.0), (6, None, -PI4)], "+3", 100),
]


@pytest.mark.parametrize("want_mask", [False, True], ids=["lines", "lines+masks"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_store_batch_equals_the_restatement_bit_for_bit(cuda, pools, case, want_mask):
    from handwriting_line_generation_amd import ops
    name, pool_name, picks, W, W_max = case
    pool, lines, masks, buf, mbuf = pools[pool_name]
    H = pool.height
    rows = _rows(lines, picks, W_max)
    widest = max(r[1] for r in rows)
    W = widest if W is None else widest + int(W)
    assert W >= 1
    B = len(rows)
    total, need = B * H * W, -(-B * H * W // 4) * 4
    front, back = 12, 21                                       # guard elements: the view starts 16-byte aligned
    bufs = [torch.full((front + need + back,), float("nan"), device=cuda) for _ in range(2 if want_mask else 1)]
    views = [b[front:front + need] for b in bufs]
    got = ops.store_batch(pool, rows, W=W, want_mask=want_mask, out=tuple(views) if want_mask else views[0])
    got = list(got) if want_mask else [got]
    want = R.store_batch(lines, rows, W, masks if want_mask else None)
    want = list(want) if want_mask else [want]
    torch.cuda.synchronize()
    for g, w, b, pad, what in zip(got, want, bufs, (-1.0, 0.0), ("out", "out_mask")):
        assert g.shape == (B, 1, H, W) and g.dtype == torch.float32 and g.data_ptr() == b.data_ptr() + 4 * front
        g, flat = g.cpu().numpy(), b.cpu().numpy()
        assert np.isfinite(flat[front:front + need]).all(), what
        assert np.isnan(flat[:front]).all() and np.isnan(flat[front + need:]).all(), "%s: elements outside the rounded-up output were written" % what
        assert (flat[front + total:front + need] == pad).all(), "%s: the surplus of the last word is padding" % what
        diff = g.view(np.uint32) != w.view(np.uint32)
        print("%-16s %-8s [%d,1,%d,%d]: %d of %d elements differ in a bit" % (name, what, B, H, W, int(diff.sum()), diff.size))
        assert not diff.any(), (name, what, np.argwhere(diff)[:5].tolist(), g[diff][:5], w[diff][:5])
        for r, (k, ow, s, m) in enumerate(rows):
            assert (g[r, 0, :, ow:] == pad).all()
    if "rest" in name:
        for r, (k, ow, s, m) in enumerate(rows):               # strech 1, m 0: the line's own bytes
            assert np.array_equal(got[0][r, 0, :, :ow].cpu().numpy(), np.float32(1) - lines[k].astype(np.float32) / np.float32(128))
    if pool_name == "h64_binary":
        # lines of 0 / 255 with border 255, masks of 0 / 255 with border 0: a level that needs the guard byte 7 in the blend shows as a
        # difference above; at rest nothing but the two levels exists
        r = [i for i, row in enumerate(rows) if row[2] == 1.0 and row[3] == 0.0][0]
        assert set(np.unique(got[0][r, 0, :, :rows[r][1]].cpu().numpy()).tolist()) <= {1.0, 1.0 - 255 / 128}
    assert torch.equal(pool.pixels.cpu(), torch.from_numpy(buf)) and torch.equal(pool.masks.cpu(), torch.from_numpy(mbuf))


def test_store_batch_allocates_rounded_up_and_launches_once(cuda, pools, monkeypatch):
    from handwriting_line_generation_amd import _lib as L, ops
    pool, lines, masks, _, _ = pools["h7"]
    rows = _rows(lines, [(0, 1.0, 0.0), (2, 0.6, PI4), (0, 1.4, -PI4)])           # W = 39
    ops.store_batch(pool, rows)                                # (the pool's own tables are uploaded with its first batch)
    calls, uploads = [], []
    plain_call, plain_h2d = L.call, ops.h2d
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), plain_call(name, *a))[1])
    monkeypatch.setattr(ops, "h2d", lambda *a, **k: (uploads.append(1), plain_h2d(*a, **k))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (_ for _ in ()).throw(AssertionError("store_batch synchronised")))
    img, fg = ops.store_batch(pool, rows, want_mask=True)
    monkeypatch.undo()
    assert calls == ["hwg_store_batch"] and uploads == [1]
    W = max(r[1] for r in rows)
    assert img.shape == fg.shape == (3, 1, 7, W) and (3 * 7 * W) % 4 != 0
    want, want_fg = R.store_batch(lines, rows, W, masks)
    assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(fg.cpu().numpy(), want_fg)


def test_store_batch_refuses_on_the_host_before_any_launch(cuda, pools, monkeypatch):
    from handwriting_line_generation_amd import _lib as L, ops
    pool, lines, _, buf, _ = pools["h64"]
    good = _rows(lines, [(0, 1.0, 0.0), (7, 1.4, PI4)])
    ops.store_batch(pool, good)
    launched = []
    plain = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (launched.append(name), plain(name, *a))[1])
    W = max(r[1] for r in good)
    for rows, kw, word in [([(8, 4, 1.0, 0.0)], {}, "line indices"), ([(-1, 4, 1.0, 0.0)], {}, "line indices"), ([(0.5, 4, 1.0, 0.0)], {}, "line indices"),
                           (good + [(3, W + 1, 1.0, 0.0)], {"W": W}, "above the batch width"), ([(1, -1, 1.0, 0.0)], {}, "out_w"),
                           ([(1, 4, float("inf"), 0.0)], {}, "strech"), ([(1, 4, float("nan"), 0.0)], {}, "strech"), ([(1, 4, 0.0, 0.0)], {}, "strech"),
                           ([(1, 4, -1.0, 0.0)], {}, "strech"), ([(1, 4, 1.0, float("nan"))], {}, "m \\(tan"), ([(1, 4, 1.0, float("-inf"))], {}, "m \\(tan"),
                           ([], {}, "non-empty"), ([(0, 0, 1.0, 0.0)], {}, "batch width 0"), (good, {"want_mask": True, "out": (torch.empty(8, device=cuda),)}, "pair"),
                           (good, {"out": torch.empty(64, device=cuda)}, "at least"), (good, {"out": torch.empty(64 * 2 * W + 4, device=cuda)[1:]}, "aligned")]:
        with pytest.raises(L.HwgError, match="store_batch: .*" + word):
            ops.store_batch(pool, rows, **kw)
    px = pool.pixels
    off, w = np.asarray(pool.offsets), np.asarray(pool.widths)
    overlap = off.copy()
    overlap[3] = off[2] + 64 * w[2] - 1                        # line 3 begins in the last byte of line 2
    beyond = off.copy()
    beyond[7] = px.numel() - 64 * w[7] + 1
    for bad_pool, word in [(ops.LinePool(px, overlap, w, 64), "overlap"), (ops.LinePool(px, beyond, w, 64), "inside the"),
                           (ops.LinePool(px, off, np.where(w == 4, 0, w), 64), "at least 1"),
                           (ops.LinePool(px, off, w, 64, masks=pool.masks[:-1]), "mask pool"), (ops.LinePool(px, off, w, 64, masks=pool.masks.cpu()), "mask pool"),
                           (ops.LinePool(px.cpu(), off, w, 64), "device tensor")]:
        with pytest.raises(L.HwgError, match="store_batch: .*" + word):
            ops.store_batch(bad_pool, good)
    with pytest.raises(L.HwgError, match="has no masks"):
        ops.store_batch(ops.LinePool(px, off, w, 64), good, want_mask=True)
    assert launched == []


# ---- the loader ------------------------------------------------------------------------------------------------------------------------------
def _disk_config(which, root, tmp_path, augmentation, bucket=0, masks=True, store=True):
    from handwriting_line_generation_amd.harness import CHAR_FILES
    cfg = json.load(open(os.path.join(ROOT, "configs", CFGS[which])))
    dl = cfg["data_loader"]
    dl.update(data_dir=root, batch_size=2, a_batch_size=2, num_workers=0, shuffle=True, char_file=CHAR_FILES[which], max_width=400,
              fg_masks_dir=str(tmp_path / "fg_masks") + "/", augmentation=augmentation, device_store=store)
    if bucket:
        dl["width_bucket"] = bucket
    cfg["validation"] = dict(cfg.get("validation", {}), batch_size=2, a_batch_size=2, shuffle=False, num_workers=0, augmentation=None)
    cfg["trainer"].update(save_dir=str(tmp_path / "saved"), save_step=10 ** 6, save_step_minor=10 ** 6, log_step=10 ** 6, val_step=7, print_dir=None,
                          encoder_weights=str(tmp_path / "enc" / "encoder.pth"), text_data=str(tmp_path / "corpus.txt"), iterations=7)
    cfg["model"]["pretrained_hwr"] = None
    cfg["seed"] = 5
    cfg["cuda"], cfg["gpu"] = True, 0
    if masks:
        cfg["no_bg_loss"] = True                               # the switch: top-level key next to the trainer's
    return cfg


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    from oracle import collate_items
    base = tmp_path_factory.mktemp("line_store_data")
    out = {}
    for which in ("iam", "rimes"):
        out[which] = str(base / which)
        os.makedirs(out[which])
        (collate_items.fake_iam if which == "iam" else collate_items.fake_rimes)(out[which])
    out["base"] = base
    return out


def _same_batch(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key in want:
        g, w = got[key], want[key]
        if key in ("image", "fg_mask"):
            assert g.is_cuda and g.dtype == torch.float32 and g.shape == w.shape, (key, g.shape, w.shape)
            assert torch.equal(g.cpu().view(torch.int32), w.view(torch.int32)), key
        elif torch.is_tensor(w):
            assert g.dtype == w.dtype and torch.equal(g, w), key
        else:
            assert g == w, (key, g, w)


@pytest.mark.parametrize("which", ["iam", "rimes"])
@pytest.mark.parametrize("bucket", [0, 128])
def test_store_loader_equals_sharded_loader_without_augmentation(cuda, roots, which, bucket):
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.line_store import StoreLoader
    base = roots["base"]
    pair = [D.getDataLoader(_disk_config(which, roots[which], base, None, bucket, store=s), "train") for s in (True, False)]
    n = 0
    for stored, host in zip(*pair):                            # the training loaders, then the validation loaders (the key is inherited)
        assert isinstance(stored, StoreLoader) and type(host) is D.ShardedLoader and len(stored) == len(host)
        assert stored.want_mask and stored.store.pool.masks is not None
        for epoch in range(2):
            got, want = list(stored), list(host)
            assert len(got) == len(want) >= 1 and stored.epoch == host.epoch == epoch + 1
            for g, w in zip(got, want):
                _same_batch(g, w)
                assert not bucket or g["image"].shape[3] % bucket == 0
                n += 1
    assert n >= 6


@pytest.mark.parametrize("which", ["iam", "rimes"])
def test_store_loader_affine_equals_the_restatement_with_the_recorded_draws(cuda, roots, which):
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    cfg = _disk_config(which, roots[which], roots["base"], "affine")
    loader, _ = D.getDataLoader(cfg, "train")
    ds, store = loader.dataset, loader.store
    batches = loader._batches()
    np.random.seed(17)
    got = list(loader)
    rs = np.random.RandomState(17)                             # the draws, replayed: per item in batch order strech, then skew
    clamped = sheared = 0
    assert len(got) == len(batches) >= 2
    for inst, indices in zip(got, batches):
        lines, masks, rows = [], [], []
        for idx in indices:
            strech = (ds.max_strech * 2) * rs.random_sample() - ds.max_strech + 1
            skew = (ds.max_rot_rad * 2) * rs.random_sample() - ds.max_rot_rad
            author, ls = ds.lineIndex[idx]
            ls = [(l + 37) % len(ds.authors[author]) if l >= len(ds.authors[author]) else l for l in ls]
            fitted = [store.line(author, l) for l in ls]
            for img in fitted:
                if img.shape[1] * strech > ds.max_width:
                    strech = ds.max_width / img.shape[1]
                    clamped += 1
            for l, img in zip(ls, fitted):
                k = store.index[(author, l)]
                rows.append((len(lines), int(img.shape[1] * strech), strech, math.tan(skew)))
                lines.append(img)
                masks.append(store.masks[store.offsets[k]:store.offsets[k] + img.size].reshape(img.shape))
            sheared += abs(skew) > 0.1
        W = max(r[1] for r in rows)
        want, want_fg = R.store_batch(lines, rows, W, masks)
        assert np.array_equal(inst["image"].cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(inst["fg_mask"].cpu().numpy().view(np.uint32), want_fg.view(np.uint32))
        assert 0 < float(inst["fg_mask"].mean()) < 1
    assert np.random.random() == rs.random_sample()            # exactly these draws were consumed
    assert sheared > 0
    print("%s: %d batches, %d clamps" % (which, len(got), clamped))


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------------
def _cycle(which, roots, workdir, augmentation, store):
    from handwriting_line_generation_amd import model as M, rng
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.synthetic import write_synthetic_corpus
    from handwriting_line_generation_amd.model import loss as loss_fns
    from handwriting_line_generation_amd.trainer import HWWithStyleTrainer
    os.makedirs(str(workdir), exist_ok=True)
    cfg = _disk_config(which, roots[which], workdir, augmentation, bucket=128, store=store)
    cfg["data_loader"]["fg_masks_dir"] = str(roots["base"] / "fg_masks") + "/"         # the cache the loader tests built
    cfg["model"].update(json.load(open(os.path.join(GOLD, "ref_ckpt_reduced_model.json"))))
    tr, dl = cfg["trainer"], cfg["data_loader"]
    os.makedirs(os.path.dirname(tr["encoder_weights"]), exist_ok=True)
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    rng.set_mode("device", seed=3)
    torch.save({"state_dict": M.Autoencoder({"type": tr.get("encoder_type", "2tight"), "hwr": cfg["model"]["num_class"]}).state_dict()}, tr["encoder_weights"])
    write_synthetic_corpus(tr["text_data"], dl["char_file"])
    loader, vloader = D.getDataLoader(cfg, "train")
    model = M.HWWithStyle(cfg["model"])
    losses = {k: getattr(loss_fns, v) for k, v in cfg["loss"].items()}
    trainer = HWWithStyleTrainer(model, losses, [], None, cfg, loader, vloader, None)
    assert trainer.no_bg_loss
    torch.manual_seed(1); np.random.seed(1); random.seed(1)
    logs = [trainer._train_iteration(it) for it in range(7)]
    val = trainer._valid_epoch()
    torch.cuda.synchronize()
    state = {k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items()}
    kinds = (type(loader).__name__, type(vloader).__name__)
    scrub(trainer)
    rng.set_mode("device")
    return logs, val, state, kinds


def test_trainer_runs_on_the_store_and_matches_the_host_loader_bit_for_bit(cuda, roots, tmp_path):
    stored = _cycle("iam", roots, tmp_path / "store", None, True)
    host = _cycle("iam", roots, tmp_path / "host", None, False)
    assert stored[3] == ("StoreLoader", "StoreLoader") and host[3] == ("ShardedLoader", "ShardedLoader")
    for logs, val, _, _ in (stored, host):
        assert len(logs) == 7 and all(log and all(np.isfinite(v) for v in log.values()) for log in logs), logs
        assert val and all(np.isfinite(v) for v in val.values()), val
    assert any("autoLoss" in log for log in stored[0])
    assert stored[0] == host[0], (stored[0], host[0])
    assert stored[1] == host[1], (stored[1], host[1])
    for k, v in host[2].items():
        assert torch.equal(v, stored[2][k]), k


def test_trainer_runs_on_the_store_with_the_affine_augmentation(cuda, roots, tmp_path):
    logs, val, state, kinds = _cycle("iam", roots, tmp_path / "affine", "affine", True)
    assert kinds == ("StoreLoader", "StoreLoader")
    assert all(log and all(np.isfinite(v) for v in log.values()) for log in logs), logs
    assert val and all(np.isfinite(v) for v in val.values()), val
    assert all(torch.isfinite(v).all() for v in state.values() if v.dtype.is_floating_point)
