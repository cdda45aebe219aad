"""GPU: the line augmentation kernels (csrc/augment.hip: Tensmeyer brightness + mesh warp on the collated batch) against the numpy restatement
tests/_augment_ref.py - and through it against the maps of the reference's grid_distortion.warp_image (tests/golden/warp_maps.npz,
tests/test_hw_dataset_cpu.py) - and the two recogniser pre-training configs end to end from a dataset directory."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
GOLDEN_CASES = ["w150", "w263", "w420", "w300_low"]
H = 64


def _text_line(rs, w):
    """a line-like image: light paper with noise, dark strokes"""
    img = rs.randint(190, 256, size=(H, w))
    for _ in range(max(w // 14, 1)):
        x, y = int(rs.randint(0, max(w - 3, 1))), int(rs.randint(4, 40))
        img[y:y + int(rs.randint(6, 22)), x:x + int(rs.randint(2, 9))] = rs.randint(10, 110)
    return img.astype(np.int64)


def _draws(rs, w, sigma):
    sy, sx = R.lattice(H, w)
    n = (len(sy), len(sx))
    return (rs.normal(0.0, sigma, size=n), rs.normal(0.0, sigma, size=n))


def _cases():
    """name -> dict(lines [levels H x w], fg_bg [B,2], disp [(dy, dx) or None], W padded width)"""
    out = {}
    g = np.load(os.path.join(GOLD, "warp_maps.npz"))
    for k, name in enumerate(GOLDEN_CASES):          # the reference's own lattices and displacements (teacher forced)
        img, src, dst = g[name + "/image"].astype(np.int64), g[name + "/source"], g[name + "/destination"]
        gy, gx = (int(v) for v in g[name + "/grid"])
        d = (dst - src).reshape(gy, gx, 2)
        out[name] = {"lines": [img], "fg_bg": np.array([[17.25 - 9 * k, -23.5 + 11 * k]]), "disp": [(d[:, :, 0], d[:, :, 1])], "W": img.shape[1]}
    rs = np.random.RandomState(21)
    widths = [1216, 161, 1003, 640, 333, 1100, 87, 950, 512, 777, 1211, 240, 405, 868, 699, 1150]
    out["ragged16"] = {"lines": [_text_line(rs, w) for w in widths], "fg_bg": rs.normal(0, 30, size=(16, 2)),
                       "disp": [_draws(rs, w, 1.5) for w in widths], "W": 1216}
    widths = [5, 130, 6]                              # a 5-pixel-wide line is not warped (grid_distortion.py:12), a 6-pixel-wide one is
    out["narrow"] = {"lines": [_text_line(rs, w) for w in widths], "fg_bg": rs.normal(0, 30, size=(3, 2)),
                     "disp": [None] + [_draws(rs, w, 1.5) for w in widths[1:]], "W": 136}
    return out


def _batch(lines, W, x_off=None):
    x = np.full((len(lines), 1, H, W), -1.0, dtype=np.float32)
    for b, l in enumerate(lines):
        o = 0 if x_off is None else x_off[b]
        x[b, 0, :, o:o + l.shape[1]] = 1.0 - l.astype(np.float32) / 128.0
    return torch.from_numpy(x)


def _run(cuda, case, x_off=None):
    from handwriting_line_generation_amd import ops
    lines = case["lines"]
    mesh = ops.LineMesh(H, [l.shape[1] for l in lines], x_off=x_off, disp=case["disp"])
    y, mp, st = ops.augment_lines(_batch(lines, case["W"], x_off).to(cuda), mesh, fg_bg=case["fg_bg"], want_map=True)
    torch.cuda.synchronize()
    return y.cpu().numpy(), mp.cpu().numpy(), st.cpu().numpy()


@pytest.fixture(scope="module")
def results(cuda):
    """every case once through the kernels and once through the restatement (fp64 and float32 maps)"""
    out = {}
    for name, case in _cases().items():
        y, mp, st = _run(cuda, case)
        ref = []
        for b, l in enumerate(case["lines"]):
            w = l.shape[1]
            t, lut, m = R.stats(l, *case["fg_bg"][b])
            r = {"t": t, "lut": lut, "m": m, "w": w}
            if case["disp"][b] is not None:
                sy, sx = R.lattice(H, w)
                f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731  (what the kernel is handed)
                r["m64"] = R.warp_map(H, w, sy, sx, *case["disp"][b], np.float64)
                r["m32"] = R.warp_map(H, w, f32(sy), f32(sx), f32(case["disp"][b][0]), f32(case["disp"][b][1]), np.float32)
            ref.append(r)
        out[name] = {"case": case, "y": y, "map": mp, "stats": st, "ref": ref}
    return out


def test_statistics_are_exact(results):
    for name, res in results.items():
        for b, (l, r) in enumerate(zip(res["case"]["lines"], res["ref"])):
            margin = R.split_margin(np.bincount(l.reshape(-1), minlength=256))
            assert margin > 1e-9, (name, b, margin)        # fp64 summation order cannot decide the threshold
            st = res["stats"][b]
            assert int(st[0]) == r["t"] and int(st[1]) == r["m"] and np.array_equal(st[2:], r["lut"]), (name, b, int(st[0]), r["t"], int(st[1]), r["m"])


def test_geometry_against_the_fp64_restatement(results):
    for name, res in results.items():
        worst_err = worst_ref = 0.0
        left_out = total = 0
        for b, r in enumerate(res["ref"]):
            if "m64" not in r:
                continue
            w, m64, m32 = r["w"], r["m64"], r["m32"]
            ky, kx, y = res["map"][b, 0, :, :w], res["map"][b, 1, :, :w], res["y"][b, 0, :, :w]
            near_border = np.abs(m64["border"]) < 1e-4        # may fall on either side of the mesh border
            left_out += int(near_border.sum()); total += H * w
            inside, outside = m64["inside"] & ~near_border, ~m64["inside"] & ~near_border
            assert np.isnan(ky[outside]).all() and np.isnan(kx[outside]).all(), (name, b)
            assert (y[outside] == np.float32(1 - r["m"] / 128)).all(), (name, b)        # outside the mesh: the border level
            assert np.isfinite(ky[inside]).all() and np.isfinite(kx[inside]).all(), (name, b)
            both = inside & m32["inside"]
            ref_err = max(np.abs(m32["map_y"][both].astype(np.float64) - m64["map_y"][both]).max(), np.abs(m32["map_x"][both].astype(np.float64) - m64["map_x"][both]).max())
            err = max(np.abs(ky[inside].astype(np.float64) - m64["map_y"][inside]).max(), np.abs(kx[inside].astype(np.float64) - m64["map_x"][inside]).max())
            worst_err, worst_ref = max(worst_err, float(err)), max(worst_ref, float(ref_err))
        bound = 4 * worst_ref        # the reference arithmetic at the kernel's precision, margin 4 for operation order
        print("geometry %-9s kernel map error %.3e px, float32 restatement error %.3e px, bound %.3e px, left out %d of %d pixels" % (name, worst_err, worst_ref, bound, left_out, total))
        assert left_out <= 0.005 * total, (name, left_out, total)
        assert worst_err <= bound, (name, worst_err, bound)
        # padding columns carry no map
        for b, r in enumerate(res["ref"]):
            assert np.isnan(res["map"][b, :, :, r["w"]:]).all()


def test_pixels_against_fp64_resampling_of_the_kernels_own_map(results):
    for name, res in results.items():
        worst = 0.0
        for b, (l, r) in enumerate(zip(res["case"]["lines"], res["ref"])):
            w = r["w"]
            y = res["y"][b, 0]
            assert (y[:, w:] == -1).all(), (name, b)                                    # padding columns exactly -1
            k = (1.0 - y[:, :w].astype(np.float64)) * 128.0
            assert np.array_equal(k, np.rint(k)) and k.min() >= 0 and k.max() <= 255, (name, b)      # every output is exactly 1 - k/128
            assert np.array_equal(y[:, :w], (1 - k / 128).astype(np.float32))
            q = r["lut"][l].astype(np.float64)
            if "m64" not in r:
                assert np.array_equal(k, q), (name, b)                                  # no warp: the LUT alone
                continue
            ky, kx = res["map"][b, 0, :, :w], res["map"][b, 1, :, :w]
            ok = np.isfinite(ky)
            v = R.bilinear(q, np.where(ok, ky, 0), np.where(ok, kx, 0), r["m"])
            assert (k[~ok] == r["m"]).all()
            d = np.abs(k - v)[ok].max()
            worst = max(worst, float(d))
            assert d <= 0.5 + 2.0 ** -12, (name, b, d)       # three fp32 lerps of values <= 255: <= 16 ulp of 2^-16
        print("pixels   %-9s worst |level - fp64 resample| %.6f (bound %.6f)" % (name, worst, 0.5 + 2.0 ** -12))


def test_identity(cuda):
    """zero displacements and no brightness shift return the input bit for bit"""
    rs = np.random.RandomState(5)
    widths = [300, 77, 256]
    lines = [_text_line(rs, w) for w in widths]
    zero = []
    for w in widths:
        sy, sx = R.lattice(H, w)
        zero.append((np.zeros((len(sy), len(sx))), np.zeros((len(sy), len(sx)))))
    case = {"lines": lines, "fg_bg": np.zeros((3, 2)), "disp": zero, "W": 320}
    y, mp, _ = _run(cuda, case)
    assert np.array_equal(y, _batch(lines, 320).numpy())
    for b, w in enumerate(widths):
        yy, xx = np.mgrid[0:H, 0:w]
        assert np.array_equal(mp[b, 0, :, :w], yy.astype(np.float32)) and np.array_equal(mp[b, 1, :, :w], xx.astype(np.float32))


def test_batch_independence_and_determinism(cuda, results):
    from handwriting_line_generation_amd import ops
    res = results["ragged16"]
    case = res["case"]
    # lines 3 and 6 of the ragged batch in another batch: other slots, other neighbours, another padded width, one of them shifted
    rs = np.random.RandomState(8)
    other = _text_line(rs, 410)
    sub = {"lines": [case["lines"][6], other, case["lines"][3]], "fg_bg": np.stack([case["fg_bg"][6], [3.0, -8.0], case["fg_bg"][3]]),
           "disp": [case["disp"][6], _draws(rs, 410, 1.5), case["disp"][3]], "W": 704}
    x_off = [11, 0, 0]
    y, mp, st = _run(cuda, sub, x_off=x_off)
    for slot, (b, o) in {0: (6, 11), 2: (3, 0)}.items():
        w = case["lines"][b].shape[1]
        assert np.array_equal(y[slot, 0, :, o:o + w], res["y"][b, 0, :, :w])
        assert np.array_equal(mp[slot, :, :, o:o + w], res["map"][b, :, :, :w], equal_nan=True) and np.array_equal(st[slot], res["stats"][b])
        assert (y[slot, 0, :, :o] == -1).all() and (y[slot, 0, :, o + w:] == -1).all()
    # device draws: same seed and offset -> same bits (and the stream advances); another rank's seed -> other draws
    x = _batch(case["lines"][:4], 1216).to(cuda)
    mesh = ops.LineMesh(H, [l.shape[1] for l in case["lines"][:4]])

    def draw(seed, offset):
        g = ops.DeviceRNG(seed)
        g.offset = offset
        out = ops.augment_lines(x, mesh, rng=g)
        assert g.offset == offset + (4 * (2 + 2 * mesh.GY * mesh.GX) + 3) // 4
        return out
    a, b, c, d = draw(1000003 * 7 + 0, 40), draw(1000003 * 7 + 0, 40), draw(1000003 * 7 + 1, 40), draw(1000003 * 7 + 0, 41)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
    assert not torch.equal(a, x) and bool((a[:, :, :, :87] != -1).all())


# ---- end to end: the two recogniser pre-training configs from a dataset directory ----------------------------------------------------------
HWR_CFG = {"iam": "cf_IAM_hwr_cnnOnly_batchnorm_aug.json", "rimes": "cf_RIMESLines_hwr_cnnOnly_batchnorm_aug.json"}


def _fabricate(which, root):
    from oracle import collate_items
    os.makedirs(root)
    if which == "iam":
        collate_items.fake_iam(root, n_pages=6, with_images=True)
    else:
        collate_items.fake_rimes(root)


def _hwr_config(which, root, tmp_path):
    from handwriting_line_generation_amd.harness import CHAR_FILES
    cfg = json.load(open(os.path.join(ROOT, "configs", HWR_CFG[which])))
    cfg["data_loader"].update(data_dir=root, batch_size=4, num_workers=0, char_file=CHAR_FILES[which])
    cfg["validation"].update(batch_size=4, num_workers=0)
    cfg["trainer"].update(save_dir=str(tmp_path / "saved"), save_step=10 ** 6, save_step_minor=10 ** 6, log_step=10 ** 6, val_step=10 ** 6, iterations=6)
    cfg["seed"] = 5
    cfg["cuda"], cfg["gpu"] = True, 0
    return cfg


@pytest.mark.parametrize("which", ["iam", "rimes"])
def test_hwr_config_trains_from_a_directory_with_device_augmentation(cuda, tmp_path, which):
    import random

    from handwriting_line_generation_amd import model as M, rng
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.data.device_augment import DeviceAugment
    from handwriting_line_generation_amd.model import loss as loss_fns
    from handwriting_line_generation_amd.trainer import HWWithStyleTrainer
    root = str(tmp_path / which)
    _fabricate(which, root)
    cfg = _hwr_config(which, root, tmp_path)
    assert cfg["data_loader"]["augmentation"] == (True if which == "iam" else "warp")       # as shipped
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    rng.set_mode("device", seed=3)
    loader, vloader = D.getDataLoader(cfg, "train")
    assert isinstance(loader, DeviceAugment) and isinstance(vloader, DeviceAugment)           # validation inherits `augmentation`
    assert loader.dataset.augmentation is None and loader.batch_size == 4 and len(loader) == len(loader.loader) > 0
    assert type(loader.dataset).__name__ == cfg["data_loader"]["data_set_name"]
    plain = []
    for wrapped in (loader.loader, vloader.loader):      # what collate hands the wrapper
        def rec(items, _orig=wrapped._collate):
            inst = _orig(items)
            plain.append(inst["image"].clone())
            return inst
        wrapped._collate = rec
    model = M.HWWithStyle(cfg["model"])
    losses = {k: getattr(loss_fns, v) for k, v in cfg["loss"].items()}
    trainer = HWWithStyleTrainer(model, losses, [], None, cfg, loader, vloader, None)
    consumed, to_tensor = [], trainer._to_tensor

    def spy(instance):
        consumed.append(instance["image"])
        return to_tensor(instance)
    trainer._to_tensor = spy
    offset0 = rng.device_rng().offset
    for it in range(6):
        log = trainer._train_iteration(it)
        assert log and all(np.isfinite(v) for v in log.values()), (it, log)
        assert "recogLoss" in log and "CER" in log, log
    val = trainer._valid_epoch()
    assert val and all(np.isfinite(v) for v in val.values()) and "val_CER" in val, val
    torch.cuda.synchronize()
    assert rng.device_rng().offset > offset0
    assert len(consumed) >= 7 and len(consumed) == len(plain)
    for got, src in zip(consumed, plain):
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == src.shape
        got = got.cpu()
        pad = src == -1
        assert torch.equal(got == -1, pad)                         # -1 exactly on the padding columns, nowhere else
        k = (1.0 - got[~pad].double()) * 128.0
        assert torch.equal(k, k.round()) and float(k.min()) >= 0 and float(k.max()) <= 255      # the 256-level grid
        assert not torch.equal(got, src)
    rng.set_mode("device")


def test_other_configs_get_no_augmentation_wrapper(cuda, tmp_path):
    """an "affine" GAN config takes exactly the path it always took"""
    from handwriting_line_generation_amd.data import author_hw_dataset as D
    from handwriting_line_generation_amd.harness import CHAR_FILES
    root = str(tmp_path / "iam")
    _fabricate("iam", root)
    name = "cf_IAMslant_noMask_charSpecSingleAppend_GANMedMT_autoAEMoPrcp2tightNewCTCUseGen_balB_hCF0.75_sMG.json"
    cfg = json.load(open(os.path.join(ROOT, "configs", name)))
    assert cfg["data_loader"]["augmentation"] == "affine"
    cfg["data_loader"].update(data_dir=root, batch_size=2, a_batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"])
    loader, vloader = D.getDataLoader(cfg, "train")
    assert type(loader) is D.ShardedLoader and type(vloader) is D.ShardedLoader and loader.dataset.augmentation == "affine"
    assert not next(iter(loader))["image"].is_cuda


def test_train_cli_pretrains_the_recogniser_from_a_directory(cuda, tmp_path):
    """`train.py -c cf_IAM_hwr_cnnOnly_batchnorm_aug.json` without --synthetic: the reference's first reproduction command"""
    from handwriting_line_generation_amd.logger import load_checkpoint
    root = str(tmp_path / "iam")
    _fabricate("iam", root)
    cfg = _hwr_config("iam", root, tmp_path)
    cfg["trainer"].update(save_step=7, val_step=4, iterations=8)
    path = str(tmp_path / HWR_CFG["iam"])
    json.dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-c", path, "--iterations", "8"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    ckpt = os.path.join(cfg["trainer"]["save_dir"], cfg["name"], "checkpoint-iteration7.pth")
    assert os.path.exists(ckpt), out[-2000:]
    ck = load_checkpoint(ckpt)
    assert ck["iteration"] == 7 and all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.dtype.is_floating_point)
    assert ck["rng"]["mode"] == "device" and ck["rng"]["offset"] > 0            # the augmentation's draws advanced the checkpointed stream
    assert "val_CER" in out, out[-2000:]
