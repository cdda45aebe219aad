"""CPU: the numpy restatement of the evaluation pictures (tests/_eval_pictures_ref.py) against what the unmodified reference hands to
cv2.imwrite (tests/golden/eval_pictures.npz, recorded by tools/gen_golden_eval_pictures.py), the quantisation on the edge values, and
new_eval.py's flag parsing and refusals."""
import os
import sys

import numpy as np
import pytest

import _eval_pictures_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "eval_pictures.npz")
sys.path.insert(0, ROOT)


def test_restatement_equals_the_recorded_reference_pictures():
    """every recorded array, byte for byte. The reference's array is in the order OpenCV reads as BGR: the restatement's RGB reversed.
    With `pred` the reference appends 50 rows and draws a caption with putText (recorded as not drawn): an empty caption here."""
    g = np.load(GOLD)
    n_cases = len([k for k in g.files if k.endswith("_image")])
    assert n_cases == 10
    seen = set()
    for i in range(n_cases):
        image, recon, with_pred = g["c%d_image" % i], g["c%d_recon" % i], bool(g["c%d_pred" % i])
        B, _, H, Wi = image.shape
        Wr = recon.shape[3]
        seen.add((Wi, Wr, with_pred))
        got = ref.eval_pairs(image, recon, [[] for _ in range(B)] if with_pred else None, np.zeros((1, 3, 2), np.uint8) if with_pred else None)
        assert got.shape == (B,) + ref.shape(H, Wi, Wr, with_pred) + (3,)
        for b in range(B):
            want = g["c%d_pic%d" % (i, b)]
            assert want.dtype == np.uint8 and want.shape == got[b].shape
            assert np.array_equal(got[b][..., ::-1], want), (i, b)
        # the frames are the colours the written file shows: green around the real line, blue around the reconstruction
        pr = abs(Wi - Wr) // 2 if Wi < Wr else 0
        pg = abs(Wi - Wr) // 2 if Wr < Wi else 0
        assert tuple(got[0, 0, pr]) == (0, 255, 0) and tuple(got[0, 2 * H + 1, pg]) == (0, 0, 255)
    assert seen == {(wi, wr, p) for wi, wr in [(7, 7), (12, 7), (7, 12), (8, 7), (1, 12)] for p in (False, True)}


def test_edge_values_tell_the_three_quantisations_apart():
    """x = fp32(1 - 2k/255) and its +-1..4 ulp neighbours, k = 0..255, clipped to [-1, 1]: the picture's bytes differ from hwg_lines_to_u8's
    (1 - x) * 127.5 truncated on 215 of the 2304 values and from round-to-nearest on 1154"""
    x = ref.edge_values()
    assert x.shape == (2304,) and x.dtype == np.float32 and x.min() == -1.0 and x.max() == 1.0
    got = ref.levels(x)
    lines = np.clip((np.float32(1) - x) * np.float32(127.5), 0, 255).astype(np.uint8)
    v = (np.float32(1) - (np.float32(1) + x) / np.float32(2)).astype(np.float64) * 255.0
    nearest = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    assert int((got != lines).sum()) == 215
    assert int((got != nearest).sum()) == 1154
    assert {0, 255} <= set(got.tolist()) and len(set(got.tolist())) > 240
    # the values a clamp decides and NaN
    assert ref.levels(np.array([np.nan, np.inf, -np.inf, 3.0, -3.0], np.float32)).tolist() == [0, 0, 255, 0, 255]


def test_restatement_caption_cells():
    atlas = (np.arange(3 * 4 * 5) % 251 + 1).astype(np.uint8).reshape(3, 4, 5)
    image = np.zeros((1, 1, 2, 9), np.float32)
    got = ref.eval_pairs(image, image, [[2, 0, -1, 1]], atlas)
    H, top = 2, 2 * 2 + 2 + (50 - 4) // 2
    assert got.shape == (1, 56, 9, 3)
    assert np.array_equal(got[0, top:top + 4, 2:7, 1], atlas[2]) and np.array_equal(got[0, top:top + 4, 7:9, 0], atlas[0][:, :2])   # clipped at Wp
    strip = got[0, 2 * H + 2:].copy()
    strip[top - 6:top - 2, 2:9] = 0
    assert not strip.any()


# ---- new_eval.py: flags and refusals, no GPU ------------------------------------------------------------------------------------------
def test_flags():
    import new_eval
    a = new_eval.parse_args(["-c", "x.pth", "-d", "out", "-g", "1", "-n", "12", "-b", "3", "-v", "3", "-s", "True", "-f", "c.json", "-T",
                             "-a", "by_author,cer_thresh=0.25,trainer=save_dir=/x,save_preds=p.csv,only=[a-b]", "-e", "[recon,pred]"])
    assert (a.checkpoint, a.savedir, a.gpu, a.number, a.batchsize, a.verbosity, a.shuffle, a.config, a.test) == \
        ("x.pth", "out", 1, 12, 3, 3, True, "c.json", True)
    assert a.to_eval == ["recon", "pred"]
    assert a.adds == [["by_author", "True"], ["cer_thresh", "0.25"], ["trainer", "save_dir", "/x"], ["save_preds", "p.csv"], ["only", "[a-b]"]]
    cfg = new_eval.apply_addtoconfig({"trainer": {}}, a.adds)
    assert cfg == {"trainer": {"save_dir": "/x"}, "by_author": "True", "cer_thresh": 0.25, "save_preds": "p.csv", "only": ["a", "b"]}
    d = new_eval.parse_args(["-c", "x.pth"])
    assert (d.savedir, d.index, d.number, d.gpu, d.batchsize, d.verbosity, d.shuffle, d.config, d.imgname, d.test, d.to_eval, d.adds) == \
        (None, None, 0, None, None, 2, False, None, None, False, None, [])
    assert new_eval.parse_args(["-c", "x.pth", "-s", "0"]).shuffle is False
    assert new_eval.parse_args(["-c", "x.pth", "-i", "-3"]).index == -3 and new_eval.parse_args(["-c", "x.pth", "-m", "a01"]).imgname == "a01"


@pytest.mark.parametrize("argv", [["-t", "0.5"], ["-N", "name"]])
def test_flags_that_do_not_exist(argv, capsys):
    import new_eval
    with pytest.raises(SystemExit):
        new_eval.parse_args(["-c", "x.pth"] + argv)
    assert "unrecognized arguments" in capsys.readouterr().err


@pytest.mark.parametrize("argv,word", [
    ([], "checkpoint"), (["-f", "c.json"], "untrained"), (["-c", "x", "-i", "1", "-m", "n"], "same time"), (["-c", "x", "-b", "0"], "-b"),
    (["-c", "x", "-e", "spaced"], "refused"), (["-c", "x", "-e", "spacing"], "refused"), (["-c", "x", "-e", "mask"], "refused"),
    (["-c", "x", "-e", "[recon,mask]"], "refused"), (["-c", "x", "-e", "[recon_gt_mask]"], "noMask"), (["-c", "x", "-e", "[recon_pred_space]"], "noMask"),
    (["-c", "x", "-e", "[gen_mask]"], "noMask"), (["-c", "x", "-e", "recon"], "list")])
def test_refused_command_lines(argv, word):
    import new_eval
    with pytest.raises(SystemExit) as e:
        new_eval.parse_args(argv)
    assert word in str(e.value) and "\n" not in str(e.value)


@pytest.mark.parametrize("key", ["save_spaced", "save_nns", "show_attention", "doSpaced"])
def test_refused_config_keys(key):
    import new_eval
    args = new_eval.parse_args(["-c", "x", "-a", "%s=out" % key])
    cfg = {"trainer": {"encoder_weights": "e.pth", "text_data": "t.txt", "print_dir": "p"}, "model": {"pretrained_hwr": "h.pth"},
           "data_loader": {"char_file": __file__, "batch_size": 2}, "optimizer_type": "Adam"}
    with pytest.raises(SystemExit) as e:
        new_eval.prepare_config(cfg, args)
    assert key in str(e.value) and "refused" in str(e.value) and "\n" not in str(e.value)


def test_prepare_config():
    import new_eval
    args = new_eval.parse_args(["-c", "x", "-b", "3", "-g", "2", "-a", "skip_train"])
    cfg = {"trainer": {"encoder_weights": "e.pth", "text_data": "t.txt", "print_dir": "p", "use_learning_schedule": "multi"},
           "model": {"pretrained_hwr": "h.pth", "pretrained_style": "s.pth"}, "data_loader": {"char_file": __file__, "batch_size": 2, "shuffle": True},
           "optimizer_type": "Adam"}
    cfg = new_eval.prepare_config(cfg, args)
    assert cfg["model"] == {"pretrained_hwr": None, "pretrained_style": None}
    assert cfg["optimizer_type"] == "none" and cfg["trainer"] == {"print_dir": None, "use_learning_schedule": False, "swa": False}
    assert cfg["data_loader"] == {"char_file": __file__, "batch_size": 3, "shuffle": False, "eval": True}
    assert cfg["validation"] == {"batch_size": 3, "shuffle": False, "eval": True}
    assert cfg["cuda"] is True and cfg["gpu"] == 2 and cfg["skip_train"] == "True"
