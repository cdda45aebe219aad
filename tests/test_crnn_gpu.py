"""GPU: the CRNN recogniser (model/cnn_lstm.py) end to end - forward against the project's fp64 restatement on the reference's recorded cases,
checkpoints, module gradients through a CTC loss, the pre-training trainer and the GAN trainer with a CRNN - and the CNN-only recogniser's
output bits, which this class's arrival must not change.

Tolerance rule (forward and gradients): err_hip = max|hip - fp64| <= 4 * max|float32 CPU - fp64| + 4 * 2^-24 * scale, the float32 CPU side
being the reference's recorded logits (forward) or torch float32 autograd of the same restatement with torch's own nn.LSTM (gradients).
Observed err_hip / bound on the MI355X (profiles/crnn_lstm.txt): forward 0.12 - 0.16 on the seven cases, gradients at most 0.25."""
import hashlib
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _crnn_ref
from _gpu_tidy import leave_nothing_behind, scrub  # noqa: F401  (leave_nothing_behind: module-scoped, autouse)
from _crnn_golden import GOLDENS, golden_case, seeded_sd

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def _build(c, dev, use_softmax=False):
    from handwriting_line_generation_amd.model.cnn_lstm import CRNN
    m = CRNN(c["nclass"], norm=c["norm"], use_softmax=use_softmax, pad=c["pad"])
    sd = seeded_sd(c["keys"], c["shapes"], c["wseed"])
    m.load_state_dict(sd, strict=True)
    return m.to(dev), sd


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_forward_against_fp64_on_the_golden_cases(cuda, path):
    c = golden_case(path)
    m, sd = _build(c, cuda)
    m.eval()
    x = torch.from_numpy(c["pixels"].astype(np.float32) / 127.5 - 1.0)
    with torch.no_grad():
        got = m(x.to(cuda)).cpu().double().numpy()
        sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
        ref = _crnn_ref.forward(sd64, x.double(), c["norm"], c["pad"]).numpy()
    err_hip, err_ref32, scale = float(np.abs(got - ref).max()), float(np.abs(c["logits"] - ref).max()), float(np.abs(ref).max())
    bound = 4 * err_ref32 + 4 * EPS * scale
    print("CRNNRATIO forward %s err_hip %.3e err_reference_fp32 %.3e scale %.3e ratio %.3f" % (os.path.basename(path), err_hip, err_ref32, scale, err_hip / bound))
    assert got.shape == c["logits"].shape and err_hip <= bound


def test_reference_format_checkpoint_round_trip(cuda, tmp_path):
    from handwriting_line_generation_amd.logger import load_checkpoint
    from handwriting_line_generation_amd.model.cnn_lstm import CRNN
    c = golden_case([p for p in GOLDENS if p.endswith("batch_nopad_w40.npz")][0])
    m, sd = _build(c, cuda, use_softmax=True)
    m.eval()
    x = torch.from_numpy(c["pixels"].astype(np.float32) / 127.5 - 1.0).to(cuda)
    with torch.no_grad():
        y = m(x)
    torch.save({"state_dict": {k: v.cpu() for k, v in m.state_dict().items()}}, str(tmp_path / "crnn.pth"))
    snap = load_checkpoint(str(tmp_path / "crnn.pth"))
    assert list(snap["state_dict"].keys()) == c["keys"]
    m2 = CRNN(c["nclass"], norm=c["norm"], use_softmax=True)
    m2.load_state_dict(snap["state_dict"], strict=True)
    m2.to(cuda).eval()
    with torch.no_grad():
        y2 = m2(x)
    assert torch.equal(y, y2) and bool(torch.isfinite(y).all())
    assert float((y.exp().sum(2) - 1).abs().max()) < 1e-5          # log-probabilities


def test_module_gradients_through_ctc(cuda):
    """CTC loss on W = 64, B = 2 (T = 14), group norm, eval mode (no dropout): loss and every parameter gradient against fp64 autograd of
    tests/_crnn_ref.py, float32 CPU autograd of the same restatement (torch's own nn.LSTM) as yardstick"""
    from handwriting_line_generation_amd import ops
    c = golden_case([p for p in GOLDENS if p.endswith("group_nopad_w64.npz")][0])
    m, sd = _build(c, cuda, use_softmax=True)
    m.eval()
    x = torch.from_numpy(c["pixels"].astype(np.float32) / 127.5 - 1.0)
    label = torch.tensor([[3, 7, 7, 12], [5, 1, 9, 0]], dtype=torch.int32)
    lens = [4, 3]
    pred = m(x.to(cuda))
    loss = ops.ctc_loss(pred, label, [pred.shape[0]] * 2, lens)
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    names = [k for k, _ in m.named_parameters()]

    def cpu_side(dtype):
        s = {k: (v.to(dtype).clone().requires_grad_(k in names) if v.dtype.is_floating_point else v) for k, v in sd.items()}
        lstm = None
        if dtype == torch.float32:
            lstm = torch.nn.LSTM(512, 512, bidirectional=True, num_layers=2).eval()
            lstm.load_state_dict({k[len("rnn.rnn."):]: v for k, v in sd.items() if k.startswith("rnn.rnn.")})
        p = _crnn_ref.forward(s, x.to(dtype), "group", use_softmax=True, torch_lstm=lstm)
        l = F.ctc_loss(p, label.long(), torch.full((2,), p.shape[0], dtype=torch.long), torch.tensor(lens), blank=0, reduction="mean")
        l.backward()
        g = {k: s[k].grad for k in names if not k.startswith("rnn.rnn.")}
        if lstm is not None:
            g.update({"rnn.rnn." + k: p_.grad for k, p_ in lstm.named_parameters()})
        else:
            g.update({k: s[k].grad for k in names if k.startswith("rnn.rnn.")})
        return float(l.detach()), g
    l64, g64 = cpu_side(torch.float64)
    l32, g32 = cpu_side(torch.float32)
    print("CRNNRATIO ctc loss hip %.7f fp32 %.7f fp64 %.7f" % (float(loss.detach()), l32, l64))
    assert abs(float(loss.detach()) - l64) <= 4 * abs(l32 - l64) + 4 * EPS * abs(l64)
    bad = []
    for k in names:
        r = g64[k].numpy()
        err_hip, err_32, scale = float(np.abs(got[k].double().numpy() - r).max()), float(np.abs(g32[k].double().numpy() - r).max()), float(np.abs(r).max())
        bound = 4 * err_32 + 4 * EPS * scale
        print("CRNNRATIO grad %s err_hip %.3e err_torch %.3e scale %.3e ratio %.3f" % (k, err_hip, err_32, scale, err_hip / max(bound, 1e-300)))
        if not err_hip <= bound:
            bad.append((k, err_hip, bound))
    assert not bad, bad


def _seed_all(s):
    torch.manual_seed(s); np.random.seed(s); random.seed(s)


def test_pretraining_trainer_steps_the_crnn(cuda, tmp_path):
    """the new config through the harness on synthetic lines (B = 2, W = 128), three iterations: finite losses, every LSTM parameter moved, and
    device_cer on / off give the same logs"""
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.harness import build_simple_trainer
    from handwriting_line_generation_amd.model.cnn_lstm import CRNN
    runs = []
    try:
        for device_cer in (False, True):
            rng.set_mode("device", seed=9)
            _seed_all(0)
            wd = tmp_path / ("on" if device_cer else "off")
            wd.mkdir()
            trainer, cfg = build_simple_trainer("iam_hwr_crnn", batch_size=2, width=128, label_len=5, workdir=str(wd))
            assert cfg["model"]["hwr"] == "CRNN batchnorm" and isinstance(trainer.model.hwr, CRNN)
            trainer.device_cer = device_cer
            before = {k: v.detach().clone() for k, v in trainer.model.named_parameters()}
            logs = [trainer._train_iteration(it) for it in range(3)] + [trainer.flush_log()]
            torch.cuda.synchronize()
            moved = {k: not torch.equal(v, before[k]) for k, v in trainer.model.named_parameters()}
            runs.append((logs, moved))
            scrub(trainer)
    finally:
        rng.set_mode("device")
    (logs_a, moved), (logs_b, _) = runs
    assert logs_a == logs_b
    assert all(np.isfinite(v) for log in logs_a for v in log.values()) and sum("loss" in log for log in logs_a) >= 3
    lstm = [k for k in moved if ".rnn.rnn." in k]
    assert len(lstm) == 16 and all(moved[k] for k in lstm), [k for k in lstm if not moved[k]]


def test_gan_trainer_with_a_frozen_crnn(cuda, tmp_path):
    """one 7-lesson cycle of the iam_gan curriculum at b2a2, width 128, label length 6 with a CRNN recogniser and skip_unused_grads: finite
    logs, the frozen recogniser's parameter gradients untouched, and a gradient that reaches the recogniser's input through it"""
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.harness import build_gan_trainer
    from handwriting_line_generation_amd.model.cnn_lstm import CRNN
    try:
        rng.set_mode("device", seed=1)
        _seed_all(0)
        trainer, _ = build_gan_trainer("iam_gan", 2, 2, width=128, label_len=6, workdir=str(tmp_path), hwr="CRNN batchnorm")
        assert isinstance(trainer.model.hwr, CRNN)
        trainer.skip_unused_grads = True
        for it in range(7):
            log = trainer._train_iteration(it)
            assert all(np.isfinite(v) for v in log.values()), (it, log)
        torch.cuda.synchronize()
        f = trainer.flat
        names = [n for n, _ in trainer.model.named_parameters()]
        touched = {names[pi]: bool(f.touched[k]) for k, pi in enumerate(f.order)}
        hwr = [k for k in touched if k.startswith("hwr.")]
        assert hwr and not any(touched[k] for k in hwr)
        if trainer.hwr_frozen:
            assert not any(p.requires_grad for p in trainer.model.hwr.parameters())
        img = torch.randn(2, 1, 64, 128, device=cuda).clamp_(-1, 1).requires_grad_(True)
        pred = trainer.model.hwr(img)
        pred.backward(torch.randn_like(pred))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(img.grad).all()) and float(img.grad.abs().max()) > 0
        assert not any(bool(f.touched[k]) for k, pi in enumerate(f.order) if names[pi].startswith("hwr."))      # still untouched
        del f
        scrub(trainer)
    finally:
        rng.set_mode("device")


# written down on the MI355X visit that ran the parent commit's tree and this one side by side (both gave these)
CNN_ONLY_PARENT_SHA = {"train": "2199db17d410b188c60b24a045a904d02c525c0977f4648e88efd688e144d093",
                       "eval": "cdac09265e917e35d0d4193b03d95aaa7c7b8f82c0fbd2d4c38480c64a29fb5b"}


def cnn_only_case_hashes(dev):
    """sha256 of the CNN-only recogniser's output bytes on one seeded case, train mode (batch statistics) and eval mode"""
    from oracle import torch_ref
    from handwriting_line_generation_amd.model import CNNOnlyHWR
    m = CNNOnlyHWR(80, norm="batch")
    m.load_state_dict(torch_ref.seeded_state_dict(m, 41))
    m.to(dev)
    x = torch.from_numpy(np.random.RandomState(17).rand(3, 1, 64, 200).astype(np.float32) * 2 - 1).to(dev)
    out = {}
    with torch.no_grad():
        for mode in ("train", "eval"):
            m.train(mode == "train")
            out[mode] = hashlib.sha256(m(x).cpu().numpy().tobytes()).hexdigest()
    return out


def test_cnn_only_recogniser_bits_are_the_parents(cuda):
    """the trunk code is now shared with the CRNN: CNNOnlyHWR's output on a seeded case must be bit-identical to the parent commit's (hashes
    recorded by running the parent commit's tree on the same MI355X visit)"""
    assert cnn_only_case_hashes(cuda) == CNN_ONLY_PARENT_SHA
