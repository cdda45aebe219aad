"""How the module tests run the oracle restatement (oracle/) per case (not collected by pytest): the oracle's forward and the inputs that
take a gradient per network, the product's module class for its parameter names, the fp64 evaluation of the oracle's gradients with the
conditioning probe, and the relative error measure. tests/test_oracle_golden.py pins the oracle to the reference's goldens with them,
tests/test_modules_gpu.py compares the HIP path with the oracle."""
import os

import torch

from oracle import cases, torch_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")


class _ByKind(dict):
    """case name -> entry of the network it exercises (the RIMES cases reuse their base case's definitions)"""

    def __getitem__(self, name):
        return dict.__getitem__(self, cases.kind(name))


ORACLE_FWD = _ByKind({
    "generator": lambda sd, i: [torch_ref.generator(sd, i["content"], i["style"])],
    "discriminator": lambda sd, i: torch_ref.discriminator(sd, i["x"]),
    "hwr": lambda sd, i: [torch_ref.hwr(sd, i["image"])],
    "spacer": lambda sd, i: [torch_ref.spacer(sd, i["onehot"], i["style"])],
    "style_extractor": lambda sd, i: [torch_ref.style_extractor(sd, i["x"], i["recog"])],
    "encoder2": lambda sd, i: list(torch_ref.encoder2(sd, i["x"])),
    "decoder": lambda sd, i: [torch_ref.decoder_noskip(sd, i["x"])],
    "e_hwr": lambda sd, i: [torch_ref.e_hwr(sd, i["x"])],
})
GRAD_INPUTS = _ByKind({"generator": ["style"], "discriminator": ["x"], "hwr": ["image"], "spacer": ["style"], "style_extractor": ["recog"],
                       "encoder2": ["x"], "decoder": ["x"], "e_hwr": ["x"]})


def product_module(name):
    """the product's module class, used here on CPU only for its parameter names/shapes (no forward is run)"""
    from handwriting_line_generation_amd import model as M
    cls = dict(generator=M.SpacedGenerator, discriminator=M.DiscriminatorAP, hwr=M.CNNOnlyHWR, spacer=M.CountCNN,
               style_extractor=M.CharStyleEncoder, encoder2=M.Encoder2, decoder=M.DecoderNoSkip, e_hwr=M.E_HWR)[cases.kind(name)]
    return cls(**cases.CASES[name]["ctor"])


def rel(a, b):
    a = torch.as_tensor(a).double(); b = torch.as_tensor(b).double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


PERTURB = 1e-6      # relative size of the conditioning probe: what fp32 kernels of different summation order differ by at intermediate layers


def _oracle_grads64(name, sd, pnames, ws, loss_fn=None, inputs=None, perturb=None):
    """parameter and input gradients of the oracle evaluated in fp64 with the draws of the fp32 run (noise is drawn in fp32 and widened;
    Dropout2d's Bernoulli masks do not depend on the dtype)"""
    sd64 = {k: (v.detach().double() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    for k in pnames:
        sd64[k].requires_grad_(True)
    oin = inputs if inputs is not None else cases.inputs(name)
    oin = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in oin.items()}
    if perturb is not None:   # fp32-rounding sized relative noise on every continuous input and weight: probes how well conditioned the gradients are
        g = torch.Generator().manual_seed(perturb)
        oin = {k: (v * (1 + PERTURB * torch.randn(v.shape, generator=g, dtype=torch.float64)) if v.dtype.is_floating_point else v) for k, v in oin.items()}
        for k in pnames:
            with torch.no_grad():
                sd64[k].mul_(1 + PERTURB * torch.randn(sd64[k].shape, generator=g, dtype=torch.float64))
    for k in GRAD_INPUTS[name]:
        oin[k] = oin[k].clone().requires_grad_(True)
    rl, rn = torch.randn_like, torch.randn
    torch.randn_like = lambda t, **kw: rl(t.to(torch.float32), **kw).double()
    torch.manual_seed(cases.FWD_SEED)
    try:
        outs = ORACLE_FWD[name](sd64, oin)
    finally:
        torch.randn_like = rl
    if loss_fn is None:
        sum((o * w.double()).sum() for o, w in zip(outs, ws)).backward()
    else:
        loss_fn(outs).backward()
    return {k: sd64[k].grad for k in pnames}, {k: oin[k].grad for k in GRAD_INPUTS[name]}
