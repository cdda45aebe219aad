"""GPU: the figure actions of generate.py - `s` (stretch film), `r` (walk through writers' styles), `A` (a writer's mean style) - on the
fabricated IAM directory (oracle.collate_items.fake_iam, 8 pages: three writers in the validation split) and the reduced REFERENCE-written
GAN checkpoint of tests/golden, its spacer spread out as tests/test_generate_cli_gpu.py explains. The module-level hook of
handwriting_line_generation_amd.generate shows the device tensors behind the pictures."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _stretch_ref as ref
from _gpu_tidy import leave_nothing_behind  # noqa: F401
from _reference_checkpoint import unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 64


@pytest.fixture(scope="module")
def program(cuda, tmp_path_factory):
    """-> dict(dir, ckpt, cfg): the spread-out checkpoint and a config on the fabricated dataset, two lines per writer item"""
    from oracle import collate_items
    from handwriting_line_generation_amd.harness import CHAR_FILES
    from handwriting_line_generation_amd.logger import load_checkpoint
    d = tmp_path_factory.mktemp("gen_modes")
    root = str(d / "iam")
    os.makedirs(root)
    collate_items.fake_iam(root, n_pages=8, with_images=True)
    ck = load_checkpoint(unpack("gan", d))
    ck["state_dict"]["spacer.mean"] = torch.tensor([3.0, 1.0]).view_as(ck["state_dict"]["spacer.mean"])
    ck["state_dict"]["spacer.std"] = torch.tensor([1.5, 0.5]).view_as(ck["state_dict"]["spacer.std"])
    path = str(d / "gan.pth")
    torch.save(ck, path)
    cfg = ck["config"]
    cfg["data_loader"].update(data_dir=root, batch_size=2, num_workers=0, char_file=CHAR_FILES["iam"], augmentation=None, a_batch_size=2, max_width=640)
    cfg["validation"] = dict(cfg.get("validation", {}), batch_size=2, num_workers=0, augmentation=None, a_batch_size=2)
    cfg["trainer"]["save_dir"] = str(d / "saved")
    cfg["trainer"]["style_together"] = True           # (how the character-style extractor is used: one style per writer item)
    cfg_path = str(d / "gan.json")
    json.dump(cfg, open(cfg_path, "w"))
    return {"dir": d, "ckpt": path, "cfg": cfg_path}


class Hooked:
    """collects what generate.hook is shown; `reseed`: the device generator is re-seeded when the hook is called"""

    def __init__(self, reseed=None):
        self.calls, self.reseed = [], reseed

    def __call__(self, kind, tensors):
        from handwriting_line_generation_amd import rng
        self.calls.append((kind, tensors))
        if self.reseed is not None:
            torch.cuda.synchronize()
            rng.set_mode("device", seed=self.reseed)

    def of(self, kind):
        return [t for k, t in self.calls if k == kind]


def _main(argv, capsys, reseed=None):
    import generate as cli
    from handwriting_line_generation_amd import generate as G, rng
    hooked = Hooked(reseed)
    G.hook = hooked
    try:
        capsys.readouterr()
        cli.main(argv)
        torch.cuda.synchronize()
    finally:
        G.hook = None
        rng.set_mode("device")
    return capsys.readouterr().out, hooked


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "L"
        return np.asarray(im).copy()


def _valid_loader(program, test=False):
    import generate as cli
    return cli.dataset_loader(json.load(open(program["cfg"])), test)


def _u8(image):
    """lines_to_u8's arithmetic on a host fp32 image [H, W]"""
    return np.clip((np.float32(1) - image) * np.float32(127.5), 0, 255).astype(np.uint8)


def test_stretch_film(cuda, program, capsys):
    from handwriting_line_generation_amd import ops, rng
    from handwriting_line_generation_amd.generate import load_for_generation, stretch_scales
    out = str(program["dir"] / "s")
    text, hooked = _main(["-c", program["ckpt"], "-f", program["cfg"], "-d", out, "-g", "0", "-r", "choice=s,batch=1"], capsys, reseed=77)
    (shown,) = hooked.of("stretch")
    aligned = shown["aligned"].cpu().numpy()
    T, B = aligned.shape
    assert B == 2 and shown["aligned"].dtype == torch.int64 and len(shown["frames"]) == 79 and tuple(shown["style"].shape) == (B, 128)
    assert torch.equal(shown["style"][0], shown["style"][1])                      # one writer's style, expanded to the batch
    instance = [inst for k, inst in enumerate(_valid_loader(program)) if k == 1][0]
    assert len(instance["gt"]) == B and aligned.max() > 0 and T >= instance["label"].shape[0]
    # every frame's one-hot is the rule applied to the hooked alignment, in both layouts
    scales = stretch_scales()
    T_out = [ref.out_len(T, s) for s in scales]
    for k, s in enumerate(scales):
        want = ref.stretch(aligned, 80, s)
        assert np.array_equal(shown["frames"][k].cpu().numpy(), want), k
        assert np.array_equal(ops.nhwc_of(shown["frames"][k]).cpu().numpy()[:, 0], want.transpose(1, 0, 2)), k
    # lines x 79 pictures of height 64, 4 columns per step; the widths grow with T_out over the first segment
    names = sorted(f for f in os.listdir(out))
    assert names == sorted("gen%d_%d.png" % (b, i) for b in range(B) for i in range(79))
    pictures = {(b, i): _png(os.path.join(out, "gen%d_%d.png" % (b, i))) for b in range(B) for i in range(79)}
    for (b, i), px in pictures.items():
        assert px.shape == (H, 4 * T_out[i]), (b, i)
    widths = [pictures[0, i].shape[1] for i in range(12)]
    assert widths == sorted(widths) and widths[-1] > widths[0] and T_out[0] == T
    assert re.search(r"^lines %d  seconds " % (B * 79), text, flags=re.M)
    # frame 0 is the generator on the plain one-hot of the alignment: same seed, a model loaded here
    model, _, _ = load_for_generation(program["ckpt"], program["cfg"], gpu=0)
    try:
        rng.set_mode("device", seed=77)
        with torch.no_grad():
            plain = ops.onehot_both(ops.h2d(torch.from_numpy(aligned.astype(np.int32)), cuda), 80)
            image = model.generator(plain, shown["style"])
            pixels, offsets = ops.lines_to_u8(image, [image.shape[3]] * B)
        host = pixels.cpu().numpy()
        for b in range(B):
            want = host[offsets[b]:offsets[b + 1]].reshape(H, image.shape[3])
            assert np.array_equal(pictures[b, 0], want), b
            assert np.array_equal(want, _u8(image[b, 0].cpu().numpy()))
        assert pictures[0, 0].min() < 128 and not np.array_equal(pictures[0, 0], pictures[1, 0])          # real, distinct lines
    finally:
        rng.set_mode("device")


def test_film_of_the_recognisers_own_output(cuda, program):
    """trainer.use_hwr_pred_for_style: interpolate_horz is handed the recogniser's output [T,B,C] instead of an alignment - there is nothing
    to index, the frames are torch's F.interpolate of it on the device"""
    import torch.nn.functional as F
    from handwriting_line_generation_amd import generate as G
    model, _, _ = G.load_for_generation(program["ckpt"], program["cfg"], gpu=0)
    pred = torch.randn(12, 1, 80, generator=torch.Generator().manual_seed(3)).log_softmax(2).to(cuda)
    style = torch.randn(1, 128, generator=torch.Generator().manual_seed(4)).to(cuda)
    hooked = Hooked()
    G.hook = hooked
    try:
        with torch.no_grad():
            images = G.interpolate_horz(model, style, pred)
    finally:
        G.hook = None
    (shown,) = hooked.of("stretch")
    scales = G.stretch_scales()
    assert len(images) == len(shown["frames"]) == 79
    for k, s in enumerate(scales):
        want = F.interpolate(pred.permute(1, 2, 0), scale_factor=s, mode="linear").permute(2, 0, 1)
        assert torch.equal(shown["frames"][k], want) and tuple(images[k].shape) == (1, 1, H, 4 * ref.out_len(12, s))
    with pytest.raises(ValueError, match="one writer"):
        G.interpolate_horz(model, torch.cat([style, style]), pred)


def test_style_walk(cuda, program, capsys):
    out = str(program["dir"] / "r")
    text, hooked = _main(["-c", program["ckpt"], "-f", program["cfg"], "-d", out, "-g", "0",
                          "-r", "choice=r,num_styles=3,step=0.2,start=0,stride=1,text=hello"], capsys)
    (shown,) = hooked.of("walk")
    walk = [s.cpu() for s in shown["styles"]]
    assert len(walk) == 3 and all(tuple(s.shape) == (1, 128) for s in walk)
    assert not torch.equal(walk[0], walk[1]) and not torch.equal(walk[1], walk[2])
    names = sorted(os.listdir(out))
    assert names == sorted(["gen0_%d.png" % i for i in range(15)] + ["styles0.pth"])
    for i in range(15):
        px = _png(os.path.join(out, "gen0_%d.png" % i))
        assert px.shape[0] == H and px.shape[1] % 4 == 0 and px.shape[1] >= 8
        border = not (px[0].any() or px[-1].any() or px[:, 0].any() or px[:, -1].any())
        assert border == (i % 5 == 0), i                                          # the black frame on every fifth picture, and only there
        assert px[1:-1, 1:-1].any()
    styles = torch.load(os.path.join(out, "styles0.pth"))
    assert isinstance(styles, list) and len(styles) == 15
    k = 0
    for a in range(3):
        style1, style2 = walk[a], walk[(a + 1) % 3]
        for alpha in np.arange(0, 1.0, 0.2):
            want = style2 * alpha + (1 - alpha) * style1                          # the reference's expression (generate.py:821)
            assert not styles[k].is_cuda and tuple(styles[k].shape) == (1, 128)
            # two products and a sum, each rounded once to fp32 here as on the device; a device that fuses a product into the sum
            # rounds once less: at most one unit in the last place of the largest entry (2^-23 relative) apart
            assert torch.allclose(styles[k], want.float(), rtol=0, atol=2.0 ** -23 * float(want.abs().max())), k
            k += 1
    assert torch.equal(styles[0], walk[0]) and torch.equal(styles[5], walk[1]) and torch.equal(styles[10], walk[2])
    assert re.search(r"^lines 15  seconds ", text, flags=re.M)


def test_author_mean(cuda, program, capsys):
    from handwriting_line_generation_amd.generate import get_style, load_for_generation
    loader = _valid_loader(program)
    authors = [inst["author"][0] for inst in loader]
    author = max(set(authors), key=authors.count)                                 # the writer with the most batches (three)
    assert authors.count(author) >= 3
    out = str(program["dir"] / "A")
    text, hooked = _main(["-c", program["ckpt"], "-f", program["cfg"], "-d", out, "-g", "0",
                          "-r", "choice=A,author=%s,text=hello,max=2" % author], capsys)
    (shown,) = hooked.of("author")
    assert os.listdir(out) == ["gen_%s.png" % author]
    px = _png(os.path.join(out, "gen_%s.png" % author))
    assert px.shape[0] == H and px.shape[1] % 4 == 0 and px.min() < 128
    model, config, _ = load_for_generation(program["ckpt"], program["cfg"], gpu=0)
    with torch.no_grad():
        mine = [get_style(config, model, inst, cuda) for inst in loader if inst["author"][0] == author][:2]
    assert len(mine) == 2 and len(shown["styles"]) == 2
    for a, b in zip(shown["styles"], mine):
        assert torch.equal(a, b)
    want = torch.cat(mine, dim=0).mean(dim=0)[None]
    assert tuple(shown["style"].shape) == (1, 128) and torch.equal(shown["style"], want)
    assert not torch.equal(mine[0], mine[1])
    # a writer the split does not hold
    import generate as cli
    with pytest.raises(SystemExit) as e:
        cli.main(["-c", program["ckpt"], "-f", program["cfg"], "-d", out, "-g", "0", "-r", "choice=A,author=nobody"])
    assert "no line of writer 'nobody'" in str(e.value.code)


def test_program_in_a_child_process(cuda, program):
    """the test split through -T (one line per batch), sharded output"""
    import generate as cli
    out = str(program["dir"] / "child")
    r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, os.path.join(ROOT, "generate.py"), "-c", program["ckpt"], "-f", program["cfg"],
                        "-d", out, "-g", "0", "-T", "--shard", "50", "-r", "choice=s"], cwd=str(program["dir"]), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "changed a_batch_size to 1" in r.stdout
    assert re.search(r"^lines 79  seconds \S+  lines/s \S+$", r.stdout, flags=re.M), r.stdout[-2000:]
    assert sorted(os.listdir(out)) == ["lines_00000.npz", "lines_00001.npz"]
    lines = cli.read_shard(os.path.join(out, "lines_00000.npz")) + cli.read_shard(os.path.join(out, "lines_00001.npz"))
    assert [i for i, _ in lines] == list(range(79))
    widths = [l.shape[1] for _, l in lines]
    T = widths[0] // 4
    assert widths == [4 * ref.out_len(T, s) for s in ref.film_scales()]
