"""The reference's checkpoints kept under tests/golden/ (ref_ckpt_*.pth.xz, made by tools/gen_golden_checkpoint.py), unpacked for a test
(not collected by pytest)."""
import lzma
import os

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def unpack(name, tmp_path):
    dst = os.path.join(str(tmp_path), "ref_ckpt_%s.pth" % name)
    with open(dst, "wb") as f:
        f.write(lzma.decompress(open(os.path.join(GOLD, "ref_ckpt_%s.pth.xz" % name), "rb").read()))
    return dst
