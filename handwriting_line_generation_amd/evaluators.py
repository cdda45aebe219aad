"""Per-line evaluation of a trained model (reference: evaluators/hwdataset_eval.py:41-316, driven by new_eval.py): what the recogniser read
in every line with its CER / WER, and pictures - the real line above its reconstruction (the paper's figure), generated lines.

The reference downloads the fp32 tensors and builds every picture on the host with numpy and OpenCV. Here the tensors stay on the device
(run_gen(..., on_device=True)): the error rates are counted there (ops.ctc_error_rates), the pair pictures composed there (ops.eval_pairs,
captions drawn from a glyph atlas), generated lines quantised there (ops.lines_to_u8); finished 8-bit pictures cross to the host on the copy
stream (ops.AsyncFetch) and a writer thread encodes and writes them (temporary name, then rename).

HWDataset_eval(...) is the reference's call. It is begin(...) + finish(): begin() enqueues a batch's work and starts the fetches, finish()
reads them, prints, composes and hands the pictures to the writer. new_eval.py begins batch k + 1 before it finishes batch k, so one
batch's counts are read while the next batch runs.

`hook`: tests set it to hook(kind, names, tensors) and see the device tensors that went into every picture ("recon": image, recon,
captions, codes, atlas, lines, pictures, outDir; "gen": gen, pixels, outDir) and every scored batch ("pred": pred, gt)."""
import os
import queue
import threading

import numpy as np
import torch

from . import ops
from .trainer.sample_sheets import _atomic_write

hook = None

REFUSED_EVAL = {
    "spaced": "it opens no picture and no file in the reference either: it prints two index tensors per line; not built",
    "spacing": "it needs the spacing predictor of configs that are not shipped",
    "mask": "it opens a debugger and an OpenCV window in the reference; the shipped configs are noMask",
}
REFUSED_GET = ("recon_gt_mask", "recon_pred_space", "mask", "gen_mask")
KNOWN_GET = ("recon", "pred", "gen", "gen_img", "gen_image", "style", "author", "gt", "name", "spaced_label")


def check_to_eval(toEval):
    """raises ValueError with the reason for what is not built; returns toEval"""
    if toEval is None:
        return None
    if isinstance(toEval, str):
        if toEval in REFUSED_EVAL:
            raise ValueError("-e %s is refused: %s" % (toEval, REFUSED_EVAL[toEval]))
        raise ValueError("unkwon just: {}".format(toEval))
    for name in toEval:
        if name in REFUSED_GET:
            raise ValueError("-e %s is refused: the shipped configs are noMask, no mask is ever generated" % name)
        if name in REFUSED_EVAL:
            raise ValueError("-e [%s] is refused: %s" % (name, REFUSED_EVAL[name]))
        if name not in KNOWN_GET:
            raise ValueError("Unknown get [{}]".format(name))
    return toEval


def default_to_eval(trainer):
    """the reference's default calls a trainer.run that it does not ship: reconstruction and prediction where there is a generator"""
    from .trainer import AutoTrainer
    if isinstance(trainer, AutoTrainer) or getattr(trainer.model, "generator", None) is not None:
        return ["recon", "pred"]
    return ["pred"]


# ---- glyph atlas -------------------------------------------------------------------------------------------------------------------
GLYPH_W, GLYPH_H = 8, 14
_atlases = {}


def glyph_atlas(idx_to_char, device):
    """-> (atlas uint8 device tensor [G, GLYPH_H, GLYPH_W], {character: code}): printable ASCII plus the character set's one-code-point
    classes, drawn once per process with PIL's default font, white on level 0; text_codes maps anything else to '?'"""
    chars = [chr(c) for c in range(32, 127)]
    chars += sorted(c for c in set(idx_to_char.values()) if len(c) == 1 and c not in chars and c.isprintable())
    key = ("".join(chars), str(device))
    hit = _atlases.get(key)
    if hit is None:
        from PIL import Image, ImageDraw, ImageFont
        font = ImageFont.load_default()
        host = np.zeros((len(chars), GLYPH_H, GLYPH_W), dtype=np.uint8)
        for k, ch in enumerate(chars):
            cell = Image.new("L", (GLYPH_W, GLYPH_H), 0)
            ImageDraw.Draw(cell).text((0, 0), ch, fill=255, font=font)
            host[k] = np.asarray(cell)
        hit = _atlases[key] = (ops.h2d(host, device), {ch: k for k, ch in enumerate(chars)})
    return hit


def text_codes(text, codes_of):
    q = codes_of["?"]
    return [codes_of.get(ch, q) for ch in text]


# ---- writer thread -------------------------------------------------------------------------------------------------------------------
def encode_png(picture):
    """uint8 [h, w] (grey) or [h, w, 3] (RGB) numpy array -> the bytes of an 8-bit PNG"""
    import io

    from PIL import Image
    picture = np.ascontiguousarray(picture)
    mode = "L" if picture.ndim == 2 else "RGB"
    buf = io.BytesIO()
    Image.frombuffer(mode, (picture.shape[1], picture.shape[0]), picture, "raw", mode, 0, 1).save(buf, format="PNG", compress_level=1)
    return buf.getvalue()


class PictureWriter:
    """one thread: waits for a fetch, cuts the pictures out of its bytes, encodes and writes each under a temporary name, renames it"""

    def __init__(self, backlog=8):
        self.jobs = queue.Queue(maxsize=backlog)       # bounded: the evaluator cannot run away from the encoder
        self.thread = None
        self.error = None

    def add(self, fetch, files):
        """files: [(path, byte offset, shape)] inside the fetched uint8 buffer"""
        if self.thread is None:
            self.thread = threading.Thread(target=self._run, name="eval-pictures", daemon=True)
            self.thread.start()
        self.jobs.put((fetch, files))

    def _run(self):
        while True:
            job = self.jobs.get()
            if job is None:
                return
            if self.error is not None:
                continue
            try:
                fetch, files = job
                host = fetch.get().numpy()
                for path, at, shape in files:
                    _atomic_write(path, encode_png(host[at:at + int(np.prod(shape))].reshape(shape)))
            except BaseException as e:  # noqa: BLE001 - handed to the caller by wait()
                self.error = e

    def wait(self):
        """returns once every picture handed over has left its file; raises what the thread raised"""
        t, self.thread = self.thread, None
        if t is not None:
            self.jobs.put(None)
            t.join()
        if self.error is not None:
            e, self.error = self.error, None
            raise RuntimeError("writing the evaluation pictures failed") from e


writer = PictureWriter()


def wait():
    writer.wait()


# ---- the evaluator -------------------------------------------------------------------------------------------------------------------
class Pending:
    """a batch whose launches are enqueued; finish() -> (metrics, out) as HWDataset_eval"""

    def finish(self):
        config, instance, trainer, out, outDir = self.config, self.instance, self.trainer, self.out, self.outDir
        gt, names = instance["gt"], list(instance["name"])
        B = len(gt)
        toRet = {}
        if self.loss_fetch is not None:
            toRet.update(zip(self.loss_names, self.loss_fetch.get().tolist()))
        cer = pred_str = None
        if "pred" in out:
            cer, wer, pred_str = self.rates.result()
            index = self.aligned.result()[0] if hasattr(self.aligned, "result") else self.aligned
            index = index.cpu().numpy()
            from .utils import string_utils
            for b in range(B):
                col = index[:, b]
                keep = (col != 0) & np.concatenate(([True], col[1:] != col[:-1]))
                aligned = string_utils.label2str_single(col[keep].tolist(), trainer.idx_to_char, False)
                print("{} GT:      {}".format(names[b], gt[b]))
                print("{} aligned: {}".format(names[b], aligned))
                print("{} pred:    {}".format(names[b], pred_str[b]))
                if self.verbosity >= 3:
                    print(out["pred"][:, b].cpu().numpy())
            out["cer"], out["pred_str"] = cer, pred_str
            toRet["cer"] = _mean(cer)
            toRet["wer"] = _mean(wer)
            if "by_author" in config:
                for b, author in enumerate(instance["author"]):
                    toRet.setdefault("cer_" + author, []).append(cer[b])
        if outDir is not None:
            if "recon" in out and self.recon_picture:
                self._pair_pictures(names, cer, pred_str)
            gen = out.get("gen") if out.get("gen") is not None else out.get("gen_img")
            if "gen" in out or "gen_img" in out:
                if gen is None:
                    raise RuntimeError("no generated images for {}".format(names))
                self._gen_pictures(names, gen)
        if self.drop_recon:
            del out["recon"]
        return toRet, out

    def _pair_pictures(self, names, cer, pred_str):
        config, out = self.config, self.out
        image, recon = self.image, out["recon"].contiguous()
        lines = list(range(len(names)))
        if "cer_thresh" in config:
            if cer is None:
                raise ValueError("cer_thresh needs `pred` among what is evaluated")
            lines = [b for b in lines if not cer[b] < config["cer_thresh"]]
            if not lines:
                return
            if len(lines) < len(names):
                sel = ops.h2d(np.asarray(lines, dtype=np.int64), image.device)
                image, recon = image.index_select(0, sel), recon.index_select(0, sel)
        captions = codes = atlas = None
        if cer is not None:
            atlas, codes_of = glyph_atlas(self.trainer.idx_to_char, image.device)
            captions = ["CER: {:.3f}, T: {}".format(cer[b], pred_str[b]) for b in lines]
            codes = [text_codes(c, codes_of) for c in captions]
        pictures = ops.eval_pairs(image, recon, codes, atlas)
        if hook is not None:
            hook("recon", [names[b] for b in lines], {"image": image, "recon": recon, "captions": captions, "codes": codes, "atlas": atlas,
                                                       "lines": lines, "pictures": pictures, "outDir": self.outDir})
        _, Hp, Wp, _ = pictures.shape
        files = []
        for k, b in enumerate(lines):
            save = "{}_recon.png".format(names[b])
            if "cer_thresh" in config:
                save = "{:.3f}_".format(cer[b]) + save
            path = os.path.join(self.outDir, save)
            files.append((path, k * Hp * Wp * 3, (Hp, Wp, 3)))
            print("saved: " + path)
        writer.add(ops.AsyncFetch(pictures.view(-1)), files)

    def _gen_pictures(self, names, gen):
        gen = gen.contiguous()
        B, _, H, W = gen.shape
        pixels, offsets = ops.lines_to_u8(gen, [W] * B)
        if hook is not None:
            hook("gen", names, {"gen": gen, "pixels": pixels, "outDir": self.outDir})
        files = [(os.path.join(self.outDir, "gen_{}.png".format(names[b])), int(offsets[b]), (H, W)) for b in range(B)]
        writer.add(ops.AsyncFetch(pixels), files)


def _mean(values):
    total = 0
    for v in values:
        total += v
    return total / len(values)


def begin(config, instance, trainer, metrics, outDir=None, startIndex=None, toEval=None, verbosity=2):
    from .trainer import AutoTrainer
    p = Pending()
    p.config, p.trainer, p.outDir, p.verbosity = config, trainer, outDir, verbosity
    toEval = check_to_eval(toEval)
    if toEval is None:
        toEval = default_to_eval(trainer)
    gpu = trainer.gpu
    p.image = ops.h2d(instance["image"], gpu).contiguous()
    instance = dict(instance, image=p.image)           # the trainers upload what is not on the device yet: one upload serves both
    p.instance = instance
    p.drop_recon, p.recon_picture, p.aligned = False, True, None
    if isinstance(trainer, AutoTrainer):
        losses, out = trainer.run_gen(instance, list(toEval), on_device=True)
        out = {k: v.detach() for k, v in out.items() if v is not None}        # (no `pred` without a 'recog' loss)
    elif trainer.curriculum is None:
        pred, losses = trainer.run_hwr(instance)
        out = {"pred": pred.detach()}
    else:
        lesson = trainer.curriculum.getEval()
        get = list(toEval)
        wants_gen = any(n in get for n in ("gen", "gen_img", "gen_image")) or "gen" in lesson
        if "recon" not in get and "auto" in lesson and ("style" in get or (wants_gen and trainer.interpolate_gen_styles)):
            # the styles of the batch come out of the reconstruction pass (reference :556-567): asked for here, shown nowhere
            get.append("recon")
            p.drop_recon, p.recon_picture = True, False
        if "pred" in get and "spaced_label" not in get:
            get.append("spaced_label")
            p.aligned = True
        losses, out = trainer.run_gen(instance, lesson, get, on_device=True)
        if p.aligned:
            p.aligned = out.pop("spaced_label")
        elif "pred" in get:
            p.aligned = out["spaced_label"]
    p.out = out
    p.loss_names = list(losses)
    p.loss_fetch = ops.AsyncFetch(torch.stack([losses[n].detach().reshape(()) for n in p.loss_names])) if p.loss_names else None
    if "pred" in out:
        if hook is not None:
            hook("pred", list(instance["name"]), {"pred": out["pred"], "gt": list(instance["gt"])})
        if config.get("beam"):                 # `-a beam=K`: the text, and with it every rate below, is the prefix beam search's
            p.rates = ops.ctc_beam_error_rates(out["pred"], instance["gt"], trainer.idx_to_char, getattr(trainer, "casesensitive", True),
                                               beam=config["beam"])
        else:
            p.rates = ops.ctc_error_rates(out["pred"], instance["gt"], trainer.idx_to_char, getattr(trainer, "casesensitive", True))
        if p.aligned is None:
            p.aligned = ops.dtw_align_async(out["pred"].detach().contiguous(), instance["label"])
    return p


def HWDataset_eval(config, instance, trainer, metrics, outDir=None, startIndex=None, toEval=None, verbosity=2):
    """-> (dict of scalars and lists, out): the losses of the lesson, `cer` / `wer` (the batch's means) and with config['by_author'] the
    `cer_<author>` lists; `out` holds what was asked for (device tensors) plus `cer` and `pred_str` per line"""
    return begin(config, instance, trainer, metrics, outDir, startIndex, toEval, verbosity).finish()


AuthorHWDataset_eval = HWDataset_eval
AuthorRIMESLinesDataset_eval = HWDataset_eval
