"""Sample sheets of GAN training (`trainer.print_dir`; reference: trainer/hw_with_style_trainer.py:164-172, 248-267, 992-1023).

Three pieces, each usable on its own:
  * PrintSchedule - WHEN a sheet is printed and under which name: the reference's counters restated, pure Python (no torch, no GPU);
  * SheetPrinter.enqueue - a printing iteration's extra work on the step's thread: the sheets are composed on the device
    (ops.sample_sheet), the discriminator's per-line means reduced there (ops.row_means), all of it in ONE byte buffer whose copy to the
    host starts on the copy stream (ops.AsyncFetch). No `.cpu()`, no `.item()`, no stream synchronisation;
  * the writer thread - waits for the copy, encodes the PNGs (zlib releases the GIL) and writes every file to a temporary name in the
    same directory, then renames it: a viewer of *_latest.png never reads half a file. At most one print is in flight.
"""
import os
import threading


class PrintSchedule:
    """The reference's print counters. step(lesson) is called once per curriculum iteration that is not skipped and answers "gen", "recon"
    or None; a printing iteration does not count `iter_to_print` down. name(typ, iteration) is the file name part of a print: the
    iteration number once per `serperate_print_every` iterations (per typ), otherwise "latest". Nothing of this is checkpointed (as in the
    reference): a resumed run counts from print_every again."""

    def __init__(self, print_every=100, serperate_print_every=2500):
        self.print_every = int(print_every)
        self.serperate_print_every = int(serperate_print_every)
        self.iter_to_print = self.print_every
        self.print_next_gen = False
        self.print_next_auto = False
        self.last_print = {}

    def step(self, lesson):
        if lesson is None:                    # an iteration without a curriculum (recogniser training): the counters are GAN-only
            return None
        if (self.iter_to_print <= 0 or self.print_next_gen) and "gen" in lesson:
            if self.iter_to_print > 0:
                self.print_next_gen = False
            else:
                self.print_next_auto = True
                self.iter_to_print = self.print_every
            return "gen"
        if (self.iter_to_print <= 0 or self.print_next_auto) and "auto" in lesson:
            if self.iter_to_print > 0:
                self.print_next_auto = False
            else:
                self.print_next_gen = True
                self.iter_to_print = self.print_every
            return "recon"
        self.iter_to_print -= 1
        return None

    def name(self, typ, iteration):
        if iteration - self.last_print.get(typ, 0) >= self.serperate_print_every:
            self.last_print[typ] = iteration
            return str(iteration)
        return "latest"


def _atomic_write(path, data):
    tmp = "%s.tmp%d" % (path, os.getpid())
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


def encode_png(sheet):
    """uint8 [Hs, Ws] numpy array -> the bytes of an 8-bit grey PNG (mode L). Level 1 of zlib: a sheet is looked at and overwritten"""
    import io

    from PIL import Image
    h, w = sheet.shape
    buf = io.BytesIO()
    Image.frombuffer("L", (w, h), sheet, "raw", "L", 0, 1).save(buf, format="PNG", compress_level=1)
    return buf.getvalue()


class SheetPrinter:
    def __init__(self, directory, print_every=100, serperate_print_every=2500, write=True, logger=None):
        self.directory = directory
        self.schedule = PrintSchedule(print_every, serperate_print_every)
        self.write = bool(write)              # data parallel: every rank runs the schedule and the launches, rank 0 alone fetches and writes
        self.logger = logger
        self.hook = None                      # tests: hook(typ, iteration, name, tensors) sees the device tensors that are printed
        self._thread = None
        self._error = None
        if self.write:
            os.makedirs(directory, exist_ok=True)

    # -- the step's thread -------------------------------------------------------------------------------------------------------------
    def enqueue(self, typ, iteration, images, text, disc=None, gt_images=None):
        """images / gt_images: device fp32 [B,1,H,W]; disc: the discriminator's predictions, one [N, n] device tensor per scale (typ "gen");
        text: the batch's lines. Returns the file name part."""
        import torch

        from .. import ops
        name = self.schedule.name(typ, iteration)
        images = images.detach().contiguous()
        gt_images = None if gt_images is None else gt_images.detach().contiguous()
        disc = [] if typ != "gen" or not disc else [d.detach().contiguous() for d in disc]
        if self.hook is not None:
            self.hook(typ, iteration, name, {"images": images, "gt_images": gt_images, "disc": disc, "text": list(text)})
        # one byte buffer: [sheet | gt sheet | means fp32 [scales][B]], every piece at a multiple of 4
        pieces, total = [], 0
        for t in (images, gt_images):
            if t is not None:
                hs, ws, _ = ops.sample_sheet_shape(t.shape[0], t.shape[2], t.shape[3])
                pieces.append((t, total, hs, ws))
                total += -(-hs * ws // 4) * 4
        B = len(text)
        rows = [min(B, d.shape[0]) for d in disc]
        means_at = total
        total += 4 * B * len(disc)
        buf = torch.empty((total,), dtype=torch.uint8, device=images.device)
        for t, at, hs, ws in pieces:
            ops.sample_sheet(t, out=buf[at:at + -(-hs * ws // 4) * 4])
        if disc:
            means = buf[means_at:].view(torch.float32)
            for s, d in enumerate(disc):
                ops.row_means(d, rows[s], out=means[s * B:s * B + rows[s]])
        if not self.write:
            return name
        self.wait()                           # at most one print in flight
        fetch = ops.AsyncFetch(buf)
        files = [("%s_samples_%s.png" % (typ, name), pieces[0][1:])]
        if gt_images is not None:
            files.append(("%s_gt_%s.png" % (typ, name), pieces[1][1:]))
        text_file = ("%s_text_%s.txt" % (typ, name), list(text), rows, means_at) if typ == "gen" else None
        self._thread = threading.Thread(target=self._run, args=(fetch, files, text_file), name="sample-sheets", daemon=True)
        self._thread.start()
        if self.logger is not None:
            self.logger.info("printing %s images, iter: %d", typ, iteration)
        return name

    def wait(self):
        """returns once the print in flight (if any) has left its files; raises what the writer thread raised"""
        t, self._thread = self._thread, None
        if t is not None:
            t.join()
        if self._error is not None:
            e, self._error = self._error, None
            raise RuntimeError("writing the sample sheets into %s failed" % self.directory) from e

    # -- the writer thread -------------------------------------------------------------------------------------------------------------
    def _run(self, fetch, files, text_file):
        try:
            host = fetch.get().numpy()
            for fname, (at, hs, ws) in files:
                _atomic_write(os.path.join(self.directory, fname), encode_png(host[at:at + hs * ws].reshape(hs, ws)))
            if text_file is not None:
                fname, text, rows, means_at = text_file
                B = len(text)
                means = host[means_at:means_at + 4 * B * len(rows)].view("float32").reshape(len(rows), B) if rows else None
                lines = []
                for i, t in enumerate(text):
                    if rows:
                        lines.append(t + "".join(", {}".format(float(means[s, i])) for s in range(len(rows)) if i < rows[s]) + "\n")
                    else:
                        lines.append(t + ("\n" if i + 1 < B else ""))
                _atomic_write(os.path.join(self.directory, fname), "".join(lines).encode("utf-8"))
        except BaseException as e:  # noqa: BLE001 - handed to the step's thread by wait()
            self._error = e
