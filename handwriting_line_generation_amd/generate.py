"""Batched generation loop (reference: generate.py:48-83 `generate()` -> `model(label, label_lengths, style)`).

`HWWithStyle.forward` has one host round trip in the middle: the spacer's predicted blank / duplicate counts go to the host, where
`insert_spaces` expands the text with numpy noise, and the expanded content comes back for the generator. Called request by request
the GPU idles during that round trip. `generate_stream` overlaps it: the spacer of request i+1 is enqueued (and its counts start
travelling to the host on the copy stream) before request i is rendered, so the host never waits for the GPU and the GPU always has
the next generator pass queued. Per request the kernels, their order within the request and the RNG draws are those of
`model(label, label_lengths, style)`; with the reference's host RNG the outputs are identical to calling the model in sequence.
"""
import numpy as np
import torch

from . import ops, rng
from .utils import string_utils


def _begin(model, label, label_lengths, style):
    """enqueue the spacer of one request and start the device->host copy of its counts"""
    counts = model.spacer(model.onehot(label), style)
    if rng.mode() == "device":      # device generator: the expansion plan is drawn on the GPU, only the expanded lengths come back
        return model.insert_spaces_device(label, label_lengths, counts, begin_only=True)
    return ops.AsyncFetch(counts)


def _render(model, label_host, label_lengths, style, fetch, device):
    if isinstance(fetch, tuple):
        idx, padded = rng.device_rng().insert_spaces_finish(fetch)
        spaced = model.onehot(idx)
    else:
        counts = fetch.get()
        idx, padded = model.insert_spaces_index(label_host, label_lengths, counts)
        spaced = model.onehot(ops.h2d(idx.astype(np.int32), device))
    spaced = model._clip_spaced(spaced)
    return model.generator(spaced, style), padded


def generate_stream(model, requests, device=None):
    """requests: iterable of (label [L,B] int tensor (host or device), label_lengths, style [B,style_dim] device tensor).
    Yields (image NCHW [B,1,64,W], padded fractions) per request, in order. Inference only (call under torch.no_grad())."""
    pending = None
    for label, label_lengths, style in requests:
        device = device or style.device
        label_host = label.cpu() if label.is_cuda else label
        label_dev = label if label.is_cuda else ops.h2d(label, device)
        fetch = _begin(model, label_dev, label_lengths, style)
        if pending is not None:
            yield _render(model, *pending, device)
        pending = (label_host, label_lengths, style, fetch)
    if pending is not None:
        yield _render(model, *pending, device)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's generation helpers (generate.py:48-83, 796-828), same names and arguments
def get_style(config, model, instance, gpu=None):
    """style vector(s) of the lines in `instance`. With `trainer.style_together` (how the shipped character-style models are used) all
    lines of one author are laid side by side - image columns and recogniser time steps alike - and go through the style extractor once:
    recogniser -> (its own log-probs | DTW alignment of the text, one-hot) -> collapse per author -> CharStyleEncoder; returns
    [authors, style_dim]. Without it the extractor sees the raw batch and the first line's style is returned (generate.py:66-67)."""
    if "lookup" in config["model"].get("style", "") or "Lookup" in config["model"].get("style", ""):
        raise NotImplementedError("author-lookup styles are not used by any shipped config")
    tr = config.get("trainer", {})
    image, label = instance["image"], instance["label"]
    if gpu is not None:
        image = ops.h2d(image, gpu) if not image.is_cuda else image
        label = ops.h2d(label, gpu) if not label.is_cuda else label
    if not tr.get("style_together", False):
        style = model.style_extractor(image)          # (a character-style extractor needs the recogniser output: TypeError, as in the reference)
        return style[0:1]
    old = model.use_hwr_pred_for_style
    model.use_hwr_pred_for_style = bool(tr.get("use_hwr_pred_for_style", False))
    try:
        model.pred = model.spaced_label = model.spaced_label_index = None
        a_batch_size = instance.get("a_batch_size", image.shape[0])
        style = model.extract_style(image, label, a_batch_size)      # [B, style_dim], every author's style repeated for its lines
        return style[::a_batch_size].contiguous()
    finally:
        model.use_hwr_pred_for_style = old
        model.pred = model.spaced_label = model.spaced_label_index = None


def _text_label(text, char_to_idx, batch_size, gpu):
    label = string_utils.str2label_single(text, char_to_idx)
    label = torch.from_numpy(label.astype(np.int32))[:, None].expand(-1, batch_size).contiguous()
    return ops.h2d(label, gpu)


def generate(model, style, text, char_to_idx, gpu):
    """one image of `text` in `style` ([1, style_dim]) -> NCHW [1,1,64,W]"""
    label = _text_label(text, char_to_idx, 1, gpu)
    return model(label, torch.IntTensor(1).fill_(label.size(0)), style)


def interpolate(model, style1, style2, text, char_to_idx, gpu, step=0.05):
    """images of `text` while the style moves from style1 to style2 in steps of `step` -> (list of images, list of styles on the host)"""
    batch_size = style1.size(0)
    label = _text_label(text, char_to_idx, batch_size, gpu)
    label_len = torch.IntTensor(batch_size).fill_(len(text))
    results, styles = [], []
    for alpha in np.arange(0, 1.0, step):
        style = (style2 * float(alpha) + float(1 - alpha) * style1).contiguous()
        results.append(model(label, label_len, style))
        styles.append(style.cpu().detach())
    return results, styles


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's figure actions: `s` stretch film, `r` walk through writers' styles, `A` a writer's mean style
# `hook`: tests set it to hook(kind, tensors) and see the device tensors behind the pictures - "stretch": aligned (the index [T,B], or the
# recogniser's output [T,B,C]), frames (the list of one-hots the generator was given), style; "walk": styles (list of [1, style_dim]);
# "author": styles (list of [1, style_dim]), style (their mean [1, style_dim])
hook = None


def stretch_scales():
    """the 79 horizontal scale factors of the reference's stretch film (generate.py:834-851), built from the same np.arange calls so that the
    float drift of the steps is the reference's: 12 from arange(1, 1.11, .01), 12 repeats of the last, 22 from arange(1.1, .89, -.01), 22 repeats
    of the last, 11 from arange(.9, 1.01, .01). The repeats are the reference's two "vertical" loops: they change nothing and render the label
    of the loop before them again, with fresh generator noise - kept, so that the film has the reference's frames."""
    wider, narrower, back = np.arange(1, 1.11, 0.01), np.arange(1.1, 0.89, -0.01), np.arange(0.9, 1.01, 0.01)
    scales = [float(s) for s in wider] + [float(wider[-1])] * len(np.arange(1, 1.11, 0.01))
    scales += [float(s) for s in narrower] + [float(narrower[-1])] * len(np.arange(1.1, 0.89, -0.01))
    return scales + [float(s) for s in back]


def interpolate_horz(model, style, aligned):
    """the reference's interpolate_horz (generate.py:830-852): the line(s) behind `aligned` rendered once per stretch_scales() entry, the
    character spacing stretched and squeezed along the line -> list of 79 images NCHW [B,1,64,4 T_out]. `aligned`: the DTW-aligned class
    indices int [T,B] on the device (correct_pred) - ONE ops.stretch_onehot launch makes all 79 interpolated one-hots, in the layout the
    generator reads - or the recogniser's own output, float [T,B,C] (trainer.use_hwr_pred_for_style): nothing to index, the frames are
    torch's F.interpolate on the device, as in the reference. `style`: one writer's, [1, style_dim], expanded to the batch. The generator is
    called directly (no _clip_spaced), as the reference does."""
    if style.numel() != style.shape[-1]:
        raise ValueError("interpolate_horz: the style must be one writer's, [1, style_dim], got %s" % (tuple(style.shape),))
    B = aligned.shape[1]
    style = style.reshape(1, -1).expand(B, -1).contiguous()
    scales = stretch_scales()
    if aligned.dim() == 2:
        frames = ops.stretch_onehot(aligned.to(torch.int32).contiguous(), model.num_class, scales)
    else:
        import torch.nn.functional as F
        orig = aligned.permute(1, 2, 0)
        frames, last = [], None
        for k, s in enumerate(scales):
            if last is None or s != scales[k - 1]:
                last = F.interpolate(orig, scale_factor=s, mode="linear").permute(2, 0, 1).contiguous()
            frames.append(last)
    if hook is not None:
        hook("stretch", {"aligned": aligned, "frames": frames, "style": style})
    return [model.generator(frame, style) for frame in frames]


def _writer_style(model, config, instance, gpu):
    """model.extract_style(image, label, a_batch_size)[::a_batch_size] of one batch (generate.py:320-323, 515-518) -> [writers, style_dim];
    the extractor's cached recogniser output and alignment are cleared around the call, and it reads the recogniser's prediction or the
    aligned text as trainer.use_hwr_pred_for_style says (as get_style does)"""
    image, label = instance["image"], instance["label"]
    if gpu is not None:
        image = image if image.is_cuda else ops.h2d(image, gpu)
        label = label if label.is_cuda else ops.h2d(label, gpu)
    a_batch_size = instance["a_batch_size"]
    old = model.use_hwr_pred_for_style
    model.use_hwr_pred_for_style = bool(config.get("trainer", {}).get("use_hwr_pred_for_style", False))
    try:
        model.pred = model.spaced_label = model.spaced_label_index = None
        return model.extract_style(image, label, a_batch_size)[::a_batch_size].contiguous()
    finally:
        model.use_hwr_pred_for_style = old
        model.pred = model.spaced_label = model.spaced_label_index = None


def walk_batches(loader, num_styles, rand, start=None, stride=None):
    """the batches the reference's `r` action takes its styles from (generate.py:314-329), as (i, instance): the first at index
    rand.randint(0, 20) (`start` when given), then every batch with i >= index whose writer differs from the last one taken, after which
    index += rand.randint(20, 50) (`stride` when given; the draw is not made then); stops after the batch at which num_styles are reached."""
    index = rand.randint(0, 20) if start is None else int(start)
    last_author, taken = None, 0
    for i, instance in enumerate(loader):
        author = instance["author"][0]
        if i >= index and author != last_author:
            yield i, instance
            taken += 1
            last_author = author
            index += rand.randint(20, 50) if stride is None else int(stride)
        if taken >= num_styles:
            break


def walk_styles(loader, model, config, num_styles, rand, gpu, start=None, stride=None):
    """the styles of the reference's `r` action: one [1, style_dim] per batch walk_batches selects. Fewer than 2 is a SystemExit."""
    seen = [0]

    def counted():
        for instance in loader:
            seen[0] += 1
            yield instance
    styles = [_writer_style(model, config, instance, gpu) for _, instance in walk_batches(counted(), num_styles, rand, start, stride)]
    if len(styles) < 2:
        raise SystemExit("generate.py: choice=r walks between the styles of at least 2 writers, found %d in the %d batches of the split "
                         "(start / stride reach fewer batches than it holds?)" % (len(styles), seen[0]))
    if hook is not None:
        hook("walk", {"styles": styles})
    return styles


def walk_film(model, styles, text, char_to_idx, gpu, step=0.1):
    """the closed walk (generate.py:335-341): interpolate(styles[i], styles[i + 1]) for every neighbour pair, then from the last back to the
    first -> (list of images, list of the host styles of every frame)"""
    images, frame_styles = [], []
    for k in range(len(styles)):
        b_im, b_sty = interpolate(model, styles[k], styles[(k + 1) % len(styles)], text, char_to_idx, gpu, step)
        images += b_im
        frame_styles += b_sty
    return images, frame_styles


def author_mean_style(loader, model, config, author, gpu, max_hits=5):
    """the style of the reference's `A` action (generate.py:511-523): the mean over the styles of the first `max_hits` batches of writer
    `author` -> [1, style_dim]. A writer the split does not hold is a SystemExit."""
    styles, seen = [], 0
    for i, instance in enumerate(loader):
        seen = i + 1
        if str(instance["author"][0]) == str(author):
            print("{} found on instance {}".format(author, i), flush=True)
            styles.append(_writer_style(model, config, instance, gpu))
            if len(styles) >= max_hits:
                break
    if not styles:
        raise SystemExit("generate.py: choice=A found no line of writer %r in the %d batches of the split" % (author, seen))
    style = torch.cat(styles, dim=0).mean(dim=0)[None, ...].contiguous()
    if hook is not None:
        hook("author", {"styles": styles, "style": style})
    return style


# ---------------------------------------------------------------------------------------------------------------------------------
# from a checkpoint to pictures: what the reference's `generate.py -c ... -d ... -s ...` program does around the calls above
def apply_add_to_config(config, adds):
    """the reference's `-a` rule (generate.py:116-136): every entry [k1, ..., kn, value] sets config[k1]...[kn] = value, the value coerced
    to int, else float, else kept as text; an empty value is None"""
    for add in adds or []:
        if len(add) < 2:
            raise ValueError("config addition %r: expected key=value (nested: key=key=value)" % "=".join(add))
        target = config
        for key in add[:-2]:
            target = target[key]
        value = add[-1]
        if value == "":
            value = None
        else:
            try:
                value = int(value)
            except ValueError:
                try:
                    value = float(value)
                except ValueError:
                    pass
        target[add[-2]] = value
    return config


def load_for_generation(checkpoint_path, config_path=None, gpu=0, add_to_config=None, checkpoint=None, averaged=False):
    """-> (model, config, char_to_idx) for a checkpoint of this package or of the reference (generate.py:88-106, 187-209): the model alone, in
    eval mode on `gpu` - no trainer, no optimizer, no data loader. `style_from_normal*` weights are dropped and `pretrained*` entries of the
    config cleared as the reference does; `checkpoint`: the file's contents where the caller has read it already; `add_to_config` entries (apply_add_to_config) are applied before the model is built; a `data_loader.char_file` that does not exist falls back to the packaged file of that name.
    `averaged`: load the averaged weights that a run with trainer.swa / trainer.weight_averaging wrote (`swa_state_dict`, the reference's key)
    instead of the live ones; a checkpoint without them is a KeyError naming the key."""
    import json
    import os
    from . import model as models
    from .logger import load_checkpoint
    if checkpoint is None:
        checkpoint = load_checkpoint(checkpoint_path)
    if averaged and checkpoint.get("swa_state_dict") is None:
        raise KeyError("averaged weights asked for, but the checkpoint %s has no 'swa_state_dict' (it was not written by a run with "
                       "trainer.swa / trainer.weight_averaging, or averaging had not started yet)" % (checkpoint_path,))
    state = {k: v for k, v in checkpoint["swa_state_dict" if averaged else "state_dict"].items() if "style_from_normal" not in k}
    if config_path is None:
        config = checkpoint["config"]
    else:
        with open(config_path) as f:
            config = json.load(f)
    for key in config:
        if "pretrained" in key:
            config[key] = None
    config["model"]["RUN"] = True        # (a missing model.pretrained_hwr file is not an error: the state dict carries the recogniser)
    config["cuda"], config["gpu"] = True, gpu
    apply_add_to_config(config, add_to_config)
    arch = config.get("arch", "HWWithStyle")
    if arch != "HWWithStyle":
        raise NotImplementedError("generation needs an HWWithStyle checkpoint, this one holds %r" % arch)
    model = getattr(models, arch)(config["model"])
    model.load_state_dict(state)
    model = model.to(torch.device("cuda", gpu) if isinstance(gpu, int) else gpu)
    model.eval()
    char_file = config["data_loader"]["char_file"]
    if not os.path.exists(char_file):
        char_file = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", os.path.basename(char_file))
    with open(char_file) as f:
        char_to_idx = json.load(f)["char_to_idx"]
    return model, config, char_to_idx


def read_style_image(path, img_height=64):
    """one line image as the reference's `f` action reads it (generate.py:655-663): grey, resized bicubic to `img_height` rows when it has
    another height (PIL here, OpenCV there), 1 - x / 128 -> float32 [1, H, W] on the host"""
    from PIL import Image
    im = Image.open(path).convert("L")
    if im.size[1] != img_height:
        percent = float(img_height) / im.size[1]
        im = im.resize((max(int(round(im.size[0] * percent)), 1), img_height), Image.BICUBIC)
    return torch.from_numpy(1.0 - np.asarray(im, dtype=np.float32)[None] / 128.0)


def style_from_images(model, paths, gpu):
    """style vectors [n, style_dim] of the line images at `paths` (the reference's `f` action, generate.py:653-686): all cropped to the
    narrowest one, stacked, one extract_style(stack, None, 1) call. Without a label there is nothing to align, so the extractor reads the
    recogniser's own prediction for the call."""
    images = [read_style_image(p, model.image_height) for p in paths]
    min_width = min(im.shape[2] for im in images)
    stack = ops.h2d(torch.stack([im[:, :, :min_width] for im in images], dim=0).contiguous(), gpu)
    old = model.use_hwr_pred_for_style
    model.use_hwr_pred_for_style = True
    try:
        model.pred = model.spaced_label = model.spaced_label_index = None
        with torch.no_grad():
            return model.extract_style(stack, None, 1)
    finally:
        model.use_hwr_pred_for_style = old
        model.pred = model.spaced_label = model.spaced_label_index = None


def load_style_file(style_loc):
    """the style pickle(s) evaluate.dump_styles / the reference's get_styles.py write -> {author: [style, ...]} (generate.py:215-239:
    `style_loc` is a prefix, every file matching style_loc + '*' is read, with or without the `ids` entry). Authors keep the order in which
    the (sorted) files name them, so that a seed reproduces."""
    import pickle
    from glob import glob
    if not style_loc.endswith("*"):
        style_loc += "*"
    files = sorted(glob(style_loc))
    if not files:
        raise FileNotFoundError("no style file matches %r" % style_loc)
    styles = {}
    for loc in files:
        with open(loc, "rb") as f:
            data = pickle.load(f)
        for i, author in enumerate(data["authors"]):
            styles.setdefault(author, []).append(np.asarray(data["styles"][i]))
    return styles


def sample_styles(styles_by_author, n, rand):
    """n styles drawn as the reference's `R` action draws them (generate.py:385-405): per instance choice(authors), randint(0, len - 1),
    choice(authors), randint(0, len - 1), random() from `rand` (a random.Random), inter = 2 r - 0.5 (extrapolates a quarter beyond either end),
    style = s1 * inter + s2 * (1 - inter) -> float32 [n, style_dim] on the host"""
    authors = list(styles_by_author.keys())
    out = []
    for _ in range(n):
        a = rand.choice(authors)
        s1 = styles_by_author[a][rand.randint(0, len(styles_by_author[a]) - 1)]
        b = rand.choice(authors)
        s2 = styles_by_author[b][rand.randint(0, len(styles_by_author[b]) - 1)]
        inter = 2 * rand.random() - 0.5
        out.append(np.asarray(s1 * inter + s2 * (1 - inter), dtype=np.float32).reshape(-1))
    return np.stack(out) if out else np.zeros((0, 0), dtype=np.float32)


def bucket_by_length(texts, char_to_idx, batch_lines=64):
    """-> (batches, skipped): `batches` a list of (label length, [text indices]) in which every batch holds only texts that encode to the
    same number of labels (characters missing from `char_to_idx` are dropped first, as str2label_single drops them), at most `batch_lines`
    of them, lengths in order of first appearance; `skipped` the indices of texts that encode to no label at all."""
    if batch_lines < 1:
        raise ValueError("batch_lines must be at least 1")
    by_len, skipped = {}, []
    for i, text in enumerate(texts):
        n = len(string_utils.str2label_single(text, char_to_idx))
        if n == 0:
            skipped.append(i)
        else:
            by_len.setdefault(n, []).append(i)
    batches = []
    for n, idx in by_len.items():
        batches.extend((n, idx[k:k + batch_lines]) for k in range(0, len(idx), batch_lines))
    return batches, skipped


def line_widths(padded, image_width):
    """columns of each line of a batch that are its own: 4 * (T - round(padded[b] * T)) with T = image_width / 4 content steps, clamped to
    [4, image_width] (`padded`: the blank-tail fractions generate_stream yields)"""
    T = image_width // 4
    return [min(max(4 * (T - int(round(p * T))), 4), image_width) for p in padded]


def _bucket_requests(texts, styles, char_to_idx, batches, gpu):
    for n, idx in batches:
        label = np.stack([string_utils.str2label_single(texts[i], char_to_idx).astype(np.int32) for i in idx], axis=1)
        style = styles[torch.as_tensor(idx, dtype=torch.long, device=styles.device)]
        yield torch.from_numpy(label), torch.IntTensor(len(idx)).fill_(n), ops.h2d(style.contiguous(), gpu)


def render_lines_device(model, texts, styles, char_to_idx, gpu, batch_lines=64, skipped=None, spacing_noise=False):
    """Generator over (text indices, pixels, offsets, widths) per bucket, nothing fetched: `pixels` a uint8 1-D DEVICE tensor in which line b
    of the bucket - text indices[b] in style styles[indices[b]] - is the finished 64 x widths[b] picture pixels[offsets[b]:offsets[b + 1]]
    (`offsets` host int64 [n + 1], `widths` a host list), the bytes the reference writes (generate.py:426), cut to the line's own width.

    Lines are batched BY LABEL LENGTH (bucket_by_length): the spacer convolves over the label axis, and a shorter line's padding labels
    (class 0 one-hot, not zeros) would reach into its last characters; with equal lengths no line sees another's padding, so a line's
    spacing depends on its own text and style only. The batches go through generate_stream; each image is converted and packed ragged on
    the GPU (ops.lines_to_u8). count_std / dup_std are 0 for the duration (generate.py:199-200; `spacing_noise`: the model's values stay)
    and restored when the generator ends or is closed. Texts that encode to no label are skipped with a warning (their indices are appended to `skipped` when a list is given)."""
    import logging
    styles = torch.as_tensor(styles)
    batches, skip = bucket_by_length(texts, char_to_idx, batch_lines)
    if skip:
        logging.getLogger("generate").warning("render_lines: %d text(s) hold no character of the character set, skipped: %s", len(skip), skip)
        if skipped is not None:
            skipped.extend(skip)
    std = (model.count_std, model.dup_std)
    if not spacing_noise:
        model.count_std = model.dup_std = 0
    try:
        stream = generate_stream(model, _bucket_requests(texts, styles, char_to_idx, batches, gpu), gpu)
        for _, idx in batches:
            with torch.no_grad():           # (not around the yield: a suspended generator would leave the caller's gradients off)
                image, padded = next(stream)
                widths = line_widths(padded, image.shape[3])
                pixels, offsets = ops.lines_to_u8(image, widths)
            yield idx, pixels, offsets, widths
    finally:
        model.count_std, model.dup_std = std


def render_lines(model, texts, styles, char_to_idx, gpu, batch_lines=64, skipped=None):
    """Generator over (index, uint8 numpy [64, w]) for every text, text i in style styles[i] ([n, style_dim], host or device), in any order:
    render_lines_device's lines on the host. Each bucket is fetched on the copy stream while the next one renders - one fetch in flight."""
    buckets = render_lines_device(model, texts, styles, char_to_idx, gpu, batch_lines, skipped)
    try:
        pending = None
        for idx, pixels, offsets, widths in buckets:
            if pending is not None:
                yield from _cut_lines(*pending)
            pending = (idx, ops.AsyncFetch(pixels), offsets, widths, model.image_height)
        if pending is not None:
            yield from _cut_lines(*pending)
    finally:
        buckets.close()            # (a consumer that stops early: the stds come back now, not when the inner generator is collected)


def _cut_lines(idx, fetch, offsets, widths, height):
    host = fetch.get().numpy()
    for b, i in enumerate(idx):
        yield i, host[offsets[b]:offsets[b + 1]].reshape(height, widths[b]).copy()      # (a copy: the pinned staging buffer is reused)
