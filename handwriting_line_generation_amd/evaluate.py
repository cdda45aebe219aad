"""Evaluation loops (reference: new_eval.py:49-, get_styles.py:19-, trainer/hw_with_style_trainer.py:894-914): how well the recogniser reads
real lines and lines generated from their text in their own extracted style, and the per-author style vectors for later generation."""
import pickle

import numpy as np
import torch

from . import ops


def eval_writer(trainer, loader, max_batches=None):
    """-> {"cer_real", "wer_real", "cer_gen", "wer_gen", "styles" [n, style_dim], "authors": [n]} over the batches of `loader`.
    Per batch: recogniser on the real lines; style of every author (lines side by side, generate.get_style semantics); the same texts rendered
    in that style; recogniser on the rendered lines. Everything under no_grad in eval mode (running BatchNorm statistics, no dropout)."""
    model = trainer.model
    was_training = model.training
    model.eval()
    tot = {"cer_real": 0.0, "wer_real": 0.0, "cer_gen": 0.0, "wer_gen": 0.0}
    styles, authors, n = [], [], 0
    try:
        with torch.no_grad():
            for bi, inst in enumerate(loader):
                if max_batches is not None and bi >= max_batches:
                    break
                image, label = trainer._to_tensor(inst)
                a = inst.get("a_batch_size", 1)
                model.pred = model.spaced_label = model.spaced_label_index = None
                pred = model.hwr(image, None)
                model.pred = pred
                style = model.extract_style(image, label, a)                 # [B, style_dim], one vector per author repeated over its lines
                gen = model(label, inst["label_lengths"], style)
                gen_pred = model.hwr(gen, None)
                cr, wr, _ = trainer.getCER(inst["gt"], pred.cpu().numpy())
                cg, wg, _ = trainer.getCER(inst["gt"], gen_pred.cpu().numpy())
                tot["cer_real"] += cr; tot["wer_real"] += wr; tot["cer_gen"] += cg; tot["wer_gen"] += wg
                styles.append(style[::a].cpu())
                authors += list(inst["author"][::a])
                model.pred = model.spaced_label = model.spaced_label_index = None
                n += 1
    finally:
        if was_training:
            model.train()
    out = {k: v / max(n, 1) for k, v in tot.items()}
    out["styles"] = torch.cat(styles, 0).numpy() if styles else np.zeros((0, model.style_dim), dtype=np.float32)
    out["authors"] = authors
    return out


def dump_styles(result, path):
    """the style pickle get_styles.py writes: {"styles": float array [n, style_dim], "authors": [n]}"""
    with open(path, "wb") as f:
        pickle.dump({"styles": result["styles"], "authors": list(result["authors"])}, f)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model alone over a dataset split (reference get_styles.py:154-255; no trainer, no optimizer)
def _reset(model):
    model.pred = model.spaced_label = model.spaced_label_index = None


def _batch(inst, gpu):
    image = inst["image"] if inst["image"].is_cuda else ops.h2d(inst["image"], gpu)
    label = inst["label"] if inst["label"].is_cuda else ops.h2d(inst["label"], gpu)
    return image, label


def _styles_result(fetches, authors, style_dim):
    styles = np.concatenate([f.get().numpy() for f in fetches], 0) if fetches else np.zeros((0, style_dim), dtype=np.float32)
    return {"styles": np.ascontiguousarray(styles, dtype=np.float32), "authors": np.array(authors)}


def extract_styles(model, loader, gpu):
    """-> {"styles": float32 [n, style_dim], "authors": array [n]}: what the reference's get_styles.py pickles for a split - the style
    model.extract_style gives every line of every batch (all B rows: an author's style once per line of theirs) next to the line's author."""
    was_training = model.training
    model.eval()
    fetches, authors = [], []
    try:
        with torch.no_grad():
            for inst in loader:
                image, label = _batch(inst, gpu)
                _reset(model)
                style = model.extract_style(image, label, inst.get("a_batch_size"))
                fetches.append(ops.AsyncFetch(style))                # the copy travels while the next batch runs
                authors += list(inst["author"])
                _reset(model)
    finally:
        _reset(model)
        if was_training:
            model.train()
    return _styles_result(fetches, authors, model.style_dim)


def _char_set(config):
    import json
    import os
    char_file = config["data_loader"]["char_file"]
    if not os.path.exists(char_file):
        char_file = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", os.path.basename(char_file))
    with open(char_file) as f:
        return {int(k): v for k, v in json.load(f)["idx_to_char"].items()}


def eval_split(model, config, loader, gpu, beam=0):
    """extract_styles, and on the way the recogniser's error rates on every real line and on the same text rendered in the line's own
    extracted style, counted on the device (ops.ctc_error_rates; a batch's counts are read while the next batch runs). Adds to
    extract_styles' result: "lines", per-line lists "cer_real_lines" / "wer_real_lines" / "cer_gen_lines" / "wer_gen_lines" and their means
    over the lines "cer_real" / "wer_real" / "cer_gen" / "wer_gen". beam > 0: the same predictions are also decoded by CTC prefix beam
    search of that width (ops.ctc_beam_error_rates) - "beam" and the same eight entries with "_beam" after the name, next to the
    unchanged greedy ones."""
    idx_to_char = _char_set(config)
    casesensitive = config.get("trainer", {}).get("casesensitive", True)
    was_training = model.training
    model.eval()
    fetches, authors, handles = [], [], []
    per_line = {"cer_real": [], "wer_real": [], "cer_gen": [], "wer_gen": []}
    if beam:
        per_line.update({"cer_real_beam": [], "wer_real_beam": [], "cer_gen_beam": [], "wer_gen_beam": []})

    def settle(keep):
        while len(handles) > keep:
            for name, handle in zip(("real", "gen", "real_beam", "gen_beam"), handles.pop(0)):
                cers, wers, _ = handle.result()
                per_line["cer_" + name] += cers
                per_line["wer_" + name] += wers
    try:
        with torch.no_grad():
            for inst in loader:
                image, label = _batch(inst, gpu)
                _reset(model)
                pred = model.hwr(image, None)
                model.pred = pred
                style = model.extract_style(image, label, inst.get("a_batch_size"))
                gen_pred = model.hwr(model(label, inst["label_lengths"], style), None)
                batch = (ops.ctc_error_rates(pred, inst["gt"], idx_to_char, casesensitive),
                         ops.ctc_error_rates(gen_pred, inst["gt"], idx_to_char, casesensitive))
                if beam:
                    batch += (ops.ctc_beam_error_rates(pred, inst["gt"], idx_to_char, casesensitive, beam),
                              ops.ctc_beam_error_rates(gen_pred, inst["gt"], idx_to_char, casesensitive, beam))
                handles.append(batch)
                fetches.append(ops.AsyncFetch(style))
                authors += list(inst["author"])
                _reset(model)
                settle(1)
            settle(0)
    finally:
        _reset(model)
        if was_training:
            model.train()
    out = _styles_result(fetches, authors, model.style_dim)
    out["lines"] = len(per_line["cer_real"])
    if beam:
        out["beam"] = int(beam)
    for name, values in per_line.items():
        total = 0
        for v in values:
            total += v
        out[name] = total / max(len(values), 1)
        out[name + "_lines"] = values
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# writer retrieval over a style file (reference eval_writer_id.py: is the nearest style to a line's style a line of the same writer?)
def author_ids(authors):
    """-> (int32 [n] ids, number of writers): equal authors (Python equality, as the reference's `author1 == author2`) get equal ids,
    numbered in order of first appearance"""
    table = {}
    ids = np.empty(len(authors), dtype=np.int32)
    for i, a in enumerate(authors):
        a = a.item() if isinstance(a, np.generic) else a
        ids[i] = table.setdefault(a, len(table))
    return ids, len(table)


def dedupe_rows(styles, ids):
    """-> bool [n]: False for a row whose writer and whose style, byte for byte, are those of the row directly above it (extract_styles
    writes a writer's style once per line of theirs)"""
    keep = np.ones(len(ids), dtype=bool)
    if len(ids) > 1:
        raw = np.ascontiguousarray(styles).view(np.uint8).reshape(len(ids), -1)
        keep[1:] = ~((ids[1:] == ids[:-1]) & (raw[1:] == raw[:-1]).all(axis=1))
    return keep


def writer_id(styles, authors, gpu, tops=(1, 5, 20), dedupe=False):
    """Writer retrieval accuracy of a style space: styles numpy [n, D] or [n, D, 1, 1], authors a sequence of n. Per row the columns are
    ordered by distance (stable: ties keep column order, the row's own column included); first_rank is the first place >= 1 that holds a
    line of the row's writer, top-k the share of rows with first_rank <= min(k, n - 1). ->
    {"lines", "dim", "writers", "l1": {...}, "l2": {...}} with {"top<k>" for k in tops, "mean_first_rank" (over the rows that have one;
    None if no row has), "rows_without_match"} per metric (l1: sum |a - b|, l2: sum (a - b)^2, fp32); with dedupe also "dropped": rows
    removed beforehand because writer and style repeat the row above. Distances and ranks are computed on the device
    (ops.writer_first_rank); nothing of size n x n is stored."""
    styles = np.asarray(styles)
    if styles.ndim == 4 and styles.shape[2:] == (1, 1):
        styles = styles[:, :, 0, 0]
    if styles.ndim != 2 or styles.shape[0] < 1 or styles.shape[1] < 1:
        raise ValueError("writer_id: styles must be [n, D] or [n, D, 1, 1] with n, D >= 1, got %s" % (tuple(styles.shape),))
    styles = np.ascontiguousarray(styles, dtype=np.float32)
    if len(authors) != styles.shape[0]:
        raise ValueError("writer_id: %d authors for %d styles" % (len(authors), styles.shape[0]))
    finite = np.isfinite(styles).all(axis=1)
    if not finite.all():
        raise ValueError("writer_id: style row %d is not finite (an order with NaN is not defined)" % int(np.argmin(finite)))
    ids, _ = author_ids(authors)
    out = {}
    if dedupe:
        keep = dedupe_rows(styles, ids)
        out["dropped"] = int((~keep).sum())
        styles, ids = np.ascontiguousarray(styles[keep]), np.ascontiguousarray(ids[keep])
    n, dim = styles.shape
    out.update(lines=n, dim=dim, writers=int(len(np.unique(ids))))
    styles_d, ids_d = ops.h2d(styles, gpu), ops.h2d(ids, gpu)
    fetches = [(name, ops.AsyncFetch(ops.writer_first_rank(styles_d, ids_d, metric)[0])) for name, metric in (("l1", ops.WID_L1), ("l2", ops.WID_L2))]
    for name, fetch in fetches:
        rank = fetch.get().numpy()
        has = rank < n
        part = {"top%d" % k: int((rank <= min(k, n - 1)).sum()) / n for k in tops}
        part["mean_first_rank"] = int(rank[has].sum(dtype=np.int64)) / int(has.sum()) if has.any() else None
        part["rows_without_match"] = int((~has).sum())
        out[name] = part
    return {k: out[k] for k in ("lines", "dim", "writers", "dropped", "l1", "l2") if k in out}


# ---------------------------------------------------------------------------------------------------------------------------------
# separation of a style space (reference play_styles.py: are two lines of one writer closer than two lines of two writers?)
PAIR_MATRIX_WRITERS = 4096      # the writers x writers matrices are left out above this many writers (ops.SP_MAX_WRITERS)


def pair_summary(count, total, total_sq):
    """count, sum of d and sum of d^2 of a set of distances -> {"pairs", "mean", "std"}: std the population standard deviation (np.std),
    0 for a single pair, mean and std None for no pair. fp64 on the host."""
    n = int(count)
    if n == 0:
        return {"pairs": 0, "mean": None, "std": None}
    mean = float(total) / n
    var = float(total_sq) / n - mean * mean
    return {"pairs": n, "mean": mean, "std": float(np.sqrt(var)) if n > 1 and var > 0 else 0.0}


def pair_edges(min_d2, max_d2, bins):
    """-> (edges fp64 [bins + 1], edge2 fp32 [bins + 1]): `bins` equal-width bins in d from sqrt(min_d2) to sqrt(max_d2); edge2 the edges
    squared in fp64 and rounded to fp32 once, the first then 0 and the last +inf (what the kernel compares d^2 with)"""
    edges = np.linspace(np.sqrt(np.float64(min_d2)), np.sqrt(np.float64(max_d2)), bins + 1)
    edge2 = (edges * edges).astype(np.float32)
    edge2[0], edge2[-1] = 0.0, np.inf
    return edges, edge2


def pair_matrices(count, total, total_sq):
    """[A, A] count / sum / sumsq -> (pair_count int64, pair_mean, pair_std fp64): NaN where a cell has no pair, std 0 where it has one"""
    count = np.asarray(count, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.asarray(total, dtype=np.float64) / count
        var = np.asarray(total_sq, dtype=np.float64) / count - mean * mean
        std = np.sqrt(np.maximum(var, 0.0))
    std[count == 1] = 0.0
    mean[count == 0] = np.nan
    std[count == 0] = np.nan
    return count, mean, std


def style_distances(styles, authors, gpu, dedupe=False, matrices=True, bins=64):
    """Same-writer and different-writer distances of a style space: styles numpy [n, D] or [n, D, 1, 1], authors a sequence of n. Over all
    pairs of lines, d = sqrt(sum (a - b)^2) (the sum in fp32 as evaluate.writer_id's l2, the root and everything after it in fp64). ->
    {"lines", "dim", "writers", "same": {"pairs", "mean", "std"}, "different": {...}, "hist": {"edges", "same", "different"}} - std the
    population standard deviation, mean and std None without a pair; the histograms over `bins` equal-width bins in d between the
    smallest and the largest distance (edges [bins + 1]; empty lists without a pair) -, with dedupe "dropped" (as writer_id), with
    matrices "writer_names" [A] (order of first appearance) and numpy [A, A] "pair_count", "pair_mean", "pair_std" (NaN where two writers
    have no pair, i.e. the diagonal cell of a single-line writer; std 0 for one pair); above 4096 writers the matrices are left out with
    a printed note. Rows are sorted by writer for the device (stable); the order of the input shows in no result. Two device calls
    (ops.style_pair_stats): the sums, then the histogram between the extremes the first call found; nothing of size n x n is stored."""
    import math
    styles = np.asarray(styles)
    if styles.ndim == 4 and styles.shape[2:] == (1, 1):
        styles = styles[:, :, 0, 0]
    if styles.ndim != 2 or styles.shape[0] < 1 or styles.shape[1] < 1:
        raise ValueError("style_distances: styles must be [n, D] or [n, D, 1, 1] with n, D >= 1, got %s" % (tuple(styles.shape),))
    styles = np.ascontiguousarray(styles, dtype=np.float32)
    if len(authors) != styles.shape[0]:
        raise ValueError("style_distances: %d authors for %d styles" % (len(authors), styles.shape[0]))
    finite = np.isfinite(styles).all(axis=1)
    if not finite.all():
        raise ValueError("style_distances: style row %d is not finite" % int(np.argmin(finite)))
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= ops.SP_MAX_BINS:
        raise ValueError("style_distances: bins must be an integer in 1..%d, got %r" % (ops.SP_MAX_BINS, bins))
    ids, writers = author_ids(authors)
    names = [None] * writers
    for a, i in zip(authors, ids.tolist()):
        if names[i] is None:
            names[i] = a.item() if isinstance(a, np.generic) else a
    out = {}
    if dedupe:
        keep = dedupe_rows(styles, ids)                       # (a writer's first row always stays: the ids stay 0 .. writers - 1)
        out["dropped"] = int((~keep).sum())
        styles, ids = styles[keep], ids[keep]
    order = np.argsort(ids, kind="stable")
    styles, ids = np.ascontiguousarray(styles[order]), np.ascontiguousarray(ids[order])
    n, dim = styles.shape
    out.update(lines=n, dim=dim, writers=writers)
    if matrices and writers > PAIR_MATRIX_WRITERS:
        print("style_distances: %d writers, the writers x writers matrices are left out above %d" % (writers, PAIR_MATRIX_WRITERS))
        matrices = False
    styles_d, ids_d = ops.h2d(styles, gpu), ops.h2d(ids, gpu)
    count, total, total_sq, d2_range, _ = ops.style_pair_stats(styles_d, ids_d, ops.SP_WRITER_PAIRS if matrices else ops.SP_SAME_DIFFERENT)
    count, total, total_sq, d2_range = (t.cpu().numpy() for t in (count, total, total_sq, d2_range))
    if matrices:
        upper = np.triu(np.ones((writers, writers), dtype=bool), 1)
        cells = {"same": np.eye(writers, dtype=bool), "different": upper}
        for name, mask in cells.items():                      # the cells a <= b, each once; fsum: the exactly rounded sum, whatever the order
            out[name] = pair_summary(count[mask].sum(dtype=np.int64), math.fsum(total[mask].tolist()), math.fsum(total_sq[mask].tolist()))
    else:
        out["same"] = pair_summary(count[0], total[0], total_sq[0])
        out["different"] = pair_summary(count[1], total[1], total_sq[1])
    if out["same"]["pairs"] + out["different"]["pairs"] == 0:
        out["hist"] = {"edges": [], "same": [], "different": []}
    else:
        edges, edge2 = pair_edges(d2_range[0], d2_range[1], bins)
        hist = ops.style_pair_stats(styles_d, ids_d, ops.SP_SAME_DIFFERENT, edge2=edge2)[4].cpu().numpy()
        out["hist"] = {"edges": edges.tolist(), "same": hist[0].tolist(), "different": hist[1].tolist()}
    if matrices:
        out["writer_names"] = names
        out["pair_count"], out["pair_mean"], out["pair_std"] = pair_matrices(count, total, total_sq)
    keys = ("lines", "dim", "writers", "dropped", "same", "different", "hist", "writer_names", "pair_count", "pair_mean", "pair_std")
    return {k: out[k] for k in keys if k in out}
