#!/usr/bin/env python
"""python new_eval.py -c checkpoint.pth [-d out_dir] [-g gpu] [-n images] [-b batch] [-f config.json] [-a k=v,...] [-T] [-e [recon,pred]] [-i index | -m name]
The reference's new_eval.py: runs a checkpoint over -n // batch batches of the validation (with -T: test) and training splits and prints,
per line, what the recogniser read (`GT: / aligned: / pred:`) and at the end '<split> metrics' with every metric's overall mean and std.
With -d the pictures go to <savedir>/valid_<name>/ and train_<name>/: <line>_recon.png - the real line in a green frame above its
reconstruction in a blue one, with `-e` holding `pred` a caption strip 'CER: ..., T: ...' below - and gen_<line>.png for `-e [gen]`.
Without -d the whole validation split is scored. Everything per pixel and per character runs on the GPU (evaluators.py); only finished
8-bit pictures and counts come to the host.

-a adds config keys: save_preds=<csv> (name, gt, pred, cer of the training batches), save_style=<path> with saveStyleEvery=<batches>
({"styles", "authors"} pickles <path>.<volume> and val_<path>.<volume>), by_author (CER lists per writer), cer_thresh=<x> (pictures only of
lines at or above it, named '<cer>_<line>_recon.png'), skip_valid, skip_train, startBatch=<k>, beam=<K> (the `pred:` text and every
rate from it come from a CTC prefix beam search of width K on the GPU instead of the greedy decode; a header line says so).
Not built, refused with the reason: the config keys of REFUSED_KEYS and `-e spaced|spacing|mask` and the mask pictures."""
import argparse
import csv
import json
import os
import pickle
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

REFUSED_KEYS = {
    "save_spaced": "the datasets here refuse `spaced_loc`, so nothing would ever read such a file",
    "save_nns": "the reference fills it from an evaluator output that no shipped evaluator produces",
    "show_attention": "it reads the attention maps of a style extractor (mhAtt1) that the shipped configs do not build",
    "doSpaced": "it pickles the one-hot alignments next to the styles for a spacing model that is not shipped",
}


def _flag(text):
    return str(text).lower() not in ("", "0", "false", "no")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="MI355X-native evaluator: per-line scores and pictures")
    ap.add_argument("-c", "--checkpoint", default=None, type=str, help="path to the checkpoint (of this package or of the reference)")
    ap.add_argument("-d", "--savedir", default=None, type=str, help="directory the pictures are written to (default: none are written)")
    ap.add_argument("-i", "--index", default=None, type=int, help="evaluate the one batch that holds this instance (> 0: train, <= 0: valid)")
    ap.add_argument("-n", "--number", default=0, type=int, help="number of images to save out (from each of train and valid)")
    ap.add_argument("-g", "--gpu", default=None, type=int, help="gpu number (default: 0; there is no CPU path)")
    ap.add_argument("-b", "--batchsize", default=None, type=int, help="batch size of both loaders (default: the config's)")
    ap.add_argument("-v", "--verbosity", default=2, type=int, help="0, 1, 2; 3 also prints every line's raw prediction array")
    ap.add_argument("-s", "--shuffle", default=False, type=_flag, help="shuffle data")
    ap.add_argument("-f", "--config", default=None, type=str, help="config file to use instead of the checkpoint's")
    ap.add_argument("-m", "--imgname", default=None, type=str, help="evaluate the batch that holds the line of this name")
    ap.add_argument("-a", "--addtoconfig", default=None, type=str, help="k1=v1,k2=k3=v2: config[k1]=v1, config[k2][k3]=v2; [a-b] is a list")
    ap.add_argument("-T", "--test", default=False, action="store_true", help="run the test split")
    ap.add_argument("-e", "--eval", default=None, type=str,
                    help='what to evaluate, a list: "pred" = the recogniser\'s reading, "recon" = reconstruction, "gen" = image generated '
                         'from interpolated styles, "style", "author" (default: [recon,pred] with a generator, else [pred])')
    ap.add_argument("--swa", default=False, action="store_true", help="evaluate the averaged weights (the checkpoint's swa_state_dict)")
    args = ap.parse_args(argv)
    if args.checkpoint is None and args.config is None:
        raise SystemExit("new_eval.py: must provide checkpoint (with -c)")
    if args.checkpoint is None:
        raise SystemExit("new_eval.py: -f alone would evaluate untrained weights; pass the checkpoint with -c")
    if args.index is not None and args.imgname is not None:
        raise SystemExit("new_eval.py: cannot index by number and name at same time")
    if args.batchsize is not None and args.batchsize < 1:
        raise SystemExit("new_eval.py: -b must be at least 1")
    args.to_eval = parse_eval(args.eval)
    args.adds = parse_addtoconfig(args.addtoconfig)
    return args


def parse_eval(text):
    """'[recon,pred]' -> ['recon', 'pred']; refuses what is not built (evaluators.check_to_eval's reasons) without importing torch"""
    if text is None:
        return None
    to_eval = text[1:-1].split(",") if text.startswith("[") and text.endswith("]") else text
    refused = {"spaced": "it prints index tensors for a debugger session", "spacing": "it needs a spacing predictor that no shipped config builds",
               "mask": "it opens a debugger and a window in the reference"}
    for name in ([to_eval] if isinstance(to_eval, str) else to_eval):
        if name in refused:
            raise SystemExit("new_eval.py: -e %s is refused: %s" % (name, refused[name]))
        if name in ("recon_gt_mask", "recon_pred_space", "gen_mask"):
            raise SystemExit("new_eval.py: -e %s is refused: the shipped configs are noMask, no mask is ever made" % name)
    if isinstance(to_eval, str):
        raise SystemExit("new_eval.py: -e takes a list like [recon,pred], got %r" % text)
    return to_eval


def parse_addtoconfig(text):
    """'k1=v1,k2=k3=v2' -> [[k1, v1], [k2, k3, v2]]; a key without '=' (by_author, skip_valid) is set to True"""
    out = []
    for kv in (text.split(",") if text else []):
        parts = kv.split("=")
        out.append(parts if len(parts) > 1 else [parts[0], "True"])
    return out


def apply_addtoconfig(config, adds):
    """the reference's rule (new_eval.py:81-103): int, else float, else text; '' is None; '[a-b]' is the list ['a', 'b']"""
    for add in adds:
        target = config
        for key in add[:-2]:
            target = target[key]
        value = add[-1]
        if value == "":
            value = None
        elif value[0] == "[" and value[-1] == "]":
            value = value[1:-1].split("-")
        else:
            try:
                value = int(value)
            except ValueError:
                try:
                    value = float(value)
                except ValueError:
                    pass
        target[add[-2]] = value
        print("added config[" + "][".join(add[:-1]) + "]={}".format(value))
    return config


def check_config(config):
    for key, why in REFUSED_KEYS.items():
        if key in config:
            raise SystemExit("new_eval.py: config key %s is refused: %s" % (key, why))


def prepare_config(config, args):
    """the reference's set-up (new_eval.py:60-143): no warm starts, no optimizer, no schedule, evaluation loaders"""
    for section in config.values():
        if isinstance(section, dict):
            for key in section:
                if key.startswith("pretrained"):
                    section[key] = None
    config["optimizer_type"] = "none"
    tr = config["trainer"]
    tr["use_learning_schedule"] = False
    tr["swa"] = False
    tr["print_dir"] = None
    tr.pop("encoder_weights", None)         # the perceptual encoder and the text corpus serve training lessons only
    tr.pop("text_data", None)
    config["cuda"], config["gpu"] = True, 0 if args.gpu is None else args.gpu
    apply_addtoconfig(config, args.adds)
    check_config(config)
    if "beam" in config:
        if isinstance(config["beam"], bool) or not isinstance(config["beam"], int) or config["beam"] < 1:
            raise SystemExit("new_eval.py: beam=K needs a width K >= 1, got %r" % (config["beam"],))
        print("decoding: CTC prefix beam search, beam {} (pred, CER / WER, by_author, cer_thresh and save_preds use its text)".format(config["beam"]))
    dl = config["data_loader"]
    val = config.setdefault("validation", {})
    dl["shuffle"] = val["shuffle"] = bool(args.shuffle)
    dl["eval"] = val["eval"] = True
    if args.batchsize is not None:
        dl["batch_size"] = val["batch_size"] = args.batchsize
    if not os.path.exists(dl["char_file"]):
        dl["char_file"] = os.path.join(ROOT, "handwriting_line_generation_amd", "data", os.path.basename(dl["char_file"]))
    return config


def save_style(location, volume, fetches, authors):
    import numpy as np
    if not fetches:
        return
    styles = np.concatenate([f.get().numpy() for f in fetches], 0)
    loc = location + ".{}".format(volume)
    with open(loc, "wb") as f:
        pickle.dump({"styles": styles, "authors": authors}, f)
    print("saved " + loc)


class _Lookahead:
    """begin() of batch k + 1 before finish() of batch k: a batch's counts and pictures are read while the next batch runs"""

    def __init__(self):
        self.pending = None

    def push(self, pending, then):
        self.flush()
        self.pending = (pending, then)

    def flush(self):
        p, self.pending = self.pending, None
        if p is not None:
            p[1](*p[0].finish())


def load_model(args, checkpoint, config):
    """the checkpoint's model with its live weights, or (--swa) with the averaged ones a run with trainer.swa / trainer.weight_averaging wrote"""
    if getattr(args, "swa", False):
        from handwriting_line_generation_amd.generate import load_for_generation
        return load_for_generation(args.checkpoint, gpu=config["gpu"], checkpoint=dict(checkpoint, config=config), averaged=True)[0]
    import handwriting_line_generation_amd.model as models
    model = getattr(models, config["arch"])(config["model"])
    state = {k: v for k, v in checkpoint["state_dict"].items() if "style_from_normal" not in k}
    model.load_state_dict(state)
    return model


def setup(args):
    """checkpoint -> (config, trainer, training loader, validation loader, what to evaluate, iteration): the model in eval mode inside a
    trainer built with resume=False, as the reference does (new_eval.py:52-192)"""
    import numpy as np
    import torch
    torch.set_num_threads(1)
    import handwriting_line_generation_amd.model.loss as losses
    import handwriting_line_generation_amd.trainer as trainers
    from handwriting_line_generation_amd import evaluators
    from handwriting_line_generation_amd.data.author_hw_dataset import getDataLoader
    from handwriting_line_generation_amd.logger import Logger, load_checkpoint
    np.random.seed(1234)
    torch.manual_seed(1234)
    torch.cuda.set_device(0 if args.gpu is None else args.gpu)
    checkpoint = load_checkpoint(args.checkpoint)
    loaded_iteration = checkpoint["iteration"]
    print("loaded iteration {}".format(loaded_iteration))
    config = checkpoint["config"] if args.config is None else json.load(open(args.config))
    config = prepare_config(config, args)
    to_eval = args.to_eval
    if "save_style" in config:
        to_eval = list(to_eval or [])
        to_eval += [n for n in ("style", "author") if n not in to_eval]
    if not args.test:
        data_loader, valid_data_loader = getDataLoader(config, "train")
    else:
        valid_data_loader, data_loader = getDataLoader(config, "test")

    model = load_model(args, checkpoint, config)
    del checkpoint
    model.eval()
    if args.verbosity > 1 and hasattr(model, "summary"):
        model.summary()
    loss = {k: getattr(losses, v) for k, v in config["loss"].items()} if isinstance(config["loss"], dict) else getattr(losses, config["loss"])
    cls = config["trainer"]["class"]
    if cls == "HWRWithSynthTrainer":        # trains a recogniser on generated lines; evaluated like recogniser pre-training
        cls = "HWWithStyleTrainer"
        config["trainer"].pop("curriculum", None)
    trainer = getattr(trainers, cls)(model, loss, [], False, config, data_loader, valid_data_loader, Logger())
    trainer.model.eval()
    if to_eval is None:
        to_eval = evaluators.default_to_eval(trainer)
    if not hasattr(evaluators, config["data_loader"]["data_set_name"] + "_eval"):
        raise SystemExit("new_eval.py: no evaluator for data set %r" % config["data_loader"]["data_set_name"])
    return config, trainer, data_loader, valid_data_loader, to_eval, loaded_iteration


def main(argv=None):
    args = parse_args(argv)
    config, trainer, data_loader, valid_data_loader, to_eval, loaded_iteration = setup(args)
    import numpy as np
    import torch
    from handwriting_line_generation_amd import evaluators, ops
    batch_size = config["data_loader"]["batch_size"]
    v_batch_size = config["validation"].get("batch_size", batch_size)
    begin = evaluators.begin
    valid_name = "valid" if not args.test else "test"
    val_comb_metrics = defaultdict(list)

    def collect(metrics_out):
        for typ, values in metrics_out.items():
            val_comb_metrics[typ] += [values] if isinstance(values, (float, int)) else values

    with torch.no_grad():
        if args.index is not None or args.imgname is not None:
            instance = _find_instance(args, data_loader, valid_data_loader, batch_size)
            if args.savedir is not None:
                os.makedirs(args.savedir, exist_ok=True)
            if instance is not None:
                begin(config, instance, trainer, [], args.savedir, 0, to_eval, args.verbosity).finish()
            evaluators.wait()
            return

        train_dir = valid_dir = None
        if args.savedir is not None:
            train_dir = os.path.join(args.savedir, "train_" + config["name"])
            valid_dir = os.path.join(args.savedir, "valid_" + config["name"])
            os.makedirs(train_dir, exist_ok=True)
            os.makedirs(valid_dir, exist_ok=True)
            with open(os.path.join(valid_dir, "z_iter_{}.txt".format(loaded_iteration)), "w") as f:
                f.write("{}".format(loaded_iteration))

        styles = {"train": ([], []), "valid": ([], [])}          # (fetches, authors)
        style_loc = style_val_loc = None
        if "save_style" in config:
            every = config.get("saveStyleEvery", 5000)
            style_loc = config["save_style"]
            head, tail = os.path.split(style_loc)
            style_val_loc = os.path.join(head, "val_" + tail)
        to_save = []
        ahead = _Lookahead()

        def after(split, batch, instance, loader_len):
            def then(metrics_out, aux):
                if split == "valid":
                    collect(metrics_out)
                if style_loc is not None:
                    fetches, authors = styles[split]
                    fetches.append(aux["style_fetch"])
                    authors += list(aux["author"])
                    if batch > 0 and batch % every == 0:
                        save_style(style_loc if split == "train" else style_val_loc, batch, fetches, list(authors))
                        del fetches[:], authors[:]
                if split == "train" and "save_preds" in config:
                    for b in range(len(instance["gt"])):
                        to_save.append([instance["name"][b], instance["gt"][b], aux["pred_str"][b], aux["cer"][b]])
            return then

        def run(split, batch, instance, loader_len, out_dir, start):
            p = begin(config, instance, trainer, [], out_dir, start, to_eval, args.verbosity)
            if style_loc is not None:
                p.out["style_fetch"] = ops.AsyncFetch(p.out["style"])
            ahead.push(p, after(split, batch, instance, loader_len))

        train_iter = iter(data_loader) if data_loader is not None else None
        valid_iter = iter(valid_data_loader) if valid_data_loader is not None else None
        n_valid = len(valid_data_loader) if valid_data_loader is not None else 0
        n_train = len(data_loader) if data_loader is not None else 0
        start_batch = config.get("startBatch", 0)
        n_batches = args.number // batch_size
        if n_batches == 0 and args.number > 1:
            n_batches = 1
        n_batches = min(n_batches, max(n_valid, n_train))
        batch = start_batch
        for batch in range(start_batch, n_batches):
            if valid_iter is not None and batch < n_valid and "skip_valid" not in config:
                run("valid", batch, next(valid_iter), n_valid, valid_dir, batch * v_batch_size)
            if not args.test and "skip_train" not in config and train_iter is not None and batch < n_train:
                run("train", batch, next(train_iter), n_train, train_dir, batch * batch_size)
        if args.savedir is None and valid_iter is not None:
            for vi in range(batch, n_valid):
                try:
                    instance = next(valid_iter)
                except StopIteration:
                    print("ERROR: ran out of valid batches early. Expected {} more".format(n_valid - vi))
                    break
                run("valid", vi, instance, n_valid, None, vi * v_batch_size)
        ahead.flush()
        if "save_preds" in config:
            with open(config["save_preds"], "w") as f:
                w = csv.writer(f, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL)
                for row in to_save:
                    w.writerow(row)
            print("wrote results to {}".format(config["save_preds"]))
        evaluators.wait()                     # every picture has left its file before the numbers are printed
        print("{} metrics".format(valid_name))
        for typ in val_comb_metrics:
            print("{} overall mean: {}, std {}".format(typ, np.mean(val_comb_metrics[typ], axis=0), np.std(val_comb_metrics[typ], axis=0)))
        if style_loc is not None:
            save_style(style_loc, n_train, *styles["train"])
            save_style(style_val_loc, n_valid, *styles["valid"])


def _find_instance(args, data_loader, valid_data_loader, batch_size):
    """-i: the batch that holds instance |index| (> 0: training split, else validation); -m: the batch that holds the line of that name"""
    if args.index is not None:
        loader = data_loader if args.index > 0 else valid_data_loader
        instance = None
        for k, instance in enumerate(loader):
            if k == abs(args.index) // batch_size:
                return instance
        print("{} is beyond the split".format(args.index))
        return None
    for loader in (data_loader, valid_data_loader):
        for instance in (loader or []):
            if args.imgname in instance["name"]:
                return instance
    print("{} not found!".format(args.imgname))
    return None


if __name__ == "__main__":
    main()
