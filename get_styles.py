#!/usr/bin/env python
"""python get_styles.py -c checkpoint.pth -d out_dir [-g gpu] [-b batch] [-f config.json] [-a k=v,...] [-T] [--cer [--beam K]] [--writer-id] [--distances]
The reference's get_styles.py: the style vector of every line of the training and validation splits (with -T: of the test split), written
as <savedir>/train_styles_<iteration>.pkl and val_styles_<iteration>.pkl (test_styles_<iteration>.pkl): {"styles": float32 [n, style_dim],
"authors": array [n]} - what `generate.py -s` samples from. Only the model is built (no trainer, no optimizer). With --cer the recogniser's
error rates on the real lines and on the same texts rendered in their own extracted style are counted on the GPU on the way and written to
<split>_cer_<iteration>.json; --beam K adds the rates of the CTC prefix beam search's text (width K) to that file. With --writer-id the written styles are scored for writer retrieval (evaluate.writer_id with dedupe: top-1 / 5 / 20
under L1 and squared L2, what eval_writer_id.py --dedupe prints) into <split>_writer_id_<iteration>.json. With --distances their same-writer and
different-writer distances (evaluate.style_distances with dedupe, without the writer x writer matrices: pairs, mean, std and the two histograms,
what play_styles.py --dedupe prints) go into <split>_distances_<iteration>.json."""
import argparse
import json
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="MI355X-native style extraction over a dataset split")
    ap.add_argument("-c", "--checkpoint", type=str, default=None, help="checkpoint of this package or of the reference")
    ap.add_argument("-d", "--savedir", type=str, default=None, help="directory the style files are written to")
    ap.add_argument("-g", "--gpu", type=int, default=0)
    ap.add_argument("-b", "--batchsize", type=int, default=None, help="batch size of both loaders (default: the config's)")
    ap.add_argument("-f", "--config", type=str, default=None, help="config file to use instead of the checkpoint's")
    ap.add_argument("-a", "--addtoconfig", type=str, default=None, help="k1=v1,k2=k3=v2: config[k1]=v1, config[k2][k3]=v2")
    ap.add_argument("-T", "--test", action="store_true", help="the test split (default: train and valid)")
    ap.add_argument("-S", "--transformstyle", action="store_true", help="(not built)")
    ap.add_argument("--cer", action="store_true", help="also score the recogniser on real and regenerated lines: <split>_cer_<iteration>.json")
    ap.add_argument("--beam", type=int, default=0, metavar="K",
                    help="with --cer: also decode by CTC prefix beam search of width K (1..32 on the GPU): beam, cer_real_beam, wer_real_beam, "
                         "cer_gen_beam, wer_gen_beam in the same file")
    ap.add_argument("--writer-id", dest="writer_id", action="store_true",
                    help="also score the written styles for writer retrieval: <split>_writer_id_<iteration>.json")
    ap.add_argument("--distances", action="store_true",
                    help="also measure same-writer against different-writer style distances: <split>_distances_<iteration>.json")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.transformstyle:
        raise SystemExit("get_styles.py: -S (styles passed through the generator's style_emb) is not built: `generate.py -s` interpolates "
                         "styles in the extractor's space and embeds them itself")
    if args.checkpoint is None and args.config is None:
        raise SystemExit("get_styles.py: must provide a checkpoint (with -c)")
    if args.checkpoint is None:
        raise SystemExit("get_styles.py: -f alone would extract styles with untrained weights; pass the checkpoint with -c")
    if args.savedir is None:
        raise SystemExit("get_styles.py: must provide a directory to write to (with -d)")
    if args.batchsize is not None and args.batchsize < 1:
        raise SystemExit("get_styles.py: -b must be at least 1")
    if args.beam < 0:
        raise SystemExit("get_styles.py: --beam must be at least 1")
    if args.beam and not args.cer:
        raise SystemExit("get_styles.py: --beam decodes what --cer scores; pass --cer with it")

    import numpy as np
    import torch
    torch.set_num_threads(1)       # host side = many tiny CPU ops; the intra-op pool only adds latency (see bench.py)
    import generate as cli
    from handwriting_line_generation_amd import evaluate
    from handwriting_line_generation_amd.data.author_hw_dataset import getDataLoader
    from handwriting_line_generation_amd.generate import load_for_generation
    from handwriting_line_generation_amd.logger import load_checkpoint
    np.random.seed(1234)
    torch.manual_seed(1234)
    torch.cuda.set_device(args.gpu)
    gpu = torch.device("cuda", args.gpu)
    checkpoint = load_checkpoint(args.checkpoint)
    iteration = checkpoint.get("iteration")
    print("loaded iteration %s" % iteration, flush=True)
    model, config, _ = load_for_generation(args.checkpoint, args.config, args.gpu, add_to_config=cli.parse_addtoconfig(args.addtoconfig),
                                           checkpoint=checkpoint)
    del checkpoint
    dl = config["data_loader"]
    val = config.setdefault("validation", {})
    dl["shuffle"] = val["shuffle"] = False
    dl["eval"] = val["eval"] = True
    if args.batchsize is not None:
        dl["batch_size"] = val["batch_size"] = args.batchsize
    if not os.path.exists(dl["char_file"]):
        dl["char_file"] = os.path.join(ROOT, "handwriting_line_generation_amd", "data", os.path.basename(dl["char_file"]))
    if args.test:
        test_loader, _ = getDataLoader(config, "test")
        splits = [("test", test_loader)]
    else:
        train_loader, valid_loader = getDataLoader(config, "train")
        splits = [("train", train_loader), ("val", valid_loader)]
    os.makedirs(args.savedir, exist_ok=True)

    for name, loader in splits:
        if loader is None:
            print("%s: no lines" % name, flush=True)
            continue
        t0 = time.time()
        result = evaluate.eval_split(model, config, loader, gpu, beam=args.beam) if args.cer else evaluate.extract_styles(model, loader, gpu)
        torch.cuda.synchronize()
        dt = time.time() - t0
        loc = os.path.join(args.savedir, "%s_styles_%s.pkl" % (name, iteration))
        with open(loc, "wb") as f:
            pickle.dump({"styles": result["styles"], "authors": result["authors"]}, f)
        print("saved %s" % loc, flush=True)
        if args.cer:
            loc = os.path.join(args.savedir, "%s_cer_%s.json" % (name, iteration))
            with open(loc, "w") as f:
                json.dump({k: v for k, v in result.items() if k not in ("styles", "authors")}, f)
            print("saved %s  cer_real %.4f  wer_real %.4f  cer_gen %.4f  wer_gen %.4f" % (
                loc, result["cer_real"], result["wer_real"], result["cer_gen"], result["wer_gen"]), flush=True)
            if args.beam:
                print("  beam %d  cer_real %.4f  wer_real %.4f  cer_gen %.4f  wer_gen %.4f" % (
                    result["beam"], result["cer_real_beam"], result["wer_real_beam"], result["cer_gen_beam"], result["wer_gen_beam"]), flush=True)
        if args.writer_id:
            loc = os.path.join(args.savedir, "%s_writer_id_%s.json" % (name, iteration))
            scores = evaluate.writer_id(result["styles"], result["authors"], gpu, dedupe=True)
            with open(loc, "w") as f:
                json.dump(scores, f)
            print("saved %s  lines %d (dropped %d)  l2 top1 %.4f top5 %.4f top20 %.4f" % (
                loc, scores["lines"], scores["dropped"], scores["l2"]["top1"], scores["l2"]["top5"], scores["l2"]["top20"]), flush=True)
        if args.distances:
            loc = os.path.join(args.savedir, "%s_distances_%s.json" % (name, iteration))
            dist = evaluate.style_distances(result["styles"], result["authors"], gpu, dedupe=True, matrices=False)
            with open(loc, "w") as f:
                json.dump(dist, f)
            print("saved %s  lines %d (dropped %d)  same writer: pairs %d mean %s  different writers: pairs %d mean %s" % (
                loc, dist["lines"], dist["dropped"], dist["same"]["pairs"], dist["same"]["mean"], dist["different"]["pairs"],
                dist["different"]["mean"]), flush=True)
        n = len(result["authors"])
        print("%s: lines %d  seconds %.3f  lines/s %.1f" % (name, n, dt, n / dt if dt > 0 else 0.0), flush=True)


if __name__ == "__main__":
    main()
