#!/usr/bin/env python
"""Records tests/golden/writer_id/: one fabricated style file and what the reference's eval_writer_id.py prints for it.

    python tools/gen_golden_writer_id.py --reference <checkout of the reference>

styles.pkl    {"styles": float32 [61, 37, 1, 1], "authors": [61]} - one file, so that the order of files cannot matter. Every value is a
              multiple of 1/4 with |value| <= 16: every L1 and squared-L2 distance is then exact in fp32 (and in the reference's fp32
              numpy sums) in any summation order, so ties are real ties for everyone.
expected.json the reference's printed numbers: "l2" / "l1": {"top1", "top5", "top20"} (asserted by the tests) and "rank" (the reference's
              bestTrue value, which indexes the sorted row by the row number: recorded, not asserted).
The input is searched over seeds until it holds what the tests need (checked here, with tests/_writer_id_ref.py): a run of three identical
consecutive rows of one writer, an identical pair across two writers, a single-line writer, and noise large enough that
top1 < top5 < top20 < 1 under both metrics with the L1 numbers differing from the L2 numbers. Without --reference only the input is
fabricated and checked; nothing is written."""
import argparse
import json
import os
import pickle
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _writer_id_ref as ref  # noqa: E402

N, D = 61, 37
OUT = os.path.join(ROOT, "tests", "golden", "writer_id")


def fabricate(seed):
    rs = np.random.RandomState(seed)
    writers = ["w%02d" % k for k in range(12)]
    authors = [writers[k] for k in rs.randint(0, len(writers), N - 1)]
    authors = sorted(authors)                                  # a writer's lines lie together, as a loader hands them out
    authors.append("solo")                                     # the single-line writer
    centres = {w: rs.randn(D) * 2.0 for w in set(authors)}
    styles = np.stack([centres[a] + rs.randn(D) * 3.0 for a in authors])
    styles = np.clip(np.round(styles * 4) / 4, -16, 16).astype(np.float32)
    # a run of three identical consecutive rows of one writer
    for i in range(N - 3):
        if authors[i] == authors[i + 1] == authors[i + 2]:
            styles[i + 1] = styles[i + 2] = styles[i]
            run = i
            break
    else:
        return None
    # an identical pair across two writers (rows outside the run)
    pair = None
    for i in range(run + 3, N - 2):
        if authors[i] != authors[i + 1]:
            styles[i + 1] = styles[i]
            pair = i
            break
    if pair is None:
        return None
    return styles.reshape(N, D, 1, 1), authors, run, pair


def check(styles4, authors, run, pair):
    s = styles4[:, :, 0, 0]
    assert styles4.shape == (N, D, 1, 1) and 40 <= N <= 80 and D % 4 != 0
    assert np.array_equal(s * 4, np.round(s * 4)) and np.abs(s).max() <= 16
    assert authors[run] == authors[run + 1] == authors[run + 2] and np.array_equal(s[run], s[run + 1]) and np.array_equal(s[run], s[run + 2])
    assert authors[pair] != authors[pair + 1] and np.array_equal(s[pair], s[pair + 1])
    assert authors.count("solo") == 1
    ids = ref.ids_of(authors)
    got = {}
    for name, metric in (("l1", 0), ("l2", 1)):
        rank, _, _ = ref.first_rank(s, ids, metric)
        got[name] = ref.summary(rank, N)
        if not got[name]["top1"] < got[name]["top5"] < got[name]["top20"] < 1:
            return None
    if any(got["l1"][k] == got["l2"][k] for k in ("top1", "top5", "top20")):
        return None
    return got


def run_reference(reference, styles4, authors):
    script = os.path.join(reference, "eval_writer_id.py")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "golden_styles.pkl"), "wb") as f:
            pickle.dump({"styles": styles4, "authors": np.array(authors)}, f)
        text = subprocess.run([sys.executable, script, os.path.join(d, "golden_styles")], check=True, stdout=subprocess.PIPE, text=True).stdout
    out = {}
    for name in ("l2", "l1"):
        m = re.search(r"^%s\ttop1:(\S+),\ttop5:\t(\S+),\ttop20:\t(\S+)$" % name, text, flags=re.M)
        r = re.search(r"^%s rank: (\S+)$" % name, text, flags=re.M)
        out[name] = {"top1": float(m.group(1)), "top5": float(m.group(2)), "top20": float(m.group(3)), "rank": float(r.group(1))}
    out["top_lines"] = [l for l in text.splitlines() if "\ttop1:" in l]
    out["shape_line"] = text.splitlines()[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="directory of the reference checkout (holds eval_writer_id.py)")
    args = ap.parse_args()
    for seed in range(1000):
        made = fabricate(seed)
        if made is None:
            continue
        mine = check(*made)
        if mine is not None:
            break
    else:
        raise SystemExit("no seed gives an input that meets the conditions")
    styles4, authors, run, pair = made
    print("seed %d: run of three at %d, cross-writer pair at %d, restatement %s" % (seed, run, pair, mine))
    if args.reference is None:
        print("no --reference: nothing written")
        return
    expected = run_reference(args.reference, styles4, authors)
    expected["seed"] = seed
    print("reference: %s" % expected)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "styles.pkl"), "wb") as f:
        pickle.dump({"styles": styles4, "authors": np.array(authors)}, f, protocol=4)
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
    print("wrote %s" % OUT)


if __name__ == "__main__":
    main()
