#!/usr/bin/env python
"""Records tests/golden/play_styles/expected.json: what the reference's play_styles.py prints for tests/golden/writer_id/styles.pkl (the
fabricated style file of tools/gen_golden_writer_id.py: 61 lines, 37 dimensions, quarter-valued, so every squared distance is exact in fp32
in any summation order).

    python tools/gen_golden_play_styles.py --reference <checkout of the reference>

The unmodified reference script is started in a child process. It imports umap (which it never uses) and matplotlib: the child's module
path holds an empty umap.py, written into a temporary directory, and MPLBACKEND=Agg keeps matplotlib from opening a display. The script
prints two lines and exits (its matrices sit behind the exit()):
    inter dist mean: <m>, stddev: <s>       <- the pairs of ONE writer (the reference's labels are swapped)
    intra dist mean: <m>, stddev: <s>       <- the pairs of two writers
expected.json holds the two lines, their four numbers and, from tests/_play_styles_ref.py on the same file, the two pair counts. The
restatement is compared with the reference here (1e-12 relative) before anything is written. Without --reference nothing is written."""
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
import _play_styles_ref as ref  # noqa: E402

STYLES = os.path.join(ROOT, "tests", "golden", "writer_id", "styles.pkl")
OUT = os.path.join(ROOT, "tests", "golden", "play_styles")
LINE = r"^%s dist mean: (\S+), stddev: (\S+)$"


def restatement():
    with open(STYLES, "rb") as f:
        data = pickle.load(f)
    d, same = ref.distances(data["styles"][:, :, 0, 0], ref.ids_of(data["authors"]))[:2]
    return {"same": {"pairs": int(same.sum()), "mean": float(np.mean(d[same])), "std": float(np.std(d[same]))},
            "different": {"pairs": int((~same).sum()), "mean": float(np.mean(d[~same])), "std": float(np.std(d[~same]))}}


def run_reference(reference):
    script = os.path.join(reference, "play_styles.py")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "umap.py"), "w"):
            pass
        env = dict(os.environ, MPLBACKEND="Agg", PYTHONPATH=d + os.pathsep + os.environ.get("PYTHONPATH", ""))
        text = subprocess.run([sys.executable, script, STYLES], check=True, stdout=subprocess.PIPE, text=True, env=env, cwd=d).stdout
    out = {"lines": [l for l in text.splitlines() if " dist mean: " in l]}
    for label, key in (("inter", "same"), ("intra", "different")):
        m = re.search(LINE % label, text, flags=re.M)
        out[key] = {"label": label, "mean": float(m.group(1)), "std": float(m.group(2))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="directory of the reference checkout (holds play_styles.py)")
    args = ap.parse_args()
    mine = restatement()
    print("restatement: %s" % mine)
    if args.reference is None:
        print("no --reference: nothing written")
        return
    expected = run_reference(args.reference)
    print("reference: %s" % expected)
    for key in ("same", "different"):
        for k in ("mean", "std"):
            assert abs(mine[key][k] - expected[key][k]) <= 1e-12 * abs(expected[key][k]), (key, k, mine[key][k], expected[key][k])
        expected[key]["pairs"] = mine[key]["pairs"]
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
    print("wrote %s" % os.path.join(OUT, "expected.json"))


if __name__ == "__main__":
    main()
