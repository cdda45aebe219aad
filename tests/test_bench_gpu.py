"""GPU: `bench.py --dump-outputs` - two plain runs with the same arguments write the same arrays, bit for bit (every step before the dumped
one depends on the arguments alone), within the 64 MB bound, and a plain run's line carries the headline only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(tmp_path, out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_identical_across_runs(cuda, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line_a, line_b = _plain_run(tmp_path, a), _plain_run(tmp_path, b)
    for line in (line_a, line_b):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert abs(line["value"] - 3 / (line["ms_per_step"] * 3e-3)) < 0.01 * line["value"]
        for key in ("whole_cycles", "roofline", "gen_lines_per_sec", "cpu_baseline", "minimum_necessary", "other_workloads", "clocks"):
            assert line[key] is None, key
    assert line_a["recorder_warmup_steps"] == line_b["recorder_warmup_steps"]
    assert line_a["timed_window"]["first_lesson"] == line_b["timed_window"]["first_lesson"]
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert any(n.startswith("log_") for n in names) and any(n.startswith("weights_") for n in names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == (np.float64 if n.startswith("log_") else np.float32), n
        assert x.size > 0 and np.isfinite(x).all(), n
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), "%s differs between two runs with the same arguments" % n
        total += os.path.getsize(a / n)
    assert total <= 64 << 20, total
