"""bench.py on one GPU, plain (no --full): the result line carries the headline figure and nothing that needs runs of its
own, `--steps` sets the timed steps, and `--dump-outputs` writes the last timed step's outputs from identical inputs on
every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "rgb_fine", "rgb_target", "flat_grad", "flat_params")


def run_bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--global-batch", "256", "--samples", "32", "--height", "64", "--width", "128", "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), {k: np.load(os.path.join(out_dir, k + ".npy")) for k in NAMES}


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out, dump = run_bench(tmp_path / "a", 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert abs(out["value"] - 256 * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
    for k in ("roofline", "inference", "extra", "cpu_baseline"):  # --full legs
        assert k not in out, k
    assert all(v.dtype in (np.float32, np.float64) for v in dump.values())
    assert sum(v.nbytes for v in dump.values()) <= 64 << 20
    assert dump["rgb_fine"].shape == (256, 3) and dump["rgb_target"].shape == (256, 3)
    assert dump["flat_grad"].shape == dump["flat_params"].shape and dump["flat_grad"].ndim == 1
    assert all(bool(np.isfinite(v).all()) for v in dump.values())
    assert float(dump["loss"]) == np.float32(out["loss"])
    # the same arguments draw the same inputs: the target colours of the last step are the same rays' on a second run
    out2, dump2 = run_bench(tmp_path / "b", 2)
    assert out2["steps"] == 2
    _, dump3 = run_bench(tmp_path / "c", 3)
    assert np.array_equal(dump["rgb_target"], dump3["rgb_target"])
    assert not np.array_equal(dump["rgb_target"], dump2["rgb_target"])  # another step, another batch
