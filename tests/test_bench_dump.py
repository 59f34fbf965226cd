"""bench.py's plain run on the GPU: `--steps` / `--warmup` are the iterations it runs, and `--dump-outputs` writes the
iterate the timed path ends on - two runs that split the same 5 iterations differently dump the same x."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
ROWS = 8192                       # cfg2's 8192 columns on one generator block of rows: 256 MiB of A


def _bench(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg2", "--rows", str(ROWS),
           "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    line = json.loads(proc.stdout.strip().splitlines()[-1])
    x = np.load(out_dir / "x.npy")
    return line, x


def test_plain_run_counts_steps_and_dumps_the_final_iterate(tmp_path):
    line_a, x_a = _bench(tmp_path / "a", steps=4, warmup=1)
    line_b, x_b = _bench(tmp_path / "b", steps=2, warmup=3)
    for line, steps, warmup in ((line_a, 4, 1), (line_b, 2, 3)):
        assert line["metric"] == "fista_iterations_per_second" and line["unit"] == "it/s" and line["higher_is_better"]
        assert line["dtype"] == "f32"
        assert (line["steps"], line["warmup"], line["repeats"]) == (steps, warmup, 1)
        assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
        assert line["roofline"] is None and line["cpu_baseline"] is None and line["target_ref"] is None
    assert x_a.dtype == np.float64 and x_a.shape == (8192,) and np.all(np.isfinite(x_a))
    assert np.linalg.norm(x_a) > 0.0, "iterate did not move"
    assert np.linalg.norm(x_a - x_b) <= 1e-12 * np.linalg.norm(x_a)
