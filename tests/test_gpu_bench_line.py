"""bench.py's plain N = 1 call end to end on a small graph: the headline line without the --full legs, and --dump-outputs -- the same
arguments twice give the same inputs and the same sampled output rows, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_reproducible_dump(cuda_device, tmp_path):
    V, E, K = 150_000, 1_500_000, 3
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    dumps = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
               "--nodes-per-gpu", str(V), "--edges-per-gpu", str(E), "--dump-outputs", str(tmp_path / run)]
        out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-500:], out.stderr[-1500:])
        d = json.loads(lines[0])
        assert d["steps"] == K and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "edges/s" and d["higher_is_better"] is True
        assert d["ms_per_step"] > 0 and abs(d["value"] - E / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
        assert "F=75" in d["metric"] and d["dtype"].startswith("f32") and d["config"]["posttrans_arith"]
        for leg in ("roofline", "parity_check", "cpu_baseline", "configs4_per_gpu_shape", "ms_per_step_cold", "kernel_ms"):
            assert leg not in d, leg                                      # (--full only)
        files = sorted(os.listdir(tmp_path / run))
        assert files == ["y_rows.npy"], files
        y = np.load(tmp_path / run / "y_rows.npy")
        assert y.dtype == np.float32 and y.shape[1] == 75 and 0 < y.shape[0] <= V and y.nbytes <= 64e6 and np.isfinite(y).all()
        dumps.append(y)
    assert np.array_equal(dumps[0], dumps[1])
