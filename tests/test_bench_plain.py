"""A plain `bench.py --gpus 1 --steps K --warmup W` run: the headline line and nothing that takes runs of its own (that is
--full's), and --dump-outputs writing the same arrays from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "AIR_BENCH_SHARE_GPU")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3",
                          "--dump-outputs", str(out_dir)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_repeatable_outputs(gpu_device, tmp_path):
    d = _bench(tmp_path / "a")
    assert d["steps"] == 12 and d["warmup"] == 3 and d["n_gpus"] == 1
    assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "f32" and "images/sec" in d["metric"]
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 / 64 - 1.0) < 2e-3
    assert d["config"]["params_finite_after_run"] is True
    for k in ("fixed_batch", "other_configs", "roofline_gemm", "roofline_sweep_st_read_fwd", "stream_reference"):
        assert k not in d, k
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["median_ms_per_step"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    for k in ("what", "where", "presence_prob", "final_canvas", "canvas", "rec_loss_per_sample", "opt_loss", "flat_params"):
        assert k + ".npy" in names, (k, names)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10 ** 6
    _bench(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "b")) == names
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, b, equal_nan=True), n     # same arguments -> same inputs -> the same outputs
