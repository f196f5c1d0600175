"""bench.py's contract: a plain run prints the headline line only; --full adds the secondary measurements; --dump-outputs writes
the last timed step's results; --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_KEYS = ("roofline", "roofline_dominant_by_time", "bf16_mode", "cpu_baseline", "dp_diagnostics")


def _bench(*args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSWIN_DIST_BACKEND")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=timeout, env=env)


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_rejects_zero_timed_steps():
    r = _bench("--steps", "0", timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_bench_is_headline_only_and_dumps_last_step(tmp_path):
    out_dir = tmp_path / "out"
    out = _line(_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--dump-outputs", str(out_dir)))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert abs(out["value"] - 4 * 1e3 / out["ms_per_step"]) <= 0.01 * out["value"]
    assert not any(k in out for k in EXTRA_KEYS), sorted(out)
    files = sorted(os.listdir(out_dir))
    assert files == ["grads.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    arrays = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    np.testing.assert_allclose(arrays["loss"], [out["final_loss"][k] for k in ("loss", "ce", "dice")], atol=1e-5)
    assert arrays["params"].shape == arrays["grads"].shape and np.abs(arrays["grads"]).max() > 0


@pytest.mark.gpu
def test_full_bench_keeps_the_secondary_measurements():
    out = _line(_bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--cpu-batch", "1", "--full"))
    assert out["steps"] == 2
    for k in ("roofline", "roofline_dominant_by_time", "bf16_mode", "cpu_baseline"):
        assert k in out, sorted(out)
    assert out["roofline"]["achieved"] > 0 and out["bf16_mode"]["value"] > 0 and out["cpu_baseline"]["value"] > 0
