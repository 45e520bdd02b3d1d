"""bench.py without --full: the headline alone (set-up, warm-up, the timed steps, the line), and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what only a --full run measures
FULL_ONLY = {"hoisted_graph", "train", "train_free", "roofline", "roofline_tconv", "deployed_b1_h16", "cpu_baseline",
             "speedup_vs_cpu_baseline"}


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *args],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0]


def test_plain_bench_run_measures_the_headline_alone(tmp_path):
    res = _bench()
    assert res["metric"] == res["unit"] == "denoising-steps/sec" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["full"] is False
    assert res["value"] > 0 and abs(res["value"] * res["ms_per_step"] / 1e3 - 1.0) < 1e-3
    assert not (FULL_ONLY | {"hoisted"}) & set(res), sorted(res)
    # --dump-outputs writes both loops' trajectories: the hoisted loop runs for its array (and is reported), nothing else does
    out = tmp_path / "dump"
    res = _bench("--dump-outputs", str(out))
    assert not FULL_ONLY & set(res), sorted(res)
    assert res["hoisted"]["steps"] == 50 and set(res["dumped_outputs"]["arrays"]) == {"trajectories", "trajectories_hoisted"}
    for name in ("trajectories", "trajectories_hoisted"):
        a = np.load(out / f"{name}.npy")
        assert a.shape == (64, 32, 7) and a.dtype == np.float32 and np.isfinite(a).all(), name
        assert (a[:, 0, :3] == 0).all(), name
