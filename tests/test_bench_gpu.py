"""bench.py as it is run: a plain run prints the headline line only, and --dump-outputs writes what the last timed step
computed, from inputs that are the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_and_train_outputs(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        j = _bench("--steps", "3", "--warmup", "1", "--batch", "8", "--dump-outputs", str(d))
        assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "patches/s" and j["higher_is_better"] is True
        assert j["dtype"] == "f32" and j["ms_per_step"] > 0
        assert abs(j["value"] - 8 * 3 / (j["ms_per_step"] * 3e-3)) < 1e-2 * j["value"]
        assert not {"roofline", "also", "cpu_baseline"} & set(j), sorted(j)       # --full only
        runs.append(_load(d))
    a, b = runs
    assert sorted(a) == ["bn_running", "ds_loss", "loss", "params", "percep_loss"]
    assert a["params"].shape == (282705,) and a["loss"].shape == (1,)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        # same arguments -> same inputs; the two runs may differ only by the order of floating-point reductions
        assert np.allclose(a[k], b[k], rtol=1e-4, atol=1e-6), (k, np.abs(a[k] - b[k]).max())


def test_infer_outputs_are_a_bounded_sample(tmp_path):
    j = _bench("--mode", "infer", "--steps", "2", "--warmup", "1", "--batch", "40", "--dump-outputs", str(tmp_path))
    assert j["unit"] == "tiles/s" and "roofline" not in j
    out = _load(tmp_path)
    assert list(out) == ["sr_tiles"] and out["sr_tiles"].shape == (32, 1, 256, 256) and out["sr_tiles"].dtype == np.float32
    assert np.isfinite(out["sr_tiles"]).all()
