"""bench.py on the GPU: a plain run prints the headline alone and `--dump-outputs` writes what the timed steps computed;
`--full` adds the measurements behind it and computes the same coherence."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--trials", "60"] + list(argv),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_runs(tmp_path):
    plain = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in HEADLINE_KEYS) and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["higher_is_better"] is True
    assert abs(plain["value"] * plain["ms_per_step"] / 1e3 - 60) < 0.01 * 60
    for k in ("roofline", "selfcheck", "secondary", "cpu_baseline", "value_f32_products", "detail"):
        assert k not in plain, k
    full = _bench("--steps", "2", "--warmup", "1", "--full", "--no-secondary", "--no-cpu-baseline",
                  "--dump-outputs", str(tmp_path / "full"))
    assert full["dtype"] == plain["dtype"] and full["selfcheck"]["max_err_over_tol"] <= 1.0 and "roofline" in full
    a = np.load(tmp_path / "plain" / "coherence_rows.npy")
    b = np.load(tmp_path / "full" / "coherence_rows.npy")
    assert a.dtype == np.float32 and a.shape == b.shape and a.nbytes <= 64 << 20
    assert np.isfinite(a).all()
    np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6)
