"""bench.py's plain run and --dump-outputs on a small mesh: the plain line carries the headline and nothing that takes runs of
its own, and the outputs of the last timed step are written as float32 arrays that are the same from run to run."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def run_bench(args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--nx", "64", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step(cuda, tmp_path):
    outs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = run_bench(["--steps", "3", "--warmup", "2", "--dump-outputs", str(d)])
        assert out["steps"] == 3 and out["warmup"] == 2 and out["n_gpus"] == 1
        assert out["ms_per_step"] > 0 and abs(out["value"] - 2.0 * out["config"]["g_ndof"] / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
        assert out["config"]["finite"]
        for key in ("stable_coefficient", "gmres_call", "roofline", "cpu_baseline", "action_ms", "roofline_sharded"):
            assert key not in out, key
        v, h = np.load(d / "krylov_vector.npy"), np.load(d / "hessenberg_column.npy")
        assert v.dtype == h.dtype == np.float32
        # five steps from the start of a cycle: the last one is k = 4, so v_5 and h_{0..5,4}
        assert v.shape == (out["config"]["n_traces"],) and h.shape == (6,)
        assert np.isfinite(v).all() and np.isfinite(h).all()
        assert abs(float(np.linalg.norm(v.astype(np.float64))) - 1.0) < 1e-4  # the new Arnoldi vector is normalised
        assert h[-1] > 0  # h_{k+1,k}: the norm v_{k+1} was divided by
        outs.append((v, h))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
