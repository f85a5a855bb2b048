"""bench.py's plain run (no --full): one result line with the headline keys, exactly --steps timed steps, and --dump-outputs files that two runs with
the same arguments reproduce."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--n", "512", "--m", "512",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]  # a plain run prints its result line and nothing else
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_result_line_and_dumped_outputs(tmp_path):
    a = _run(tmp_path / "a", 3)
    b = _run(tmp_path / "b", 4)
    for line, steps in ((a, 3), (b, 4)):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == steps and line["dtype"] == "f64" and line["higher_is_better"] is True
        assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 1.0) < 1e-9
        assert line["parity"]["rel_kkt_residual"] <= 1e-10
        assert "roofline" not in line and "legs" not in line  # the per-kernel pass and the secondary legs are --full only
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"predictor_x.npy", "corrector_x.npy", "predictor_z_l.npy", "corrector_z_u.npy"} <= set(names)
    # 3 and 4 steps end on different states and right-hand sides (they alternate): compare runs of the same length for reproducibility
    c = _run(tmp_path / "c", 3)
    assert c["steps"] == 3
    for f in names:
        x, z = np.load(tmp_path / "a" / f), np.load(tmp_path / "c" / f)
        assert x.dtype == np.float64 and x.size and np.all(np.isfinite(x)), f
        assert np.abs(x - z).max() <= 1e-9 * (1.0 + np.abs(x).max()), f
