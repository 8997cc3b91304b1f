"""bench.py --dump-outputs on the device: exactly --steps timed steps, and two runs with the same
arguments write the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "2",
           "--rays", "20000", "--no-cpu-baseline", "--no-extra-legs", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dumped_outputs_are_the_same_from_run_to_run(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line_a, line_b = _bench(a, 3), _bench(b, 3)
    assert line_a["steps"] == line_b["steps"] == 3
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert names == sorted(k + ".npy" for k in line_a["dumped_outputs"]["arrays"])
    for must in ("error.npy", "front_parameters.npy", "back_parameters.npy", "ray_counts.npy",
                 "finished_y_end.npy", "finished_z_end.npy"):
        assert must in names
    total = 0
    for name in names:
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape, name
        assert np.all(np.isfinite(x)), name
        total += x.nbytes
        if name == "ray_counts.npy" or name.endswith("_rows.npy"):
            np.testing.assert_array_equal(x, y, err_msg=name)
        else:
            np.testing.assert_allclose(x, y, rtol=1e-9, atol=0, err_msg=name)
    assert total <= 64_000_000
    assert float(np.load(os.path.join(a, "error.npy"))) > 0.0
    counts = np.load(os.path.join(a, "ray_counts.npy"))
    assert counts.shape[1] == 8 and counts[0, :4].sum() == 20000     # every source ray enters pass 1
