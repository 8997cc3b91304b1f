"""bench.py command line (no GPU): `--gpus N` never lets one process stand for N ranks."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_gpus_n_without_torchrun_spawns_n_ranks(monkeypatch):
    """`python bench.py --gpus 2` (the driver's form, no WORLD_SIZE): the parent starts 2 worker
    ranks through torch.distributed.run before touching a GPU and exits with their status."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env

        class R:
            returncode = 7
        return R()

    import subprocess
    monkeypatch.setattr(subprocess, "run", fake_run)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available",
                        lambda: pytest.fail("the parent must not touch the GPU"))
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "2", "--steps", "3", "--warmup", "1"])
    assert e.value.code == 7                      # the children's status
    cmd = seen["cmd"]
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=2" in cmd and "127.0.0.1" in cmd
    k = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[k + 1:] == ["--gpus", "2", "--steps", "3", "--warmup", "1"]
    assert seen["env"].get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"


def test_world_size_mismatch_is_refused(monkeypatch):
    """Under a launcher, --gpus must equal the number of ranks actually running."""
    import torch
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    import tensorflowraytrace_amd.distributed as tdist
    monkeypatch.setattr(tdist, "init_from_env", lambda backend=None: (0, 1, 0))
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "8"])
    assert "--gpus 8" in str(e.value.code)


def test_single_gpu_needs_a_gpu(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(SystemExit) as e:
        bench.main([])
    assert "no CPU fallback" in str(e.value.code)


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main(["--steps", "0"])
    assert e.value.code == 2                      # argparse's usage error


class _Engine:
    """What snapshot_outputs reads of an engine: the last trace's counts and the four ray sets."""
    def __init__(self, n):
        import torch
        self.last_trace = {"counts": [torch.arange(8), torch.arange(8, 16)]}
        self.finished_rays = {"x_end": torch.arange(n, dtype=torch.float32),
                              "object_coords": torch.arange(3 * n, dtype=torch.float64).reshape(n, 3),
                              "ray_id": torch.arange(n, dtype=torch.int32)}
        self.dead_rays = {"x_end": torch.ones(5, dtype=torch.float32)}
        self.active_rays = self.stopped_rays = {}


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path):
    import numpy as np
    import torch
    n = bench.DUMP_ROWS_MAX + 1000
    params = {"front_parameters": torch.linspace(0, 1, 7, dtype=torch.float64, requires_grad=True)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), bench.snapshot_outputs(0.25, params, _Engine(n)))
    bench.dump_outputs(str(tmp_path / "b"), bench.snapshot_outputs(0.25, params, _Engine(n)))
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(k + ".npy" for k in shapes)
    assert {"error.npy", "front_parameters.npy", "ray_counts.npy", "finished_rows.npy",
            "finished_x_end.npy", "finished_object_coords.npy", "finished_ray_id.npy",
            "dead_x_end.npy"} == set(files)
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64), f
        np.testing.assert_array_equal(a, b)              # the same sample from run to run
        total += a.nbytes
    assert total <= bench.DUMP_BYTES_MAX
    assert float(np.load(tmp_path / "a" / "error.npy")) == 0.25
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "ray_counts.npy"),
                                  np.arange(16).reshape(2, 8))
    rows = np.load(tmp_path / "a" / "finished_rows.npy")
    assert rows.shape == (bench.DUMP_ROWS_MAX,) and np.all(np.diff(rows) > 0) and rows[-1] < n
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "finished_x_end.npy"), rows)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "finished_ray_id.npy"), rows)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "finished_object_coords.npy")[:, 0],
                                  3 * rows)
    assert np.load(tmp_path / "a" / "dead_x_end.npy").shape == (5,)   # small sets are kept whole
