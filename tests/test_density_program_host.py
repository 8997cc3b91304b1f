"""The density points program without a GPU: csrc/density_map.h (the search and interpolation the
kernels inline) compiled for the host into a program of its own and held to
tests/density_reference.py; ``ArbitraryBasePoints`` on the CPU device, which stays out of device
mode and gives the numbers of the host code; ``auto_reroll=False``; and the ctypes mirror of the
fields appended to tfrt_points_program.  No kernel is launched here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import density_reference as dr
import source_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "density_map", "density_map_main.cpp")
N_HOST = 65536


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def density_map_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("density_map") / "density_map_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC,
                    MAIN, "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, tmp_path, t, bx, by):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([t.x_count, t.y_count, len(bx)], dtype=np.int64).tofile(f)
        np.array([t.x_min, t.x_max, t.y_min, t.y_max], dtype=np.float64).tofile(f)
        dr.pack(t).tofile(f)
        np.ascontiguousarray(bx, dtype=np.float64).tofile(f)
        np.ascontiguousarray(by, dtype=np.float64).tofile(f)
    subprocess.run([exe, str(src), str(dst)], check=True)
    out = np.fromfile(dst, dtype=np.float64)
    assert out.shape == (2 * len(bx),)
    return out[:len(bx)], out[len(bx):]


@pytest.mark.parametrize("which", [0, 1], ids=["points", "ranks"])
@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_host_compile_of_the_device_function_equals_the_reference(density_map_program, tmp_path,
                                                                 name, which):
    t = dr.case_tables(name)[which]
    u0, u1 = sr.philox_uv(sr.SEED, sr.STREAM, 1, N_HOST)
    bx, by = dr.seeds(t, u0, u1)
    want_x, want_y, cell = dr.density_map(t, bx, by)
    x, y = _run(density_map_program, tmp_path, t, bx, by)
    print(f"{name}: max |host program - reference| = "
          f"{max(np.abs(x - want_x).max(), np.abs(y - want_y).max()):.3e}")
    np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-13)
    np.testing.assert_allclose(y, want_y, rtol=0, atol=1e-13)
    if name == "callable53":
        assert (cell >= 3).any() and not y[cell >= 3].any()          # exactly 0


def test_host_compile_reads_inside_the_tables_for_seeds_outside_them(density_map_program, tmp_path):
    """The limits, seeds beyond them, infinities and a NaN: the search stays inside the table (a
    clamped segment is extrapolated) and the cell rule decides y; nothing is read by position."""
    t = dr.case_tables("array12")[0]
    bx = np.array([t.x_min, t.x_max, t.x_min - 1.0, t.x_max + 1.0, np.inf, -np.inf, np.nan, 0.3])
    by = np.array([t.y_min + 0.5, t.y_max, t.y_max + 5.0, t.y_min - 5.0, 2.5, 2.5, 2.5, np.nan])
    x, y = _run(density_map_program, tmp_path, t, bx, by)
    assert abs(x[0] - t.x_min) < 1e-13 and abs(x[1] - t.x_max) < 1e-13
    assert x[2] < t.x_min and y[2] == 0.0 and x[3] > t.x_max and y[3] == 0.0
    assert y[4] == 0.0 and y[5] == 0.0 and y[6] == 0.0
    assert np.isfinite(x[7]) and np.isnan(y[7])


def test_on_the_cpu_device_the_host_code_runs_number_for_number():
    import tfrt.distributions as d
    import tensorflowraytrace_amd.config as config
    assert config.get_device().type == "cpu"
    base, rank = dr.distributions("array12")
    n = 500
    d.seed(77)
    dist = d.ArbitraryBasePoints(base, n, rank_distribution=rank)
    d.BasePointTransformation(dist, translation=(-3.0, 0.0, 0.0))
    factor = dist.rank_scale_factor
    dist.update()
    assert not dist.__dict__.get("_device_active")
    # the code as it stands, recomputed: two draws per update (x seeds, then y seeds), scipy's map
    d.seed(77)
    t, _ = dr.case_tables("array12")
    for update in range(2):
        bx = d._uniform(n, t.x_min, t.x_max).cpu().numpy()
        by = d._uniform(n, t.y_min, t.y_max).cpu().numpy()
        pts = np.stack(base(bx, by), 1)
        ranks = np.stack(rank(bx, by), 1)
        if update == 0:     # enforce_etendue at construction: mean distances from the origin
            want_factor = float(torch.linalg.norm(torch.from_numpy(pts), dim=1).mean()
                                / torch.linalg.norm(torch.from_numpy(ranks), dim=1).mean())
            assert factor == want_factor
    assert np.array_equal(_np(dist.points), np.concatenate([np.zeros((n, 1)), pts], 1)
                          + np.array([-3.0, 0.0, 0.0]))
    assert np.array_equal(_np(dist.ranks), factor * ranks)
    # a source over it has no device program on the CPU
    import tfrt.sources as sources
    end = d.StaticUniformCircle(n, 0.5)
    d.BasePointTransformation(end)
    src = sources.AperatureSource(3, dist, end, [500.0], dense=False,
                                  extra_fields={"goal": ("start_point", dist, "ranks")})
    assert src._device_program() is None
    assert np.array_equal(_np(src["goal"]), _np(dist.ranks))


def test_without_auto_reroll_the_draw_is_kept_until_reroll():
    import tfrt.distributions as d
    base, rank = dr.distributions("callable53")
    d.seed(5)
    dist = d.ArbitraryBasePoints(base, 100, rank_distribution=rank, auto_reroll=False)
    first, first_ranks = dist.points.clone(), dist.ranks.clone()
    for _ in range(2):
        dist.update()
        assert torch.equal(dist.points, first) and torch.equal(dist.ranks, first_ranks)
    dist.reroll()
    dist.update()
    assert not torch.equal(dist.points, first)
    moving = d.ArbitraryBasePoints(base, 100, rank_distribution=rank)
    before = moving.points.clone()
    moving.update()
    assert not torch.equal(moving.points, before)


def test_device_mode_is_refused_where_the_program_cannot_say_the_same(monkeypatch):
    """Forced past the device check (no GPU here): what ``_device_mode`` itself decides."""
    import tfrt.distributions as d
    monkeypatch.setattr(d._DeviceRandom, "_device_mode", lambda self: True)
    base, rank = dr.distributions("array12")

    def mode(base_d, rank_d):
        dist = d.ArbitraryBasePoints.__new__(d.ArbitraryBasePoints)
        dist.base_point_distribution, dist.rank_distribution = base_d, rank_d
        return d.ArbitraryBasePoints._device_mode(dist)

    assert mode(base, None) and mode(base, rank)
    other_limits = d.ArbitraryDistribution(np.ones((12, 12)), ((-0.5, 1.5), (2.0, 3.5)))
    other_grid = d.ArbitraryDistribution(np.ones((6, 6)), ((-0.5, 1.5), (2.0, 3.0)))
    assert not mode(base, other_limits) and not mode(base, other_grid)
    assert not mode(lambda x, y: (x, y), None) and not mode(base, lambda x, y: (x, y))


def test_points_program_mirror_carries_the_density_fields_last(tmp_path):
    from tensorflowraytrace_amd import _lib
    names = [f[0] for f in _lib.PointsProgram._fields_]
    assert names[-5:] == ["x_count", "y_count", "density", "rank_density", "rank_scale"]
    assert names[-6] == "epoch" and _lib.PTS_DENSITY == 5
    # the fields before them sit where they sat: epoch at 160, the new ones behind it
    assert _lib.PointsProgram.epoch.offset == 160 and _lib.PointsProgram.x_count.offset == 168
    src = tmp_path / "kind.c"
    src.write_text('#include <stdio.h>\n#include "tfrt_hip.h"\n'
                   'int main(void){printf("%d %zu\\n", TFRT_PTS_DENSITY, sizeof(tfrt_points_program));'
                   'return 0;}\n')
    exe = tmp_path / "kind"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    kind, size = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(kind) == 5 and int(size) == ctypes.sizeof(_lib.PointsProgram)
