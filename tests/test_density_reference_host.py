"""Guards of tests/density_reference.py, the float64 numpy reference that
tests/test_gpu_density_program.py holds the density points program (TFRT_PTS_DENSITY) to: the
restated search against ``ArbitraryDistribution.__call__`` (scipy's interp1d in the reference
project's loop) bit for bit, the host path of ``ArbitraryBasePoints`` fed the generator's numbers, and
the conditions on the GPU tests' inputs under which a one-ulp difference cannot move a sample to
another cell or another segment of a curve."""
import numpy as np
import pytest
import torch

import density_reference as dr
import source_reference as sr

N_HOST = 65536


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("which", [0, 1], ids=["points", "ranks"])
@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_restated_search_is_scipy_interp1d_in_the_reference_loop_bit_for_bit(name, which):
    dist = dr.distributions(name)[which]
    t = dr.case_tables(name)[which]
    u0, u1 = sr.philox_uv(sr.SEED, sr.STREAM, 1, N_HOST)
    bx, by = dr.seeds(t, u0, u1)
    want_x, want_y = dist(bx, by)
    x, y, cell = dr.density_map(t, bx, by)
    assert x.dtype == np.float64 and y.dtype == np.float64
    assert np.array_equal(x, want_x)
    assert np.array_equal(y, want_y)
    assert cell.min() >= 0 and cell.max() == t.x_count - 1          # every column is drawn from
    assert x.min() >= t.x_min and x.max() <= t.x_max and y.min() >= t.y_min and y.max() <= t.y_max
    # the packed layout is the one of the header, from the interp1d objects' own arrays
    packed = dist.packed_tables()
    assert packed.dtype == np.float64 and np.array_equal(packed, dr.pack(t))
    assert np.array_equal(packed[:t.x_count + 1], dist._x_quantile.x)
    assert bool((np.diff(packed[:t.x_count + 1]) >= 0).all())


def test_cells_the_reference_loop_never_visits_give_exactly_zero():
    """x_count = 5, y_count = 3: ``for i in range(self._y_count)`` visits cells 0, 1, 2."""
    dist, _ = dr.distributions("callable53")
    t, _ = dr.case_tables("callable53")
    assert (t.x_count, t.y_count) == (5, 3) and len(t.qy) == 5
    u0, u1 = sr.philox_uv(sr.SEED, sr.STREAM, 1, N_HOST)
    bx, by = dr.seeds(t, u0, u1)
    x, y, cell = dr.density_map(t, bx, by)
    late = cell >= 3
    assert 0.1 * N_HOST < late.sum() < 0.9 * N_HOST and set(np.unique(cell)) == {0, 1, 2, 3, 4}
    assert not y[late].any() and not dist(bx, by)[1][late].any()
    assert bool((y[~late] != 0.0).all())


def test_zero_stretches_leave_equal_knots_and_no_sample_between_them():
    """The 12 x 12 array: equal neighbours in three y tables; nothing is drawn where the density is
    zero, and the nearly empty column gets its share (1e-3 of a column's)."""
    t, _ = dr.case_tables("array12")
    density = dr.CASES["array12"][0][0]
    for column in (2, 7, 4):
        assert int((np.diff(t.qy[column][0]) == 0).sum()) >= 2
    u0, u1 = sr.philox_uv(sr.SEED, sr.STREAM, 1, N_HOST)
    x, y, cell = dr.density_map(t, *dr.seeds(t, u0, u1))
    assert np.isfinite(x).all() and np.isfinite(y).all()
    row = np.minimum(np.floor((y - t.y_min) * 12 / (t.y_max - t.y_min)).astype(int), 11)
    assert bool((density[row, cell] > 0).all())
    share = (cell == 5).mean()
    assert 0 < share < 5e-3 * density[:, 5].sum() / density.sum() * 1e3


@pytest.mark.parametrize("ranked", [False, True])
@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_reference_equals_the_host_path_fed_the_same_numbers(name, ranked, monkeypatch):
    """distributions._uniform hands out low + (high - low) u with u from ``philox_uv``: u0 for the x
    seeds, u1 for the y seeds, of the epoch the update makes."""
    import tfrt.distributions as d
    n = 257
    calls = [0]

    def uniform(count, low=0.0, high=1.0):
        assert int(count) == n
        epoch, which = calls[0] // 2 + 1, calls[0] % 2
        calls[0] += 1
        u = torch.from_numpy(sr.philox_uv(sr.SEED, sr.STREAM, epoch, n)[which].copy())
        return low + (high - low) * u

    monkeypatch.setattr(d, "_uniform", uniform)
    base, rank = dr.distributions(name)
    dist = d.ArbitraryBasePoints(base, n, rank_distribution=rank if ranked else None,
                                 conserve_etendue=False)
    assert not dist.__dict__.get("_device_active")
    dist.rank_scale_factor = 0.75
    dist.update()
    pts, a0, a1 = dr.case_reference(name, ranked, False, 2, count=n, rank_scale=0.75)
    assert np.array_equal(_np(dist.points), pts[:, 1:])
    if ranked:
        assert np.array_equal(_np(dist.ranks), np.stack([a0, a1], axis=1))
    else:
        assert dist.ranks is None and not a0.any() and not a1.any()


def test_reference_applies_source_references_transformation():
    t, rt = dr.case_tables("gauss64")
    u0, u1 = sr.philox_uv(3, 1, 1, 64)
    plain = dr.points(t, u0, u1)[0]
    moved, a0, a1 = dr.points(t, u0, u1, rt, 2.0, **sr.TRANSFORMATION)
    from oracle import sources as osources
    want = osources.rotate_vector_by_quaternion(sr.TRANSFORMATION["quat"],
                                                plain * np.array(sr.TRANSFORMATION["scale"]))
    np.testing.assert_allclose(moved, want + np.array(sr.TRANSFORMATION["shift"]), rtol=0, atol=1e-14)
    assert not plain[:, 0].any()
    # the flat rank density maps the seeds onto themselves: u in [0, 1) onto [-1, 1), times the scale
    np.testing.assert_allclose(a0, 2.0 * (2 * u0 - 1), rtol=0, atol=1e-14)
    np.testing.assert_allclose(a1, 2.0 * (2 * u1 - 1), rtol=0, atol=1e-14)


# ------------------------------------------------- conditions on the GPU tests' inputs
@pytest.mark.parametrize("label,name,seed,stream,epoch,first,count", dr.GPU_DRAWS,
                         ids=[c[0].replace(" ", "_") for c in dr.GPU_DRAWS])
def test_no_sample_of_the_gpu_tests_sits_on_a_cell_edge_or_a_knot(label, name, seed, stream, epoch,
                                                                  first, count):
    """The kernel may contract a product and a sum into one fma where numpy rounds twice: a sample
    whose cell coordinate is an integer to within rounding could take the next cell's y curve, and a
    seed on a knot the next segment.  With both kept away, the GPU comparison at 1e-13 leaves no
    sample out: the guards, not a tolerance, keep a one-ulp difference from switching curves."""
    cell_gap, knot_gap = dr.input_conditions(name, seed, stream, epoch, count, first)
    assert cell_gap > 1e-9, (label, cell_gap)
    assert knot_gap > 1e-12, (label, knot_gap)


def test_the_shared_references_are_computed_once_and_read_only():
    a = dr.case_reference("array12", True, False, 1)
    assert dr.case_reference("array12", True, False, 1) is a
    assert a[0].shape == (dr.N, 3) and not a[0].flags.writeable
    with pytest.raises(ValueError):
        a[1][0] = 1.0
