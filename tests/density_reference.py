"""Plain float64 numpy reference of the density points program (TFRT_PTS_DENSITY, TEST
INFRASTRUCTURE): scipy's linear interp1d restated as a lower-bound search, the x cell, the y = 0 rule
for cells the reference's loop never visits, the ranks from a second set of tables at the same
seeds, and ``source_reference``'s generator and transformation -- written from the reference
project's ArbitraryDistribution / ArbitraryBasePoints (tfrt/distributions.py:2123-2280, 2635-2798)
and the contract in include/tfrt_hip.h, not from the kernels.

Also the inputs the value tests share (``CASES``, ``GPU_DRAWS``): tests/test_density_reference_host.py
holds this restatement to ``ArbitraryDistribution.__call__`` bit for bit and asserts that no sample
of the GPU tests sits where one ulp could move it to another curve, so that
tests/test_gpu_density_program.py compares every sample."""
import collections
import functools

import numpy as np

import source_reference as sr

DENSITY = 5                  # TFRT_PTS_DENSITY of include/tfrt_hip.h

Tables = collections.namedtuple("Tables", "x_min x_max y_min y_max x_count y_count qx qy")


def interp(xs, ys, v):
    """scipy.interpolate.interp1d(xs, ys)(v), linear, xs sorted: k = clamp(first index with
    xs[k] >= v, 1, m - 1), the line through knots k - 1 and k."""
    xs, ys, v = np.asarray(xs), np.asarray(ys), np.asarray(v, dtype=np.float64)
    k = np.clip(np.searchsorted(xs, v, side="left"), 1, len(xs) - 1)
    x0, y0 = xs[k - 1], ys[k - 1]
    return (ys[k] - y0) / (xs[k] - x0) * (v - x0) + y0


def tables_of(distribution):
    """The knots of the interp1d objects an ArbitraryDistribution evaluates (their own sorted
    ``x`` / ``y``), with its rectangle and grid."""
    d = distribution
    return Tables(float(d._x_min), float(d._x_max), float(d._y_min), float(d._y_max),
                  int(d._x_count), int(d._y_count),
                  (np.array(d._x_quantile.x, dtype=np.float64), np.array(d._x_quantile.y, dtype=np.float64)),
                  [(np.array(q.x, dtype=np.float64), np.array(q.y, dtype=np.float64))
                   for q in d._y_quantiles])


def pack(t):
    """tfrt_points_program.density: [Qx.xs | Qx.ys | x_count x (Qy.xs | Qy.ys)]."""
    parts = [t.qx[0], t.qx[1]]
    for xs, ys in t.qy:
        parts.extend((xs, ys))
    out = np.concatenate(parts)
    assert out.shape == (2 * (t.x_count + 1) + 2 * t.x_count * (t.y_count + 1),)
    return out


def seeds(t, u0, u1):
    """The uniform point of the rectangle: tf.random.uniform's low + (high - low) u."""
    return t.x_min + (t.x_max - t.x_min) * u0, t.y_min + (t.y_max - t.y_min) * u1


def cell_coordinate(t, x):
    return (x - t.x_min) * t.x_count / (t.x_max - t.x_min)


def density_map(t, bx, by):
    """(x, y, cell): x = Qx(bx), cell = floor(cell_coordinate(x)), y = Qy[cell](by) -- 0 where the
    cell is not in [0, min(x_count, y_count)): the reference's loop runs over range(y_count)."""
    bx, by = np.asarray(bx, dtype=np.float64), np.asarray(by, dtype=np.float64)
    x = interp(t.qx[0], t.qx[1], bx)
    cell = np.floor(cell_coordinate(t, x)).astype(np.int64)
    y = np.zeros_like(by)
    for i in range(min(t.x_count, t.y_count)):
        pick = cell == i
        if pick.any():
            y[pick] = interp(t.qy[i][0], t.qy[i][1], by[pick])
    return x, y, cell


def points(t, u0, u1, rank_tables=None, rank_scale=1.0, scale=None, quat=None, shift=None):
    """Samples of the program from their two uniform numbers: (points (n, 3), aux0, aux1) -- the
    point (0, x, y) scaled, rotated and translated as ``source_reference.points`` does; aux the
    rank point (rank_scale times the rank tables' map of the same seeds), 0 without rank tables."""
    from oracle import sources as osources
    bx, by = seeds(t, np.asarray(u0, dtype=np.float64), np.asarray(u1, dtype=np.float64))
    x, y, _ = density_map(t, bx, by)
    pts = np.stack([np.zeros_like(x), x, y], axis=1)
    if scale is not None:
        pts = pts * np.asarray(scale, dtype=np.float64)
    if quat is not None:
        pts = osources.rotate_vector_by_quaternion(quat, pts)
    if shift is not None:
        pts = pts + np.asarray(shift, dtype=np.float64)
    if rank_tables is None:
        return pts, np.zeros_like(x), np.zeros_like(x)
    rx, ry, _ = density_map(rank_tables, bx, by)
    return pts, rank_scale * rx, rank_scale * ry


# ------------------------------------------------------------- the value tests' inputs
def _two_bumps(gx, gy):
    return 0.05 + np.exp(-((gx - 0.6) ** 2 + gy ** 2) / 0.08) + 0.6 * np.exp(-((gx - 1.5) ** 2 + (gy - 0.4) ** 2) / 0.05)


def _tilt(gx, gy):
    return 1.0 + 0.3 * gx + 0.1 * gy


def _array12():
    a = np.random.default_rng(5).uniform(0.2, 1.0, size=(12, 12))
    a[3:6, 2] = 0.0                  # zero stretches inside columns: equal neighbours in Qy.xs,
    a[0:2, 7] = 0.0                  # at the start of one,
    a[9:, 4] = 0.0                   # and at the end of another
    a[:, 5] *= 1e-3                  # a nearly empty column: a steep stretch of Qx
    return a


def _gauss64():
    g = np.linspace(-1.0, 1.0, 64)
    return np.exp(-(g[:, None] ** 2 + g[None, :] ** 2) / (2 * 0.35 ** 2))


# name: (density, evaluation limits) of the points' and of the ranks' distribution
CASES = {
    "one": ((np.ones((1, 1)), ((-1.0, 1.0), (-2.0, 2.0))),
            (np.full((1, 1), 3.0), ((-1.0, 1.0), (-2.0, 2.0)))),
    # x_count 5, y_count 3: cells 3 and 4 are never visited, their samples keep y = 0
    "callable53": ((_two_bumps, ((0.0, 2.0, 5), (-1.0, 1.0, 3))),
                   (_tilt, ((0.0, 2.0, 5), (-1.0, 1.0, 3)))),
    "array12": ((_array12(), ((-0.5, 1.5), (2.0, 3.0))),
                (np.ones((12, 12)), ((-0.5, 1.5), (2.0, 3.0)))),
    "gauss64": ((_gauss64(), ((-1.0, 1.0), (-1.0, 1.0))),
                (np.ones((64, 64)), ((-1.0, 1.0), (-1.0, 1.0)))),
}
GPU_CASES = ("callable53", "array12", "gauss64")
COUNTS = (1, 63, 64, 65, 1000)       # the wavefront's edges, and more than one block
N = max(COUNTS)


@functools.lru_cache(maxsize=None)
def distributions(name):
    """(points' ArbitraryDistribution, ranks' ArbitraryDistribution) of a case, made once."""
    import tfrt.distributions as d
    (density, limits), (rank_density, rank_limits) = CASES[name]
    return d.ArbitraryDistribution(density, limits), d.ArbitraryDistribution(rank_density, rank_limits)


@functools.lru_cache(maxsize=None)
def case_tables(name):
    return tuple(tables_of(x) for x in distributions(name))


# (label, case, seed, stream, epoch, first, count) of every draw the GPU tests compare: the classes
# (source_reference.SEED, stream 2, epochs 1 and 2), the C ABI's key and counter edges, the sources
# (stream 1, epochs 2 and 3) and the fused step's rays are not compared value by value
GPU_DRAWS = [(f"{name} epoch {epoch}", name, sr.SEED, sr.STREAM, epoch, 0, N)
             for name in GPU_CASES for epoch in sr.EPOCHS]
GPU_DRAWS += [(f"{name} C ABI", name, sr.ABI_SEED, sr.ABI_STREAM, sr.ABI_EPOCH, sr.ABI_FIRST, sr.ABI_N)
              for name in GPU_CASES]
GPU_DRAWS += [(f"{name} source epoch {epoch}", name, sr.SOURCE_SEED, 1, epoch, 0, N)
              for name in GPU_CASES for epoch in sr.SOURCE_EPOCHS]


@functools.lru_cache(maxsize=None)
def case_reference(name, ranked, transformed, epoch, seed=sr.SEED, stream=sr.STREAM, count=N, first=0,
                   rank_scale=1.0):
    """(points, aux0, aux1) of a case at (seed, stream, epoch), samples first .. first + count - 1;
    computed once, shared and never written to."""
    t, rt = case_tables(name)
    u0, u1 = sr.philox_uv(seed, stream, epoch, count, first)
    out = points(t, u0, u1, rt if ranked else None, rank_scale, **sr.transformation(transformed))
    for a in out:
        a.setflags(write=False)
    return out


def input_conditions(name, seed, stream, epoch, count, first=0):
    """From the reference alone, over both sets of tables of a case: (smallest distance of a
    sample's cell coordinate to an integer, smallest distance of a seed to a knot of the table it
    is looked up in, as a fraction of the table's range)."""
    u0, u1 = sr.philox_uv(seed, stream, epoch, count, first)
    cell_gap, knot_gap = np.inf, np.inf
    for t in case_tables(name):
        bx, by = seeds(t, u0, u1)
        x, _, cell = density_map(t, bx, by)
        c = cell_coordinate(t, x)
        cell_gap = min(cell_gap, float(np.abs(c - np.round(c)).min()))
        knot_gap = min(knot_gap, float(np.abs(bx[:, None] - t.qx[0][None, :]).min()) / (t.x_max - t.x_min))
        for i in range(min(t.x_count, t.y_count)):
            pick = cell == i
            if pick.any():
                gap = float(np.abs(by[pick][:, None] - t.qy[i][0][None, :]).min())
                knot_gap = min(knot_gap, gap / (t.y_max - t.y_min))
    return cell_gap, knot_gap
