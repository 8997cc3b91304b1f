"""Plain float64 numpy reference of the 3-D source programs (TEST INFRASTRUCTURE): the generator, the
four procedural point distributions with their transformation, and the draw of a ray pool -- written
from the reference project's formulas (tfrt/distributions.py:1375-1393 square, 1396-1447 theta wedge,
1586-1598 circle, 1751-1775 / 1814-1850 spherical caps, 2014-2120 BasePointTransformation;
tfrt/sources.py:1099-1358 PrecompiledSource) and from the contract in include/tfrt_hip.h, not from
the kernels.  The assembly of rays from points is oracle/sources.py's; nothing of it is repeated here.

Also the inputs the value tests share (``POINT_CASES``, ``SEED``, ...): tests/test_source_reference_host.py
asserts on the reference alone that none of their samples sits where rounding could move a result by
more than the tests' tolerance, so that tests/test_gpu_source_programs_exact.py compares every sample."""
import functools
import math

import numpy as np

from oracle import sources as osources

PI = math.pi
# TFRT_PTS_* of include/tfrt_hip.h
CIRCLE, SQUARE, SPHERE_UNIFORM, SPHERE_LAMBERT = 1, 2, 3, 4

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


# ------------------------------------------------------------------------------ generator
def philox_words(seed, stream, epoch, n, first=0):
    """The four 32-bit output words (uint64 arrays of n) of Philox4x32-10 for samples
    first .. first + n - 1: counter (sample lo, sample hi, epoch lo, epoch hi), key
    (seed lo, seed hi ^ stream); seed, epoch and the sample numbers are 64-bit."""
    seed, epoch, first = int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), int(first) & (2 ** 64 - 1)
    i = np.arange(n, dtype=np.uint64) + np.full(n, first, dtype=np.uint64)      # (wraps at 2^64)
    c = [i & _M32, i >> _S32, np.full(n, epoch & 0xFFFFFFFF, dtype=np.uint64),
         np.full(n, epoch >> 32, dtype=np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) ^ int(stream)) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]          # (32 x 32 bits: no overflow in 64)
        p1 = np.uint64(0xCD9E8D57) * c[2]
        n0 = (p1 >> _S32) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & _M32, n2, p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def words_to_uv(words):
    """Two float64 in [0, 1): the upper 53 bits of words (0, 1) and of words (2, 3)."""
    a, b = (words[0] << _S32) | words[1], (words[2] << _S32) | words[3]
    return ((a >> np.uint64(11)).astype(np.float64) * 2.0 ** -53,
            (b >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)


def philox_uv(seed, stream, epoch, n, first=0):
    """Both float64 numbers in [0, 1) of Philox4x32-10 at (seed, stream, epoch) for samples
    first .. first + n - 1 (``philox_words`` through ``words_to_uv``)."""
    return words_to_uv(philox_words(seed, stream, epoch, n, first))


# ------------------------------------------------------------------------------- points
def theta_mod(theta, theta_start, theta_end):
    """ThetaMod (distributions.py:1434-1446): the identity for (0, 2 pi), else theta folded into
    [theta_start, theta_end) with the sign of the divisor (Python's %)."""
    if theta_start == 0 and theta_end == 2 * PI:
        return theta
    return np.mod(theta, theta_end - theta_start) + theta_start


def unfolded_theta(kind, u1):
    """The azimuth before ``theta_mod``: 2 pi u (circle), pi (1 + sqrt 5) u (caps); None: no azimuth."""
    if kind == CIRCLE:
        return 2 * PI * u1
    if kind in (SPHERE_UNIFORM, SPHERE_LAMBERT):
        return PI * (1 + 5 ** 0.5) * u1
    return None


def points(kind, params, u0, u1, scale=None, quat=None, shift=None):
    """Samples of a procedural distribution from their two uniform numbers: (points (n, 3), aux0,
    aux1).  ``params`` as tfrt_points_program.p: circle (radius, theta_start, theta_end, -), square
    (x_size, -, -, y_size), caps (radius, theta_start, theta_end, lo) with lo = cos(angular size)
    [uniform] or its square [Lambertian].  A planar distribution lies in the y-z plane.  aux: (r,
    theta) of a circle, the plane point of a square, (phi, theta) of a cap.  Then scale, rotation
    by the unit quaternion (w, x, y, z), translation."""
    u0, u1 = np.asarray(u0, dtype=np.float64), np.asarray(u1, dtype=np.float64)
    zero = np.zeros_like(u0)
    if kind == CIRCLE:
        radius, t0, t1 = params[0], params[1], params[2]
        r = np.sqrt(u0)
        theta = theta_mod(unfolded_theta(kind, u1), t0, t1)
        pts = radius * np.stack([zero, r * np.cos(theta), r * np.sin(theta)], axis=1)
        aux0, aux1 = r, theta
    elif kind == SQUARE:
        xs, ys = params[0], params[3]
        y = -xs + (xs - -xs) * u0                     # tf.random.uniform(minval, maxval)
        z = -ys + (ys - -ys) * u1
        pts = np.stack([zero, y, z], axis=1)
        aux0, aux1 = y, z
    elif kind in (SPHERE_UNIFORM, SPHERE_LAMBERT):
        radius, t0, t1, lo = params
        c = lo + (1.0 - lo) * u0
        phi = np.arccos(np.sqrt(c) if kind == SPHERE_LAMBERT else c)
        theta = theta_mod(unfolded_theta(kind, u1), t0, t1)
        pts = radius * np.stack([np.cos(phi), np.sin(phi) * np.cos(theta),
                                 np.sin(phi) * np.sin(theta)], axis=1)
        aux0, aux1 = phi, theta
    else:
        raise ValueError(f"points: kind {kind}")
    if scale is not None:
        pts = pts * np.asarray(scale, dtype=np.float64)
    if quat is not None:
        pts = osources.rotate_vector_by_quaternion(quat, pts)
    if shift is not None:
        pts = pts + np.asarray(shift, dtype=np.float64)
    return pts, aux0, aux1


def class_properties(kind, params, pts, aux0, aux1, transformed):
    """What the distribution classes publish, from ``points``' results (distributions.py:1352-1372,
    1540-1567, 1709-1715): a circle's and a square's ``points`` are the plane's two columns until a
    transformation lifts them."""
    out = {"points": pts if (transformed or kind in (SPHERE_UNIFORM, SPHERE_LAMBERT)) else pts[:, 1:]}
    if kind == CIRCLE:
        out["ranks"] = np.stack([aux0 * np.cos(aux1), aux0 * np.sin(aux1)], axis=1)
        out["polar_ranks"] = np.stack([aux0, np.mod(aux1, 2 * PI)], axis=1)
    elif kind == SQUARE:
        out["ranks"] = np.stack([aux0, aux1], axis=1) / max(params[0], params[3])
    else:
        out["ranks"] = np.stack([aux0, np.mod(aux1, 2 * PI)], axis=1)
        out["angles"] = out["points"]
    return out


# --------------------------------------------------------------------------------- pool
def pool_rays(pool, numbers, sigma_start, sigma_end, downsample):
    """The draw of a TFRT_SRC_POOL program as include/tfrt_hip.h states it: (rows, start, end).
    ``pool`` (count, 2 axes) records, start point then end point; ``numbers[0]`` the (u0, u1) of
    stream pool_stream (the rows), ``numbers[1 + q]`` the (u, v) of stream pool_stream + 1 + q
    (the normals of axis q).  Row min(floor(u0 count), count - 1), or the ray's own number without
    down-sampling; r = sqrt(-2 log(1 - u)), the start moves by sigma r cos 2 pi v, the end by
    sigma r sin 2 pi v; a coordinate whose sigma is 0 is the stored one."""
    pool = np.asarray(pool, dtype=np.float64)
    count, axes = pool.shape[0], pool.shape[1] // 2
    n = len(numbers[0][0])
    if downsample:
        rows = np.minimum(np.floor(numbers[0][0] * count), count - 1).astype(np.int64)
    else:
        rows = np.arange(n, dtype=np.int64)
    start, end = pool[rows, :axes].copy(), pool[rows, axes:].copy()
    for q in range(axes):
        if sigma_start[q] == 0.0 and sigma_end[q] == 0.0:
            continue
        u, v = numbers[1 + q]
        r = np.sqrt(-2.0 * np.log(1.0 - u))
        if sigma_start[q] != 0.0:
            start[:, q] += sigma_start[q] * (r * np.cos(2 * PI * v))
        if sigma_end[q] != 0.0:
            end[:, q] += sigma_end[q] * (r * np.sin(2 * PI * v))
    return rows, start, end


# ------------------------------------------------------------- the value tests' inputs
COUNTS = (1, 257, 5003)      # one lane; a partial second block; no multiple of any block size
N = max(COUNTS)              # (sample i does not depend on the count: the smaller are prefixes)
SEED = 92
STREAM = 2                   # (a filler distribution takes stream 1)
EPOCHS = (1, 2)

_Q = np.array([0.9, 0.1, -0.3, 0.2])
TRANSFORMATION = dict(scale=(1.0, 2.0, 0.5), quat=tuple(_Q / np.sqrt((_Q * _Q).sum())),
                      shift=(-3.0, 1.0, 2.0))

# name: (class, constructor arguments after / around the sample count, kind, params)
CAP = 1.2                    # angular size of the caps
POINT_CASES = {
    "circle": dict(cls="RandomUniformCircle", make=lambda c, n: c(n, 0.7),
                   kind=CIRCLE, params=(0.7, 0.0, 2 * PI, 0.0)),
    "circle_wedge": dict(cls="RandomUniformCircle",
                         make=lambda c, n: c(n, 1.3, theta_start=0.0, theta_end=PI / 6),
                         kind=CIRCLE, params=(1.3, 0.0, PI / 6, 0.0)),
    "square": dict(cls="RandomUniformSquare", make=lambda c, n: c(0.5, n, 0.25, 1),
                   kind=SQUARE, params=(0.5, 0.0, 0.0, 0.25)),
    "sphere_uniform": dict(cls="RandomUniformSphere", make=lambda c, n: c(CAP, n, radius=2.0),
                           kind=SPHERE_UNIFORM, params=(2.0, 0.0, 2 * PI, math.cos(CAP))),
    "sphere_lambert": dict(cls="RandomLambertianSphere", make=lambda c, n: c(CAP, n, radius=2.0),
                           kind=SPHERE_LAMBERT, params=(2.0, 0.0, 2 * PI, math.cos(CAP) ** 2)),
    # (beyond the five above: a whole hemisphere, and a wedge that does not start at 0 on a cap)
    "hemisphere": dict(cls="RandomUniformSphere", make=lambda c, n: c(PI / 2, n, radius=2.0),
                       kind=SPHERE_UNIFORM, params=(2.0, 0.0, 2 * PI, math.cos(PI / 2))),
    "sphere_wedge": dict(cls="RandomUniformSphere",
                         make=lambda c, n: c(CAP, n, radius=1.5, theta_start=-PI / 4, theta_end=PI / 3),
                         kind=SPHERE_UNIFORM, params=(1.5, -PI / 4, PI / 3, math.cos(CAP))),
}

# the C ABI's key and counter edges: the seed's high word set (the stream XORs into it), the
# epoch's high word set, samples read through `first` and an index
ABI_SEED = 0x9E3779B97F4A7C15
ABI_STREAM = 5
ABI_EPOCH = 2 ** 32 + 3
ABI_COUNT, ABI_FIRST, ABI_N = 1300, 1000, 257
# (sample 1000 + j, j < 257, with the largest u0 lies too close to the pole for the narrower caps'
# acos -- see input_conditions -- so the caps are represented by the hemisphere here)
ABI_CASES = ("circle", "circle_wedge", "square", "hemisphere")


# the sources' inputs: POINT_CASES entries on the streams the sources' distributions take after
# seed(SOURCE_SEED), first drawn from by the source's constructor (epoch 2: every distribution
# updated once at its own construction) and again after one more update (epoch 3)
SOURCE_SEED = 216
SOURCE_EPOCHS = (2, 3)
TRANSFORMATION_B = dict(quat=tuple(_Q[[1, 0, 3, 2]] / np.sqrt((_Q * _Q).sum())), shift=(4.0, -0.5, 0.25))
SOURCE_CAPS = (("sphere_lambert", 1), ("sphere_uniform", 2))      # (case, stream): see the sources


def transformation(transformed):
    return TRANSFORMATION if transformed else {}


@functools.lru_cache(maxsize=None)
def case_reference(name, transformed, epoch, seed=SEED, stream=STREAM, count=N):
    """(points, aux0, aux1) of a POINT_CASES entry at (seed, stream, epoch), all `count` samples;
    computed once, shared and never written to."""
    case = POINT_CASES[name]
    u0, u1 = philox_uv(seed, stream, epoch, count)
    out = points(case["kind"], case["params"], u0, u1, **transformation(transformed))
    for a in out:
        a.setflags(write=False)
    return out


def fold_distance(theta, span):
    """Distance of every theta to the nearest multiple of span."""
    m = np.mod(theta, span)
    return np.minimum(m, span - m)


def input_conditions(name, seed, stream, epoch, count, first=0):
    """The two conditions on a case's inputs, from the reference alone: (smallest distance of an
    azimuth to a fold -- of the unfolded one to a multiple of the wedge's span, of the folded one
    to a multiple of 2 pi, where the ranks' floormod folds -- or None; the error bound
    8 * 2^-52 / sin(phi_min) of a cap's acos, or None), over samples first .. first + count - 1."""
    case = POINT_CASES[name]
    kind, params = case["kind"], case["params"]
    u0, u1 = philox_uv(seed, stream, epoch, count, first)
    theta = unfolded_theta(kind, u1)
    fold = None
    if theta is not None:
        fold = float(fold_distance(theta_mod(theta, params[1], params[2]), 2 * PI).min())
        if not (params[1] == 0 and params[2] == 2 * PI):
            fold = min(fold, float(fold_distance(theta, params[2] - params[1]).min()))
    acos_bound = None
    if kind in (SPHERE_UNIFORM, SPHERE_LAMBERT):
        phi = points(kind, params, u0, u1)[1]
        acos_bound = 8 * 2.0 ** -52 / float(np.sin(phi).min())
    return fold, acos_bound
