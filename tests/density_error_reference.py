"""Plain numpy restatement of ``DensityError`` (TEST INFRASTRUCTURE): float64 and int64, no torch,
written from the definition in the class's docstring / include/tfrt_hip.h at tfrt_density_error,
not from the kernels.

For the points (x, y) that count -- finite coordinates, ``mask[i] >= 0`` where a mask is given --:

* outside the closed domain on any axis: nothing goes to the histogram; the error gains
  ``oob_weight * (ex**2 + ey**2)``, ``ex = max(x0 - x, 0) + max(x - x1, 0)``;
* inside: ``u = (x - x0) * sx - 0.5``, ``i0 = floor(u)``, ``t = u - i0``; weight ``1 - t`` to column
  ``clamp(i0)``, ``t`` to ``clamp(i0 + 1)``; y alike; the four weights are the products;
* every weight enters its bin as the integer ``rint(w * 2**32)`` (``quantise=False``: as itself);
* ``H = Hq / 2**32``, ``s = ||H||``, ``h = H / s``, ``r = h - g``, ``E_hist = sum r**2``,
  ``D_b = (2 / s) (r_b - h_b sum_c h_c r_c)``; ``s == 0``: ``E_hist = sum g**2``, ``D = 0``.

``pairwise`` picks the order of the floating-point sums over bins and over penalties: numpy's
pairwise ``sum`` or a plain left-to-right one.  The tests' bounds must hold between the two.

Also the bounds the tests share, with their derivation (``error_bound``, ``gradient_bound``), and
the input sets (``points``)."""
import numpy as np

TWO32 = 4294967296.0
EPS = float(np.finfo(np.float64).eps)


def _sum(a, pairwise):
    a = np.asarray(a, dtype=np.float64).ravel()
    if a.size == 0:
        return 0.0
    return float(np.sum(a)) if pairwise else float(np.cumsum(a)[-1])


def _axis(v, lo, scale, nb):
    u = (v - lo) * scale - 0.5
    f = np.floor(u)
    i0 = f.astype(np.int64)
    return np.clip(i0, 0, nb - 1), np.clip(i0 + 1, 0, nb - 1), u - f


def normalise(goal):
    g = np.asarray(goal, dtype=np.float64)
    return g / np.sqrt(np.sum(g * g))


def density_error(x, y, goal, domain, oob_weight=0.0, mask=None, quantise=True, pairwise=True):
    """``goal``: (ny, nx) with ``y`` given, (nx,) with ``y`` None (normalised here).  Returns a
    dict: Hq (int64, None unquantised), H, s, error, e_hist, penalty, n_penalised, D, grad_x,
    grad_y (None without y), contributions (weights that entered each bin)."""
    g = normalise(goal)
    two = y is not None
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64) if two else np.zeros_like(x)
    nx = g.shape[-1]
    ny = g.shape[0] if two else 1
    (x0, x1) = domain[0]
    sx = np.float64(nx) / (np.float64(x1) - np.float64(x0))
    if two:
        (y0, y1) = domain[1]
        sy = np.float64(ny) / (np.float64(y1) - np.float64(y0))
    counts = np.isfinite(x) & np.isfinite(y)
    if mask is not None:
        counts &= np.asarray(mask) >= 0
    with np.errstate(invalid="ignore"):
        out = (x < x0) | (x > x1)
        if two:
            out |= (y < y0) | (y > y1)
    inside, outside = counts & ~out, counts & out

    gx, gy = np.zeros_like(x), np.zeros_like(x)
    xo, yo = x[outside], y[outside]
    ex = np.maximum(x0 - xo, 0.0) + np.maximum(xo - x1, 0.0)
    ey = (np.maximum(y0 - yo, 0.0) + np.maximum(yo - y1, 0.0)) if two else np.zeros_like(xo)
    penalty = _sum(oob_weight * (ex * ex + ey * ey), pairwise)
    gx[outside] = oob_weight * (2.0 * ex) * ((xo > x1).astype(np.float64) - (xo < x0))
    if two:
        gy[outside] = oob_weight * (2.0 * ey) * ((yo > y1).astype(np.float64) - (yo < y0))

    xi, yi = x[inside], y[inside]
    ia, ib, tx = _axis(xi, x0, sx, nx)
    if two:
        ja, jb, ty = _axis(yi, y0, sy, ny)
        index = [ja * nx + ia, ja * nx + ib, jb * nx + ia, jb * nx + ib]
        weight = [(1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx]
    else:
        index, weight = [ia, ib], [1.0 - tx, tx]
    bins = nx * ny
    contributions = np.zeros(bins, dtype=np.int64)
    for k in index:
        np.add.at(contributions, k, 1)
    if quantise:
        Hq = np.zeros(bins, dtype=np.int64)
        for k, w in zip(index, weight):
            np.add.at(Hq, k, np.rint(w * TWO32).astype(np.int64))
        H = Hq.astype(np.float64) / TWO32
    else:
        Hq = None
        H = np.zeros(bins, dtype=np.float64)
        for k, w in zip(index, weight):
            np.add.at(H, k, w)
    gf = g.reshape(-1)
    s = float(np.sqrt(_sum(H * H, pairwise)))
    if s == 0.0:
        e_hist, D = _sum(gf * gf, pairwise), np.zeros(bins)
    else:
        h = H / s
        r = h - gf
        e_hist = _sum(r * r, pairwise)
        D = (2.0 / s) * (r - h * _sum(h * r, pairwise))
    if two:
        d00, d01, d10, d11 = (D[k] for k in index)
        gx[inside] = sx * ((1.0 - ty) * (d01 - d00) + ty * (d11 - d10))
        gy[inside] = sy * ((1.0 - tx) * (d10 - d00) + tx * (d11 - d01))
    else:
        gx[inside] = sx * (D[ib] - D[ia])
    shape = g.shape
    return dict(Hq=None if Hq is None else Hq.reshape(shape), H=H.reshape(shape), s=s,
                error=e_hist + penalty, e_hist=e_hist, penalty=penalty,
                n_penalised=int(outside.sum()), D=D.reshape(shape), grad_x=gx,
                grad_y=gy if two else None, contributions=contributions.reshape(shape),
                sx=float(sx), sy=float(sy) if two else 0.0, bins=bins)


# ------------------------------------------------------------------------------ the bounds
def error_bound(ref):
    """|error - reference error| between two evaluations that agree on Hq and differ in the order
    of their float sums.  Histogram part: ``16 B eps`` -- both histograms have unit norm, so
    E_hist <= 4, and each of its B terms is summed with relative error below B eps.  Penalty part:
    a sum of m non-negative terms in any order is within (m - 1) eps of its exact value relative to
    the sum (Higham, Accuracy and Stability, eq. 4.4), so two orders differ by at most
    ``2 m eps * penalty``; without penalised rays the term is 0 and the bound is the first alone."""
    return 16.0 * ref["bins"] * EPS + 2.0 * ref["n_penalised"] * EPS * ref["penalty"]


def gradient_bound(ref):
    """|gradient - reference gradient| per entry of a ray inside: ``64 B eps (2 / s) max(sx, sy)``
    (the pulls are (2 / s) times differences of unit-norm quantities summed over B bins, a ray's
    gradient is sx or sy times a convex combination of differences of two pulls).  Rays outside
    and rays that do not count are computed by the same operations in the same order everywhere:
    they agree to the bit, which the bound admits."""
    s = ref["s"] if ref["s"] > 0 else 1.0
    return 64.0 * ref["bins"] * EPS * (2.0 / s) * max(ref["sx"], ref["sy"])


# ------------------------------------------------------------------------------ the inputs
DOMAIN = ((-1.0, 0.75), (0.5, 2.0))
BINS = ((1, 1), (4, 4), (7, 3), (64, 64), (256, 256))      # (nx, ny)


def goal_of(nx, ny, two=True):
    """A smooth positive goal with a zero stretch, (ny, nx) or (nx,)."""
    gx = (np.arange(nx) + 0.5) / nx
    if not two:
        g = 0.1 + np.exp(-((gx - 0.4) ** 2) / 0.05)
        if nx > 2:
            g[-1] = 0.0
        return g
    gy = (np.arange(ny) + 0.5) / ny
    g = 0.1 + np.exp(-((gx[None, :] - 0.4) ** 2 + (gy[:, None] - 0.6) ** 2) / 0.08)
    if nx > 2:
        g[:, -1] = 0.0
    return g


def points(n, dtype=np.float64, seed=11, domain=DOMAIN):
    """n points as (x, y, mask) in ``dtype``: most inside, about one in eight outside (either
    axis, either side), and -- as far as n allows -- the edge cases at fixed places: exactly on
    x0, on x1, on a bin centre of the 4-bin grid, a NaN, an infinity, a point outside on both axes.
    The mask switches every fifth point off."""
    rng = np.random.default_rng(seed + n)
    (x0, x1), (y0, y1) = domain
    x = rng.uniform(x0, x1, n)
    y = rng.uniform(y0, y1, n)
    far = rng.random(n) < 0.125
    x = np.where(far & (rng.random(n) < 0.5), x + (x1 - x0) * rng.choice([-1.0, 1.0], n), x)
    y = np.where(far & (rng.random(n) < 0.5), y - (y1 - y0) * rng.choice([-1.0, 1.0], n), y)
    special = [(x0, 0.5 * (y0 + y1)), (x1, y1), (x0 + 2.5 * (x1 - x0) / 4, y0 + 0.5 * (y1 - y0) / 4),
               (np.nan, y0), (x0, np.inf), (x1 + 0.25, y0 - 0.5)]
    for k, (sx, sy) in enumerate(special):
        at = 1 + 2 * k           # (odd places: 5 and 11 are masked off only where the mask is used)
        if at < n:
            x[at], y[at] = sx, sy
    mask = np.where(np.arange(n) % 5 == 4, -1, np.arange(n) % 7).astype(np.int32)
    return x.astype(dtype), y.astype(dtype), mask
