"""Plain numpy restatement of ``DistortionError`` (TEST INFRASTRUCTURE): float64 and int64, no
torch, written from the definition in include/tfrt_hip.h at tfrt_distortion_error, not from the
kernels -- the order of every sum over the groups included.

The columns, the four cases of a counting column and the records ``{count, Sx, Sy, 0}`` are
``SpotError``'s (tests/spot_error_reference.py).  A group with ``count > 0`` is USED:
``w = count``, ``cx = x0 + (Sx / w) / qsx``, ``p`` its row of ``points``; with one field every y
component is 0.0.  Over the used groups:

* ``W = sum w``, ``pm = (sum w * p) / W``, ``cm = (sum w * c) / W``;
* ``dp = p - pm``, ``dc = c - cm``; ``Sxx, Sxy, Syy = sum w * (dp_a * dp_b)``;
  ``Cxx, Cxy, Cyx, Cyy = sum w * (dc_a * dp_b)``;
* ``"scale"`` (and ``"affine"`` with one field): ``M = (Cxx + Cyy) / (Sxx + Syy)``, ``A = M I``,
  valid iff two groups are used and ``Sxx + Syy > 0``; ``"affine"``: ``det = Sxx * Syy - Sxy *
  Sxy``, valid iff ``det > min_cond * (h * h)``, ``h = (Sxx + Syy) / 2``, ``A = Scp Spp^-1`` by
  cofactors;
* ``r = c - (cm + A dp)`` (zeros without a valid fit, NaN for an unused group),
  ``t = cm - A pm``;
* ``error = (sum w * (rx * rx) + sum w * (ry * ry)) + penalties``; a ray inside has the gradient
  ``2 * rx``, ``2 * ry`` of its group.

``fixed_sum`` is the shape of every sum over the groups.  Also the bound the tests share, with
its derivation (``error_bound``), and the inputs (``rays``).
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
BLOCK = 1024            # the threads of the one workgroup that sums over the groups
MIN_COND = 1e-9


def qbits_of(n_source):
    return min(52, 62 - int(n_source).bit_length())


def fixed_sum(values, used):
    """The sum of ``values[used]``: thread j of 1,024 adds the groups j, j + 1024, ... in
    ascending order onto 0.0, skipping unused ones; within each wave of 64 threads
    ``v[lane] += v[lane ^ d]`` for d = 32, 16, 8, 4, 2, 1; then the 16 waves are added in index
    order onto 0.0."""
    G = values.shape[0]
    lanes = np.zeros(BLOCK)
    for first in range(0, G, BLOCK):
        v, u = values[first:first + BLOCK], used[first:first + BLOCK]
        m = v.shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            lanes[:m] = np.where(u, lanes[:m] + v, lanes[:m])
    w = lanes.reshape(BLOCK // 64, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w[:, :d] + w[:, d:2 * d]
    total = np.float64(0.0)
    for wave in w[:, 0]:
        total = total + wave
    return total


def distortion_error(x, y, group, n_groups, points, domain, fit="scale", min_cond=MIN_COND,
                     oob_weight=0.0, mask=None, perm=None, qbits=None):
    """``y`` None: one field (``points`` is then (G, 1)).  Returns a dict: acc ((G, 4) int64),
    centroids ((G, k), NaN for unused groups), fit_out (8,), residual ((G, 2)), matrix, offset,
    valid, groups_used, used, means (pmx, pmy, cmx, cmy), moments (Sxx, Sxy, Syy, Cxx, Cxy, Cyx,
    Cyy), error, terms, mean, grad_x, grad_y (None without y), abs_sum, n,
    n_groups, n_inside, n_penalised, counting, inside, outside, label."""
    two = y is not None
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    y = np.asarray(y, dtype=np.float64) if two else np.zeros_like(x)
    group = np.asarray(group)
    points = np.asarray(points, dtype=np.float64)
    G = int(n_groups)
    assert points.shape == (G, 2 if two else 1) and fit in ("scale", "affine")
    if qbits is None:
        qbits = qbits_of(group.shape[0])
    one = np.ldexp(np.float64(1.0), qbits)
    (x0, x1) = (np.float64(v) for v in domain[0])
    qsx = one / (x1 - x0)
    (y0, y1) = (np.float64(v) for v in domain[1]) if two else (np.float64(0), np.float64(0))
    qsy = one / (y1 - y0) if two else np.float64(0)

    counting = np.ones(n, dtype=bool) if mask is None else np.asarray(mask)[:n] >= 0
    finite = np.isfinite(x) & np.isfinite(y)
    s = np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm)[:n].astype(np.int64)
    s_ok = (s >= 0) & (s < group.shape[0])
    label = np.full(n, -1, dtype=np.int64)
    label[s_ok] = group[s[s_ok]]
    spot = counting & finite & s_ok & (label >= 0) & (label < G)
    with np.errstate(invalid="ignore"):
        out = (x < x0) | (x > x1)
        if two:
            out |= (y < y0) | (y > y1)
    inside, outside = spot & ~out, spot & out

    gx, gy = np.zeros(n), np.zeros(n)
    xo, yo = x[outside], y[outside]
    ex = np.maximum(x0 - xo, 0.0) + np.maximum(xo - x1, 0.0)
    ey = (np.maximum(y0 - yo, 0.0) + np.maximum(yo - y1, 0.0)) if two else np.zeros_like(xo)
    penalties = oob_weight * (ex * ex + ey * ey)
    gx[outside] = oob_weight * (2.0 * ex) * ((xo > x1).astype(np.float64) - (xo < x0))
    if two:
        gy[outside] = oob_weight * (2.0 * ey) * ((yo > y1).astype(np.float64) - (yo < y0))

    xi, yi, li = x[inside], y[inside], label[inside]
    acc = np.zeros((G, 4), dtype=np.int64)
    np.add.at(acc[:, 0], li, 1)
    np.add.at(acc[:, 1], li, np.clip(np.rint((xi - x0) * qsx), 0.0, one).astype(np.int64))
    if two:
        np.add.at(acc[:, 2], li, np.clip(np.rint((yi - y0) * qsy), 0.0, one).astype(np.int64))

    used = acc[:, 0] > 0
    w = acc[:, 0].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cx = x0 + (acc[:, 1].astype(np.float64) / w) / qsx
        cy = (y0 + (acc[:, 2].astype(np.float64) / w) / qsy) if two else np.zeros(G)
        px = points[:, 0]
        py = points[:, 1] if two else np.zeros(G)
        W = fixed_sum(w, used)
        pmx, pmy = fixed_sum(w * px, used) / W, fixed_sum(w * py, used) / W
        cmx, cmy = fixed_sum(w * cx, used) / W, fixed_sum(w * cy, used) / W
        dpx, dpy, dcx, dcy = px - pmx, py - pmy, cx - cmx, cy - cmy
        Sxx = fixed_sum(w * (dpx * dpx), used)
        Sxy = fixed_sum(w * (dpx * dpy), used)
        Syy = fixed_sum(w * (dpy * dpy), used)
        Cxx = fixed_sum(w * (dcx * dpx), used)
        Cxy = fixed_sum(w * (dcx * dpy), used)
        Cyx = fixed_sum(w * (dcy * dpx), used)
        Cyy = fixed_sum(w * (dcy * dpy), used)
        n_used = int(used.sum())
        trp = Sxx + Syy
        if fit == "affine" and two:
            det = Sxx * Syy - Sxy * Sxy
            h = trp / 2.0
            valid = bool(det > min_cond * (h * h))
            A = np.array([(Cxx * Syy - Cxy * Sxy) / det, (Cxy * Sxx - Cxx * Sxy) / det,
                          (Cyx * Syy - Cyy * Sxy) / det, (Cyy * Sxx - Cyx * Sxy) / det])
        else:
            valid = n_used >= 2 and bool(trp > 0.0)
            M = (Cxx + Cyy) / trp
            A = np.array([M, 0.0, 0.0, M])
        fit_out = np.full(8, np.nan)
        residual = np.full((G, 2), np.nan)
        if valid:
            fit_out[:4] = A
            fit_out[4] = cmx - (A[0] * pmx + A[1] * pmy)
            fit_out[5] = cmy - (A[2] * pmx + A[3] * pmy)
            residual[used, 0] = (cx - (cmx + (A[0] * dpx + A[1] * dpy)))[used]
            residual[used, 1] = (cy - (cmy + (A[2] * dpx + A[3] * dpy)))[used]
        else:
            residual[used] = 0.0
        fit_out[6], fit_out[7] = float(valid), float(n_used)
        tx, ty = w * (residual[:, 0] * residual[:, 0]), w * (residual[:, 1] * residual[:, 1])
        e_inside = fixed_sum(tx, used) + fixed_sum(ty, used)
    gx[inside] = 2.0 * residual[li, 0]
    if two:
        gy[inside] = 2.0 * residual[li, 1]
    error = float(e_inside + np.sum(penalties))
    n_terms = float(int(counting.sum()) * (2 if two else 1))
    centroids = np.where(used[:, None], np.stack([cx, cy], axis=1), np.nan)[:, :2 if two else 1]
    k = 2 if two else 1
    return dict(acc=acc, centroids=centroids, fit_out=fit_out, residual=residual,
                matrix=fit_out[:4].reshape(2, 2)[:k, :k], offset=fit_out[4:4 + k], valid=valid,
                groups_used=n_used, error=error, terms=n_terms, used=used,
                means=np.array([pmx, pmy, cmx, cmy]),
                moments=np.array([Sxx, Sxy, Syy, Cxx, Cxy, Cyx, Cyy]),
                mean=error / n_terms if n_terms > 0 else float("nan"),
                grad_x=gx, grad_y=gy if two else None,
                abs_sum=float(np.sum(tx[used]) + np.sum(ty[used]) + np.sum(np.abs(penalties))),
                n=n, n_groups=G, n_inside=int(inside.sum()), n_penalised=int(outside.sum()),
                counting=counting, inside=inside, outside=outside, label=label)


def error_bound(ref):
    """|error - reference error| between two evaluations that agree on every group's term and
    every penalty and differ in the order of their float sums: a sum of m numbers in ANY order is
    within (m - 1) eps sum|a_i| of the exact sum to first order (Higham, Accuracy and Stability,
    eq. 4.4), so two orders differ by at most twice that; here m <= n penalties + 2 G group terms,
    all non-negative.  Derived, not measured."""
    return 2.0 * (ref["n"] + 2 * ref["n_groups"]) * EPS * ref["abs_sum"]


# ------------------------------------------------------------------------------ the inputs
DOMAIN = ((-1.0, 0.75), (0.5, 2.0))
PLANTED_A = np.array([[1.1, 0.15], [-0.2, 0.9]])
PLANTED_T = np.array([-0.1, 1.2])
OOB = 0.3


def object_points(n_groups):
    """(G, 2) object points: a square grid over [-0.5, 0.5]^2, row by row."""
    G = int(n_groups)
    side = max(int(np.ceil(np.sqrt(G))), 2)
    g = np.arange(G)
    return np.stack([(g % side) / (side - 1) - 0.5, (g // side) / (side - 1) - 0.5], axis=1)


def image_of(points, cubic=0.1):
    """The planted image of the object points: ``A p + t`` plus the cubic distortion
    ``cubic * |p|^2 p``; it lies inside ``DOMAIN``."""
    r2 = (points * points).sum(axis=1, keepdims=True)
    return points @ PLANTED_A.T + PLANTED_T + cubic * r2 * points


def rays(n, n_groups=3, dtype=np.float64, permuted=False, seed=41, noise=0.01, cubic=0.1):
    """n columns as (x, y, mask, group, perm, points) with x, y in ``dtype``.  ``group`` holds one
    label per SOURCE ray (n + 3 of them); ``perm`` is a random permutation of the first n source
    rays with -- as far as n allows -- one entry below 0 and one past the source.  Column i lies
    at the planted image of the object point of ITS group (through ``perm`` when ``permuted``)
    plus noise; about one column in sixteen is thrown outside the domain (either axis, either
    side); at fixed places: exactly x0, exactly (x1, y1), a NaN, an infinity, a point outside on
    both axes, the labels -1 and G.  The last group is empty when G > 3.  The mask switches every
    fifth column off."""
    rng = np.random.default_rng(seed + 7 * n + n_groups + (1000003 if permuted else 0))
    G = int(n_groups)
    (x0, x1), (y0, y1) = DOMAIN
    points = object_points(G)
    image = image_of(points, cubic)
    n_source = n + 3
    used = G - 1 if G > 3 else G       # (three groups are the fewest a case may use)
    group = rng.integers(0, used, n_source).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    for c in (12, 14):           # columns 12 and 14 are their own source rays, with and without perm
        if c < n:
            at = int(np.nonzero(perm == c)[0][0])
            perm[at], perm[c] = perm[c], c
    if n > 14:
        group[12], group[14] = -1, G
    if n > 22:
        perm[20], perm[22] = -1, n_source
    s = perm.astype(np.int64) if permuted else np.arange(n)
    lab = group[np.clip(s, 0, n_source - 1)].astype(np.int64)
    at = image[np.clip(lab, 0, G - 1)]
    x = at[:, 0] + noise * rng.standard_normal(n)
    y = at[:, 1] + noise * rng.standard_normal(n)
    far = rng.random(n) < 1.0 / 16.0
    x = np.where(far & (rng.random(n) < 0.5), x + (x1 - x0) * rng.choice([-1.0, 1.0], n), x)
    y = np.where(far & (rng.random(n) < 0.5), y - (y1 - y0) * rng.choice([-1.0, 1.0], n), y)
    special = [(x0, 0.5 * (y0 + y1)), (x1, y1), (np.nan, y0), (x0, np.inf), (x1 + 0.25, y0 - 0.5)]
    for k, (sx, sy) in enumerate(special):
        if 1 + 2 * k < n:        # (odd places: 9 is masked off only where the mask is used)
            x[1 + 2 * k], y[1 + 2 * k] = sx, sy
    mask = np.where(np.arange(n) % 5 == 4, -1, np.arange(n) % 7).astype(np.int32)
    return x.astype(dtype), y.astype(dtype), mask, group, perm, points


def assert_generator(ref):
    """What a case with n >= 1000 must give, on the reference alone: a valid fit, at least three
    used groups, more than half of the counting columns inside."""
    assert ref["valid"], ref["fit_out"]
    assert ref["groups_used"] >= 3, ref["groups_used"]
    assert 2 * ref["n_inside"] > int(ref["counting"].sum()), (ref["n_inside"], ref["counting"].sum())
