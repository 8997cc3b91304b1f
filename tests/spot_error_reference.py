"""Plain numpy restatement of ``SpotError`` (TEST INFRASTRUCTURE): float64 and int64, no torch,
written from the definition in include/tfrt_hip.h at tfrt_spot_error, not from the kernels.

With k fields, a column i counts if ``mask`` is None or ``mask[i] >= 0``; ``terms = k *`` the
number of counting columns.  A counting column goes to the first case that applies:

* a coordinate is non-finite: nothing, gradient 0;
* ``s = perm[i]`` (``i`` without perm), ``label = group[s]``; ``s`` outside ``[0, n_source)`` or
  ``label`` outside ``[0, G)``: no spot, nothing, gradient 0;
* outside the closed domain on any axis: ``oob_weight * (ex**2 + ey**2)``,
  ``ex = max(x0 - x, 0) + max(x - x1, 0)``, and that expression's derivative;
* inside: ``qx = min(max(rint((x - x0) * qsx), 0), 2**qbits)`` (half to even), ``{1, qx, qy}`` is
  added to record ``label`` of the int64 table ``acc`` (``quantise=False``: ``{1, x, y}`` in
  float64, the plain form).

``cx = x0 + (Sx / count) / qsx`` (plain form: ``Sx / count``), ``dx = x - cx``, the terms are
``dx * dx`` and ``dy * dy``, the gradient rows ``2 * dx`` and ``2 * dy``.

Also the bound the tests share, with its derivation (``error_bound``), and the inputs (``points``).
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def qbits_of(n_source):
    return min(52, 62 - int(n_source).bit_length())


def spot_error(x, y, group, n_groups, domain, oob_weight=0.0, mask=None, perm=None, qbits=None,
               quantise=True):
    """``y`` None: one field.  Returns a dict: acc ((G, 4) int64, None unquantised), centroids
    ((G, k), NaN for empty groups), error, terms, mean, grad_x, grad_y (None without y),
    abs_sum (the sum of the absolute values of every term and penalty), n_inside, n_penalised, n,
    qsx, qsy."""
    two = y is not None
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    y = np.asarray(y, dtype=np.float64) if two else np.zeros_like(x)
    group = np.asarray(group)
    G = int(n_groups)
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
    if quantise:
        acc = np.zeros((G, 4), dtype=np.int64)
        np.add.at(acc[:, 0], li, 1)
        np.add.at(acc[:, 1], li, np.clip(np.rint((xi - x0) * qsx), 0.0, one).astype(np.int64))
        if two:
            np.add.at(acc[:, 2], li, np.clip(np.rint((yi - y0) * qsy), 0.0, one).astype(np.int64))
        with np.errstate(invalid="ignore", divide="ignore"):
            cnt = np.where(acc[:, 0] > 0, acc[:, 0].astype(np.float64), np.nan)
            cx = x0 + (acc[:, 1].astype(np.float64) / cnt) / qsx
            cy = (y0 + (acc[:, 2].astype(np.float64) / cnt) / qsy) if two else None
    else:
        acc = None
        cnt = np.zeros(G)
        sx, sy = np.zeros(G), np.zeros(G)
        np.add.at(cnt, li, 1.0)
        np.add.at(sx, li, xi)
        np.add.at(sy, li, yi)
        with np.errstate(invalid="ignore", divide="ignore"):
            cnt = np.where(cnt > 0, cnt, np.nan)
            cx = sx / cnt
            cy = sy / cnt if two else None
    dx = xi - cx[li]
    gx[inside] = 2.0 * dx
    terms = dx * dx
    if two:
        dy = yi - cy[li]
        gy[inside] = 2.0 * dy
        terms = terms + dy * dy
    error = float(np.sum(terms)) + float(np.sum(penalties))
    n_terms = float(int(counting.sum()) * (2 if two else 1))
    return dict(acc=acc, centroids=np.stack([cx, cy], axis=1) if two else cx[:, None],
                error=error, terms=n_terms, mean=error / n_terms if n_terms > 0 else float("nan"),
                grad_x=gx, grad_y=gy if two else None,
                abs_sum=float(np.sum(np.abs(terms)) + np.sum(np.abs(penalties))),
                n_inside=int(inside.sum()), n_penalised=int(outside.sum()), n=n,
                qsx=float(qsx), qsy=float(qsy), inside=inside, outside=outside)


def error_bound(ref):
    """|error - reference error| between two evaluations that agree on every term and penalty and
    differ in the order of their float sums: a sum of n numbers in ANY order is within
    (n - 1) eps sum|a_i| of the exact sum to first order (Higham, Accuracy and Stability, eq. 4.4);
    ``n eps sum|terms and penalties|`` is the worst case of any summation order.  Derived, not
    measured."""
    return ref["n"] * EPS * ref["abs_sum"]


# ------------------------------------------------------------------------------ the inputs
DOMAIN = ((-1.0, 0.75), (0.5, 2.0))
GROUPS = (1, 3, 64, 1024, 1025, 5000)


def points(n, dtype=np.float64, n_groups=3, seed=23, domain=DOMAIN):
    """n points as (x, y, mask, group, perm) in ``dtype``.  ``group`` holds one label per SOURCE
    ray (n + 3 of them, so a label table longer than the columns is covered), ``perm`` is a random
    permutation of the first n source rays with -- as far as n allows -- one entry below 0 and one
    past the source.  Most points are inside, about one in eight outside (either axis, either
    side); at fixed places: exactly x0, exactly x1 (closed domain: q = 0 and q = 2**qbits), a NaN,
    an infinity, a point outside on both axes, the labels -1 and G.  The last group is empty when
    G > 1 and the group before it holds a single ray when G > 2 and n allows.  The mask switches
    every fifth point off."""
    rng = np.random.default_rng(seed + 7 * n + n_groups)
    (x0, x1), (y0, y1) = domain
    x = rng.uniform(x0, x1, n)
    y = rng.uniform(y0, y1, n)
    far = rng.random(n) < 0.125
    x = np.where(far & (rng.random(n) < 0.5), x + (x1 - x0) * rng.choice([-1.0, 1.0], n), x)
    y = np.where(far & (rng.random(n) < 0.5), y - (y1 - y0) * rng.choice([-1.0, 1.0], n), y)
    special = [(x0, 0.5 * (y0 + y1)), (x1, y1), (np.nan, y0), (x0, np.inf), (x1 + 0.25, y0 - 0.5),
               (x1, y0)]
    for k, (sx, sy) in enumerate(special):
        at = 1 + 2 * k           # (odd places: 9 is masked off only where the mask is used)
        if at < n:
            x[at], y[at] = sx, sy
    mask = np.where(np.arange(n) % 5 == 4, -1, np.arange(n) % 7).astype(np.int32)
    n_source = n + 3
    G = int(n_groups)
    used = max(G - 2, 1) if G > 2 else 1          # labels that many rays share
    group = rng.integers(0, used, n_source).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    # columns 12, 14 and 16 are their own source rays, with and without perm
    for c in (12, 14, 16):
        if c < n:
            at = int(np.nonzero(perm == c)[0][0])
            perm[at], perm[c] = perm[c], c
    if n > 14:
        group[12], group[14] = -1, G
    if G > 2 and n > 16:
        group[16] = G - 2                         # a group of a single ray, inside and counting
        x[16], y[16] = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
        mask[16] = 0
    if n > 22:
        perm[20], perm[22] = -1, n_source
    return x.astype(dtype), y.astype(dtype), mask, group, perm
