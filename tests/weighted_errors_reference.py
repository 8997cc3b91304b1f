"""Plain numpy restatement of the WEIGHTED ``DensityError`` and ``SpotError`` (TEST
INFRASTRUCTURE): float64, int64 and Python integers, no torch, written from the definitions in
include/tfrt_hip.h at tfrt_density_error_weighted and tfrt_spot_error_weighted, not from the
kernels.

Every source ray carries a weight; column i is source ray ``s = perm[i]`` (``i`` without perm).  A
counting column whose ``s`` lies outside ``[0, n_source)``, or whose ``w = weight[s]`` is not
finite or not in [0, 1], "does not count" (density) / is in "no spot" (spot): no error, gradient 0.

Density: an inside ray adds ``rint(((bx * by) * w) * 2**32)`` to its bins, its gradient is the
unweighted expression times ``w`` last; an outside ray's penalty and gradient are multiplied by
``w`` last; norm, pulls and E_hist come from the weighted histogram as in
tests/density_error_reference.py.

Spot: ``wq = rint(w * 2**wbits)`` (half to even), ``wr = wq * 2**-wbits`` is the weight everywhere;
``wq == 0``: no spot.  With ``h = qbits // 2`` the record of a group is
``{W = sum wq, Xhi = sum wq * (qx >> h), Xlo = sum wq * (qx & (2**h - 1)), Yhi, Ylo, count, 0, 0}``,
held here as Python integers (object arrays) next to the exact, unsplit ``sum wq * qx``;
``X = ldexp(float(Xhi), h) + float(Xlo)``, ``cx = x0 + (X / float(W)) / qsx``, ``dx = x - cx``, the
terms ``wr * (dx * dx)`` and ``wr * (dy * dy)``, the gradient ``(2 * dx) * wr``; an outside ray's
penalty and gradient are multiplied by ``wr`` last.

The bounds are those of the unweighted references (``error_bound`` of each, derived there: the
weights are at most 1, so every term they bound only shrinks)."""
import numpy as np

import density_error_reference as dr
import spot_error_reference as sr

TWO32 = dr.TWO32


def wbits_of(n_source):
    qbits = sr.qbits_of(n_source)
    return min(20, 62 - int(n_source).bit_length() - (qbits + 1) // 2)


def _column_weights(weight, perm, n):
    """(w, ok) per column: the weight of the column's source ray and whether it counts."""
    weight = np.asarray(weight, dtype=np.float64)
    s = np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm)[:n].astype(np.int64)
    s_ok = (s >= 0) & (s < weight.shape[0])
    w = np.zeros(n, dtype=np.float64)
    w[s_ok] = weight[s[s_ok]]
    with np.errstate(invalid="ignore"):
        ok = s_ok & np.isfinite(w) & (w >= 0.0) & (w <= 1.0)
    return w, ok


# ------------------------------------------------------------------------------ DensityError
def density_error(x, y, goal, domain, weight, oob_weight=0.0, mask=None, perm=None, quantise=True,
                  pairwise=True, pulls=None):
    """``y`` None: one field.  ``pulls``: take D from the caller (the implementation's own, to
    compare what a ray makes of them bit for bit) instead of computing it.  Returns the dict of
    ``density_error_reference.density_error`` plus ``w`` and ``counts``."""
    g = dr.normalise(goal)
    two = y is not None
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
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
        counts &= np.asarray(mask)[:n] >= 0
    w, w_ok = _column_weights(weight, perm, n)
    counts &= w_ok
    with np.errstate(invalid="ignore"):
        out = (x < x0) | (x > x1)
        if two:
            out |= (y < y0) | (y > y1)
    inside, outside = counts & ~out, counts & out

    gx, gy = np.zeros_like(x), np.zeros_like(x)
    xo, yo, wo = x[outside], y[outside], w[outside]
    ex = np.maximum(x0 - xo, 0.0) + np.maximum(xo - x1, 0.0)
    ey = (np.maximum(y0 - yo, 0.0) + np.maximum(yo - y1, 0.0)) if two else np.zeros_like(xo)
    penalty = dr._sum((oob_weight * (ex * ex + ey * ey)) * wo, pairwise)
    gx[outside] = (oob_weight * (2.0 * ex) * ((xo > x1).astype(np.float64) - (xo < x0))) * wo
    if two:
        gy[outside] = (oob_weight * (2.0 * ey) * ((yo > y1).astype(np.float64) - (yo < y0))) * wo

    xi, yi, wi = x[inside], y[inside], w[inside]
    ia, ib, tx = dr._axis(xi, x0, sx, nx)
    if two:
        ja, jb, ty = dr._axis(yi, y0, sy, ny)
        index = [ja * nx + ia, ja * nx + ib, jb * nx + ia, jb * nx + ib]
        share = [(1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx]
    else:
        index, share = [ia, ib], [1.0 - tx, tx]
    bins = nx * ny
    if quantise:
        Hq = np.zeros(bins, dtype=np.int64)
        for k, b in zip(index, share):
            np.add.at(Hq, k, np.rint((b * wi) * TWO32).astype(np.int64))
        H = Hq.astype(np.float64) / TWO32
    else:
        Hq = None
        H = np.zeros(bins, dtype=np.float64)
        for k, b in zip(index, share):
            np.add.at(H, k, b * wi)
    gf = g.reshape(-1)
    s = float(np.sqrt(dr._sum(H * H, pairwise)))
    if s == 0.0:
        e_hist, D = dr._sum(gf * gf, pairwise), np.zeros(bins)
    else:
        h = H / s
        r = h - gf
        e_hist = dr._sum(r * r, pairwise)
        D = (2.0 / s) * (r - h * dr._sum(h * r, pairwise))
    if pulls is not None:
        D = np.asarray(pulls, dtype=np.float64).reshape(-1)
    if two:
        d00, d01, d10, d11 = (D[k] for k in index)
        gx[inside] = (sx * ((1.0 - ty) * (d01 - d00) + ty * (d11 - d10))) * wi
        gy[inside] = (sy * ((1.0 - tx) * (d10 - d00) + tx * (d11 - d01))) * wi
    else:
        gx[inside] = (sx * (D[ib] - D[ia])) * wi
    shape = g.shape
    return dict(Hq=None if Hq is None else Hq.reshape(shape), H=H.reshape(shape), s=s,
                error=e_hist + penalty, e_hist=e_hist, penalty=penalty,
                n_penalised=int(outside.sum()), D=D.reshape(shape), grad_x=gx,
                grad_y=gy if two else None, sx=float(sx), sy=float(sy) if two else 0.0, bins=bins,
                w=w, counts=counts, inside=inside, outside=outside)


# ------------------------------------------------------------------------------ SpotError
def _ints(a):
    return [int(v) for v in a]


def spot_error(x, y, group, n_groups, domain, weight, oob_weight=0.0, mask=None, perm=None,
               qbits=None, wbits=None, quantise=True):
    """``y`` None: one field.  ``quantise=False``: the plain form -- positions in float64, the
    quantised weights ``wr``, ``c = sum wr x / sum wr``.  Returns a dict: acc ((G, 8) int64 from
    the Python integers; None unquantised), exact ((G, 2) object array of the unsplit
    ``sum wq * qx`` and ``sum wq * qy``), limbs ((G, 8) object array), h, centroids, error, terms,
    mean, grad_x, grad_y, abs_sum, n, inside, outside, wq, wr."""
    two = y is not None
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    y = np.asarray(y, dtype=np.float64) if two else np.zeros_like(x)
    group = np.asarray(group)
    G = int(n_groups)
    if qbits is None:
        qbits = sr.qbits_of(group.shape[0])
    if wbits is None:
        wbits = wbits_of(group.shape[0])
    h = qbits // 2
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
    w, w_ok = _column_weights(np.asarray(weight, dtype=np.float64)[:group.shape[0]], perm, n)
    wq = np.where(w_ok, np.rint(w * np.ldexp(np.float64(1.0), wbits)), 0.0)
    wr = wq * np.ldexp(np.float64(1.0), -wbits)
    spot = counting & finite & s_ok & (label >= 0) & (label < G) & (wq > 0)
    with np.errstate(invalid="ignore"):
        out = (x < x0) | (x > x1)
        if two:
            out |= (y < y0) | (y > y1)
    inside, outside = spot & ~out, spot & out

    gx, gy = np.zeros(n), np.zeros(n)
    xo, yo, wo = x[outside], y[outside], wr[outside]
    ex = np.maximum(x0 - xo, 0.0) + np.maximum(xo - x1, 0.0)
    ey = (np.maximum(y0 - yo, 0.0) + np.maximum(yo - y1, 0.0)) if two else np.zeros_like(xo)
    penalties = (oob_weight * (ex * ex + ey * ey)) * wo
    gx[outside] = (oob_weight * (2.0 * ex) * ((xo > x1).astype(np.float64) - (xo < x0))) * wo
    if two:
        gy[outside] = (oob_weight * (2.0 * ey) * ((yo > y1).astype(np.float64) - (yo < y0))) * wo

    xi, yi, li, wri = x[inside], y[inside], label[inside], wr[inside]
    limbs = exact = acc = None
    if quantise:
        limbs = np.zeros((G, 8), dtype=object)
        exact = np.zeros((G, 2), dtype=object)
        low = (1 << h) - 1
        qx = _ints(np.clip(np.rint((xi - x0) * qsx), 0.0, one))
        qy = _ints(np.clip(np.rint((yi - y0) * qsy), 0.0, one)) if two else [0] * len(qx)
        for g_, q_, a, b in zip(_ints(li), _ints(wq[inside]), qx, qy):
            limbs[g_, 0] += q_
            limbs[g_, 1] += q_ * (a >> h)
            limbs[g_, 2] += q_ * (a & low)
            limbs[g_, 3] += q_ * (b >> h)
            limbs[g_, 4] += q_ * (b & low)
            limbs[g_, 5] += 1
            exact[g_, 0] += q_ * a
            exact[g_, 1] += q_ * b
        assert all(int(v) < 2 ** 62 for v in limbs.reshape(-1))
        acc = limbs.astype(np.int64)
        cx, cy = np.full(G, np.nan), np.full(G, np.nan)
        for g_ in range(G):
            if limbs[g_, 0] > 0:
                W = np.float64(float(limbs[g_, 0]))
                X = np.ldexp(np.float64(float(limbs[g_, 1])), h) + np.float64(float(limbs[g_, 2]))
                Y = np.ldexp(np.float64(float(limbs[g_, 3])), h) + np.float64(float(limbs[g_, 4]))
                cx[g_] = x0 + (X / W) / qsx
                if two:
                    cy[g_] = y0 + (Y / W) / qsy
    else:
        W, sx_, sy_ = np.zeros(G), np.zeros(G), np.zeros(G)
        np.add.at(W, li, wri)
        np.add.at(sx_, li, wri * xi)
        np.add.at(sy_, li, wri * yi)
        with np.errstate(invalid="ignore", divide="ignore"):
            W = np.where(W > 0, W, np.nan)
            cx, cy = sx_ / W, sy_ / W
    dx = xi - cx[li]
    gx[inside] = (2.0 * dx) * wri
    terms = wri * (dx * dx)
    if two:
        dy = yi - cy[li]
        gy[inside] = (2.0 * dy) * wri
        terms = terms + wri * (dy * dy)
    error = float(np.sum(terms)) + float(np.sum(penalties))
    n_terms = float(int(counting.sum()) * (2 if two else 1))
    return dict(acc=acc, limbs=limbs, exact=exact, h=h, qbits=qbits, wbits=wbits,
                centroids=np.stack([cx, cy], axis=1) if two else cx[:, None],
                error=error, terms=n_terms, mean=error / n_terms if n_terms > 0 else float("nan"),
                grad_x=gx, grad_y=gy if two else None,
                abs_sum=float(np.sum(np.abs(terms)) + np.sum(np.abs(penalties))),
                n_inside=int(inside.sum()), n_penalised=int(outside.sum()), n=n,
                qsx=float(qsx), qsy=float(qsy), inside=inside, outside=outside, wq=wq, wr=wr)


# ------------------------------------------------------------------------------ the inputs
#: source rays that carry the special weights, and the columns that are made their own source
#: rays (with and without perm), inside the domain and not masked off
SPECIAL_AT = (30, 31, 32, 33, 35, 36, 37, 38, 40)


def special_weights(wbits):
    q = np.ldexp(1.0, -wbits)
    return (0.0, 1.0, 0.5 * q,      # half a quantum: a tie, rounds to even -- to 0
            1.5 * q,                # one and a half quanta: a tie, rounds to even -- to 2
            0.25 * q,               # below half a quantum: 0
            np.nan, np.inf, -0.25, 1.5)


def weights(n_source, wbits, seed=5):
    """One weight per source ray: uniform in (0, 1], the ``special_weights`` at ``SPECIAL_AT`` as
    far as the source is long enough."""
    rng = np.random.default_rng(seed + n_source)
    w = 1.0 - rng.random(n_source)
    for at, v in zip(SPECIAL_AT, special_weights(wbits)):
        if at < n_source:
            w[at] = v
    return w


def spot_inputs(n, dtype=np.float64, n_groups=3, domain=sr.DOMAIN):
    """``spot_error_reference.points`` with weights: (x, y, mask, group, perm, weight, wbits).  The
    columns ``SPECIAL_AT`` are their own source rays (perm[c] = c), inside the domain, counting
    and in group 0, so every special weight meets a ray that would otherwise be in a spot."""
    x, y, mask, group, perm = sr.points(n, dtype, n_groups=n_groups, domain=domain)
    n_source = group.shape[0]
    wbits = wbits_of(n_source)
    (x0, x1), (y0, y1) = domain
    for k, c in enumerate(SPECIAL_AT):
        if c < n:
            at = int(np.nonzero(perm == c)[0][0]) if (perm == c).any() else c
            perm[at], perm[c] = perm[c], c
            x[c] = x0 + (0.2 + 0.05 * k) * (x1 - x0)
            y[c] = y0 + (0.7 - 0.05 * k) * (y1 - y0)
            mask[c] = 0
            group[c] = 0
    return x, y, mask, group, perm, weights(n_source, wbits), wbits


def density_inputs(n, dtype=np.float64, domain=dr.DOMAIN):
    """``density_error_reference.points`` with weights: (x, y, mask, perm, weight).  ``perm`` is
    a permutation of the first n of the n + 3 source rays with -- as far as n allows -- one entry
    below 0 and one past the source; the columns ``SPECIAL_AT`` are their own source rays, inside
    the domain and counting."""
    x, y, mask = dr.points(n, dtype, domain=domain)
    n_source = n + 3
    rng = np.random.default_rng(3 + n)
    perm = rng.permutation(n).astype(np.int32)
    (x0, x1), (y0, y1) = domain
    for k, c in enumerate(SPECIAL_AT):
        if c < n:
            at = int(np.nonzero(perm == c)[0][0])
            perm[at], perm[c] = perm[c], c
            x[c] = x0 + (0.2 + 0.05 * k) * (x1 - x0)
            y[c] = y0 + (0.7 - 0.05 * k) * (y1 - y0)
            mask[c] = 0
    if n > 22:
        perm[20], perm[22] = -1, n_source
    return x, y, mask, perm, weights(n_source, 20)


def guard(n, inside_weighted, weight, perm, special):
    """What the inputs promise (checked on the CPU): at least half of the columns are inside with
    a weight that counts (from 63 columns on: the few points of a shorter set fall where the
    unweighted generators put them), and -- from 64 columns on -- every special weight is the weight of some
    column's source ray, and (with a perm) one ``perm`` entry lies below 0 and one past the
    source."""
    assert n < 63 or 2 * int(inside_weighted.sum()) >= n, (n, int(inside_weighted.sum()))
    if n < 64:
        return
    if perm is None:
        s = np.arange(n, dtype=np.int64)
    else:
        s = np.asarray(perm)[:n].astype(np.int64)
        assert (s < 0).any() and (s >= weight.shape[0]).any()
    seen = weight[s[(s >= 0) & (s < weight.shape[0])]]
    for v in special:
        assert (np.isnan(seen).any() if np.isnan(v) else (seen == v).any()), v
