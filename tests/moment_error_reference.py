"""Plain numpy restatement of ``MomentError`` (TEST INFRASTRUCTURE): Python integers for the
records, float64 in the stated order for everything else, no torch; written from the definition in
include/tfrt_hip.h at tfrt_moment_error, not from the kernels -- the order of every sum over the
groups and over the penalties included.

The columns, the four cases of a counting column, the penalties and their gradient are
``SpotError``'s, taken from tests/spot_error_reference.py on the grid of ``mbits`` bits (imported,
not edited); ``fixed_sum`` and ``penalty_sum`` are tests/centroid_error_reference.py's; fields and
the chain rule of a direction field come from tests/direction_fields_reference.py.

* grid: ``mbits = min(40, 2 * ((61 - bit_length(N)) // 2))``, ``h = mbits // 2``,
  ``ms = 2**mbits / (x1 - x0)``, ``m = min(max(rint((x - x0) * ms), 0), 2**mbits)``;
* pass 1: ``{n, Sx, Sy}`` per group; a group with ``n >= 2`` is USED,
  ``kx = (2 * Sx + n) // (2 * n)``, ``cx = x0 + kx / ms``;
* pass 2: ``dx = mx - kx``, ``dxl = dx & (2**h - 1)``, ``dxh = dx >> h``; per pair (a, b) in
  xx, xy, yy: ``HH += ah * bh``, ``HL += ah * bl + al * bh``, ``LL += al * bl``;
* ``Mf = (ldexp(HH, mbits) + ldexp(HL, h)) + LL``, ``C = (Mf / n) / (ms_a * ms_b)``;
* ``D = C - t`` (0 where t is NaN), or round: ``s = (Cxx + Cyy) / 2``, ``Dxx = Cxx - s``,
  ``Dxy = Cxy``, ``Dyy = Cyy - s``;
* ``e_g = n * ((Dxx * Dxx + 2 * (Dxy * Dxy)) + Dyy * Dyy)``,
  ``error = fixed_sum(e_g over used groups) + penalty_sum(penalties)``;
* ``F = 4 * D``; a ray inside a used group: ``gx = Fxx * (x - cx) + Fxy * (y - cy)``,
  ``gy = Fxy * (x - cx) + Fyy * (y - cy)``.

Also the plain definition the gradient is checked against (``plain_covariance_error``, torch
autograd, the centroid as the mean, no grid) and the inputs (``rays``, ``targets_for``,
``clouds``).
"""
import numpy as np

import centroid_error_reference as cr
import direction_fields_reference as dfr
import spot_error_reference as sr

EPS = float(np.finfo(np.float64).eps)
DOMAIN = sr.DOMAIN
OOB = 0.3
LDS_GROUPS = 256        # the largest group count whose tables the kernels keep in LDS
ACC_CAPACITY = cr.ACC_MAX_GRID * cr.ACC_BLOCK       # columns of one trip of the accumulate loops
SEED_CAPACITY = 2048 * 256                          # ... of the seed loop


def mbits_of(n_source):
    return min(40, 2 * ((61 - int(n_source).bit_length()) // 2))


def limb_sums(dx, dy, h):
    """The nine Python-integer sums {xx, xy, yy} x {HH, HL, LL} of the integer offsets ``dx``,
    ``dy`` (lists of Python ints)."""
    low = (1 << h) - 1
    out = [0] * 9
    for a, b in zip(dx, dy):
        al, ah, bl, bh = a & low, a >> h, b & low, b >> h
        for first, (pl, ph, ql, qh) in ((0, (al, ah, al, ah)), (3, (al, ah, bl, bh)),
                                        (6, (bl, bh, bl, bh))):
            out[first] += ph * qh
            out[first + 1] += ph * ql + pl * qh
            out[first + 2] += pl * ql
    return out


def moment_error(x, y, group, n_groups, domain, covariance=None, shape=None, oob_weight=0.0,
                 mask=None, perm=None, mbits=None):
    """``y`` None: one field (``covariance`` is then (G, 1)).  Exactly one of ``covariance``
    ((G, 3) or (G, 1), NaN: free) and ``shape`` ("round").  Returns a dict: acc ((G, 4) int64), mom
    ((G, 9) int64), mom_exact (per group the Python integers [Mxx, Mxy, Myy]), centres ((G, 2)
    Python ints, -1 where not used), centroids ((G, k), NaN without rays), cov ((G, 6) {C, D}, NaN
    where not used), group_rows ((G, 8)), used, rays, groups_used, error, terms, mean, grad_x,
    grad_y (None without y), abs_sum, n, n_groups, inside, outside, label, limb_max."""
    assert (covariance is None) != (shape is None)
    two = y is not None
    G = int(n_groups)
    if mbits is None:
        mbits = mbits_of(np.asarray(group).shape[0])
    h = mbits // 2
    spot = sr.spot_error(x, y, group, G, domain, oob_weight, mask=mask, perm=perm, qbits=mbits)
    acc = spot["acc"]
    n = spot["n"]
    one = np.ldexp(np.float64(1.0), mbits)
    (x0, x1) = (np.float64(v) for v in domain[0])
    msx = one / (x1 - x0)
    (y0, y1) = (np.float64(v) for v in domain[1]) if two else (np.float64(0), np.float64(0))
    msy = one / (y1 - y0) if two else np.float64(0)

    inside, outside = spot["inside"], spot["outside"]
    group = np.asarray(group)
    s = np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm)[:n].astype(np.int64)
    label = np.full(n, -1, dtype=np.int64)
    s_ok = (s >= 0) & (s < group.shape[0])
    label[s_ok] = group[s[s_ok]]
    xv = np.asarray(x, dtype=np.float64)
    yv = np.asarray(y, dtype=np.float64) if two else np.zeros(n)
    with np.errstate(invalid="ignore"):
        mx = np.clip(np.rint((xv - x0) * msx), 0.0, one)
        my = np.clip(np.rint((yv - y0) * msy), 0.0, one) if two else np.zeros(n)

    if covariance is not None:
        covariance = np.asarray(covariance, dtype=np.float64)
        assert covariance.shape == (G, 3 if two else 1)
    members = [[] for _ in range(G)]
    for i in np.nonzero(inside)[0]:
        members[label[i]].append(int(i))
    mom = np.zeros((G, 9), dtype=np.int64)
    mom_exact, centres = [], []
    group_rows = np.zeros((G, 8))
    cov = np.full((G, 6), np.nan)
    used = np.zeros(G, dtype=bool)
    rays = np.zeros(G, dtype=bool)
    e_g = np.zeros(G)
    limb_max = 0
    for g in range(G):
        cnt, Sx, Sy = (int(v) for v in acc[g, :3])
        assert cnt == len(members[g])
        rays[g], used[g] = cnt > 0, cnt >= 2
        if not rays[g]:
            group_rows[g, :2] = np.nan
            centres.append((-1, -1))
            mom_exact.append([0, 0, 0])
            continue
        kx = (2 * Sx + cnt) // (2 * cnt)
        ky = (2 * Sy + cnt) // (2 * cnt) if two else 0
        group_rows[g, 0] = x0 + np.float64(kx) / msx
        group_rows[g, 1] = y0 + np.float64(ky) / msy if two else 0.0
        if not used[g]:
            centres.append((-1, -1))
            mom_exact.append([0, 0, 0])
            continue
        centres.append((kx, ky))
        dx = [int(mx[i]) - kx for i in members[g]]
        dy = [int(my[i]) - ky for i in members[g]] if two else [0] * cnt
        assert all(abs(d) <= 1 << mbits for d in dx + dy)
        sums = limb_sums(dx, dy, h)
        if not two:
            sums[3:] = [0] * 6
        limb_max = max(limb_max, max(abs(v) for v in sums))
        mom[g] = sums
        exact = [sums[c] * (1 << mbits) + sums[c + 1] * (1 << h) + sums[c + 2] for c in (0, 3, 6)]
        mom_exact.append(exact)
        nf = np.float64(cnt)
        Mf = [(np.ldexp(np.float64(sums[c]), mbits) + np.ldexp(np.float64(sums[c + 1]), h))
              + np.float64(sums[c + 2]) for c in (0, 3, 6)]
        C = [(Mf[0] / nf) / (msx * msx),
             (Mf[1] / nf) / (msx * msy) if two else np.float64(0.0),
             (Mf[2] / nf) / (msy * msy) if two else np.float64(0.0)]
        if shape is not None:
            assert shape == "round" and two
            size = (C[0] + C[2]) / 2.0
            D = [C[0] - size, C[1], C[2] - size]
        else:
            t = [covariance[g, 0], covariance[g, 1] if two else np.nan,
                 covariance[g, 2] if two else np.nan]
            D = [np.float64(0.0) if np.isnan(t[c]) else C[c] - t[c] for c in range(3)]
        cov[g, :3], cov[g, 3:] = C, D
        group_rows[g, 2:5] = [4.0 * d for d in D]
        group_rows[g, 5] = 1.0
        e_g[g] = nf * ((D[0] * D[0] + 2.0 * (D[1] * D[1])) + D[2] * D[2])
    e_inside = cr.fixed_sum(e_g, used)

    gx = np.where(outside, spot["grad_x"], 0.0)
    gy = np.where(outside, spot["grad_y"], 0.0) if two else None
    live = inside.copy()
    live[inside] = used[label[inside]]
    row = group_rows[label[live]]
    ux = xv[live] - row[:, 0]
    if two:
        uy = yv[live] - row[:, 1]
        gx[live] = row[:, 2] * ux + row[:, 3] * uy
        gy[live] = row[:, 3] * ux + row[:, 4] * uy
    else:
        gx[live] = row[:, 2] * ux
    xo, yo = xv[outside], yv[outside]
    ex = np.maximum(x0 - xo, 0.0) + np.maximum(xo - x1, 0.0)
    ey = (np.maximum(y0 - yo, 0.0) + np.maximum(yo - y1, 0.0)) if two else np.zeros_like(xo)
    penalties = oob_weight * (ex * ex + ey * ey)
    per_column = np.zeros(n)
    per_column[outside] = penalties
    error = float(e_inside + cr.penalty_sum(per_column, outside))
    n_terms = spot["terms"]
    k = 2 if two else 1
    return dict(acc=acc, mom=mom, mom_exact=mom_exact, centres=centres,
                centroids=group_rows[:, :k].copy(), cov=cov, group_rows=group_rows, used=used,
                rays=rays, groups_used=int(used.sum()), error=error, terms=n_terms,
                mean=error / n_terms if n_terms > 0 else float("nan"), grad_x=gx, grad_y=gy,
                abs_sum=float(np.sum(e_g[used]) + np.sum(penalties)), n=n, n_groups=G,
                inside=inside, outside=outside, label=label, limb_max=limb_max, mbits=mbits,
                msx=float(msx), msy=float(msy), mx=mx, my=my)


def fields(block, codes, group, n_groups, domain, **kw):
    """MomentError of the fields ``codes`` of the (2d, n) geometry block ``block``: the dict of
    ``moment_error`` plus ``grad`` (2d, n) -- through the chain rule with a direction field --
    and ``counts`` (the columns in a group or penalised)."""
    vals, d, L, ok = dfr.field_values(block, codes)
    two = len(codes) == 2
    ref = moment_error(vals[0], vals[1] if two else None, group, n_groups, domain, **kw)
    gv = [ref["grad_x"]] + ([ref["grad_y"]] if two else [])
    return dfr._compose(ref, gv, codes, d, L, ok, ref["inside"] | ref["outside"])


def per_ray_terms(ref, two=True):
    """The (n, k) terms of the generic path: an inside ray of a used group carries
    ``(Dxx**2 + Dxy**2, Dxy**2 + Dyy**2)`` of its group; penalties are the caller's."""
    n = ref["n"]
    out = np.zeros((n, 2 if two else 1))
    for i in np.nonzero(ref["inside"])[0]:
        g = ref["label"][i]
        if ref["used"][g]:
            D = ref["cov"][g, 3:]
            cross = D[1] * D[1]
            out[i, 0] = D[0] * D[0] + cross
            if two:
                out[i, 1] = cross + D[2] * D[2]
    return out


# ------------------------------------------------------------------------------ the inputs
def rays(n, n_groups=3, dtype=np.float64, seed=23):
    """spot_error_reference's ``points``: (x, y, mask, group, perm); the last group is empty when
    G > 1, the one before it has a single ray when G > 2, the labels -1 and G occur, about one
    point in eight is outside."""
    return sr.points(n, dtype, n_groups, seed)


def targets_for(n_groups, two=True, seed=5):
    """(G, 3) positive definite targets of about the size of a uniform cloud in ``DOMAIN``
    ((G, 1) with one field); row 1 (G > 2) has a NaN in its LAST entry, row 2 (G > 4) in its
    first and row 0 (two fields) in ``txy``: free components."""
    rng = np.random.default_rng(seed + n_groups)
    (x0, x1), (y0, y1) = DOMAIN
    sx = rng.uniform(0.1, 0.4, n_groups) * (x1 - x0)
    sy = rng.uniform(0.1, 0.4, n_groups) * (y1 - y0)
    rho = rng.uniform(-0.8, 0.8, n_groups)
    t = np.stack([sx * sx, rho * sx * sy, sy * sy], axis=1)
    t = np.ascontiguousarray(t if two else t[:, :1])
    if n_groups > 2:
        t[1, -1] = np.nan
    if n_groups > 4:
        t[2, 0] = np.nan
    if two:
        t[0, 1] = np.nan
    return t


def clouds(n=4000, n_groups=5, seed=3):
    """(x, y, group, domain, cov): ``n`` points in ``n_groups`` anisotropic, rotated Gaussian
    clouds with separate centres, ``domain`` four times their extent, and each cloud's exact
    sample covariance rows {Cxx, Cxy, Cyy}."""
    rng = np.random.default_rng(seed)
    group = (np.arange(n) % n_groups).astype(np.int32)
    x, y = np.zeros(n), np.zeros(n)
    for g in range(n_groups):
        at = group == g
        m = int(at.sum())
        a, b = rng.uniform(0.05, 0.12), rng.uniform(0.2, 0.4)
        th = rng.uniform(0, np.pi)
        u, v = rng.normal(0, a, m), rng.normal(0, b, m)
        x[at] = 2.0 * g - 4.0 + np.cos(th) * u - np.sin(th) * v
        y[at] = 0.5 * g + np.sin(th) * u + np.cos(th) * v
    ext_x, ext_y = x.max() - x.min(), y.max() - y.min()
    cx, cy = 0.5 * (x.max() + x.min()), 0.5 * (y.max() + y.min())
    domain = ((cx - 2 * ext_x, cx + 2 * ext_x), (cy - 2 * ext_y, cy + 2 * ext_y))
    cov = np.zeros((n_groups, 3))
    for g in range(n_groups):
        at = group == g
        dx, dy = x[at] - x[at].mean(), y[at] - y[at].mean()
        cov[g] = [(dx * dx).mean(), (dx * dy).mean(), (dy * dy).mean()]
    return x, y, group, domain, cov


def plain_covariance_error(x, y, group, n_groups, covariance=None, shape=None):
    """The plain definition under torch autograd (float64): per group of >= 2 points the centroid
    is the mean, ``C`` the mean of the outer products about it, ``D`` as above, and the error
    ``sum n * (Dxx**2 + 2 * Dxy**2 + Dyy**2)``.  No grid.  ``x``, ``y``: torch tensors with
    ``requires_grad``; returns the scalar error."""
    import torch
    total = torch.zeros((), dtype=torch.float64)
    for g in range(n_groups):
        at = torch.as_tensor(np.asarray(group) == g)
        m = int(at.sum())
        if m < 2:
            continue
        dx, dy = x[at] - x[at].mean(), y[at] - y[at].mean()
        C = [(dx * dx).mean(), (dx * dy).mean(), (dy * dy).mean()]
        if shape is not None:
            s = (C[0] + C[2]) / 2.0
            D = [C[0] - s, C[1], C[2] - s]
        else:
            D = [torch.zeros((), dtype=torch.float64) if np.isnan(covariance[g][c])
                 else C[c] - float(covariance[g][c]) for c in range(3)]
        total = total + m * (D[0] * D[0] + 2.0 * (D[1] * D[1]) + D[2] * D[2])
    return total
