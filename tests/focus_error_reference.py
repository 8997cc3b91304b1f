"""Plain numpy restatement of ``FocusError`` (TEST INFRASTRUCTURE): float64 and int64, no torch,
written from the definition in include/tfrt_hip.h at tfrt_focus_error, not from the kernels.  The
line of a column is ``direction_fields_reference.directions`` (imported, not edited).

For a column of a d-D geometry block (rows 0..d-1 the start s, d..2d-1 the end e), every operation
rounded on its own, sums of products left to right::

    v = e - s,  L = sqrt(v.v),  u = v / L                 ok: all finite, L finite and > 0

A column counts if ``mask`` is None or ``mask[i] >= 0``, the link is ok, ``src = perm[i]`` (``i``
without perm) lies in ``[0, n_source)``, ``label = group[src]`` lies in ``[0, G)`` and
``lo_a <= e_a <= hi_a`` on every axis.  With ``c = 0.5 * (lo + hi)``, ``R = max 0.5 * (hi - lo)``,
``iR = 1 / R``::

    m_a = (e_a - c_a) * iR
    P_aa = 1 - u_a * u_a,  P_ab = -(u_a * u_b),  w = u.m,  t_a = m_a - w * u_a
    record {count, Pxx, Pxy, Pxz, Pyy, Pyz, Pzz, tx, ty, tz} += {1, rint(P * 2**pbits),
                                                                 rint(t * 2**pbits)}

``pbits = min(40, 60 - bit_length(n_source))``.  Per group ``n = count``,
``a = (Aq * 2**-pbits) / n``, ``b = (bq * 2**-pbits) / n``, the cofactor solve of the header; a
focus if ``count >= 2`` and ``det >= min_det``.  A counting ray of a group with a focus::

    q = m - x,  a = u.q,  rho = R * (q - a * u),  lever = (R * a) / L,  term = rho.rho
    grad[end] = (2 * rho) * (1 - lever),  grad[start] = (2 * rho) * lever

``quantise=False`` keeps the records in float64 (the plain form, for the size of the quantisation).

Also the bounds the tests share, with their derivations (``error_bound``, ``SOLVE_BACKWARD_EPS``),
and the inputs (``rays``) with their guard (``assert_generator``).
"""
import numpy as np

import direction_fields_reference as dfr

EPS = float(np.finfo(np.float64).eps)
SLOTS = 10
Z_SLOTS = (3, 5, 6, 9)
MIN_DET = 1e-6      # the tests' min_det: far above a collimated group's 2**-pbits, far below 1e-3

# The componentwise backward error max |A x - b| / (|A| |x| + |b|) of the cofactor solve over the
# groups with a focus of ``rays(n, 7)``, n in (64, 65, 1000, 20000), both dimensions, float32 and
# float64 rows, residuals in exact rational arithmetic, measured on the CPU
# (tests/test_focus_error_host.py prints every figure): between 0.30 and 0.64 eps, the largest at
# n = 65, 3-D, float32 rows.  The test asserts 4 x that.
SOLVE_BACKWARD_EPS = 0.64


def pbits_of(n_source):
    return min(40, 60 - int(n_source).bit_length())


def box_of(domain):
    """(lo, hi, c, R, iR) of a d-axis domain."""
    lo = np.array([d[0] for d in domain], dtype=np.float64)
    hi = np.array([d[1] for d in domain], dtype=np.float64)
    c = 0.5 * (lo + hi)
    R = np.float64(np.max(0.5 * (hi - lo)))
    return lo, hi, c, R, np.float64(1.0) / R


def _dot(v, w):
    s = v[0] * w[0] + v[1] * w[1]
    return s + v[2] * w[2] if v.shape[0] == 3 else s


def solve(acc, pbits, min_det, dim):
    """(x (G, 3), has (G,), det (G,)) of a (G, 10) record table; x is NaN without a focus (2-D:
    x[:, 2] = 0 with one)."""
    inv = np.ldexp(np.float64(1.0), -pbits)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = acc[:, 0].astype(np.float64)
        a00, a01, a02, a11, a12, a22, b0, b1, b2 = (
            (acc[:, p].astype(np.float64) * inv) / n for p in range(1, 10))
        if dim == 2:
            det = a00 * a11 - a01 * a01
            xs = [(a11 * b0 - a01 * b1) / det, (a00 * b1 - a01 * b0) / det, np.zeros_like(det)]
        else:
            c00 = a11 * a22 - a12 * a12
            c01 = a02 * a12 - a01 * a22
            c02 = a01 * a12 - a02 * a11
            c11 = a00 * a22 - a02 * a02
            c12 = a01 * a02 - a00 * a12
            c22 = a00 * a11 - a01 * a01
            det = a00 * c00 + a01 * c01 + a02 * c02
            xs = [(c00 * b0 + c01 * b1 + c02 * b2) / det, (c01 * b0 + c11 * b1 + c12 * b2) / det,
                  (c02 * b0 + c12 * b1 + c22 * b2) / det]
        has = (acc[:, 0] >= 2) & (det >= min_det)
    x = np.stack([np.where(has, v, np.nan) for v in xs], axis=1)
    return x, has, det


def focus_error(block, group, n_groups, domain, min_det=MIN_DET, mask=None, perm=None,
                quantise=True):
    """Returns a dict: acc ((G, 10) int64; float64 unquantised), table ((G, 4) {x, y, z,
    has_focus} normalised), foci ((G, d) scene coordinates), det, error, terms, mean, grad
    ((2d, n)), term ((n,), 0 without one), counts, has (the columns with a term), abs_sum, n,
    pbits, u, m, L."""
    block = np.asarray(block)
    dim = block.shape[0] // 2
    n = block.shape[1]
    group = np.asarray(group)
    G = int(n_groups)
    pbits = pbits_of(group.shape[0])
    one = np.ldexp(np.float64(1.0), pbits)
    lo, hi, c, R, iR = box_of(domain[:dim])
    u, L, ok = dfr.directions(block)
    e = block[dim:].astype(np.float64)

    counts = ok.copy() if mask is None else ok & (np.asarray(mask)[:n] >= 0)
    s = np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm)[:n].astype(np.int64)
    s_ok = (s >= 0) & (s < group.shape[0])
    label = np.full(n, -1, dtype=np.int64)
    label[s_ok] = group[s[s_ok]]
    counts &= s_ok & (label >= 0) & (label < G)
    with np.errstate(invalid="ignore"):
        for a in range(dim):
            counts &= (e[a] >= lo[a]) & (e[a] <= hi[a])
        m = (e - c[:, None]) * iR
        w = _dot(u, m)
        slots = {1: 1.0 - u[0] * u[0], 2: -(u[0] * u[1]), 4: 1.0 - u[1] * u[1],
                 7: m[0] - w * u[0], 8: m[1] - w * u[1]}
        if dim == 3:
            slots.update({3: -(u[0] * u[2]), 5: -(u[1] * u[2]), 6: 1.0 - u[2] * u[2],
                          9: m[2] - w * u[2]})
    li = label[counts]
    if quantise:
        acc = np.zeros((G, SLOTS), dtype=np.int64)
        np.add.at(acc[:, 0], li, 1)
        for p, v in slots.items():
            np.add.at(acc[:, p], li, np.rint(v[counts] * one).astype(np.int64))
        x, has_focus, det = solve(acc, pbits, min_det, dim)
    else:
        acc = np.zeros((G, SLOTS))
        np.add.at(acc[:, 0], li, 1.0)
        for p, v in slots.items():
            np.add.at(acc[:, p], li, v[counts])
        A = np.zeros((G, 3, 3))
        for p, (a, b) in {1: (0, 0), 2: (0, 1), 3: (0, 2), 4: (1, 1), 5: (1, 2), 6: (2, 2)}.items():
            A[:, a, b] = A[:, b, a] = acc[:, p]
        if dim == 2:
            A[:, 2, 2] = 1.0
        cnt = np.maximum(acc[:, 0], 1.0)
        det = np.linalg.det(A / cnt[:, None, None])
        has_focus = (acc[:, 0] >= 2) & (det >= min_det)
        x = np.full((G, 3), np.nan)
        for k in np.nonzero(has_focus)[0]:
            x[k] = np.linalg.solve(A[k], acc[k, 7:])

    lab = np.clip(label, 0, G - 1)
    has = counts & has_focus[lab]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = m - x[lab, :dim].T
        a = _dot(u, q)
        rho = R * (q - a * u)
        lever = (R * a) / L
        term = _dot(rho, rho)
        two = 2.0 * rho
        g_end, g_start = two * (1.0 - lever), two * lever
    grad = np.zeros((2 * dim, n))
    grad[:dim] = np.where(has[None, :], g_start, 0.0)
    grad[dim:] = np.where(has[None, :], g_end, 0.0)
    term = np.where(has, term, 0.0)
    n_terms = float(int(has.sum()))
    error = float(np.sum(term[has]))
    table = np.concatenate([x, has_focus[:, None].astype(np.float64)], axis=1)
    return dict(acc=acc, table=table, foci=c[None, :] + R * x[:, :dim], det=det, error=error,
                terms=n_terms, mean=error / n_terms if n_terms > 0 else float("nan"), grad=grad,
                term=term, counts=counts, has=has, abs_sum=float(np.sum(np.abs(term))), n=n,
                pbits=pbits, u=u, m=m, L=L, label=label, has_focus=has_focus)


def error_bound(ref):
    """|error - reference error| between two evaluations that agree on every term and differ in
    the order of their float sums: a sum of n numbers in ANY order is within (n - 1) eps sum|a_i|
    of the exact sum to first order (Higham, Accuracy and Stability, eq. 4.4); ``n eps sum|terms|``
    is the worst case of any summation order.  Derived, not measured."""
    return ref["n"] * EPS * ref["abs_sum"]


# ------------------------------------------------------------------------------ the inputs
DOMAIN = ((4.0, 7.5), (-1.2, 1.3), (-1.0, 1.5))


def specials(G):
    """The labels of the special groups among G: (parallel, single, empty); the empty one needs a
    fourth group (G = 3: converging, parallel, single)."""
    if G >= 4:
        return G - 3, G - 2, G - 1
    return G - 2, G - 1, None


def rays(n, G, dtype=np.float64, dimension=3, permuted=False, seed=41):
    """(block, mask, group, perm): a (2 * dimension, n) geometry block in ``dtype`` whose columns
    are lines that converge, per group, to a point of the box ``DOMAIN`` with noise of 0.01.

    ``group`` holds one label per SOURCE ray (n + 3 of them); a source ray's line is made for ITS
    label, and column i shows source ray ``perm[i]`` with ``permuted`` (``perm``: a random
    permutation of the first n source rays with, as far as n allows, one entry below 0 and one past
    the source), source ray i without.  The converging groups 0 .. share the source rays evenly;
    group ``specials(G)[0]`` holds rays that are all PARALLEL (no focus), ``[1]`` a single ray
    (source ray 26), ``[2]`` none (G >= 4); the labels -1 and G occur at source rays 12 and 14.
    By column: 16::17 are degenerate (end = start), 22::23 carry a NaN in x_end, 29::31 have
    their end outside the
    box (pushed 10 along the line).  The mask switches every fifth column off.  The 2-D block is
    made the same way in the plane."""
    assert G >= 3
    rng = np.random.default_rng(seed + 7 * n + G + 1000 * dimension + int(permuted))
    d = dimension
    ns = n + 3
    par, single, empty = specials(G)
    n_conv = par
    # (even shares at random places: a label of period n_conv would meet the columns' periods)
    group = rng.permutation(np.arange(ns) % n_conv).astype(np.int32)
    group[5::9] = par                                   # one source ray in nine
    if ns > 26:
        group[26] = single
    if ns > 14:
        group[12], group[14] = -1, G
    centre = np.array([(a + b) / 2 for a, b in DOMAIN])
    focus = centre[:, None] + rng.uniform(-0.5, 0.5, (3, G)) * np.array([1.5, 1.0, 1.0])[:, None]
    u = np.stack([np.ones(ns), rng.normal(0, .3, ns), rng.normal(0, .3, ns)])
    lab = np.clip(group, 0, G - 1)
    u[:, lab == par] = np.array([1.0, 0.2, -0.1])[:, None]
    u = u[:d] / np.sqrt((u[:d] * u[:d]).sum(axis=0))
    tau = rng.uniform(-0.8, 0.8, ns)
    end = focus[:d, lab] + tau * u + rng.normal(0, 0.01, (d, ns))
    spread = rng.uniform(-0.6, 0.6, (d, ns))
    end[:, lab == par] = (centre[:d, None] + spread)[:, lab == par]
    start = end - u * rng.uniform(.5, 3, ns)
    perm = rng.permutation(n).astype(np.int32)
    # columns 12, 14 and 26 are their own source rays, with and without perm
    for c in (12, 14, 26):
        if c < n:
            at = int(np.nonzero(perm == c)[0][0])
            perm[at], perm[c] = perm[c], c
    if n > 22:
        perm[20], perm[21] = -1, ns
    col = np.clip(perm, 0, ns - 1) if permuted else np.arange(n)
    s, e = start[:, col].copy(), end[:, col].copy()
    uc = u[:, col]
    e[:, 29::31] += 10.0 * uc[:, 29::31]
    s[:, 29::31] += 10.0 * uc[:, 29::31]
    e[:, 16::17] = s[:, 16::17]
    e[0, 22::23] = np.nan
    mask = np.where(np.arange(n) % 5 == 4, -1, np.arange(n) % 7).astype(np.int32)
    block = np.ascontiguousarray(np.concatenate([s, e]).astype(dtype))
    return block, mask, group, perm


def census(n, G, dtype=np.float64, dimension=3, permuted=False, masked=False):
    """What the generator's columns are: counting, with_term, degenerate, non_finite, outside,
    excluded labels (-1 and G) among the columns' source rays, the count of the parallel, the
    single and the empty group, the groups with a focus and the least det(A / count) among the
    converging groups."""
    block, mask, group, perm = rays(n, G, dtype, dimension, permuted)
    ref = focus_error(block, group, G, DOMAIN, mask=mask if masked else None,
                      perm=perm if permuted else None)
    dim = dimension
    b = block.astype(np.float64)
    finite = np.isfinite(b).all(axis=0)
    _, _, ok = dfr.directions(block)
    lo, hi, *_ = box_of(DOMAIN[:dim])
    with np.errstate(invalid="ignore"):
        outside = ok & ~((b[dim:] >= lo[:, None]) & (b[dim:] <= hi[:, None])).all(axis=0)
    par, single, empty = specials(G)
    cnt = ref["acc"][:, 0]
    conv = ref["det"][:par]
    return dict(counting=int(ref["counts"].sum()), with_term=int(ref["has"].sum()),
                degenerate=int((finite & ~ok).sum()), non_finite=int((~finite).sum()),
                outside=int(outside.sum()),
                excluded=int(((ref["label"] < 0) | (ref["label"] >= G)).sum()),
                parallel=int(cnt[par]), parallel_has_focus=bool(ref["has_focus"][par]),
                single=int(cnt[single]), empty=None if empty is None else int(cnt[empty]),
                foci=int(ref["has_focus"].sum()),
                min_count=int(cnt[:par].min()), min_det=float(np.nanmin(conv)))


def assert_generator(n, G, c):
    """The generator's guard -- a condition, not a measurement -- on a ``census``: at least half
    of the columns count; from 64 columns on every special case occurs; and where the source has
    at least 8 rays per group (n >= 8 * G) every converging group holds at least 4 counting rays
    and has det(A / count) > 1e-3.  (With fewer rays per group a converging group may hold one
    ray, or two nearly parallel ones: the kernels' own cases, but no ground for a bound on the
    determinant.)"""
    assert c["counting"] >= n / 2, c
    if n >= 64:
        assert c["degenerate"] >= 1 and c["non_finite"] >= 1 and c["outside"] >= 1, c
        assert c["excluded"] >= 2 and c["parallel"] >= 2 and not c["parallel_has_focus"], c
        assert c["single"] == 1 and c["empty"] in (None, 0), c
    if n >= 64 and n >= 8 * G:
        assert c["min_count"] >= 4 and c["min_det"] > 1e-3, c
    return c
