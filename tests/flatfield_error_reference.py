"""Plain numpy restatement of ``FlatFieldError`` (TEST INFRASTRUCTURE): float64 and int64, no
torch, written from the definition in include/tfrt_hip.h at tfrt_flatfield_error, not from the
kernels.  The rays, the records and the foci are ``focus_error_reference``'s (imported, not
edited): everything up to a group's focus ``x = A^-1 b`` is FocusError's.

With the unit normal ``a = axis / sqrt(axis . axis)`` (products summed left to right), every
operation rounded on its own, a group with a focus is USED and has::

    n = (double) count,  h = a.x,  y = A^-1 a    (the cofactors of the focus' solve, same order)

Sums over the used groups, in the order of ``group_sum``::

    W = sum n,  S = sum n * h,  hbar = S / W;      the plane is VALID with >= 2 used groups
    r = h - hbar,  s = R * r,  e_g = s * s,  mu = (2 * s) * y          (2-D: mu_2 = 0)
    inside = sum n * e_g;   terms = sum count (an integer);  error = {inside, terms, inside / terms}

Without a valid plane ``e_g = mu = 0`` and ``inside = 0``.  A counting ray of a used group under a
valid plane, against ``x`` and ``mu`` of its group::

    q = m - x,  alpha = u.q,  lever = (R * alpha) / L,  rest = 1 - lever,  beta = mu.u,  k = beta / L
    rho = R * (q - alpha * u),  muP = mu - beta * u,  turn = k * rho
    grad[end] = muP * rest - turn,  grad[start] = muP * lever + turn

Every other column has a zero gradient.

``group_sum`` is the fixed shape and order of every float sum over the groups: thread j of 1,024
takes the groups j, j + 1024, ... ascending from 0.0, unused groups skipped; the 64 lanes of a wave
by ``v += v[lane ^ d]``, d = 32 .. 1; the 16 waves in index order from 0.0.

Also the inputs (``rays``, ``case``) with their guard: every case that is handed out has at least
two used groups, unless it is asked for without a plane.
"""
import numpy as np

import focus_error_reference as fr

EPS = fr.EPS
MIN_DET = fr.MIN_DET
DOMAIN = fr.DOMAIN
BLOCK = 1024
AXIS3 = (0.8, -0.35, 0.5)            # a general direction: no component vanishes
AXIS2 = (0.8, -0.35)


def axis_of(axis, dim):
    """a = axis / sqrt(axis . axis) as three float64 (2-D: the third is 0)."""
    v = [np.float64(c) for c in axis]
    assert len(v) == dim
    s = v[0] * v[0] + v[1] * v[1]
    if dim == 3:
        s = s + v[2] * v[2]
    r = np.sqrt(s)
    return np.array([c / r for c in v] + [0.0] * (3 - dim), dtype=np.float64)


def group_sum(values, used):
    """The sum of ``values[used]`` over the groups in the definition's fixed shape and order."""
    values = np.asarray(values, dtype=np.float64)
    G = values.shape[0]
    trips = max((G + BLOCK - 1) // BLOCK, 1)
    v = np.zeros(trips * BLOCK)
    u = np.zeros(trips * BLOCK, dtype=bool)
    v[:G], u[:G] = values, used
    s = np.zeros(BLOCK)
    with np.errstate(invalid="ignore"):
        for vt, ut in zip(v.reshape(trips, BLOCK), u.reshape(trips, BLOCK)):
            s = np.where(ut, s + vt, s)
    w = s.reshape(BLOCK // 64, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w[:, :d] + w[:, d:2 * d]
    total = np.float64(0.0)
    for wave in w[:, 0]:
        total = total + wave
    return total


def _dot3(a, x, dim):
    s = a[0] * x[0] + a[1] * x[1]
    return s + a[2] * x[2] if dim == 3 else s


def solve_y(acc, pbits, a, dim):
    """y = A^-1 a (G, 3) of a (G, 10) record table by the cofactors of the header (garbage
    without a focus; 2-D: y[:, 2] = 0)."""
    inv = np.ldexp(np.float64(1.0), -pbits)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = acc[:, 0].astype(np.float64)
        a00, a01, a02, a11, a12, a22 = (
            (acc[:, p].astype(np.float64) * inv) / n for p in range(1, 7))
        if dim == 2:
            det = a00 * a11 - a01 * a01
            ys = [(a11 * a[0] - a01 * a[1]) / det, (a00 * a[1] - a01 * a[0]) / det,
                  np.zeros_like(det)]
        else:
            c00 = a11 * a22 - a12 * a12
            c01 = a02 * a12 - a01 * a22
            c02 = a01 * a12 - a02 * a11
            c11 = a00 * a22 - a02 * a02
            c12 = a01 * a02 - a00 * a12
            c22 = a00 * a11 - a01 * a01
            det = a00 * c00 + a01 * c01 + a02 * c02
            ys = [(c00 * a[0] + c01 * a[1] + c02 * a[2]) / det,
                  (c01 * a[0] + c11 * a[1] + c12 * a[2]) / det,
                  (c02 * a[0] + c12 * a[1] + c22 * a[2]) / det]
    return np.stack(ys, axis=1)


def flatfield_error(block, group, n_groups, domain, axis, min_det=MIN_DET, mask=None, perm=None):
    """Returns a dict: acc ((G, 10) int64), table ((G, 8) {x0, x1, x2, used, mu0, mu1, mu2, e_g}),
    fit ((8,) {hbar, a.c + R hbar, W, groups used, valid, 0, 0, 0}), error, terms, mean, grad
    ((2d, n)), term ((n,): e_g of a counting ray's used group, else 0), used ((G,)), heights
    ((G,) a . focus in scene coordinates), residuals ((G,) R r, NaN unused, 0 without a plane),
    foci ((G, d) scene coordinates), has (the columns with a gradient), counts, a, focus (the
    dict of ``focus_error_reference.focus_error``)."""
    block = np.asarray(block)
    dim = block.shape[0] // 2
    G = int(n_groups)
    f = fr.focus_error(block, group, G, domain, min_det=min_det, mask=mask, perm=perm)
    a = axis_of(axis, dim)
    _, _, c, R, _ = fr.box_of(domain[:dim])
    acc, used = f["acc"], f["has_focus"]
    x = f["table"][:, :3]
    y = solve_y(acc, f["pbits"], a, dim)
    n = acc[:, 0].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = _dot3(a, x.T, dim)
        W, S = group_sum(n, used), group_sum(n * h, used)
        n_used = int(used.sum())
        terms = int(acc[used, 0].sum())
        hbar = S / W
        valid = n_used >= 2
        table = np.zeros((G, 8))
        table[:, :3] = x
        table[:, 3] = used
        inside = np.float64(0.0)
        if valid:
            s = R * (h - hbar)
            two = 2.0 * s
            e = s * s
            for b in range(dim):
                table[:, 4 + b] = np.where(used, two * y[:, b], 0.0)
            table[:, 7] = np.where(used, e, 0.0)
            inside = group_sum(n * e, used)
        fit = np.zeros(8)
        fit[0], fit[1], fit[2] = hbar, _dot3(a, np.concatenate([c, [0.0]]), dim) + R * hbar, W
        fit[3], fit[4] = n_used, valid

        u, m, L = f["u"], f["m"], f["L"]
        lab = np.clip(f["label"], 0, G - 1)
        has = f["counts"] & used[lab] & valid
        row = table[lab]
        q = m - row[:, :dim].T
        alpha = fr._dot(u, q)
        lever = (R * alpha) / L
        rest = 1.0 - lever
        mu = row[:, 4:4 + dim].T
        beta = fr._dot(mu, u)
        k = beta / L
        rho = R * (q - alpha * u)
        muP = mu - beta * u
        turn = k * rho
        g_end, g_start = muP * rest - turn, muP * lever + turn
    cols = block.shape[1]
    grad = np.zeros((2 * dim, cols))
    grad[:dim] = np.where(has[None, :], g_start, 0.0)
    grad[dim:] = np.where(has[None, :], g_end, 0.0)
    term = np.where(f["counts"] & used[lab], row[:, 7], 0.0)
    heights = f["foci"] @ a[:dim]
    residuals = np.where(used, (R * (h - hbar)) if valid else 0.0, np.nan)
    return dict(acc=acc, table=table, fit=fit, error=float(inside), terms=float(terms),
                mean=float(inside) / terms if terms > 0 else float("nan"), grad=grad, term=term,
                used=used, heights=heights, residuals=residuals, foci=f["foci"], has=has,
                counts=f["counts"], a=a, valid=bool(valid), n_used=n_used, focus=f, hbar=hbar,
                offset=float(fit[1]), R=float(R))


# ------------------------------------------------------------------------------ the inputs
def rays(n, G, dtype=np.float64, dimension=3, permuted=False, seed=41):
    """``focus_error_reference.rays`` with at least two converging groups among the labels
    ``[0, G)``: that generator keeps its last three labels for a parallel group, a single ray and
    an empty group, which leaves ONE converging group at G = 3 -- no plane.  Below five groups
    the lines are made for G + 2 labels, so that among the first G there are G - 1 converging
    groups and the parallel one; the labels G and G + 1 (the single ray, the empty group) then
    count as out of range, as -1 and G + 2 do."""
    return fr.rays(n, G if G >= 5 else G + 2, dtype, dimension, permuted, seed)


def case(n, G, dtype=np.float64, dimension=3, permuted=False, masked=False, plane=True):
    """(block, mask, group, perm, ref) of one case.  The guard: a case has at least two used
    groups -- a valid plane --, unless it is asked for with ``plane=False``: then it has none."""
    block, mask, group, perm = rays(n, G, dtype, dimension, permuted)
    as64 = block.astype(np.float64) if np.dtype(dtype) == np.float16 else block
    ref = flatfield_error(as64, group, G, DOMAIN, AXIS3 if dimension == 3 else AXIS2,
                          mask=mask if masked else None, perm=perm if permuted else None)
    if plane:
        assert ref["n_used"] >= 2 and ref["valid"], (n, G, dimension, ref["n_used"])
    else:
        assert not ref["valid"], (n, G, dimension, ref["n_used"])
    return block, mask, group, perm, ref


def error_bound(ref):
    """|error - reference error| between two evaluations that agree on every group's term and
    differ in the order of their float sums (``focus_error_reference.error_bound``'s argument over
    the groups): ``G eps sum n e_g``."""
    return ref["table"].shape[0] * EPS * abs(ref["error"])
