"""Plain numpy restatement of the DIRECTION FIELDS of DensityError and SpotError (TEST
INFRASTRUCTURE): float64, no torch, written from the definition in include/tfrt_hip.h at
tfrt_density_error_fields, not from the kernels.

For a column of a d-D geometry block (rows 0..d-1 start, d..2d-1 end), every operation rounded on
its own::

    e_a = (double) end_a - (double) start_a
    q   = e_x*e_x + e_y*e_y [+ e_z*e_z]          summed left to right
    L   = sqrt(q),  d_a = e_a / L

A column with a non-finite geometry row, or with L not finite or not > 0, has no direction: with a
direction field among the fields it is "a coordinate is non-finite" to the errors.  Field code
``c < 2d`` is block row c, ``2d <= c < 3d`` is ``d_(c - 2d)``.

The chain rule from ``gv_k = d error / d (field k)`` to the 2d gradient rows::

    t   = sum over the direction fields k, in field order, of gv_k * d_(a_k)
    G_b = ((gv_k of the direction field of axis b, else 0.0) - t * d_b) / L
    grad[end_b] = G_b, grad[start_b] = -G_b, then + gv_k of a position field naming the row

``density`` / ``spot`` compose this with tests/density_error_reference.py and
tests/spot_error_reference.py (imported, not edited): the field values go in, their ``grad_x`` /
``grad_y`` come back as ``gv`` and go through ``chain``.
"""
import numpy as np

import density_error_reference as dr
import spot_error_reference as sr

EPS = float(np.finfo(np.float64).eps)
DOMAIN = ((-0.45, 0.3), (-0.2, 0.5))          # for (y_dir, z_dir)


def directions(block):
    """``block``: (2d, n) in any float dtype.  Returns (d (d, n), L (n,), ok (n,) bool)."""
    block = np.asarray(block)
    dim = block.shape[0] // 2
    s = block[:dim].astype(np.float64)
    e = block[dim:].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v = e - s
        q = v[0] * v[0] + v[1] * v[1]
        if dim == 3:
            q = q + v[2] * v[2]
        L = np.sqrt(q)
        ok = np.isfinite(s).all(axis=0) & np.isfinite(e).all(axis=0) & np.isfinite(L) & (L > 0)
        d = v / L
    return d, L, ok


def field_values(block, codes):
    """The float64 values of the fields ``codes`` (NaN in every field of a column without a
    direction, when a direction field is among them), and (d, L, ok)."""
    block = np.asarray(block)
    dim = block.shape[0] // 2
    d, L, ok = directions(block)
    has_dir = any(c >= 2 * dim for c in codes)
    vals = []
    for c in codes:
        assert 0 <= c < 3 * dim
        v = block[c].astype(np.float64) if c < 2 * dim else d[c - 2 * dim].copy()
        if has_dir:
            v = np.where(ok, v, np.nan)
        vals.append(v)
    return vals, d, L, ok


def chain(gv, codes, d, L, ok):
    """``gv``: one (n,) array per field.  Returns the (2d, n) gradient; a column with ``ok`` false
    gets zeros (its gv are zeros anyway: it does not count)."""
    dim = d.shape[0]
    n = d.shape[1]
    axes = [c - 2 * dim for c in codes]
    t = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for g, a in zip(gv, axes):
            if a >= 0:
                t = g * d[a] if t is None else t + g * d[a]
        assert t is not None, "chain: no direction field"
        grad = np.zeros((2 * dim, n))
        for b in range(dim):
            gvb = np.zeros(n)
            for g, a in zip(gv, axes):
                if a == b:
                    gvb = g
            G = (gvb - t * d[b]) / L
            start, end = -G, G
            for g, c in zip(gv, codes):
                if c == b:
                    start = start + g
                if c == dim + b:
                    end = end + g
            grad[b], grad[dim + b] = start, end
    return grad


def _compose(ref, gv, codes, d, L, ok, counts):
    dim = d.shape[0]
    if any(c >= 2 * dim for c in codes):
        grad = np.where(counts[None, :], chain(gv, codes, d, L, ok), 0.0)
    else:
        grad = np.zeros((2 * dim, d.shape[1]))
        for g, c in zip(gv, codes):
            grad[c] = g
    ref = dict(ref)
    ref.update(grad=grad, gv=gv, L=L, ok=ok, d=d, counts=counts)
    return ref


def density(block, codes, goal, domain, oob_weight=0.0, mask=None):
    """DensityError of the fields ``codes`` of ``block``: density_error_reference's dict plus
    ``grad`` (2d, n), ``gv``, ``d``, ``L``, ``ok``, ``counts`` (the columns that count) and
    ``inside``."""
    vals, d, L, ok = field_values(block, codes)
    two = len(codes) == 2
    ref = dr.density_error(vals[0], vals[1] if two else None, goal, domain, oob_weight, mask=mask)
    counts = np.isfinite(vals[0]) & (np.isfinite(vals[1]) if two else True)
    if mask is not None:
        counts &= np.asarray(mask)[:counts.shape[0]] >= 0
    with np.errstate(invalid="ignore"):
        out = np.zeros_like(counts)
        for v, (lo, hi) in zip(vals, domain):
            out |= (v < lo) | (v > hi)
    gv = [ref["grad_x"]] + ([ref["grad_y"]] if two else [])
    ref = _compose(ref, gv, codes, d, L, ok, counts)
    ref["inside"] = counts & ~out
    return ref


def spot(block, codes, group, n_groups, domain, oob_weight=0.0, mask=None, perm=None, qbits=None):
    """SpotError of the fields ``codes`` of ``block``: spot_error_reference's dict plus ``grad``
    (2d, n), ``gv``, ``d``, ``L``, ``ok``, ``counts`` (the columns in a spot or penalised)."""
    vals, d, L, ok = field_values(block, codes)
    two = len(codes) == 2
    ref = sr.spot_error(vals[0], vals[1] if two else None, group, n_groups, domain, oob_weight,
                        mask=mask, perm=perm, qbits=qbits)
    gv = [ref["grad_x"]] + ([ref["grad_y"]] if two else [])
    return _compose(ref, gv, codes, d, L, ok, ref["inside"] | ref["outside"])


# ------------------------------------------------------------------------------ the inputs
def rays(n, dtype=np.float64, seed=5, dimension=3):
    """A (2 * dimension, n) geometry block in ``dtype``: starts uniform in [-1, 1], directions
    normalise((1, N(0, .35), N(0, .35))), lengths uniform in [.5, 3]; columns 16::17 degenerate
    (end = start), columns 22::23 with a NaN in x_end.  The 2-D block is the 3-D one without its z
    rows."""
    rng = np.random.default_rng(seed)
    start = rng.uniform(-1, 1, (3, n))
    u = np.stack([np.ones(n), rng.normal(0, .35, n), rng.normal(0, .35, n)])
    u = u / np.sqrt((u * u).sum(axis=0))
    length = rng.uniform(.5, 3, n)
    end = start + u * length
    end[:, 16::17] = start[:, 16::17]
    end[0, 22::23] = np.nan
    block = np.concatenate([start, end]).astype(dtype)
    if dimension == 2:
        block = block[[0, 1, 3, 4]]
    return np.ascontiguousarray(block)


def census(block, codes, domain):
    """(counting, inside, penalised, degenerate, non-finite, the least distance of a counting
    column's field value from a domain edge) of the generator's columns."""
    vals, d, L, ok = field_values(block, codes)
    inside = ok.copy()
    edge = np.inf
    for v, (lo, hi) in zip(vals, domain):
        with np.errstate(invalid="ignore"):
            inside &= (v >= lo) & (v <= hi)
        edge = min(edge, float(np.abs(v[ok] - lo).min()), float(np.abs(v[ok] - hi).min())) \
            if ok.any() else edge
    finite = np.isfinite(np.asarray(block, dtype=np.float64)).all(axis=0)
    return dict(counting=int(ok.sum()), inside=int(inside.sum()),
                penalised=int((ok & ~inside).sum()), degenerate=int((finite & ~ok).sum()),
                non_finite=int((~finite).sum()), edge=edge, min_L=float(L[ok].min()) if ok.any()
                else np.inf)


def assert_generator(n, block, codes, domain, compare_f32=False):
    """What every test that uses ``rays`` relies on."""
    c = census(block, codes, domain)
    assert c["inside"] >= n / 4 and c["penalised"] >= n / 8, c
    if n >= 64:
        assert c["degenerate"] >= 1 and c["non_finite"] >= 1, c
    if compare_f32:
        assert c["edge"] > 1e-6, c
    return c
