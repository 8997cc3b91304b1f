"""Plain numpy restatement of ``MixingError`` (TEST INFRASTRUCTURE): float64, int64 and Python
integers, no torch, written from the definition in include/tfrt_hip.h at tfrt_mixing_error, not
from the kernels -- the order of every float sum included.

Column i is source ray ``s = perm[i]`` (``i`` without perm).  A column COUNTS if its coordinates
are finite, ``mask[i] >= 0`` where a mask is given, ``s`` lies in ``[0, n_source)``, its label
``group[s]`` lies in ``[0, G)`` and -- with weights -- ``w = weight[s]`` is finite and in [0, 1].

* outside the closed domain on any axis: nothing goes to the histogram; the error gains
  ``oob_weight * (ex**2 + ey**2)`` (times ``w`` last), ``ex = max(x0 - x, 0) + max(x - x1, 0)``;
* inside: ``u = (x - x0) * sx - 0.5``, ``i0 = floor(u)``, ``t = u - i0``; share ``1 - t`` to column
  ``clamp(i0)``, ``t`` to ``clamp(i0 + 1)``; y alike; the four shares are the products; a share
  ``b`` enters its bin of plane ``group[s]`` as the Python integer ``rint(b * 2**32)`` (weighted:
  ``rint((b * w) * 2**32)``; ``quantise=False``: as the float itself);
* the margins are Python-integer sums: ``nq_g``, ``Pq_b``, ``Nq``; B bins;
* ``p = Hq_gb / nq_g``, ``m = Pq_b / Nq``, ``d = p - m``, ``e_g = B * bins_sum(d * d)``,
  ``E_mix = groups_sum((nq_g / Nq) * e_g)``, ``error = E_mix + penalty_sum``;
  ``D = ((2 * B) / N) * d`` with ``N = Nq * 2**-32``; a group with ``nq_g == 0`` is not used
  (``e_g`` NaN, ``D`` 0); ``Nq == 0``: ``E_mix = 0``, ``D = 0``;
* a ray inside: ``gx = sx * ((1 - ty) * (D[j0, i1] - D[j0, i0]) + ty * (D[j1, i1] - D[j1, i0]))``
  on its own group's plane, ``gy`` symmetric, each times ``w`` last.

``bins_sum``: thread j of 1,024 adds the bins j, j + 1024, ... of a group in ascending order onto
0.0; within each wave of 64 threads ``v[lane] += v[lane ^ d]`` for d = 32 .. 1; then the 16 waves
in index order onto 0.0.  ``groups_sum`` is ``centroid_error_reference.fixed_sum`` (the same shape
over the groups) and the penalties are summed by ``centroid_error_reference.penalty_sum`` (the
splat launch has the accumulate launch's geometry).

Also ``plain_torch``, the plain float definition in torch for autograd, and the inputs.
"""
import numpy as np

import centroid_error_reference as cr
import density_error_reference as dr
import direction_fields_reference as dfr

TWO32 = dr.TWO32
EPS = dr.EPS
BLOCK = 1024
DOMAIN = dr.DOMAIN
OOB = 0.3


def bins_sum(values):
    """(G, B) -> (G,): the fixed-shape sum over the bins of every group (module docstring)."""
    G, B = values.shape
    trips = max((B + BLOCK - 1) // BLOCK, 1)
    v = np.zeros((G, trips * BLOCK))
    v[:, :B] = values
    lanes = np.zeros((G, BLOCK))
    for trip in range(trips):
        lanes = lanes + v[:, trip * BLOCK:(trip + 1) * BLOCK]      # (squares: >= 0)
    w = lanes.reshape(G, BLOCK // 64, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :d] + w[:, :, d:2 * d]
    total = np.zeros(G)
    for wave in range(BLOCK // 64):
        total = total + w[:, wave, 0]
    return total


def _rint_int(v):
    """rint (half to even) of the non-negative floats ``v`` as Python integers."""
    return [int(q) for q in np.rint(v)]


def mixing_error(x, y, group, n_groups, bins, domain, oob_weight=0.0, mask=None, perm=None,
                 weight=None, quantise=True):
    """``y`` None: one field, ``bins`` = (nx,) or nx; else (nx, ny).  Returns a dict: Hq ((G, ny,
    nx) int64 -- (G, nx) with one field --, None unquantised), H (float), nq, Pq, Nq (Python
    integers; floats unquantised), N, D (Hq's shape), group_errors (G,), used, groups_used, e_mix,
    penalty, error, grad_x, grad_y (None without y), counts, inside, outside, label, w, and the
    intermediate sq ((G, B): d * d), sq_sum ((G,): their fixed-shape sums), term ((G,): the
    groups' terms of E_mix) and scale (2 B / N)."""
    two = y is not None
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    y = np.asarray(y, dtype=np.float64) if two else np.zeros_like(x)
    group = np.asarray(group)
    G = int(n_groups)
    counts_b = (int(bins),) if np.ndim(bins) == 0 else tuple(int(b) for b in bins)
    nx, ny = counts_b[0], (counts_b[1] if two else 1)
    B = nx * ny
    (x0, x1) = domain[0]
    sx = np.float64(nx) / (np.float64(x1) - np.float64(x0))
    if two:
        (y0, y1) = domain[1]
        sy = np.float64(ny) / (np.float64(y1) - np.float64(y0))
    counts = np.isfinite(x) & np.isfinite(y)
    if mask is not None:
        counts &= np.asarray(mask)[:n] >= 0
    s = np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm)[:n].astype(np.int64)
    s_ok = (s >= 0) & (s < group.shape[0])
    label = np.full(n, -1, dtype=np.int64)
    label[s_ok] = group[s[s_ok]]
    counts &= s_ok & (label >= 0) & (label < G)
    w = None
    if weight is not None:
        weight = np.asarray(weight, dtype=np.float64)
        w = np.zeros(n)
        w[s_ok] = weight[s[s_ok]]
        with np.errstate(invalid="ignore"):
            counts &= np.isfinite(w) & (w >= 0.0) & (w <= 1.0)
    with np.errstate(invalid="ignore"):
        out = (x < x0) | (x > x1)
        if two:
            out |= (y < y0) | (y > y1)
    inside, outside = counts & ~out, counts & out

    gx, gy = np.zeros(n), np.zeros(n)
    xo, yo = x[outside], y[outside]
    ex = np.maximum(x0 - xo, 0.0) + np.maximum(xo - x1, 0.0)
    ey = (np.maximum(y0 - yo, 0.0) + np.maximum(yo - y1, 0.0)) if two else np.zeros_like(xo)
    pens = oob_weight * (ex * ex + ey * ey)
    gxo = oob_weight * (2.0 * ex) * ((xo > x1).astype(np.float64) - (xo < x0))
    gyo = oob_weight * (2.0 * ey) * ((yo > y1).astype(np.float64) - (yo < y0)) if two else None
    if w is not None:
        pens, gxo = pens * w[outside], gxo * w[outside]
        gyo = gyo * w[outside] if two else None
    gx[outside] = gxo
    if two:
        gy[outside] = gyo
    per_column = np.zeros(n)
    per_column[outside] = pens
    penalty = float(cr.penalty_sum(per_column, outside))

    xi, yi, li = x[inside], y[inside], label[inside]
    wi = w[inside] if w is not None else None
    ia, ib, tx = dr._axis(xi, x0, sx, nx)
    if two:
        ja, jb, ty = dr._axis(yi, y0, sy, ny)
        index = [ja * nx + ia, ja * nx + ib, jb * nx + ia, jb * nx + ib]
        share = [(1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx]
    else:
        index, share = [ia, ib], [1.0 - tx, tx]
    if wi is not None:
        share = [b * wi for b in share]
    cell = [li * B + k for k in index]

    if quantise:
        table = [0] * (G * B)                       # Python integers
        for c, b in zip(cell, share):
            for at, q in zip(c.tolist(), _rint_int(b * TWO32)):
                table[at] += q
        assert all(0 <= v < 2 ** 63 for v in table)
        Hq = np.array(table, dtype=np.int64).reshape(G, B) if G * B else np.zeros((G, B), np.int64)
        nq = [sum(table[g * B:(g + 1) * B]) for g in range(G)]
        Pq = [sum(table[b::B]) for b in range(B)]
        Nq = sum(nq)
        assert Nq < 2 ** 63
        Hf = np.array([float(v) for v in table], dtype=np.float64).reshape(G, B)
        nqf = np.array([float(v) for v in nq], dtype=np.float64)
        Pqf = np.array([float(v) for v in Pq], dtype=np.float64)
        Nqf = np.float64(float(Nq))
        N = Nqf * np.float64(2.0 ** -32)
    else:
        Hq = None
        Hf = np.zeros(G * B)
        for c, b in zip(cell, share):
            np.add.at(Hf, c, b)
        Hf = Hf.reshape(G, B)
        nqf, Pqf = Hf.sum(axis=1), Hf.sum(axis=0)
        nq, Pq = nqf, Pqf
        Nqf = np.float64(nqf.sum())
        Nq = float(Nqf)
        N = Nqf
    used = nqf > 0
    D = np.zeros((G, B))
    group_errors = np.full(G, np.nan)
    e_mix = np.float64(0.0)
    sq, sq_sum, term, scale = np.zeros((G, B)), np.zeros(G), np.zeros(G), np.float64(0.0)
    if Nqf > 0:
        safe = np.where(used, nqf, 1.0)
        d = Hf / safe[:, None] - (Pqf / Nqf)[None, :]
        scale = (2.0 * np.float64(B)) / N
        D = np.where(used[:, None], scale * d, 0.0)
        sq = np.where(used[:, None], d * d, 0.0)
        sq_sum = bins_sum(sq)
        e_g = np.float64(B) * sq_sum
        group_errors = np.where(used, e_g, np.nan)
        term = np.where(used, (safe / Nqf) * e_g, 0.0)
        e_mix = cr.fixed_sum(term, used)
    Dflat = D.reshape(-1)
    if two:
        d00, d01, d10, d11 = (Dflat[c] for c in cell)
        gxi = sx * ((1.0 - ty) * (d01 - d00) + ty * (d11 - d10))
        gyi = sy * ((1.0 - tx) * (d10 - d00) + tx * (d11 - d01))
        gy[inside] = gyi if wi is None else gyi * wi
    else:
        gxi = sx * (Dflat[cell[1]] - Dflat[cell[0]])
    gx[inside] = gxi if wi is None else gxi * wi
    shape = (G, ny, nx) if two else (G, nx)
    error = float(e_mix + penalty)
    return dict(Hq=None if Hq is None else Hq.reshape(shape), H=(Hf / (TWO32 if quantise else 1.0)
                                                                 ).reshape(shape),
                nq=nq, Pq=Pq, Nq=Nq, N=float(N), D=D.reshape(shape), group_errors=group_errors,
                used=used, groups_used=int(used.sum()), e_mix=float(e_mix), penalty=penalty,
                sq=sq, sq_sum=sq_sum, term=term, scale=float(scale),
                error=error, grad_x=gx, grad_y=gy if two else None, counts=counts, inside=inside,
                outside=outside, label=label, w=w, n=n, bins=B, n_groups=G,
                n_penalised=int(outside.sum()), sx=float(sx), sy=float(sy) if two else 0.0)


def fields(block, codes, group, n_groups, bins, domain, **kw):
    """MixingError of the fields ``codes`` of the (2d, n) geometry block ``block``: the dict of
    ``mixing_error`` plus ``grad`` (2d, n) -- through the chain rule with a direction field."""
    vals, d, L, ok = dfr.field_values(block, codes)
    two = len(codes) == 2
    ref = mixing_error(vals[0], vals[1] if two else None, group, n_groups, bins, domain, **kw)
    gv = [ref["grad_x"]] + ([ref["grad_y"]] if two else [])
    return dfr._compose(ref, gv, codes, d, L, ok, ref["counts"])


def plain_torch(x, y, label, n_groups, bins, domain, oob_weight=0.0, w=None):
    """The plain float definition in torch, differentiable in ``x`` / ``y`` (float64 tensors of
    the columns that count, ``label`` their int64 labels in [0, G), ``w`` their weights or None):
    bilinear shares with the clamped indices, the shares' sums per group and per bin,
    ``E_mix = sum_g (n_g / N) * B * sum_b (H_gb / n_g - P_b / N)**2`` plus the penalties.  Nothing
    is detached: autograd differentiates m, n_g and N too."""
    import torch
    two = y is not None
    G = int(n_groups)
    counts_b = (int(bins),) if np.ndim(bins) == 0 else tuple(int(b) for b in bins)
    nx, ny = counts_b[0], (counts_b[1] if two else 1)
    B = nx * ny
    (x0, x1) = domain[0]
    sx = nx / (x1 - x0)
    out = (x < x0) | (x > x1)
    if two:
        (y0, y1) = domain[1]
        sy = ny / (y1 - y0)
        out = out | (y < y0) | (y > y1)
    zero = torch.zeros((), dtype=torch.float64)
    ex = torch.maximum(x0 - x, zero) + torch.maximum(x - x1, zero)
    pens = ex * ex
    if two:
        ey = torch.maximum(y0 - y, zero) + torch.maximum(y - y1, zero)
        pens = pens + ey * ey
    pens = oob_weight * pens
    if w is not None:
        pens = pens * w
    penalty = pens[out].sum()
    ins = ~out

    def axis(v, lo, scale, nb):
        u = (v - lo) * scale - 0.5
        f = torch.floor(u.detach())
        i0 = f.long()
        return i0.clamp(0, nb - 1), (i0 + 1).clamp(0, nb - 1), u - f

    xi, li = x[ins], label[ins]
    ia, ib, tx = axis(xi, x0, sx, nx)
    if two:
        ja, jb, ty = axis(y[ins], y0, sy, ny)
        index = [ja * nx + ia, ja * nx + ib, jb * nx + ia, jb * nx + ib]
        share = [(1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx]
    else:
        index, share = [ia, ib], [1.0 - tx, tx]
    H = torch.zeros(G * B, dtype=torch.float64)
    for k, b in zip(index, share):
        if w is not None:
            b = b * w[ins]
        H = H.index_add(0, li * B + k, b)
    H = H.reshape(G, B)
    ng = H.sum(dim=1)
    N = ng.sum()
    used = ng > 0
    safe = torch.where(used, ng, torch.ones_like(ng))
    d = H / safe[:, None] - (H.sum(dim=0) / N)[None, :]
    e_g = B * (d * d).sum(dim=1)
    e_mix = torch.where(used, (ng / N) * e_g, torch.zeros_like(e_g)).sum()
    return e_mix + penalty


# ------------------------------------------------------------------------------ the inputs
def labels_for(n_source, n_groups, seed=17, empty=None):
    """One int32 label per source ray in [0, G) with -- as far as the source is long enough -- a
    -1 at place 3 and a G at place 9 (both excluded); ``empty``: a group that gets no ray."""
    rng = np.random.default_rng(seed + n_source + 31 * n_groups)
    lab = rng.integers(0, n_groups, n_source).astype(np.int32)
    if empty is not None and n_groups > 1:
        lab[lab == empty] = (empty + 1) % n_groups
    if n_source > 3:
        lab[3] = -1
    if n_source > 9:
        lab[9] = n_groups
    return lab


def inputs(n, dtype=np.float64, n_groups=4, domain=DOMAIN, empty=None):
    """``weighted_errors_reference.density_inputs`` with labels: (x, y, mask, perm, weight,
    group) -- the points of density_error_reference (edge cases at fixed places, about one in
    eight outside), a perm over n + 3 source rays with one entry below 0 and one past the source,
    the special weights at ``SPECIAL_AT`` and one label per source ray."""
    import weighted_errors_reference as wr
    x, y, mask, perm, weight = wr.density_inputs(n, dtype, domain=domain)
    return x, y, mask, perm, weight, labels_for(n + 3, n_groups, empty=empty)
