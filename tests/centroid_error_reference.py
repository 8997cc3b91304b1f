"""Plain numpy restatement of ``CentroidError`` (TEST INFRASTRUCTURE): float64 and int64, no
torch, written from the definition in include/tfrt_hip.h at tfrt_centroid_error, not from the
kernels -- the order of every sum over the groups included.

The columns, the four cases of a counting column, the records ``{count, Sx, Sy, 0}``, the
penalties and their gradient are ``SpotError``'s, taken from tests/spot_error_reference.py
(imported, not edited); fields and the chain rule of a direction field from
tests/direction_fields_reference.py.  A group with ``count > 0`` HAS RAYS: ``w = count``,
``cx = x0 + (Sx / w) / qsx``; with one field every y component is 0.0.

* ``targets``: ``t_g = targets[g]``; the group has a target iff the row is finite;
* ``parents``: the group has a target iff ``0 <= parents[g] < P``; the record of parent p is the
  integer sum of the records of its groups with rays and a target, ``C_p`` its centroid by the
  same expression, ``t_g = C_parents[g]``;
* a group is USED iff it has rays and a target: ``r = c - t``; the residual table holds ``r``,
  0.0 for a group with rays that is not used, NaN for a group without rays;
* ``error = (sum w * (rx * rx) + sum w * (ry * ry)) + penalties`` with ``fixed_sum``, the shape
  of every sum over the groups, and ``penalty_sum``, the shape of the sum of the penalties (the
  accumulate launch's workgroups, then their partials in index order); a ray inside has the
  gradient ``2 * rx``, ``2 * ry`` of its group.

Also the bound the tests share, with its derivation (``error_bound``), and the inputs (``rays``,
``targets_for``, ``parents_for``).
"""
import numpy as np

import direction_fields_reference as dfr
import spot_error_reference as sr

EPS = float(np.finfo(np.float64).eps)
BLOCK = 1024            # the threads of the one workgroup that sums over the groups
ACC_BLOCK = 256         # the threads of a workgroup of the accumulate launch
ACC_COLUMNS = 4 * ACC_BLOCK     # one workgroup per that many columns ...
ACC_MAX_GRID = 512      # ... and at most that many workgroups
DOMAIN = sr.DOMAIN
OOB = 0.3


def qbits_of(n_source):
    return sr.qbits_of(n_source)


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


def _wave_tree(lanes):
    """(W, 64) lanes -> (W,): ``v[lane] += v[lane ^ d]`` for d = 32, 16, 8, 4, 2, 1, lane 0."""
    w = lanes
    for d in (32, 16, 8, 4, 2, 1):
        w = w[:, :d] + w[:, d:2 * d]
    return w[:, 0]


def penalty_sum(penalty, outside):
    """The sum of ``penalty[outside]`` over the n columns in the shape and order of the launches:
    the accumulate launch has ``B = min(512, ceil(n / 1024))`` workgroups of 256 threads; thread
    t of workgroup b adds its columns ``256 b + t``, ``+ 256 B``, ... in ascending order onto 0.0
    (columns that are not penalised add nothing); within each wave of 64 threads
    ``v[lane] += v[lane ^ d]`` for d = 32 .. 1, then the workgroup's 4 waves in index order onto
    0.0: one partial per workgroup.  The table launch's thread j takes the partials j, j + 1024,
    ... (at most one: B <= 512), its waves the same tree, then its 16 waves in index order onto
    0.0."""
    n = penalty.shape[0]
    if n == 0:
        return np.float64(0.0)
    B = min(ACC_MAX_GRID, (n + ACC_COLUMNS - 1) // ACC_COLUMNS)
    stride = B * ACC_BLOCK
    trips = (n + stride - 1) // stride
    v = np.zeros(trips * stride)
    v[:n] = np.where(outside, penalty, 0.0)
    lanes = np.zeros(stride)
    for trip in v.reshape(trips, stride):
        lanes = lanes + trip                   # (penalties are >= 0: adding 0.0 changes no bit)
    waves = _wave_tree(lanes.reshape(B * (ACC_BLOCK // 64), 64)).reshape(B, ACC_BLOCK // 64)
    partial = np.zeros(B)
    for k in range(ACC_BLOCK // 64):
        partial = partial + waves[:, k]
    lanes = np.zeros(BLOCK)
    lanes[:B] = partial
    total = np.float64(0.0)
    for wave in _wave_tree(lanes.reshape(BLOCK // 64, 64)):
        total = total + wave
    return total


def _centroids(table, x0, qsx, y0, qsy, two):
    """(has rays, cx, cy) of a record table; 0.0 where a record has no rays."""
    rays = table[:, 0] > 0
    w = np.where(rays, table[:, 0], 1).astype(np.float64)
    cx = np.where(rays, x0 + (table[:, 1].astype(np.float64) / w) / qsx, 0.0)
    cy = np.where(rays, y0 + (table[:, 2].astype(np.float64) / w) / qsy, 0.0) if two \
        else np.zeros(table.shape[0])
    return rays, cx, cy


def centroid_error(x, y, group, n_groups, domain, targets=None, parents=None, n_parents=None,
                   oob_weight=0.0, mask=None, perm=None, qbits=None):
    """``y`` None: one field (``targets`` is then (G, 1)).  Exactly one of ``targets`` and
    ``parents`` (with ``n_parents``).  Returns a dict: acc ((G, 4) int64), parent_acc ((P, 4)
    int64 or None), centroids ((G, k), NaN without rays), parent_centroids ((P, k) or None),
    residual ((G, 2)), used, rays, groups_used, parents_used, error, terms, mean, grad_x, grad_y
    (None without y), abs_sum, n, n_groups, n_inside, n_penalised, inside, outside, label."""
    assert (targets is None) != (parents is None)
    two = y is not None
    k = 2 if two else 1
    G = int(n_groups)
    spot = sr.spot_error(x, y, group, G, domain, oob_weight, mask=mask, perm=perm, qbits=qbits)
    acc = spot["acc"]
    n = spot["n"]
    if qbits is None:
        qbits = qbits_of(np.asarray(group).shape[0])
    one = np.ldexp(np.float64(1.0), qbits)
    (x0, x1) = (np.float64(v) for v in domain[0])
    qsx = one / (x1 - x0)
    (y0, y1) = (np.float64(v) for v in domain[1]) if two else (np.float64(0), np.float64(0))
    qsy = one / (y1 - y0) if two else np.float64(0)

    rays, cx, cy = _centroids(acc, x0, qsx, y0, qsy, two)
    w = acc[:, 0].astype(np.float64)
    parent_acc = parent_centroids = None
    if targets is not None:
        targets = np.asarray(targets, dtype=np.float64)
        assert targets.shape == (G, k)
        tx = targets[:, 0]
        ty = targets[:, 1] if two else np.zeros(G)
        has = np.isfinite(tx) & np.isfinite(ty)
        parents_used = 0
    else:
        parents = np.asarray(parents).astype(np.int64)
        P = int(n_parents)
        assert parents.shape == (G,) and P >= 1
        has = (parents >= 0) & (parents < P)
        sel = rays & has
        parent_acc = np.zeros((P, 4), dtype=np.int64)
        np.add.at(parent_acc, parents[sel], acc[sel])
        prays, Cx, Cy = _centroids(parent_acc, x0, qsx, y0, qsy, two)
        at = np.clip(parents, 0, P - 1)
        tx, ty = Cx[at], Cy[at]
        parents_used = int(prays.sum())
        parent_centroids = np.where(prays[:, None], np.stack([Cx, Cy], axis=1), np.nan)[:, :k]
    used = rays & has
    residual = np.full((G, 2), np.nan)
    residual[rays] = 0.0
    with np.errstate(invalid="ignore"):
        residual[used, 0] = (cx - tx)[used]
        residual[used, 1] = (cy - ty)[used]
    r = np.where(used[:, None], residual, 0.0)
    ex_t, ey_t = w * (r[:, 0] * r[:, 0]), w * (r[:, 1] * r[:, 1])
    e_inside = fixed_sum(ex_t, used) + fixed_sum(ey_t, used)

    # the rays: SpotError's penalties and their gradient outside; 2 r of the ray's group inside
    inside, outside = spot["inside"], spot["outside"]
    group = np.asarray(group)
    s = np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm)[:n].astype(np.int64)
    label = np.full(n, -1, dtype=np.int64)
    s_ok = (s >= 0) & (s < group.shape[0])
    label[s_ok] = group[s[s_ok]]
    li = label[inside]
    gx = np.where(outside, spot["grad_x"], 0.0)
    gx[inside] = 2.0 * residual[li, 0]
    gy = None
    if two:
        gy = np.where(outside, spot["grad_y"], 0.0)
        gy[inside] = 2.0 * residual[li, 1]
    xv = np.asarray(x, dtype=np.float64)
    yv = np.asarray(y, dtype=np.float64) if two else np.zeros(n)
    xo, yo = xv[outside], yv[outside]
    ex = np.maximum(x0 - xo, 0.0) + np.maximum(xo - x1, 0.0)
    ey = (np.maximum(y0 - yo, 0.0) + np.maximum(yo - y1, 0.0)) if two else np.zeros_like(xo)
    penalties = oob_weight * (ex * ex + ey * ey)
    per_column = np.zeros(n)
    per_column[outside] = penalties
    error = float(e_inside + penalty_sum(per_column, outside))
    n_terms = spot["terms"]
    return dict(acc=acc, parent_acc=parent_acc, centroids=spot["centroids"],
                parent_centroids=parent_centroids, residual=residual, used=used, rays=rays,
                groups_used=int(used.sum()), parents_used=parents_used, error=error,
                terms=n_terms, mean=error / n_terms if n_terms > 0 else float("nan"),
                grad_x=gx, grad_y=gy,
                abs_sum=float(np.sum(ex_t[used]) + np.sum(ey_t[used]) + np.sum(penalties)),
                n=n, n_groups=G, n_inside=int(inside.sum()), n_penalised=int(outside.sum()),
                inside=inside, outside=outside, label=label, qsx=float(qsx), qsy=float(qsy))


def error_bound(ref):
    """(For the sums torch makes -- the penalty sum of the CPU path of ``ops.centroid_error``,
    the generic path's sum of its (n, k) terms; the kernels' error is the reference's bit for
    bit.)  |error - reference error| between two evaluations that agree on every group's term and
    every penalty and differ in the order of their float sums: a sum of m numbers in ANY order is
    within (m - 1) eps sum|a_i| of the exact sum to first order (Higham, Accuracy and Stability,
    eq. 4.4), so two orders differ by at most twice that; here m <= n penalties + 2 G group terms,
    all non-negative.  Derived, not measured."""
    return 2.0 * (ref["n"] + 2 * ref["n_groups"]) * EPS * ref["abs_sum"]


def fields(block, codes, group, n_groups, domain, **kw):
    """CentroidError of the fields ``codes`` of the (2d, n) geometry block ``block``: the dict of
    ``centroid_error`` plus ``grad`` (2d, n) -- through the chain rule with a direction field --
    and ``counts`` (the columns in a group or penalised)."""
    vals, d, L, ok = dfr.field_values(block, codes)
    two = len(codes) == 2
    ref = centroid_error(vals[0], vals[1] if two else None, group, n_groups, domain, **kw)
    gv = [ref["grad_x"]] + ([ref["grad_y"]] if two else [])
    return dfr._compose(ref, gv, codes, d, L, ok, ref["inside"] | ref["outside"])


# ------------------------------------------------------------------------------ the inputs
def rays(n, n_groups=3, dtype=np.float64, seed=23):
    """spot_error_reference's ``points``: (x, y, mask, group, perm); the last group is empty when
    G > 1, the labels -1 and G occur, about one point in eight is outside."""
    return sr.points(n, dtype, n_groups, seed)


def targets_for(n_groups, two=True, seed=5):
    """(G, k) targets inside ``DOMAIN``; row 1 (G > 2) has a NaN in its LAST entry and row 2
    (G > 4) in its first: not pinned."""
    rng = np.random.default_rng(seed + n_groups)
    (x0, x1), (y0, y1) = DOMAIN
    t = np.stack([rng.uniform(x0, x1, n_groups), rng.uniform(y0, y1, n_groups)], axis=1)
    t = np.ascontiguousarray(t[:, :2 if two else 1])
    if n_groups > 2:
        t[1, -1] = np.nan
    if n_groups > 4:
        t[2, 0] = np.nan
    return t


def parents_for(n_groups, n_parents, seed=9):
    """(G,) int32 parent labels: group g belongs to parent g % P; group 1 (G > 2) has the label
    -1 and group 3 (G > 4) the label P -- both left out."""
    p = (np.arange(n_groups) % n_parents).astype(np.int32)
    if n_groups > 2:
        p[1] = -1
    if n_groups > 4:
        p[3] = n_parents
    return p
