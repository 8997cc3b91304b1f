"""
numpy float64 restatement of the two definitions behind SumError (include/tfrt_hip.h at
tfrt_goal_error_columns and tfrt_error_combine), with the same operation order: every numpy
operation below is one IEEE float64 operation per element, rounded on its own.
"""
import numpy as np

EPS = 2.0 ** -52


def goal_error_columns(rows, fields, goal, mask=None, perm=None, by_ray=False, n_source=None):
    """``rows`` (n_rows, n) of any float dtype, ``fields`` the rows compared with the goal,
    ``goal`` (fields, n_source) or -- ``by_ray`` -- (n_source, fields).  Returns a dict: ``grad``
    (n_rows, n) float64 (the fields' rows; every other row stays 0.0), ``counts`` (n,) bool,
    ``terms_each`` the (fields, n) error terms (0.0 where a column does not count), ``error``
    (sum in numpy's order, terms, mean)."""
    n_rows, n = rows.shape
    goal = np.asarray(goal, dtype=np.float64)
    rays = goal.shape[0 if by_ray else 1]
    n_source = rays if n_source is None else n_source
    counts = np.ones(n, dtype=bool) if mask is None else np.asarray(mask)[:n] >= 0
    s = np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm)[:n].astype(np.int64)
    counts = counts & (s >= 0) & (s < n_source)
    at = np.clip(s, 0, max(n_source - 1, 0))
    grad = np.zeros((n_rows, n), dtype=np.float64)
    each = np.zeros((len(fields), n), dtype=np.float64)
    for c, f in enumerate(fields):
        if n_source == 0 or n == 0:
            continue
        g = goal[at, c] if by_ray else goal[c, at]
        o = rows[f].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            d = o - g
            each[c] = np.where(counts, d * d, 0.0)
            grad[f] = np.where(counts, 2.0 * d, 0.0)
    total = float(each.sum())
    terms = float(len(fields) * int(counts.sum()))
    return {"grad": grad, "counts": counts, "terms_each": each,
            "error": (total, terms, total / terms if terms > 0 else float("nan"))}


def sum_bound(each):
    """|any float64 sum of the m non-negative ``each`` - the exact sum| <= m * 2^-52 * sum."""
    return each.size * EPS * float(each.sum())


def error_combine(terms, weights, reduce="sum", n=0, n_rows=6):
    """``terms``: a list of (grad (n_rows, >= n) float64 or None, row_mask, error triple).  Returns
    a dict: ``coeff`` (K,), ``error`` (E, 1.0, E), ``grad`` (n_rows, n) float64, or None when no
    term has a gradient block or n == 0."""
    weights = np.asarray(weights, dtype=np.float64)
    coeff = np.zeros(len(terms), dtype=np.float64)
    for k, (_, _, e) in enumerate(terms):
        if reduce == "sum":
            coeff[k] = weights[k]
        else:
            coeff[k] = weights[k] / np.float64(e[1]) if e[1] > 0 else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        E = coeff[0] * np.float64(terms[0][2][0])
        for k in range(1, len(terms)):
            E = E + coeff[k] * np.float64(terms[k][2][0])
    out = None
    if n > 0 and all(t[0] is not None for t in terms):
        out = np.zeros((n_rows, n), dtype=np.float64)
        for r in range(n_rows):
            acc = None
            for k, (g, row_mask, _) in enumerate(terms):
                if (row_mask >> r) & 1:
                    with np.errstate(invalid="ignore", over="ignore"):
                        p = coeff[k] * np.asarray(g, dtype=np.float64)[r, :n]
                        acc = p if acc is None else acc + p
            if acc is not None:
                out[r] = acc
    return {"coeff": coeff, "error": (float(E), 1.0, float(E)), "grad": out}


def bits(a):
    """The float64 values of ``a`` as uint64 words: equal words, equal bits (signed zeros and NaN
    payloads included)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
