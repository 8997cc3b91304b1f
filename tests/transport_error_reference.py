"""Plain numpy restatement of ``TransportError`` (TEST INFRASTRUCTURE): float64 and int64, no
torch, written from the definition in the class's docstring / include/tfrt_hip.h at
tfrt_transport_error, not from the kernels.

Quantile tables: every goal bin split into 4 x 4 sub-points (4 with one field) at the sub-cells'
centres in normalised coordinates, each with the bin's mass, empty ones dropped; per direction
``p = c * xi + s * eta`` sorted stably, ``cm = (cumsum(w) - w / 2) / sum(w)``,
``T = interp(arange(Q + 1) / Q, cm, p_sorted)``.

For the points that count -- finite coordinates, ``mask[i] >= 0`` where a mask is given -- and
every direction: ``xi = (x - x0) * ix``, ``p = c * xi + s * eta``; the key
``q = clamp(floor((p - lo) * scale), 0, 2**26 - 2)`` with ``lo = a - (b - a)``,
``scale = 2**26 / (3 (b - a))``, ``a = min(0, c) + min(0, s)``, ``b = max(0, c) + max(0, s)``
(2**26 - 1 for a point that does not count); ``first`` / ``count`` from ``np.searchsorted`` left /
right on the sorted keys; ``rank2 = 2 first + count``, ``u = (first + count / 2) / n_valid``;
``z = u Q``, ``m = min(floor(z), Q - 1)``, ``f = z - m``, ``t = T[m] + f (T[m + 1] - T[m])``,
``d = p - t``; term ``d * d``; ``gx += ((2 d) c) ix``, ``gy += ((2 d) s) iy`` over k in order.

Also the bound the tests share, with its derivation (``error_bound``), and the input families
(``points``)."""
import numpy as np

KEY_BITS = 26                       # transport_math.h TRANSPORT_KEY_BITS, ops.TRANSPORT_KEY_BITS
KEY_INVALID = (1 << KEY_BITS) - 1
SUBCELLS = 4
EPS = float(np.finfo(np.float64).eps)

DOMAIN = ((-1.0, 0.75), (0.5, 2.0))
FAMILIES = ("uniform", "ties", "outside", "nonfinite", "masked", "all_invalid", "one_valid")


def directions(k, two=True):
    """(K, 2) cos, sin of the angles pi k / K (an int) or of the angles given; one field: (1, 0)."""
    if not two:
        return np.array([[1.0, 0.0]])
    theta = np.pi * np.arange(k, dtype=np.float64) / np.float64(k) if np.ndim(k) == 0 \
        else np.asarray(k, dtype=np.float64)
    return np.stack([np.cos(theta), np.sin(theta)], axis=1)


def tables(goal, cs, knots):
    g = np.asarray(goal, dtype=np.float64)
    two = g.ndim == 2
    nx = g.shape[-1]
    xs = (np.arange(nx * SUBCELLS) + 0.5) / (nx * SUBCELLS)
    if two:
        ny = g.shape[0]
        ys = (np.arange(ny * SUBCELLS) + 0.5) / (ny * SUBCELLS)
        eta, xi = (a.reshape(-1) for a in np.meshgrid(ys, xs, indexing="ij"))
        w = np.kron(g, np.ones((SUBCELLS, SUBCELLS))).reshape(-1)
    else:
        xi, eta, w = xs, np.zeros_like(xs), np.kron(g, np.ones(SUBCELLS))
    keep = w > 0
    xi, eta, w = xi[keep], eta[keep], w[keep]
    at = np.arange(knots + 1, dtype=np.float64) / np.float64(knots)
    out = []
    for c, s in (cs if two else [(1.0, 0.0)]):
        p = c * xi + s * eta if two else xi
        order = np.argsort(p, kind="stable")
        ws = w[order]
        cm = (np.cumsum(ws) - ws / 2.0) / np.sum(ws)
        out.append(np.interp(at, cm, p[order]))
    return np.stack(out)


def key_map(c, s):
    a = min(0.0, c) + min(0.0, s)
    b = max(0.0, c) + max(0.0, s)
    return a - (b - a), float(1 << KEY_BITS) / (3.0 * (b - a))


def keys_of(p, counts, c, s):
    lo, scale = key_map(c, s)
    with np.errstate(invalid="ignore"):
        v = np.floor((p - lo) * scale)
        q = np.where(v >= 0.0, np.minimum(v, float(KEY_INVALID - 1)), 0.0)
    q = np.where(np.isnan(q), 0.0, q).astype(np.int64)
    return np.where(counts, q, KEY_INVALID)


def target(T, knots, rank2, n_valid):
    u = (rank2.astype(np.float64) * 0.5) / np.float64(n_valid)
    z = u * np.float64(knots)
    fm = np.minimum(np.floor(z), np.float64(knots - 1))
    m = fm.astype(np.int64)
    f = z - fm
    return T[m] + f * (T[m + 1] - T[m])


def transport_error(x, y, T, cs, domain, mask=None):
    """``T``: (K, Q + 1) tables, ``cs``: (K, 2); ``y`` None: one field.  Returns a dict: keys
    (K, n) int64, rank2 (K, n) int64 (-1 where a point does not count), n_valid, p, t, terms
    (K, n), grad_x, grad_y (None without y), error {sum, terms, mean}."""
    two = y is not None
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64) if two else np.zeros_like(x)
    n = x.shape[0]
    K, Q = T.shape[0], T.shape[1] - 1
    x0, x1 = domain[0]
    ix = np.float64(1.0) / (np.float64(x1) - np.float64(x0))
    y0, iy = 0.0, 0.0
    if two:
        y0, y1 = domain[1]
        iy = np.float64(1.0) / (np.float64(y1) - np.float64(y0))
    counts = np.isfinite(x) & np.isfinite(y)
    if mask is not None:
        counts &= np.asarray(mask) >= 0
    nv = int(counts.sum())
    with np.errstate(invalid="ignore", over="ignore"):
        xi = (x - x0) * ix
        eta = (y - y0) * iy if two else np.zeros_like(x)
    keys = np.zeros((K, n), dtype=np.int64)
    rank2 = np.full((K, n), -1, dtype=np.int64)
    ps, ts, terms = (np.zeros((K, n)) for _ in range(3))
    gx, gy = np.zeros(n), np.zeros(n)
    for k in range(K):
        c, s = (float(cs[k, 0]), float(cs[k, 1])) if two else (1.0, 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            p = c * xi + s * eta if two else xi
        keys[k] = keys_of(p, counts, c, s)
        sk = np.sort(keys[k][counts])
        first = np.searchsorted(sk, keys[k], "left")
        count = np.searchsorted(sk, keys[k], "right") - first
        rank2[k] = np.where(counts, 2 * first + count, -1)
        if nv == 0:
            continue
        v = np.nonzero(counts)[0]
        t = target(T[k], Q, rank2[k][v], nv)
        d = p[v] - t
        ps[k][v], ts[k][v], terms[k][v] = p[v], t, d * d
        gx[v] = gx[v] + ((2.0 * d) * c) * ix
        gy[v] = gy[v] + ((2.0 * d) * s) * iy
    total = float(np.sum(terms))
    n_terms = float(K * nv)
    return {"keys": keys, "rank2": rank2, "n_valid": nv, "p": ps, "t": ts, "terms": terms,
            "grad_x": gx, "grad_y": gy if two else None,
            "error": (total, n_terms, total / n_terms if n_terms > 0 else float("nan"))}


def error_bound(ref):
    """|error sum - reference sum| between two evaluations whose terms agree bit for bit and whose
    sums differ in order: a sum of m non-negative terms in any order is within (m - 1) eps of its
    exact value relative to the sum (Higham, Accuracy and Stability, eq. 4.4), so two orders
    differ by at most ``2 m eps * sum`` with m = K * n_valid, the number of terms."""
    return 2.0 * ref["error"][1] * EPS * ref["error"][0]


# ------------------------------------------------------------------------------ the inputs
def goal_of(nx, ny, two=True):
    """Two Gaussians on a pedestal-free grid (empty stretches included)."""
    xs = (np.arange(nx) + 0.5) / nx
    if not two:
        g = np.exp(-((xs - 0.3) / 0.08) ** 2) + 0.5 * np.exp(-((xs - 0.8) / 0.05) ** 2)
        return np.where(g > 1e-3, g, 0.0)
    ys = (np.arange(ny) + 0.5) / ny
    X, Y = np.meshgrid(xs, ys, indexing="xy")
    g = np.exp(-((X - 0.3) ** 2 + (Y - 0.35) ** 2) / 0.02) \
        + 0.6 * np.exp(-((X - 0.75) ** 2 + (Y - 0.7) ** 2) / 0.01)
    return np.where(g > 1e-3, g, 0.0)


def points(family, n, seed=0, domain=DOMAIN):
    """(x, y, mask) of a family, float64 and int32 (mask None where the family has none)."""
    rng = np.random.default_rng(seed + 1000 * FAMILIES.index(family))
    (x0, x1), (y0, y1) = domain
    x = rng.uniform(x0, x1, n)
    y = rng.uniform(y0, y1, n)
    mask = None
    if family == "ties":
        x[:], y[:] = 0.25 * x0 + 0.75 * x1, 0.6 * y0 + 0.4 * y1
    elif family == "outside":
        far = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(0.5, 6.0, n)
        half = np.arange(n) % 2 == 0
        x = np.where(half, x + far * (x1 - x0), x)
        y = np.where(half, y - far * (y1 - y0), y)
    elif family == "nonfinite":
        bad = rng.integers(0, 4, n)
        x = np.where(bad == 1, np.nan, x)
        y = np.where(bad == 2, np.inf, y)
        x = np.where((bad == 3) & (np.arange(n) % 2 == 0), -np.inf, x)
    elif family == "masked":
        mask = np.where(rng.uniform(size=n) < 0.4, -1, rng.integers(0, 50, n)).astype(np.int32)
    elif family == "all_invalid":
        mask = np.full(n, -1, dtype=np.int32)
        x[::2] = np.nan
    elif family == "one_valid":
        mask = np.full(n, -1, dtype=np.int32)
        mask[n // 2] = 3
    return x, y, mask
