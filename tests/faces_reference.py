"""
Plain numpy restatement, at ``np.longdouble`` (80-bit), of the face construction and of its reverse
(boundaries.py:890-923, 1065-1078), with the meshes the face tests run on.  No torch, no GPU.

Forward, per face f with corners (i0, i1, i2)::

    P0, P1, P2 = vertices[i0], vertices[i1], vertices[i2]          face_verts[f] = (P0, P1, P2)
    A = P1 - P0,  B = P2 - P1,  C = A x B,  N = C / |C|            norm[f] = N

Reverse, from the mathematics of the normalised cross product.  For an upstream ``n`` on N::

    dN = (I - N N^T) dC / |C|          so   c = (n - N (N.n)) / |C|   is the upstream on C
    dC = dA x B + A x dB               so   a = B x c,  b = c x A     (triple-product identity)
    dA = dP1 - dP0,  dB = dP2 - dP1    so   p0 = -a,  p1 = a - b,  p2 = b

to which the upstream on the face coordinates adds directly.  A corner whose entry of the
``(F,3)`` update mask is false is a constant (stop_gradient): it sends nothing to its vertex.
The corners are scattered into the vertices with ``np.add.at``.

The parametric form is ``vertices = zero + p[:,None]*vectors`` (formed in float64, product and
sum rounded one by one, as every implementation under test forms them) and
``grad_p[v] = dot(grad_vertices_masked[v], vectors[v])``.
"""
import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _corners(vertices, faces, dtype):
    v = np.asarray(vertices, dtype=dtype)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]], f


def forward(vertices, faces, dtype=LD):
    """-> face_verts (F,9), norm (F,3) in ``dtype``."""
    p0, p1, p2, _ = _corners(vertices, faces, dtype)
    c = _cross(p1 - p0, p2 - p1)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = c / np.sqrt(np.sum(c * c, axis=1, keepdims=True))
    return np.concatenate([p0, p1, p2], axis=1), n


def corner_grads(vertices, faces, grad_face_verts=None, grad_norm=None, dtype=LD):
    """(F,9): the gradient on every face coordinate, before mask and scatter."""
    p0, p1, p2, f = _corners(vertices, faces, dtype)
    g = np.zeros((f.shape[0], 9), dtype=dtype)
    if grad_face_verts is not None:
        g = g + np.asarray(grad_face_verts, dtype=dtype).reshape(-1, 9)
    if grad_norm is not None:
        n_up = np.asarray(grad_norm, dtype=dtype).reshape(-1, 3)
        a, b = p1 - p0, p2 - p1
        c = _cross(a, b)
        with np.errstate(invalid="ignore", divide="ignore"):
            length = np.sqrt(np.sum(c * c, axis=1, keepdims=True))
            unit = c / length
            c_up = (n_up - unit * np.sum(unit * n_up, axis=1, keepdims=True)) / length
            a_up, b_up = _cross(b, c_up), _cross(c_up, a)
            g = g + np.concatenate([-a_up, a_up - b_up, b_up], axis=1)
    return g


def _scatter(corner, faces, mask, n_vertices):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keep = np.ones(f.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    out = np.zeros((n_vertices, 3), dtype=corner.dtype)
    g = corner.reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):
        np.add.at(out, f[keep], g[keep])
    return out


def backward_vertices(vertices, faces, grad_face_verts=None, grad_norm=None, mask=None, dtype=LD):
    """-> grad_vertices (V,3) in ``dtype``."""
    g = corner_grads(vertices, faces, grad_face_verts, grad_norm, dtype)
    return _scatter(g, faces, mask, np.asarray(vertices).shape[0])


def param_vertices(zero, vectors, params):
    """float64 vertices of the parametric surface: product and sum are separate roundings."""
    zero, vectors = np.asarray(zero, dtype=np.float64), np.asarray(vectors, dtype=np.float64)
    step = np.asarray(params, dtype=np.float64).reshape(-1, 1) * vectors
    return zero + step


def backward_params(zero, vectors, params, faces, grad_face_verts=None, grad_norm=None, mask=None,
                    dtype=LD):
    """-> grad_parameters (V,) in ``dtype``."""
    gv = backward_vertices(param_vertices(zero, vectors, params), faces, grad_face_verts,
                           grad_norm, mask, dtype)
    with np.errstate(invalid="ignore"):
        return np.sum(gv * np.asarray(vectors, dtype=dtype), axis=1)


def rounding_scale(vertices, faces, grad_face_verts=None, grad_norm=None, mask=None, vectors=None):
    """(V,) float64: the size of what is summed into each vertex, for a float64 rounding bound.

    A float64 evaluation of the reverse differs from the exact one by a few roundings of every
    term it adds.  The terms of a corner are its upstream on the coordinates and the normal's
    part, |a| + |b| <= (|A| + |B|) |n| / |C|.  The normal's part is itself computed from C, a
    difference of products of size |A||B| that keeps only |C| of it: it carries the relative
    rounding of one operation times kappa = |A||B| / |C| (1/sin of the angle at P1, ~1e6 for a
    sliver), not one rounding.  With ``vectors`` the scale is that of grad_p (times |vector|_1).
    """
    p0, p1, p2, f = _corners(vertices, faces, LD)
    s = np.zeros((f.shape[0], 3), dtype=LD)
    if grad_face_verts is not None:
        s = s + np.abs(np.asarray(grad_face_verts, dtype=LD).reshape(-1, 3, 3)).max(axis=2)
    if grad_norm is not None:
        a, b = p1 - p0, p2 - p1
        la, lb = np.sqrt((a * a).sum(1)), np.sqrt((b * b).sum(1))
        lc = np.sqrt((_cross(a, b) ** 2).sum(1))
        ln = np.sqrt((np.asarray(grad_norm, dtype=LD).reshape(-1, 3) ** 2).sum(1))
        with np.errstate(invalid="ignore", divide="ignore"):
            part = (la * lb / lc) * (la + lb) * ln / lc
        s = s + part[:, None]
    keep = np.ones(f.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    out = np.zeros(np.asarray(vertices).shape[0], dtype=LD)
    with np.errstate(invalid="ignore"):
        np.add.at(out, f[keep], s[keep])
    if vectors is not None:
        out = out * np.abs(np.asarray(vectors, dtype=LD)).sum(axis=1)
    return out.astype(np.float64)


def valence(faces, n_vertices):
    """(V,) corners per vertex."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1)
    return np.bincount(f, minlength=n_vertices)[:n_vertices]


# ------------------------------------------------------------------------------------ meshes
# Every mesh is a dict: faces (F,3) int32, zero (V,3), vectors (V,3), params (V,) and
# vertices (V,3) == param_vertices(zero, vectors, params) bit for bit, so that the vertex form
# and the parametric form describe the same triangles.  ``exact`` lists vertices whose parameter
# is 0: they sit exactly where they were put.

def _mesh(points, faces, seed, exact=()):
    rng = np.random.default_rng(seed + 1000)
    points = np.asarray(points, dtype=np.float64)
    V = points.shape[0]
    vectors = rng.standard_normal((V, 3))
    params = rng.uniform(-0.2, 0.2, V)
    params[list(exact)] = 0.0
    zero = points - params.reshape(-1, 1) * vectors
    zero[list(exact)] = points[list(exact)]
    return dict(faces=np.asarray(faces, dtype=np.int32).reshape(-1, 3), zero=zero, vectors=vectors,
                params=params, vertices=param_vertices(zero, vectors, params))


def _distinct_faces(rng, F, pool):
    """F triples of different vertices drawn from ``pool``."""
    pool = np.asarray(pool)
    return np.stack([rng.choice(pool, size=3, replace=False) for _ in range(F)])


def soup(F, V, seed, used=None):
    """Random triangles over V shared vertices; only the first ``used`` are referenced.  With
    fewer than 3 vertices to draw from, faces repeat a vertex (zero area)."""
    rng = np.random.default_rng(seed)
    used = V if used is None else used
    if used >= 3:
        faces = _distinct_faces(rng, F, np.arange(used))
    else:
        faces = rng.integers(0, used, size=(F, 3))
    return _mesh(rng.standard_normal((V, 3)), faces, seed)


def fan(n, seed):
    """n triangles round vertex 0 (valence n); the centre sits at corner f % 3 of face f."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n + 1) / (n + 1) + rng.uniform(-0.2, 0.2, n + 1) / (n + 1)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.3 * rng.standard_normal(n + 1)], axis=1)
    rim *= rng.uniform(0.7, 1.3, (n + 1, 1))
    points = np.concatenate([[[0.05, -0.02, 0.4]], rim])
    faces = np.array([np.roll([0, 1 + i, 2 + i], i % 3) for i in range(n)])
    return _mesh(points, faces, seed)


def repeated(F, V, seed):
    """Random triangles; every third face names a vertex twice (patterns aab, aba, abb, aaa)."""
    rng = np.random.default_rng(seed)
    faces = _distinct_faces(rng, F, np.arange(V))
    for k, f in enumerate(range(0, F, 3)):
        a, b = faces[f, 0], faces[f, 1]
        faces[f] = [(a, a, b), (a, b, a), (a, b, b), (a, a, a)][k % 4]
    return _mesh(rng.standard_normal((V, 3)), faces, seed)


def slivers(F, height, seed):
    """A strip of F triangles (i, i+1, i+2) over points on a line, offset sideways by
    +-height/2 in turn: bases of ~0.2, heights of ~``height``, in a random orientation."""
    rng = np.random.default_rng(seed)
    V = F + 2
    i = np.arange(V)
    points = np.stack([0.1 * i + 0.01 * rng.uniform(-1, 1, V),
                       0.5 * height * (-1.0) ** i * (1 + 0.2 * rng.uniform(-1, 1, V)),
                       0.2 * height * rng.uniform(-1, 1, V)], axis=1)
    # turned out of the axes: the cross product then cancels products of the size of the bases
    # down to base x height, which is what makes a sliver ill-conditioned
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    points = points @ q.T + rng.standard_normal(3)
    faces = np.stack([i[:-2], i[1:-1], i[2:]], axis=1)
    return _mesh(points, faces, seed)


def zero_area(F, V, seed):
    """F good random triangles over V vertices, and among them five of zero area: two on three
    exactly collinear points (vertices V-3..V-1, also used by good faces) and three that repeat
    an index.  -> (mesh, rows of the zero-area faces)."""
    rng = np.random.default_rng(seed)
    points = rng.standard_normal((V, 3))
    points[V - 3:] = [[0.25, -0.5, 1.0], [0.75, 0.0, 1.5], [1.25, 0.5, 2.0]]
    faces = _distinct_faces(rng, F, np.arange(V))
    while True:     # the random faces are good ones: none lies on the collinear triple alone
        on_line = np.all(faces >= V - 3, axis=1)
        if not on_line.any():
            break
        faces[on_line] = _distinct_faces(rng, int(on_line.sum()), np.arange(V))
    bad = np.array([[V - 3, V - 2, V - 1], [V - 1, V - 3, V - 2], [2, 2, 5], [7, 4, 7], [9, 9, 9]])
    order = rng.permutation(F + 5)
    faces = np.concatenate([faces, bad])[order]
    rows = np.sort(np.nonzero(order >= F)[0])
    return _mesh(points, faces, seed, exact=(V - 3, V - 2, V - 1)), rows


SLIVER_HEIGHT = 1e-6


def cases():
    """name -> mesh, the cases of the face tests.  F in {1, 255, 256, 257} (a face block is 256
    threads), V in {1, 3, 31, 32, 33, 257} (a gather block holds 32 vertices)."""
    out = {
        "soup_F1_V3": soup(1, 3, 1),
        "soup_F255_V31": soup(255, 31, 2),
        "soup_F256_V32": soup(256, 32, 3),
        "soup_F257_V33": soup(257, 33, 4),
        "soup_F257_V257": soup(257, 257, 5),
        "soup_F255_V1": soup(255, 1, 6),
        "unreferenced_F40_V33": soup(40, 33, 7, used=20),
        "repeated_F50_V20": repeated(50, 20, 8),
        "slivers_F60": slivers(60, SLIVER_HEIGHT, 9),
        "zero_area_F105_V40": zero_area(100, 40, 10)[0],
    }
    for n in (1, 7, 8, 9, 64, 300):
        out[f"fan_{n}"] = fan(n, 20 + n)
    return out


def masks(mesh, seed):
    """None, a random (F,3) mask, and that mask with every corner of the vertex of the highest
    valence switched off as well."""
    f = mesh["faces"]
    rng = np.random.default_rng(seed)
    rand = rng.random(f.shape) < 0.6
    off = rand & (f != int(np.argmax(valence(f, mesh["vertices"].shape[0]))))
    return {"nomask": None, "mask": rand.astype(np.uint8), "vertex_off": off.astype(np.uint8)}


def upstreams(n_faces, seed):
    """The three upstream combinations: name -> (grad_face_verts or None, grad_norm or None)."""
    rng = np.random.default_rng(seed)
    g_fv, g_n = rng.standard_normal((n_faces, 9)), rng.standard_normal((n_faces, 3))
    return {"fv": (g_fv, None), "norm": (None, g_n), "both": (g_fv, g_n)}
