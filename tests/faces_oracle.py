"""The oracle's side of the face tests: float64 torch autograd through
``oracle.tracer.faces_from_vertices`` on the meshes of tests/faces_reference.py, and E_oracle,
its distance from the 80-bit restatement.  CPU only; shared by the host and the GPU test."""
import functools

import numpy as np
import torch

import faces_reference as fr
from oracle import tracer

_COLS = ("xp", "yp", "zp", "x1", "y1", "z1", "x2", "y2", "z2")
F64 = torch.float64


def oracle_forward(vertices, faces, mask=None):
    """-> face_verts (F,9), norm (F,3) as the oracle builds them (torch, on vertices' graph)."""
    f = tracer.faces_from_vertices(vertices, torch.as_tensor(np.asarray(faces), dtype=torch.int64),
                                   None if mask is None else torch.as_tensor(np.asarray(mask)).bool())
    return torch.stack([f[c] for c in _COLS], dim=1), f["norm"]


def _loss(fv, norm, g_fv, g_norm):
    out = 0.0
    if g_fv is not None:
        out = out + (fv * torch.as_tensor(g_fv, dtype=F64)).sum()
    if g_norm is not None:
        out = out + (norm * torch.as_tensor(g_norm, dtype=F64)).sum()
    return out


def oracle_backward_vertices(mesh, g_fv, g_norm, mask):
    v = torch.tensor(mesh["vertices"], dtype=F64, requires_grad=True)
    fv, norm = oracle_forward(v, mesh["faces"], mask)
    g, = torch.autograd.grad(_loss(fv, norm, g_fv, g_norm), v)
    return g.numpy()


def oracle_backward_params(mesh, g_fv, g_norm, mask):
    p = torch.tensor(mesh["params"], dtype=F64, requires_grad=True)
    v = torch.tensor(mesh["zero"]) + p.reshape(-1, 1) * torch.tensor(mesh["vectors"])
    fv, norm = oracle_forward(v, mesh["faces"], mask)
    g, = torch.autograd.grad(_loss(fv, norm, g_fv, g_norm), p)
    return g.numpy()


def reference(mesh, form, g_fv, g_norm, mask):
    """The 80-bit gradient: (V,3) for form "build", (V,) for form "param"."""
    if form == "build":
        return fr.backward_vertices(mesh["vertices"], mesh["faces"], g_fv, g_norm, mask)
    return fr.backward_params(mesh["zero"], mesh["vectors"], mesh["params"], mesh["faces"], g_fv,
                              g_norm, mask)


def relative_error(got, ref):
    """max |got - ref| / max |ref| over the entries where ``ref`` is finite (0 if none is)."""
    fin = np.isfinite(ref)
    if not fin.any() or float(np.abs(ref[fin]).max()) == 0.0:
        return 0.0 if np.array_equal(np.asarray(got)[fin], ref[fin].astype(np.float64)) else np.inf
    with np.errstate(invalid="ignore"):
        return float(np.abs(np.asarray(got, dtype=fr.LD)[fin] - ref[fin]).max()
                     / np.abs(ref[fin]).max())


@functools.lru_cache(maxsize=None)
def _cases():
    return fr.cases()


def case(name):
    return _cases()[name]


def combos(mesh, seed=0):
    """Every (upstream name, mask name) -> (g_fv, g_norm, mask) of a mesh: 3 x 3."""
    ups, mks = fr.upstreams(mesh["faces"].shape[0], seed + 1), fr.masks(mesh, seed + 2)
    return {(u, m): (*ups[u], mks[m]) for u in ups for m in mks}


@functools.lru_cache(maxsize=None)
def e_oracle(name, form):
    """E_oracle of a case and form: the largest, over the nine upstream/mask combinations, of
    max|oracle float64 autograd - longdouble| / max|longdouble|.  Computed once per session."""
    mesh = case(name)
    back = oracle_backward_vertices if form == "build" else oracle_backward_params
    worst = 0.0
    for g_fv, g_norm, mask in combos(mesh).values():
        ref = reference(mesh, form, g_fv, g_norm, mask)
        worst = max(worst, relative_error(back(mesh, g_fv, g_norm, mask), ref))
    return worst


def bound(name, form):
    """The device bound of a case, relative to the largest reference entry:
    8 x max(E_oracle, eps x max valence)."""
    mesh = case(name)
    val = int(fr.valence(mesh["faces"], mesh["vertices"].shape[0]).max())
    return 8.0 * max(e_oracle(name, form), fr.EPS64 * val)
