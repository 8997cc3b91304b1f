"""
csrc/trace_math.h::adjoint3d, kind of record by kind: the gradient with respect to the pass's
input ray (gs, ge) and to the hit face's vertices (gP) against torch.autograd through the oracle.

adjoint3d sums the two gradients that reach C = E1 x E2 -- the one through the hit parameter and,
when the ray has a child, the one through the face normal -- and runs the reverse of the cross
product once on the sum.  Which of the two is present, and what the second one is made of, depends
on the kind of record, so every kind is checked on its own rows (a kind without rows fails):

  no child                 only the hit parameter's term
  refracted from outside   n.u <= 0, radicand >= 0
  refracted from inside    n.u > 0,  radicand >= 0
  total internal reflection   radicand < 0
  mirror                   n_in == 0

Tolerance 1e-10 (max |difference| / max |autograd| over the kind's rows), the one
tests/test_host_math.py::test_snell3d_and_adjoint3d uses for the same function.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import geom, tracer
from test_host_math import _hit_case

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
D, I = ctypes.c_double, ctypes.c_int64

TOL = 1e-10
KINDS = ("no child", "refracted from outside", "refracted from inside",
         "total internal reflection", "mirror")


@pytest.fixture(scope="module")
def records(host_math):
    """4,000 random hits, their kinds, adjoint3d's gradients and autograd's."""
    rng = np.random.default_rng(8)
    n = 4000
    L = 1.7
    s, e, P9 = _hit_case(rng, n)
    n_in = rng.choice([1.0, 1.5, 0.0, 1.33], size=n)
    n_out = rng.choice([1.0, 1.5, 1.2], size=n)
    child = (rng.random(n) < 0.8).astype(np.uint8)

    st, et, Pt = [torch.tensor(a, requires_grad=True) for a in (s, e, P9)]
    x, y, z, valid, ru, tu, tv = geom.raw_line_triangle_intersect(
        *[st[:, i] for i in range(3)], *[et[:, i] for i in range(3)], *[Pt[:, i] for i in range(9)], 1e-10)
    h = torch.stack([x, y, z], 1)
    norm = tracer.faces_from_vertices(Pt.reshape(-1, 3), np.arange(3 * n).reshape(n, 3))["norm"]
    o = geom.snells_law_3D(st[:, 0], st[:, 1], st[:, 2], x, y, z, norm, torch.tensor(n_in),
                           torch.tensor(n_out), L)
    cs, ce = torch.stack(o[:3], 1), torch.stack(o[3:], 1)
    g = [rng.normal(size=(n, 3)) for _ in range(4)]
    cm = torch.tensor(child.astype(np.float64)).reshape(-1, 1)
    loss = (st * torch.tensor(g[0])).sum() + (h * torch.tensor(g[1])).sum() + \
        (cm * (cs * torch.tensor(g[2]) + ce * torch.tensor(g[3]))).sum()
    want = [t.numpy() for t in torch.autograd.grad(loss, [st, et, Pt])]

    gs, ge, gP = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 9))
    ruu = ru.detach().numpy().copy()
    gh = g[1] + child[:, None] * g[2]
    host_math.hm_adjoint3d(I(n), P(s), P(e), P(P9), P(ruu), P(child), P(n_in), P(n_out), D(L),
                           P(g[0]), P(gh), P(g[3]), P(gs), P(ge), P(gP))

    # the forward's branches (csrc/trace_math.h::snell3d_core, geometry.py:715-753)
    nn = norm.detach().numpy()
    u = h.detach().numpy() - s
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    nu = (nn * u).sum(1)
    internal = nu > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        eta = np.where(internal, n_in / n_out, np.where(n_in != 0.0, n_out / n_in, 0.0))
    k = 1.0 - eta * eta + (eta * nu) ** 2
    has = child != 0
    mirror = has & (n_in == 0.0)
    tir = has & ~mirror & (k < 0.0)
    kind = {
        "no child": ~has,
        "refracted from outside": has & ~mirror & ~tir & ~internal,
        "refracted from inside": has & ~mirror & ~tir & internal,
        "total internal reflection": tir,
        "mirror": mirror,
    }
    assert sum(int(m.sum()) for m in kind.values()) == n     # every record has one kind
    return kind, (gs, ge, gP), want


@pytest.mark.parametrize("name", KINDS)
def test_adjoint3d_ray_and_face_gradients_match_autograd(records, name):
    kind, got, want = records
    rows = kind[name]
    print(f"{name}: {int(rows.sum())} records")
    assert rows.sum() > 0, f"no record of kind '{name}'"
    for what, a, b in zip(("gs", "ge", "gP"), got, want):
        diff, ref = np.abs(a[rows] - b[rows]).max(), np.abs(b[rows]).max()
        print(f"  {what}: max |difference| {diff:.3e}, max |autograd| {ref:.3e}")
        assert ref > 0.0
        assert diff < TOL * ref, f"{name}, {what}: {diff:.3e} against {ref:.3e}"
