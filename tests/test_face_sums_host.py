"""
The four-sum form of the reverse sweep's face gradient on the host: csrc/trace_math.h::adjoint3d
with ``face_sums = true`` hands back (Cb[3], numb) -- the gradient w.r.t. C = E1 x E2 and w.r.t. the
hit parameter's numerator -- instead of the nine face-vertex terms, and ``face_sums_expand`` takes a
face's vertices and the SUMS of the four over the rays that hit it to the nine vertex gradients.

The hits are the 4,000 of tests/test_adjoint3d_face_terms_host.py (same generator, same seed),
grouped onto faces of 1, 2, 7 and 64 rays: a group's rays are carried onto its first record's
triangle by the affine map that takes the ray's own triangle there (vertices to vertices, unit
normal to unit normal), which keeps the hit inside the triangle and the hit parameter what it was.
Every one of the five kinds of record must be present among the grouped hits.

  identity    per face, face_sums_expand(P, sum (Cb, numb)) and the sum of the nine-term gP both lie
              within 1e-12 x sum |terms| (per entry, the terms being the rays' nine-term addends) of
              the nine-term sum taken in np.longdouble: two roundings of one real number, 64 addends x
              about 30 roundings x 2^-53 ~ 2e-13.  gs and ge: the same bits in both modes.
  autograd    record by record the four-sum route (expand of the record's own four) agrees with
              torch.autograd through the oracle at 1e-10 of the kind's largest entry, kind by kind.
  non-finite  a non-finite Cb (the critical angle's infinite 1 / sqrt(k): a totally reflected record
              handed over as refracted, so the re-derived radicand is clamped to zero) leaves all
              nine entries of its face non-finite and every other face's bits untouched, in both
              forms.
  C ABI       the gather's descriptor with both forms of the face gradient, or with no upstream at
              all, is refused before any launch.

The harness is this file's own: a few lines of C++ around the header, compiled like tests/host_math
(g++ -O2 -ffp-contract=off) into the test's temporary directory.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import geom, tracer
from test_adjoint3d_face_terms_host import KINDS, TOL
from test_host_math import _hit_case

HARNESS = r"""
#include <stdint.h>
#include "trace_math.h"
extern "C" {
// mode 0: the nine-term call, gP <- the nine terms; mode 1: face_sums = true, S <- (Cb, numb) and
// gP <- face_sums_expand(P, S) of the record alone
void run(int64_t n, int mode, const double* s, const double* e, const double* P, const double* ray_u,
         const uint8_t* has_child, const double* n_in, const double* n_out, const int32_t* branch,
         double L, const double* g_s, const double* g_h, const double* g_ce, double* gs, double* ge,
         double* gP, double* S) {
  for (int64_t i = 0; i < n; ++i) {
    const double *si = s + 3 * i, *ei = e + 3 * i, *Pi = P + 9 * i;
    const double *a = g_s + 3 * i, *b = g_h + 3 * i, *c = g_ce + 3 * i;
    double *o1 = gs + 3 * i, *o2 = ge + 3 * i, *o3 = gP + 9 * i;
    const bool ch = has_child[i] != 0;
    if (mode == 0) {
      tfrt::adjoint3d(si, ei, Pi, ray_u[i], ch, n_in[i], n_out[i], L, a, b, c, o1, o2, o3, nullptr,
                      branch[i]);
    } else {
      double four[9] = {-1, -1, -1, -1, -7, -7, -7, -7, -7};
      tfrt::adjoint3d(si, ei, Pi, ray_u[i], ch, n_in[i], n_out[i], L, a, b, c, o1, o2, four, nullptr,
                      branch[i], true, true, nullptr, true);
      for (int q = 0; q < 4; ++q) S[4 * i + q] = four[q];
      for (int q = 4; q < 9; ++q)
        if (four[q] != -7) S[4 * i] = -12345.678;   // (gP[4..8] must be left untouched)
      tfrt::face_sums_expand(Pi, four, o3);
    }
  }
}
// per face f (records start[f] .. start[f + 1], all on the vertices Pf + 9 f): the nine-term sum
// and the expansion of the summed four
void faces(int64_t nf, const int64_t* start, const double* Pf, const double* gP, const double* S,
           double* sum9, double* expanded) {
  for (int64_t f = 0; f < nf; ++f) {
    double acc9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, acc4[4] = {0, 0, 0, 0};
    for (int64_t i = start[f]; i < start[f + 1]; ++i) {
      for (int q = 0; q < 9; ++q) acc9[q] += gP[9 * i + q];
      for (int q = 0; q < 4; ++q) acc4[q] += S[4 * i + q];
    }
    for (int q = 0; q < 9; ++q) sum9[9 * f + q] = acc9[q];
    tfrt::face_sums_expand(Pf + 9 * f, acc4, expanded + 9 * f);
  }
}
}
"""

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
SIZES = (1, 2, 7, 64)


def _frames(P9):
    """Per triangle: origin P0 and the matrix with columns (P1 - P0, P2 - P0, unit normal)."""
    P0, E1, E2 = P9[:, 0:3], P9[:, 3:6] - P9[:, 0:3], P9[:, 6:9] - P9[:, 0:3]
    C = np.cross(E1, E2)
    return P0, np.stack([E1, E2, C / np.linalg.norm(C, axis=1, keepdims=True)], axis=2)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("face_sums_host")
    src, out = d / "harness.cpp", d / "libharness.so"
    src.write_text(HARNESS)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "tensorflowraytrace_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           "-I", csrc, str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))

    # the hits of test_adjoint3d_face_terms_host.py
    rng = np.random.default_rng(8)
    n, L = 4000, 1.7
    s, e, P9 = _hit_case(rng, n)
    n_in = rng.choice([1.0, 1.5, 0.0, 1.33], size=n)
    n_out = rng.choice([1.0, 1.5, 1.2], size=n)
    child = (rng.random(n) < 0.8).astype(np.uint8)
    g = [rng.normal(size=(n, 3)) for _ in range(4)]

    # faces of 1, 2, 7, 64, 1, 2, ... consecutive records; every ray carried onto its face
    start = [0]
    while start[-1] < n:
        start.append(min(n, start[-1] + SIZES[(len(start) - 1) % len(SIZES)]))
    start = np.asarray(start, dtype=np.int64)
    nf = len(start) - 1
    face = np.repeat(np.arange(nf), np.diff(start))
    lead = start[:-1][face]
    o_src, m_src = _frames(P9)
    o_dst, m_dst = o_src[lead], m_src[lead]
    A = m_dst @ np.linalg.inv(m_src)
    s = o_dst + np.einsum("nij,nj->ni", A, s - o_src)
    e = o_dst + np.einsum("nij,nj->ni", A, e - o_src)
    Pf = np.ascontiguousarray(P9[start[:-1]])
    P9 = np.ascontiguousarray(P9[lead])
    s, e = np.ascontiguousarray(s), np.ascontiguousarray(e)

    st, et, Pt = [torch.tensor(a, requires_grad=True) for a in (s, e, P9)]
    x, y, z, valid, ru, tu, tv = geom.raw_line_triangle_intersect(
        *[st[:, i] for i in range(3)], *[et[:, i] for i in range(3)], *[Pt[:, i] for i in range(9)], 1e-10)
    assert bool(valid.all())
    h = torch.stack([x, y, z], 1)
    norm = tracer.faces_from_vertices(Pt.reshape(-1, 3), np.arange(3 * n).reshape(n, 3))["norm"]
    o = geom.snells_law_3D(st[:, 0], st[:, 1], st[:, 2], x, y, z, norm, torch.tensor(n_in),
                           torch.tensor(n_out), L)
    cs, ce = torch.stack(o[:3], 1), torch.stack(o[3:], 1)
    cm = torch.tensor(child.astype(np.float64)).reshape(-1, 1)
    loss = (st * torch.tensor(g[0])).sum() + (h * torch.tensor(g[1])).sum() + \
        (cm * (cs * torch.tensor(g[2]) + ce * torch.tensor(g[3]))).sum()
    want = [t.numpy() for t in torch.autograd.grad(loss, [st, et, Pt])]
    ruu = ru.detach().numpy().copy()
    gh = np.ascontiguousarray(g[1] + child[:, None] * g[2])

    # the kinds (test_adjoint3d_face_terms_host.py)
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
    assert sum(int(m.sum()) for m in kind.values()) == n

    def run(mode, branch):
        gs, ge, gP, S = [np.zeros((n, w)) for w in (3, 3, 9, 4)]
        lib.run(ctypes.c_int64(n), ctypes.c_int(mode), P(s), P(e), P(P9), P(ruu), P(child), P(n_in),
                P(n_out), P(branch), ctypes.c_double(L), P(g[0]), P(gh), P(g[3]), P(gs), P(ge),
                P(gP), P(S))
        return gs, ge, gP, S

    def faces(gP, S):
        sum9, expanded = np.zeros((nf, 9)), np.zeros((nf, 9))
        lib.faces(ctypes.c_int64(nf), P(start), P(Pf), P(gP), P(S), P(sum9), P(expanded))
        return sum9, expanded

    derive = np.full(n, -1, dtype=np.int32)          # (adjoint3d re-derives the forward's branches)
    nine, four = run(0, derive), run(1, derive)

    # one totally reflected record of a seven-ray face, handed over as refracted: its re-derived
    # radicand is below zero, clamped to zero, and 1 / sqrt(k) is infinite
    sizes = np.diff(start)
    victims = [i for i in np.flatnonzero(tir) if sizes[face[i]] == 7]
    assert victims, "no totally reflected record on a seven-ray face"
    victim = int(victims[0])
    poisoned = derive.copy()
    poisoned[victim] = 1 if internal[victim] else 0
    nine_p, four_p = run(0, poisoned), run(1, poisoned)

    return dict(kind=kind, want=want, start=start, face=face, nine=nine, four=four,
                sums=faces(nine[2], four[3]), victim=victim, nine_p=nine_p, four_p=four_p,
                sums_p=faces(nine_p[2], four_p[3]))


def test_every_face_size_and_kind_is_present(case):
    sizes = np.diff(case["start"])
    print("faces by size:", {int(k): int((sizes == k).sum()) for k in np.unique(sizes)})
    assert set(SIZES) <= set(int(k) for k in sizes)
    for name in KINDS:
        print(f"{name}: {int(case['kind'][name].sum())} records")
        assert case["kind"][name].sum() > 0, f"no record of kind '{name}'"


def test_four_sum_mode_keeps_the_ray_gradients_bits(case):
    nine, four = case["nine"], case["four"]
    assert np.array_equal(nine[0], four[0], equal_nan=True)      # gs
    assert np.array_equal(nine[1], four[1], equal_nan=True)      # ge
    assert not np.any(four[3][:, 0] == -12345.678)               # gP[4..8] left untouched


@pytest.mark.parametrize("size", SIZES)
def test_expanded_sums_equal_the_summed_nine_terms(case, size):
    start, gP = case["start"], case["nine"][2]
    sum9, expanded = case["sums"]
    rows = np.flatnonzero(np.diff(start) == size)
    assert rows.size > 0
    worst = [0.0, 0.0]
    for f in rows:
        terms = gP[start[f]:start[f + 1]].astype(np.longdouble)
        exact = terms.sum(axis=0)
        bound = 1e-12 * np.abs(terms).sum(axis=0)
        assert np.all(bound > 0)
        for k, got in enumerate((sum9[f], expanded[f])):
            ratio = float((np.abs(got - exact) / bound).max())
            worst[k] = max(worst[k], ratio)
    print(f"faces of {size} rays ({rows.size}): largest |difference| / (1e-12 x sum |terms|): "
          f"summed nine terms {worst[0]:.3e}, expanded four sums {worst[1]:.3e}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


@pytest.mark.parametrize("name", KINDS)
def test_four_sum_route_matches_autograd(case, name):
    rows = case["kind"][name]
    assert rows.sum() > 0, f"no record of kind '{name}'"
    for what, a, b in zip(("gs", "ge", "expanded gP"), case["four"][:3], case["want"]):
        diff, ref = np.abs(a[rows] - b[rows]).max(), np.abs(b[rows]).max()
        print(f"{name}, {what}: max |difference| {diff:.3e}, max |autograd| {ref:.3e}")
        assert ref > 0.0
        assert diff < TOL * ref, f"{name}, {what}: {diff:.3e} against {ref:.3e}"


def test_a_non_finite_term_spoils_its_face_and_no_other(case):
    victim, face = case["victim"], case["face"]
    f = int(face[victim])
    assert not np.isfinite(case["four_p"][3][victim, :3]).any()        # Cb of the record
    others = np.arange(len(case["start"]) - 1) != f
    for form, clean, spoilt in zip(("nine terms", "four sums"), case["sums"], case["sums_p"]):
        print(f"{form}: face {f}: {spoilt[f]}")
        assert not np.isfinite(spoilt[f]).any(), form
        assert np.isfinite(clean[f]).all(), form
        assert np.array_equal(clean[others], spoilt[others]), form


def test_gather_descriptor_refuses_both_forms_and_no_upstream():
    """tfrt_param_faces_backward_multi: grad_face_verts and grad_face_sums both set -> -1, every
    upstream NULL -> -1, the four sums without the face block -> -1; all before any launch (the
    pointers are host memory, as in tests/test_cabi.py)."""
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    lib = _lib.lib()
    dummy = ctypes.create_string_buffer(1 << 12)
    ptr = ctypes.cast(dummy, ctypes.c_void_p)

    def surface(**kw):
        d = _lib.FaceSurfaceGrad()
        for k in ("grad_norm", "face_verts", "vectors", "corner_start", "corner_list",
                  "grad_parameters"):
            setattr(d, k, ptr)
        d.n_vertices = 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d):
        arr = (_lib.FaceSurfaceGrad * 2)(surface(n_vertices=0, grad_face_verts=ptr), d)
        return lib.tfrt_param_faces_backward_multi(arr, 2, None)

    assert _lib.FaceSurfaceGrad._fields_[-1][0] == "grad_face_sums"
    assert _lib.Scene3D._fields_[-1][0] == "face_sums" and _lib.Scene3D().face_sums == 0
    assert call(surface(grad_face_verts=ptr, grad_face_sums=ptr)) == -1
    assert call(surface(grad_face_verts=ptr, grad_face_sums=ptr, grad_norm=None)) == -1
    assert call(surface(grad_norm=None)) == -1                       # all three upstreams NULL
    assert call(surface(grad_face_sums=ptr, grad_norm=None, face_verts=None)) == -1
    assert call(surface(grad_face_sums=ptr, n_vertices=0)) == 0      # (nothing to launch)
