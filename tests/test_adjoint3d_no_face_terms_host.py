"""
csrc/trace_math.h::adjoint3d with ``face_terms = false`` (a face nobody differentiates) and with the
index ratios handed over (``ratios``), on the host, kind of record by kind
(tests/test_adjoint3d_face_terms_host.py has the kinds and the hits):

  face_terms = false   gs and ge equal the face_terms = true call bit for bit, gP is left untouched
  ratios               snell_ratios(n_in, n_out) handed over with the forward's branches: gs, ge and
                       gP equal the call that divides n_in and n_out itself, bit for bit

The harness is this file's own: a few lines of C++ around the header, compiled like
tests/host_math (g++ -O2 -ffp-contract=off) into the test's temporary directory.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from oracle import geom
from test_adjoint3d_face_terms_host import KINDS
from test_host_math import _hit_case

HARNESS = r"""
#include <stdint.h>
#include "trace_math.h"
extern "C" {
// mode 0: the plain call; 1: face_terms = false; 2: the forward's branches handed over;
// 3: the branches and snell_ratios(n_in, n_out) handed over, n_in = n_out = 1 passed
void run(int64_t n, int mode, const double* s, const double* e, const double* P, const double* ray_u,
         const uint8_t* has_child, const double* n_in, const double* n_out, const int32_t* branch,
         double L, const double* g_s, const double* g_h, const double* g_ce, double* gs, double* ge,
         double* gP) {
  for (int64_t i = 0; i < n; ++i) {
    const double *si = s + 3 * i, *ei = e + 3 * i, *Pi = P + 9 * i;
    const double *a = g_s + 3 * i, *b = g_h + 3 * i, *c = g_ce + 3 * i;
    double *o1 = gs + 3 * i, *o2 = ge + 3 * i, *o3 = gP + 9 * i;
    const bool ch = has_child[i] != 0;
    if (mode == 0) {
      tfrt::adjoint3d(si, ei, Pi, ray_u[i], ch, n_in[i], n_out[i], L, a, b, c, o1, o2, o3);
    } else if (mode == 1) {
      tfrt::adjoint3d(si, ei, Pi, ray_u[i], ch, n_in[i], n_out[i], L, a, b, c, o1, o2, o3, nullptr,
                      -1, true, false);
    } else if (mode == 2) {
      tfrt::adjoint3d(si, ei, Pi, ray_u[i], ch, n_in[i], n_out[i], L, a, b, c, o1, o2, o3, nullptr,
                      branch[i], false, true);
    } else {
      double r[2];
      tfrt::snell_ratios(n_in[i], n_out[i], &r[0], &r[1]);
      tfrt::adjoint3d(si, ei, Pi, ray_u[i], ch, 1.0, 1.0, L, a, b, c, o1, o2, o3, nullptr,
                      branch[i], false, true, r);
    }
  }
}
}
"""

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import os
    d = tmp_path_factory.mktemp("adjoint3d_no_face_terms")
    src, out = d / "harness.cpp", d / "libharness.so"
    src.write_text(HARNESS)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "tensorflowraytrace_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           "-I", csrc, str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))

    rng = np.random.default_rng(8)
    n, L = 4000, 1.7
    s, e, P9 = _hit_case(rng, n)
    n_in = rng.choice([1.0, 1.5, 0.0, 1.33], size=n)
    n_out = rng.choice([1.0, 1.5, 1.2, 0.0], size=n)      # (n_out == 0: the other safe-value rule)
    child = (rng.random(n) < 0.8).astype(np.uint8)
    g = [rng.normal(size=(n, 3)) for _ in range(3)]

    st, et, Pt = [torch.tensor(a) for a in (s, e, P9)]
    x, y, z, _, ru, _, _ = geom.raw_line_triangle_intersect(
        *[st[:, i] for i in range(3)], *[et[:, i] for i in range(3)], *[Pt[:, i] for i in range(9)], 1e-10)
    ru = ru.numpy().copy()

    # the forward's branches, from the quantities adjoint3d itself re-derives without them
    E1, E2 = P9[:, 3:6] - P9[:, 0:3], P9[:, 6:9] - P9[:, 0:3]
    C = np.cross(E1, E2)
    nn = C / np.linalg.norm(C, axis=1, keepdims=True)
    u = np.stack([x.numpy(), y.numpy(), z.numpy()], 1) - s
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    nu = (nn * u).sum(1)
    internal = nu > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        eta = np.where(internal, np.where(n_out != 0.0, np.where(n_in != 0.0, n_in, 1.0) / n_out, 0.0),
                       np.where(n_in != 0.0, np.where(n_out != 0.0, n_out, 1.0) / n_in, 0.0))
    k = 1.0 - eta * eta + (eta * nu) ** 2
    mirror = n_in == 0.0
    reflect = (k < 0.0) | mirror
    branch = (internal.astype(np.int32) | (reflect.astype(np.int32) << 1)).astype(np.int32)

    def run(mode):
        gs, ge, gP = [np.full((n, w), SENTINEL) for w in (3, 3, 9)]
        lib.run(ctypes.c_int64(n), ctypes.c_int(mode), P(s), P(e), P(P9), P(ru), P(child), P(n_in),
                P(n_out), P(branch), ctypes.c_double(L), P(g[0]), P(g[1]), P(g[2]), P(gs), P(ge),
                P(gP))
        return gs, ge, gP

    has = child != 0
    tir = has & ~mirror & (k < 0.0)
    kind = {
        "no child": ~has,
        "refracted from outside": has & ~mirror & ~tir & ~internal,
        "refracted from inside": has & ~mirror & ~tir & internal,
        "total internal reflection": tir,
        "mirror": has & mirror,
    }
    return kind, [run(m) for m in range(4)]


@pytest.mark.parametrize("name", KINDS)
def test_without_face_terms_the_ray_gradients_keep_their_bits_and_gP_is_untouched(runs, name):
    kind, (full, bare, _, _) = runs
    rows = kind[name]
    print(f"{name}: {int(rows.sum())} records")
    assert rows.sum() > 0, f"no record of kind '{name}'"
    assert np.array_equal(full[0][rows], bare[0][rows], equal_nan=True)      # gs
    assert np.array_equal(full[1][rows], bare[1][rows], equal_nan=True)      # ge
    assert np.all(bare[2][rows] == SENTINEL)                                # gP: never written
    assert np.all(full[2][rows] != SENTINEL)


@pytest.mark.parametrize("name", KINDS)
def test_ratios_handed_over_give_the_bits_of_the_division(runs, name):
    kind, (_, _, divided, picked) = runs      # (both calls are handed the same branches)
    rows = kind[name]
    print(f"{name}: {int(rows.sum())} records")
    assert rows.sum() > 0, f"no record of kind '{name}'"
    for a, b in zip(divided, picked):
        assert np.array_equal(a[rows], b[rows], equal_nan=True)
