"""
The three quotients of the exact test behind ONE reciprocal refinement (trace_math.h quotients3,
used by beam_decide: k_trace_inplace*, k_intersect_beam) against the plain divisions of the
ALL-PAIRS trace (k_intersect3d keeps exact_triangle's `/`), BIT FOR BIT -- counts, ids, rows and
faces of every class (test_gpu_fuzz_inplace._same), the in-place route and both beam routes.

quotients3 shares the refinement where v_div_scale_f64 scales the denominator alike for the three
numerators, and falls back to the plain divisions in a lane where it does not: a numerator that is
zero (the instruction answers NaN) or below 2^-969 in magnitude over a normal denominator (it
scales by 2^128).  A subnormal denominator is scaled alike for the three, whatever the numerators
(which are subnormal too where the quotient is of ordinary size), and stays on the shared path.

float64 ray state, 65 and 127 rays (32-ray bundles: a last wavefront with one ray, with all but
one), 3 passes:

  * the smallest lens that is walked, (k_front, k_back) = (3, 2), 80 faces: ordinary pairs only;
  * a hand-made scene of 66 faces: 64 triangles of an 8 x 4 grid in the plane x = 0 -- axis-aligned,
    through the origin, every coordinate a multiple of 1/4 -- the half y < 0 optical, the half
    y >= 0 a target, and a stop wall of two triangles at x = -5.  Most rays cross the grid head-on
    (ordinary pairs); the first rays are made for one class each:
      subnormal   start and end at x = +-2^-1040: den = 2^-1039 * (g k - f l), subnormal; the ray
                  meets the plane at ray_u = 1/2.  eps_int = 0, or every such pair is invalid;
      zero        along x through a grid vertex (r = t = 0: nu = nv = 0 exactly) and through a
                  grid edge (one of them zero);
      tiny        along x at z = 2^-1000 (nu or nv = a * 2^-1000 for the faces whose corner lies
                  on z = 0) and a start at x = 2^-1000 (nr = q (g k - f l));
      small den   the same scene traced with eps_int = 1e-10: the subnormal rays, and rays with
                  start and end at x = +-1e-12, take the sd = 1 arm.

The classes are found by evaluating the same six-term sums in float64 on the CPU (the expressions
of oracle/geom.py raw_line_triangle_intersect, whose quotients and validity are taken from it), and
every class must be present among pairs that REACH the exact test.  Which pairs reach it is not
an output of a trace, so the test counts what is certain: a pair that the CPU finds to be its ray's
valid nearest hit in pass 1 must have been tested on every route, or the route's result -- checked
here against the CPU's face for that ray -- would be another.  The sd = 1 arm's pairs are invalid by
definition and can never be seen as a hit: there the test counts the pairs that ARE such hits with
eps_int = 0 and have |den| < 1e-10 -- the float32 filter in front of the exact test reads
eps_size and eps_start, never eps_int (tfrt_trace3d.hip beam_pass), so the same pairs come through
it in both traces.  Wavefronts: after the Hilbert order the rays are cut into the in-place
trace's 32-ray wavefronts; at least one must hold only shared-path hit pairs and at least one
hit pairs of both paths.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import geom
from test_gpu_beam_walk_records import _check_routes
from test_gpu_fuzz_inplace import _same
from test_gpu_inplace import _flags, assert_in_place

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PASSES = 3
TINY = 2.0 ** -969      # below it v_div_scale_f64 rescales a numerator
SUB = 2.0 ** -1040
CLASSES = ("ordinary", "subnormal", "zero", "tiny")


def _hand_made(n_rays):
    ys = np.arange(-1.0, 1.0 + 1e-9, 0.25)            # 9 grid lines: 8 cells
    zs = np.arange(-0.5, 0.5 + 1e-9, 0.25)            # 5 grid lines: 4 cells
    tris, cat = [], []
    for iy in range(8):
        for iz in range(4):
            p00, p10 = (0.0, ys[iy], zs[iz]), (0.0, ys[iy + 1], zs[iz])
            p11, p01 = (0.0, ys[iy + 1], zs[iz + 1]), (0.0, ys[iy], zs[iz + 1])
            tris += [p00 + p10 + p11, p00 + p11 + p01]
            cat += [0 if ys[iy] < 0 else 2] * 2
    w = 4.0
    tris += [(-5.0, -w, -w, -5.0, w, -w, -5.0, w, w), (-5.0, -w, -w, -5.0, w, w, -5.0, -w, w)]
    cat += [1, 1]
    P = torch.tensor(tris, dtype=torch.float64)
    M = P.shape[0]
    special = [
        # subnormal denominator (three, over the target half)
        (SUB, 0.30, 0.10, -SUB, 0.41, 0.17), (SUB, 0.55, -0.30, -SUB, 0.66, -0.23),
        (SUB, 0.05, 0.30, -SUB, 0.16, 0.37),
        # numerators exactly zero: through grid vertices, along grid edges
        (1.0, 0.25, 0.25, -1.0, 0.25, 0.25), (1.0, 0.0, 0.0, -1.0, 0.0, 0.0),
        (1.0, 0.5, -0.25, -1.0, 0.5, -0.25), (1.0, 0.25, 0.1, -1.0, 0.25, 0.1),
        (1.0, 0.6, 0.25, -1.0, 0.6, 0.25),
        # tiny numerators, normal denominator
        (1.0, 0.1, 2.0 ** -1000, -1.0, 0.1, 2.0 ** -1000),
        (1.0, 0.6, 2.0 ** -1000, -1.0, 0.6, 2.0 ** -1000),
        (2.0 ** -1000, 0.3, 0.2, -1.0, 0.3, 0.2), (2.0 ** -1000, 0.8, -0.4, -1.0, 0.85, -0.4),
        # a denominator below eps_int = 1e-10 that is not subnormal
        (1e-12, 0.35, -0.10, -1e-12, 0.45, 0.0), (1e-12, 0.70, 0.30, -1e-12, 0.80, 0.40),
    ]
    k = np.arange(n_rays - len(special))
    y = -0.95 + 1.9 * ((k * 0.6180339887498949) % 1.0)
    z = -0.45 + 0.9 * ((k * 0.7548776662466927) % 1.0)
    plain = np.stack([np.ones_like(y), y, z, -np.ones_like(y), y + 0.05, z - 0.03])
    rays = torch.tensor(np.concatenate([np.array(special).T, plain], axis=1), dtype=torch.float64)
    return dict(P=P, cat=torch.tensor(cat), n_in=torch.full((M,), 1.0, dtype=torch.float64),
                n_out=torch.full((M,), 1.5, dtype=torch.float64), rays=rays, L=1.0)


def _cpu_pairs(sc, eps):
    """Pass 1 of every (face, ray) pair on the CPU: the sums, the quotients and the valid mask."""
    r, P = sc["rays"], sc["P"]
    x, y, z, valid, ray_u, trig_u, trig_v = geom.line_triangle_intersect(
        r[0], r[1], r[2], r[3], r[4], r[5], *[P[:, j] for j in range(9)], eps[0])
    s, e = r[:3].T[None], r[3:].T[None]                        # (1, N, 3)
    p0, e1, e2 = P[:, None, 0:3], P[:, None, 3:6] - P[:, None, 0:3], P[:, None, 6:9] - P[:, None, 0:3]
    a, d, h = [(s - e)[..., j] for j in range(3)]
    b, f, k = [e1[..., j] for j in range(3)]
    c, g, l = [e2[..., j] for j in range(3)]
    q, rr, t = [(s - p0)[..., j] for j in range(3)]
    den = a * g * k + b * d * l + c * f * h - a * f * l - b * g * h - c * d * k
    nr = b * l * rr + c * f * t + g * k * q - b * g * t - c * k * rr - f * l * q
    nu = a * g * t + c * h * rr + d * l * q - a * l * rr - c * d * t - g * h * q
    nv = a * k * rr + b * d * t + f * h * q - a * f * t - b * h * rr - d * k * q
    valid = valid & (trig_u >= -eps[1]) & (trig_v >= -eps[1]) & (trig_u + trig_v <= 1.0 + eps[1]) \
        & (ray_u >= eps[2])
    return den, torch.stack([nr, nu, nv]), valid, ray_u


def _nearest(valid, ray_u):
    """Every ray's valid nearest hit of pass 1: the face (lowest index on a tie), or -1."""
    key = torch.where(valid, ray_u, torch.full_like(ray_u, float("inf")))
    best = key.min(dim=0).values
    first = torch.argmax((key == best[None]).int(), dim=0)
    return torch.where(torch.isfinite(best), first, torch.full_like(first, -1))


def _classes(den, num, eps_int):
    """The class of every pair, by value (masks of shape (M, N))."""
    mag = num.abs()
    small = den.abs() < eps_int
    zero = (mag == 0.0).any(dim=0)
    tiny = ((mag > 0.0) & (mag < TINY)).any(dim=0)
    subnormal = (den != 0.0) & (den.abs() < 2.0 ** -1022)
    # (a subnormal denominator under a quotient of ordinary size has subnormal numerators: it is
    # the denominator's class -- the instruction looks at the denominator first)
    out = {"small den": small, "zero": ~small & zero, "subnormal": ~small & subnormal & ~zero,
           "tiny": ~small & tiny & ~zero & ~subnormal}
    out["ordinary"] = ~small & ~zero & ~tiny & ~subnormal
    return out


@functools.lru_cache(maxsize=None)
def _traced(n_rays, eps_int):
    from tensorflowraytrace_amd import ops
    sc0 = _hand_made(n_rays)
    fv = sc0["P"].to(DEV)
    cat = sc0["cat"].int().to(DEV)
    base = dict(n_in=sc0["n_in"].to(DEV), n_out=sc0["n_out"].to(DEV))
    r = sc0["rays"].to(DEV).contiguous()
    eps = (eps_int, 1e-10, 0.0)
    kw = dict(max_passes=PASSES, flags=_flags(), new_ray_length=sc0["L"])
    plain = ops.Scene3DArgs(fv, cat, **base)
    plain.eps = eps
    ref = ops.trace3d(r, fv, plain, **kw)
    return sc0, fv, cat, base, r, eps, kw, ref


@pytest.mark.parametrize("n_rays", [65, 127])
def test_lens_routes_equal_the_all_pairs_trace(n_rays):
    _check_routes(n_rays, 3, 2, torch.float64)


@pytest.mark.parametrize("eps_int", [0.0, 1e-10])
@pytest.mark.parametrize("n_rays", [65, 127])
def test_hand_made_scene_routes_equal_the_all_pairs_trace(n_rays, eps_int):
    from tensorflowraytrace_amd import ops
    sc0, fv, cat, base, r, eps, kw, ref = _traced(n_rays, eps_int)
    assert fv.shape[0] >= 64
    assert int(ref["counts"][:, :3].sum()) > 0
    order = ops.ray_order(r)
    for route in ("beam64", "beam32", "inplace"):
        args = ops.Scene3DArgs(fv, cat, cluster_order=ops.cluster_order(fv), coherent_rays=True, **base)
        args.eps = eps
        args.coherent_only = route != "beam64"
        args.in_place = route == "inplace"
        if args.in_place:
            assert_in_place(args, fv, n_rays, PASSES)
        out = ops.trace3d(r[:, order.long()].contiguous(), fv, args, **kw)
        _same(ops.restore_order(out, order), ref, (route, n_rays, eps_int))


@pytest.mark.parametrize("n_rays", [65, 127])
def test_every_pair_class_reaches_the_exact_test(n_rays):
    from tensorflowraytrace_amd import ops
    sc0, fv, cat, base, r, eps, kw, ref = _traced(n_rays, 0.0)
    den, num, valid, ray_u = _cpu_pairs(sc0, eps)
    hit = _nearest(valid, ray_u)                               # (N,)
    rays = torch.arange(n_rays)
    on = hit >= 0
    # the GPU's pass 1 is the CPU's: rays the CPU sees finish in pass 1 are the first finished
    # rays, with the CPU's faces (so the CPU's hit pairs were tested on the GPU)
    target = on & (sc0["cat"][hit.clamp(min=0)] == 2)
    n_fin1 = int(ref["counts"][0, 1])
    assert n_fin1 == int(target.sum())
    assert torch.equal(ref["finished_id"][:n_fin1].cpu().long(), rays[target])
    assert torch.equal(ref["finished_face"][:n_fin1].cpu().long(), hit[target])
    cls = _classes(den, num, 0.0)
    hits = {c: int(m[hit[on], rays[on]].sum()) for c, m in cls.items()}
    for c in CLASSES:
        assert hits[c] >= 1, (c, hits)
    # the sd = 1 arm: pairs that are hits with eps_int = 0 and invalid with eps_int = 1e-10
    small = (den.abs() < 1e-10)[hit[on], rays[on]]
    assert int(small.sum()) >= 1
    sub_small = ((den != 0.0) & (den.abs() < 2.0 ** -1022))[hit[on], rays[on]]
    assert int((small & ~sub_small).sum()) >= 1                # ... one of them not subnormal
    _, _, valid10, ray_u10 = _cpu_pairs(sc0, (1e-10, eps[1], eps[2]))
    assert not bool(valid10[hit[on], rays[on]][small].any())
    # wavefronts of the in-place trace: 32 rays of the Hilbert order each
    order = ops.ray_order(r).cpu().long()
    # which arm a lane takes: quotients3 falls back where the three denominator-side scalings
    # DIFFER, not wherever a numerator is zero or tiny -- three zero numerators (NaN thrice) or
    # three tiny ones (2^128 thrice) agree and share.  Per numerator the scaling is told by value:
    # 0 = unscaled, 1 = NaN (zero numerator), 2 = 2^128 (subnormal denominator, looked at before
    # the numerator; else a tiny numerator).  The instruction's remaining cases (exponents 768
    # apart, a reciprocal or quotient that would be subnormal) need magnitudes this scene has not.
    mag = num.abs()
    sub = ((den != 0.0) & (den.abs() < 2.0 ** -1022))[None].expand_as(mag)
    code = torch.where(mag == 0.0, 1, torch.where(sub | (mag < TINY), 2, 0))
    fallback = (code[0] != code[1]) | (code[0] != code[2])
    assert bool((fallback <= (cls["zero"] | cls["tiny"] | cls["subnormal"])).all())
    only_shared = mixed = 0
    for w0 in range(0, n_rays, 32):
        members = order[w0:w0 + 32]
        members = members[on[members]]
        if members.numel() == 0:
            continue
        fb = fallback[hit[members], members]
        only_shared += int(not bool(fb.any()))
        mixed += int(bool(fb.any()) and not bool(fb.all()))
    assert only_shared >= 1 and mixed >= 1, (only_shared, mixed)
