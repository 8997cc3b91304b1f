"""
Every route of the 3-D reverse sweep that is not the in-place one (trace3d_backward_t in
csrc/tfrt_trace3d.hip, reached through ops.trace3d / _Trace3D.backward) with every seed and both
outputs, against torch.autograd through the float64 oracle -- never against another HIP route.

  route  taken when                                                     kernels
  A      natural order, N < 16384 (or more than 32 face windows)        k_backward3d, float64 atomics
  B      natural order, N >= 16384, M <= 32 x FACE_WINDOW               k_backward3d -> k_face_accumulate
  C      Scene3DArgs(deterministic=True)                                k_backward3d -> k_stash_absmax,
                                                                        k_face_accumulate_fixed, k_fixed_finish
  D      coherent_rays, not in place, P > CHAIN_MAXP                    k_backward3d(wave_sums = 1)
  E      coherent_rays, not in place, 1 <= P <= CHAIN_MAXP              k_backward_chain, tape mode 0

(the in-place route, F, is tests/test_gpu_inplace_oracle.py's.)  One scalar over all four ray
classes in which every row of every class carries a gradient (test_gpu_inplace_oracle._error) is
evaluated on the ops.trace3d outputs and on the oracle's trace of the same scene.  Before any
gradient is compared the case asserts its route (the profile records of the sweep and the restated
predicate, see _route_of), then that the two traces hold the same rays in the same classes and
order, the same coordinates and the same error.  Then d error / d face vertices (M x 9) and
d error / d source rays (6 x N) are compared with test_reference_golden._check_grad: identical
non-finite entries, finite ones to 1e-8 (float64 state) or 1e-5 (float32 state) of the largest
finite reference entry; float64 state also holds the source gradient row by row.

Routes D and E hand the rays over in ops.ray_order order with perm=, so the class seeds also travel
through the restored-order path of _Trace3D.backward.

What the cases reach that no other test does:
  1  all four classes seeded, dead rays with and without dead_ray_length, the source gradient and
     both state types on each of A, B, C, D, E; 16383 rays (A) beside 16384 (B);
  2  the ordered sweep at 1, 2 and 3 passes (both parities of its two-entry scale buffer; the
     single pass whose only k_fixed_finish clears a slot nobody reads); the chain at one pass;
  3  one class seeded at a time on A, C, E (the other three arrive as null seed pointers), and
     the start rows of the active history alone;
  4  the fixture soups (coplanar ties, mirrors, stops) on A without a hierarchy, C and E;
  5  ray counts around a wavefront (A, D, E) and around a block of the ordered kernels (C); below
     64 rays a trace with coherent_rays set has no coherent forward and no in-place route, its
     sweep still sums per wavefront;
  6  the ordered sweep's bits from run to run with every class seeded;
  7  index mode (materials and a table column per ray, every ray its own wavelength) on A, C, D
     and E: the lens, gradients with respect to the lens parameters and the source rays.
"""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import oracle_util
import scene_util
import test_gpu_inplace_oracle as _io
from oracle import tracer
from test_gpu_inplace_oracle import CLASSES, NAMES, _light_guide, _oracle_blocks, _oracle_soup
from test_reference_golden import SOUP, _check_grad, _soup_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# What the sweep's plan reads (csrc/tfrt_trace3d.hip, csrc/tfrt_common.h), restated;
# constants_in_the_sources() reads them back and the CPU test beside this module holds them equal.
BLOCK = 256                 # k_stash_absmax / k_face_accumulate_fixed / k_fixed_finish blocks
FACE_WINDOW = 2048          # faces per LDS window of k_face_accumulate
CHAIN_MAXP = 8              # passes k_backward_chain holds without an in-place tape
STASH_MIN_RAYS = 16384      # natural order: rays from which the stash replaces the atomics
COHERENT_MIN_RAYS = 64      # rays below which the forward has no coherent (or in-place) route
PROF_BACKWARD, PROF_ACCUMULATE = 2, 3       # include/tfrt_hip.h TFRT_PROF_*
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "tensorflowraytrace_amd", "csrc")
# profile records (TFRT_PROF_BACKWARD, TFRT_PROF_ACCUMULATE) of one sweep of P passes.  A, C and D
# leave the same counts: what tells them apart is the scene's own switch (deterministic,
# coherent_rays), which the case sets and _route_of restates.
RECORDS = {"A": lambda P: (P, 0), "B": lambda P: (P, 1), "C": lambda P: (P, 0),
           "D": lambda P: (P, 0), "E": lambda P: (1, 0)}


def constants_in_the_sources():
    """The constants above as csrc/ defines them, provided the plan uses them as _route_of says."""
    with open(os.path.join(CSRC, "tfrt_trace3d.hip")) as f:
        text = f.read()
    with open(os.path.join(CSRC, "tfrt_common.h")) as f:
        common = f.read()
    plan = text[text.index("static int trace3d_backward_t("):]
    plan = plan[:plan.index("}  // namespace tfrt")]
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    plan = squeeze(plan)
    stash = re.search(r"const bool stash = ordered \|\| \(!wave_sums && M > 0 && N >= (\d+) && "
                      r"windows <= 32\);", plan)
    assert stash, "the stash predicate changed"
    assert "const bool ordered = sc->deterministic != 0 && M > 0 && c.g_fverts != nullptr;" in plan
    assert ("const bool wave_sums = !ordered && sc->coherent_rays != 0 && M > 0 && "
            "c.g_fverts != nullptr;") in plan
    assert "const int windows = cdiv(M > 0 ? M : 1, FACE_WINDOW);" in plan
    assert "const bool chain = wave_sums && P >= 1 && (P <= CHAIN_MAXP || inplace);" in plan
    for kernel in ("k_stash_absmax<G>", "k_face_accumulate_fixed<G>"):
        assert f"hipLaunchKernelGGL(({kernel}), dim3(pl.nblk), dim3(BLOCK)," in plan, kernel
    assert "hipLaunchKernelGGL(k_fixed_finish, dim3(cdiv((int64_t)M * 9, BLOCK)), dim3(BLOCK)," \
        in plan
    coherent = re.search(r"const bool coherent = sc->coherent_rays != 0 && ac\.order != nullptr && "
                         r"N >= (\d+);", squeeze(text))
    in_place = re.search(r"has_hierarchy\(sc, M\) && N >= (\d+) && P >= 1;", squeeze(text))
    assert coherent and in_place and coherent.group(1) == in_place.group(1)
    grab = lambda name, s: int(re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", s).group(1))
    return dict(BLOCK=grab("BLOCK", common), FACE_WINDOW=grab("FACE_WINDOW", text),
                CHAIN_MAXP=grab("CHAIN_MAXP", text), STASH_MIN_RAYS=int(stash.group(1)),
                COHERENT_MIN_RAYS=int(coherent.group(1)))


def _route_of(n_rays, n_faces, passes, deterministic, coherent):
    """trace3d_backward_t's choice for a trace that is not in place, with faces and a face
    gradient asked for."""
    if deterministic:
        return "C"
    if coherent:
        return "E" if 1 <= passes <= CHAIN_MAXP else "D"
    windows = -(-max(n_faces, 1) // FACE_WINDOW)
    return "B" if n_rays >= STASH_MIN_RAYS and windows <= 32 else "A"


# ------------------------------------------------------------------------------------ the scalar

def _error_columns(b, k):
    """Class k's part of test_gpu_inplace_oracle._error, ray by ray (b: its (6, n) block)."""
    w = torch.arange(1, 7, dtype=torch.float64, device=b.device)[:, None] * (0.3 + k)
    return 1e-2 * (w * b * b).sum(0) + (b[3:] * b[:3]).sum(0)


def _error(blocks, mode="all"):
    """test_gpu_inplace_oracle._error of the classes' (6, n) float64 blocks.  "all": every class,
    every row; a class name: that class alone (the others take no seed at all); "active_start":
    only rows 0-2 (the start points) of the active history."""
    if mode == "all":
        return _io._error(blocks)
    if mode == "active_start":
        b = blocks.get("active")
        if b is None or b.shape[1] == 0:
            return 0.0
        k = CLASSES.index("active")
        w = torch.arange(1, 4, dtype=torch.float64, device=b.device)[:, None] * (0.3 + k)
        return 1e-2 * (w * b[:3] * b[:3]).sum() + (b[0] * b[1]).sum() + (b[1] * b[2]).sum()
    assert mode in CLASSES, mode
    return _io._error({mode: blocks.get(mode)})


def _flags():
    return _io._flags()


# ------------------------------------------------------------------------ scenes and references

GUIDE = ("guide", 700, 3)            # 100 faces, one face window; seed 3 as counted for the cases
GUIDE_STASH = ("guide", 16384, 3)
GUIDE_DEEP = ("guide", 3000, 3)
SOUP_SEEDS = (2, 16, 25)


@functools.lru_cache(maxsize=None)
def _scene_for(key):
    """(face vertices (M, 9), category, n_in, n_out, rays (6, N), new_ray_length, the fixture's pass
    count and dead_ray_length or None) of ("guide", n_rays, seed) / ("soup", seed)."""
    if key[0] == "guide":
        return _light_guide(key[1], seed=key[2]) + (1.0, None, None)
    g = np.load(SOUP)
    sc = _soup_case(g, key[1])
    return (sc["P"], sc["cat"], sc["n_in"], sc["n_out"], sc["rays"], sc["L"], int(g["passes"]),
            sc["dead"])


def _source(rays, n_rays, f32):
    """The first n_rays source rays as the device reads them: rounded to float32 when the ray state
    is float32."""
    rays = rays[:, :n_rays]
    return rays.float().double() if f32 else rays.clone()


@functools.lru_cache(maxsize=None)
def _reference(key, n_rays, f32, passes, dead_len, mode):
    """The oracle's trace of the first n_rays rays of _scene_for(key) and the gradients of
    _error(mode) with respect to the face vertices and the six source rows.  Computed once per
    case and shared; nobody writes to it."""
    P0, cat, n_in, n_out, rays0, L, _, _ = _scene_for(key)
    P = P0.clone().requires_grad_(True)
    rays = _source(rays0, n_rays, f32).requires_grad_(True)
    ref = _oracle_soup(P, cat, n_in, n_out, rays, passes, L, dead_len)
    blocks = _oracle_blocks(ref)
    loss = _error(blocks, mode)
    if isinstance(loss, torch.Tensor) and loss.requires_grad:
        g_fv, g_src = torch.autograd.grad(loss, [P, rays], allow_unused=True)
    else:
        g_fv = g_src = None
    g_fv = torch.zeros_like(P) if g_fv is None else g_fv
    g_src = torch.zeros_like(rays) if g_src is None else g_src
    sets = {c: {k: v.detach() for k, v in ref[c].items()} if c in blocks else {} for c in CLASSES}
    return types.SimpleNamespace(
        sets=sets, counts={c: (blocks[c].shape[1] if c in blocks else 0) for c in CLASSES},
        loss=float(loss.detach()) if isinstance(loss, torch.Tensor) else float(loss),
        g_fv=g_fv, g_src=g_src)


def _rel(got, want):
    """Largest error over the entries finite on both sides / largest finite reference entry."""
    g, w = got.detach().double().cpu(), want.double()
    fin = torch.isfinite(w)
    both = fin & torch.isfinite(g)
    if not both.any() or float(w[fin].abs().max()) == 0.0:
        return 0.0
    return float((g[both] - w[both]).abs().max() / w[fin].abs().max())


def _close(got, want, tol, tag, what):
    """_check_grad; where the reference has no finite non-zero entry at all (its scale is 0) the
    device must give exact zeros in the same places.  Returns the relative error it printed."""
    w = want.double()
    g = got.detach().double().cpu()
    fin = torch.isfinite(w)
    if fin.any() and float(w[fin].abs().max()) > 0.0:
        rel = _rel(g, w)
        print(f"{tag} {what}: rel err {rel:.2e}")
        _check_grad(g.numpy(), w.numpy(), tag, what, tol)
        return rel
    assert torch.equal(~torch.isfinite(g), ~fin), f"{tag} {what}: non-finite pattern differs"
    assert not fin.any() or float(g[fin].abs().max()) == 0.0, f"{tag} {what}: the reference is zero"
    print(f"{tag} {what}: zero on both sides")
    return 0.0


def _profiled_grad(loss, leaves):
    """torch.autograd.grad(loss, leaves) and the number of TFRT_PROF_BACKWARD and
    TFRT_PROF_ACCUMULATE records its reverse sweep left."""
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    L.tfrt_profile_enable(1)
    try:
        grads = torch.autograd.grad(loss, leaves)
        records = (L.tfrt_profile_read_kind(PROF_BACKWARD, buf, 64),
                   L.tfrt_profile_read_kind(PROF_ACCUMULATE, buf, 64))
    finally:
        L.tfrt_profile_enable(0)
    return grads, records


def _sweep(route, key, dtype, passes=None, dead_len=None, mode="all", n_rays=None, hierarchy=True,
           tag=None):
    """ops.trace3d of the scene, set up for `route`, with all four classes compiled, and the
    gradients of _error(mode) with respect to (face vertices, source rays) checked against
    _reference.  Returns the device's gradients, the reference and the measured errors.

    Bars: 1e-9 / 1e-5 for the rays (test_forward_lens), 1e-8 / 1e-5 for the gradients
    (test_backward_lens, test_gpu_inplace_oracle), float64 / float32 state."""
    from tensorflowraytrace_amd import _lib, ops
    f32 = dtype == torch.float32
    set_tol, tol = (1e-5, 1e-5) if f32 else (1e-9, 1e-8)
    P0, cat, n_in, n_out, rays0, L, fixture_passes, _ = _scene_for(key)
    passes = fixture_passes if passes is None else passes
    n_rays = rays0.shape[1] if n_rays is None else n_rays
    M = P0.shape[0]
    tag = tag or f"{route} {key[0]}{key[1]} N={n_rays} P={passes} {'f32' if f32 else 'f64'} " \
                 f"dead={dead_len} {mode}"
    ref = _reference(key, n_rays, f32, passes, dead_len, mode)

    coherent, ordered = route in "DE", route == "C"
    fv = P0.to(DEV).requires_grad_(True)
    src = rays0[:, :n_rays].to(DEV, dtype).requires_grad_(True)
    args = ops.Scene3DArgs(fv.detach(), cat.int().to(DEV), n_in=n_in.to(DEV), n_out=n_out.to(DEV),
                           cluster_order=ops.cluster_order(fv.detach()) if hierarchy else None,
                           deterministic=ordered, coherent_rays=coherent)
    assert _route_of(n_rays, M, passes, ordered, coherent) == route, tag
    assert _lib.lib().tfrt_trace3d_in_place(ctypes.byref(args.struct(fv.detach())), n_rays,
                                            passes) == 0, tag
    kw = dict(max_passes=passes, flags=_flags(), new_ray_length=L, dead_ray_length=dead_len)
    if coherent:
        order = ops.ray_order(src.detach())
        out = ops.trace3d(src[:, order.long()].contiguous(), fv, args, perm=order, **kw)
    else:
        out = ops.trace3d(src, fv, args, **kw)
    loss = _error({c: out[c].double() for c in CLASSES}, mode)
    seeded = isinstance(loss, torch.Tensor) and loss.requires_grad
    if seeded:
        (g_fv, g_src), records = _profiled_grad(loss, [fv, src])
        print(f"{tag}: route {route}, records {records}")
        assert records == RECORDS[route](passes), (tag, records)
    else:           # (no row of the seeded class exists: nothing to sweep)
        assert ref.loss == 0.0 and float(ref.g_fv.abs().max()) == 0.0, tag
        g_fv, g_src = torch.zeros_like(fv), torch.zeros_like(src)
        print(f"{tag}: route {route}, the seeded class is empty")

    _io._same_sets(out, ref.sets, set_tol, tag)
    print(f"{tag}: error {float(loss):.17g} oracle {ref.loss:.17g}")
    assert abs(float(loss) - ref.loss) <= 10 * tol * abs(ref.loss), tag
    assert g_src.dtype == dtype and g_src.shape == src.shape and g_fv.shape == (M, 9)
    rel = dict(face=_close(g_fv, ref.g_fv, tol, tag, "face vertices"),
               source=_close(g_src, ref.g_src, tol, tag, "source rays"))
    if not f32:
        # row by row: the start rows' own scale, not the larger one of the end rows
        for r, name in enumerate(NAMES):
            _close(g_src[r], ref.g_src[r], tol, tag, f"source {name}")
    return types.SimpleNamespace(g_fv=g_fv, g_src=g_src, ref=ref, out=out, rel=rel)


def _bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def _every_class_and_every_source_ray(r):
    assert all(r.ref.counts[c] > 0 for c in CLASSES), r.ref.counts
    assert bool(torch.isfinite(r.ref.g_fv).all()) and bool(torch.isfinite(r.ref.g_src).all())
    assert bool((r.ref.g_src != 0).any(0).all())
    assert bool((r.g_src != 0).any(0).all()), "a source ray took no gradient"


# Float32 state: no output of this module needed a bar of its own.  Measured on an MI355X (largest
# error over an output / largest finite reference entry, kernel and oracle reading the same
# float32-rounded source), worst case per route, face vertices / source rays:
#
#   route   float64 state          float32 state
#   A       6.2e-13 / 6.8e-13      2.0e-6 / 9.0e-6   (16383 rays; 700 rays: 1.0e-6 / 8.6e-7)
#   B       7.5e-14 / 6.8e-13      2.0e-6 / 9.0e-6
#   C       6.4e-12 / 6.1e-13      9.8e-7 / 8.6e-7
#   D       1.7e-13 / 2.2e-12      3.0e-7 / 3.7e-6
#   E       6.2e-13 / 6.1e-13      4.1e-7 / 3.6e-6
#
# (the ordered sweep's face sums carry their 2^-40 fixed-point grain: 6e-12.)  The float32 figures
# are the ray state's rounding of every pass's hit and child points -- the sweep itself works in
# float64 either way -- and are the same with and without dead_ray_length.

# ------------------------------------------------------------------- 1. all classes, all outputs

ROUTE_CASES = [("A", GUIDE, 700, 4), ("B", GUIDE_STASH, 16384, 3), ("A", GUIDE_STASH, 16383, 3),
               ("C", GUIDE, 700, 4), ("D", GUIDE_DEEP, 3000, 9), ("E", GUIDE_DEEP, 3000, 8)]


@pytest.mark.parametrize("dead_len", [None, 0.25])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("route,key,n_rays,passes", ROUTE_CASES,
                         ids=[f"{r}-{n}x{p}" for r, _, n, p in ROUTE_CASES])
def test_every_class_seeded_every_gradient_against_oracle_autograd(route, key, n_rays, passes,
                                                                   dtype, dead_len):
    """Every row of every class seeded; face-vertex and source gradients on each route.  Class
    counts (finished / active / stopped / dead): 700 rays, 4 passes 35 / 2275 / 83 / 78; 16384
    rays, 3 passes 502 / 40609 / 2048 / 2124 (16383 rays stay on the atomics: route A); 3000 rays,
    8 and 9 passes.  Every gradient entry is finite and every source ray takes one."""
    r = _sweep(route, key, dtype, passes, dead_len, n_rays=n_rays)
    _every_class_and_every_source_ray(r)


# ------------------------------------------------------------------------- 2. pass-count edges

@pytest.mark.parametrize("passes", [1, 2, 3])
def test_pass_count_edges_of_the_ordered_sweep(passes):
    """Route C at 1, 2 and 3 passes: pass p scales by fix_max[(P-1-p) & 1] and its k_fixed_finish
    clears the other entry -- both parities, and the single pass whose only finish clears an entry
    nobody reads.  (One pass: 2 / 698 / 0 / 0, the stopped and dead classes seeded and empty;
    two and three passes hold rays of every class.)"""
    r = _sweep("C", GUIDE, torch.float64, passes, 0.25)
    assert r.ref.counts["active"] > 0 and r.ref.counts["finished"] > 0
    assert (passes == 1) == (r.ref.counts["stopped"] == 0) == (r.ref.counts["dead"] == 0)
    assert bool((r.g_src != 0).any(0).all())


def test_one_pass_chain_is_the_source_slot_alone():
    """Route E at one pass: a ray's chain of slots is its source slot (2 / 698 / 0 / 0)."""
    r = _sweep("E", GUIDE, torch.float64, 1, 0.25)
    assert r.ref.counts["active"] > 0 and r.ref.counts["finished"] > 0
    assert bool((r.g_src != 0).any(0).all())


# ----------------------------------------------------------------- 3. one class seeded at a time

@pytest.mark.parametrize("mode", ["finished", "active", "stopped", "dead", "active_start"])
@pytest.mark.parametrize("route", ["A", "C", "E"])
def test_one_class_seeded_the_others_take_none(route, mode):
    """The error reads one class only: the other three, present in the trace and holding rays,
    arrive in backward() as None (null seed pointers in the sweep).  "active_start": only the
    start rows of the active history, the seed of links that also have a child."""
    r = _sweep(route, GUIDE, torch.float64, 4, 0.25, mode=mode)
    assert all(r.ref.counts[c] > 0 for c in CLASSES), r.ref.counts
    # the seed reaches exactly the source rays that have a row in the seeded class
    rows = r.ref.sets["active" if mode == "active_start" else mode]["ray_id"]
    cols = int((r.g_src != 0).any(0).sum())
    assert cols == len(set(rows.tolist())), (mode, cols)
    assert float(r.ref.g_fv.abs().max()) > 0.0


# -------------------------------------------------------------------------------- 4. fixture soups

@pytest.mark.parametrize("seed", SOUP_SEEDS)
@pytest.mark.parametrize("route", ["A", "C", "E"])
def test_fixture_soups_against_oracle_autograd(route, seed):
    """tests/golden/reference_soup3d.npz at the fixture's pass count, new_ray_length and
    dead_ray_length: coplanar ties, mirrors, total internal reflection, stops.  Route A without a
    hierarchy (all-pairs intersect), C and E with one."""
    key = ("soup", seed)
    r = _sweep(route, key, torch.float64, None, _scene_for(key)[7], hierarchy=route != "A")
    assert sum(n > 0 for n in r.ref.counts.values()) >= 3, r.ref.counts


# ------------------------------------------------------------------------------ 5. ray-count edges

@pytest.mark.parametrize("route,n_rays", (
    [("A", n) for n in (1, 63, 64, 65)] + [("C", n) for n in (1, BLOCK - 1, BLOCK, BLOCK + 1)]
    + [(r, n) for r in "DE" for n in (64, 65, 129)]))
def test_ray_counts_at_the_edges(route, n_rays):
    """The first n rays of the 700-ray light guide, 4 passes (9 for route D): one ray, a wavefront
    and a block of the ordered kernels, each minus and plus one; the coherent sweeps with one full
    wavefront, one ray more, and two and one ray."""
    r = _sweep(route, GUIDE, torch.float64, 9 if route == "D" else 4, 0.25, n_rays=n_rays)
    assert sum(r.ref.counts.values()) >= n_rays


@pytest.mark.parametrize("route", ["D", "E"])
def test_below_a_wavefront_of_rays_there_is_no_coherent_trace(route):
    """63 rays with coherent_rays set: the forward's coherent route and the in-place route both
    need COHERENT_MIN_RAYS = 64 rays (constants_in_the_sources() holds that to the text of the
    plan; asked to go in place, the trace does at 64 rays and does not at 63).  The reverse
    sweep's choice does not read the ray count: it still sums per wavefront, over the tape the
    grouped forward wrote, and is held to the oracle like every other case."""
    from tensorflowraytrace_amd import _lib, ops
    n = COHERENT_MIN_RAYS - 1
    P0, cat, n_in, n_out, _, _, _, _ = _scene_for(GUIDE)
    fv = P0.to(DEV)
    args = ops.Scene3DArgs(fv, cat.int().to(DEV), n_in=n_in.to(DEV), n_out=n_out.to(DEV),
                           cluster_order=ops.cluster_order(fv), coherent_rays=True)
    args.coherent_only = args.in_place = True
    passes = 9 if route == "D" else 4
    query = lambda n_rays: _lib.lib().tfrt_trace3d_in_place(ctypes.byref(args.struct(fv)), n_rays,
                                                            passes)
    assert query(n) == 0 and query(n + 1) == 1
    _sweep(route, GUIDE, torch.float64, passes, 0.25, n_rays=n)


# --------------------------------------------------------------------------------- 6. ordered sums

def test_ordered_sweep_repeats_itself_bit_for_bit():
    """Case 1's route C, float64 state, three times: face and source gradients bit-equal."""
    runs = [_sweep("C", GUIDE, torch.float64, 4, 0.25) for _ in range(3)]
    for other in runs[1:]:
        assert _bits(other.g_fv) == _bits(runs[0].g_fv)
        assert _bits(other.g_src) == _bits(runs[0].g_src)


# ------------------------------------------------------------------------ 7. index mode, the lens

@functools.lru_cache(maxsize=None)
def _lens():
    """2,000 rays through the lens (248 faces), every ray with a wavelength of its own: the
    refractive indices come from a table column per ray."""
    scene = dict(scene_util.lens_scene(2000, k_front=5, k_back=4))
    scene["wavelength"] = np.random.default_rng(9).uniform(450.0, 650.0, 2000)
    return scene


@functools.lru_cache(maxsize=None)
def _lens_reference(passes, dead_len):
    scene = _lens()
    system, (q_f, q_b), _ = oracle_util.lens_oracle(scene)
    osrc = oracle_util.source_dict(scene["rays"], scene["wavelength"])
    leaves = [osrc[n].requires_grad_(True) for n in NAMES]
    ref = tracer.ray_trace(system, osrc, max_iterations=passes, inherit=("wavelength", "ray_id"),
                           flags=dict(compile_dead_rays=True, compile_stopped_rays=True,
                                      dead_ray_length=dead_len))
    blocks = _oracle_blocks(ref)
    loss = _error(blocks)
    r_f, r_b, *r_src = torch.autograd.grad(loss, [q_f, q_b] + leaves)
    sets = {c: {k: v.detach() for k, v in ref[c].items()} if c in blocks else {} for c in CLASSES}
    return types.SimpleNamespace(sets=sets, loss=float(loss.detach()), g_f=r_f, g_b=r_b,
                                 g_src=torch.stack(r_src),
                                 counts={c: (blocks[c].shape[1] if c in blocks else 0)
                                         for c in CLASSES})


@pytest.mark.parametrize("route", ["A", "C", "D", "E"])
def test_index_mode_lens_against_oracle_autograd(route):
    """The routes' reading of the indices through the ray's own table column -- in the coherent
    routes the column of the permuted table -- checked on d error / d (front and back lens
    parameters, source rays), 4 passes (9 for route D), float64 state.  The lens has no stop and
    every ray reaches the target (2000 / 3504 / 0 / 0: the stopped and dead classes are seeded
    and empty); route D sweeps nine passes of which the last six hold no ray."""
    from tensorflowraytrace_amd import _lib, ops
    from test_gpu_trace3d import _gpu_scene
    passes, tol = (9 if route == "D" else 4), 1e-8
    scene = _lens()
    ref = _lens_reference(passes, 0.25)
    assert ref.counts["finished"] == 2000 and ref.counts["active"] > 3000
    coherent, ordered = route in "DE", route == "C"
    src0, fv, sc, (p_f, p_b) = _gpu_scene(scene, torch.float64, cluster="group")
    src = src0.detach().clone().requires_grad_(True)
    order = ops.ray_order(src.detach()) if coherent else None
    table = sc.n_table[:, order.long()].contiguous() if coherent else sc.n_table
    args = ops.Scene3DArgs(fv.detach(), sc.catagory, mat_in=sc.mat_in, mat_out=sc.mat_out,
                           n_table=table, face_grad_mask=sc.face_grad_mask,
                           cluster_order=sc.cluster_order, deterministic=ordered,
                           coherent_rays=coherent)
    n, M = src.shape[1], fv.shape[0]
    tag = f"{route} lens N={n} P={passes} f64 dead=0.25 all"
    assert _route_of(n, M, passes, ordered, coherent) == route
    assert _lib.lib().tfrt_trace3d_in_place(ctypes.byref(args.struct(fv.detach())), n, passes) == 0
    kw = dict(max_passes=passes, flags=_flags(), dead_ray_length=0.25)
    if coherent:
        out = ops.trace3d(src[:, order.long()].contiguous(), fv, args, perm=order, **kw)
    else:
        out = ops.trace3d(src, fv, args, **kw)
    loss = _error({c: out[c].double() for c in CLASSES})
    (g_f, g_b, g_src), records = _profiled_grad(loss, [p_f, p_b, src])
    print(f"{tag}: route {route}, records {records}")
    assert records == RECORDS[route](passes), (tag, records)
    _io._same_sets(out, ref.sets, 1e-9, tag)
    print(f"{tag}: error {float(loss):.17g} oracle {ref.loss:.17g}")
    assert abs(float(loss) - ref.loss) <= 10 * tol * abs(ref.loss), tag
    _close(g_f, ref.g_f, tol, tag, "front parameters")
    _close(g_b, ref.g_b, tol, tag, "back parameters")
    _close(g_src, ref.g_src, tol, tag, "source rays")
    for r, name in enumerate(NAMES):
        _close(g_src[r], ref.g_src[r], tol, tag, f"source {name}")
    assert bool((g_src != 0).any(0).all())
