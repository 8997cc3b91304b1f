"""
The 2-D reverse sweep (k_backward2d, driven by trace2d_backward_t, reached through ops.trace2d /
_Trace2D.backward) with every seed and every output, against torch.autograd through the float64
oracle -- not against another HIP path.

One scalar over all four ray classes (finished, active, stopped, dead) in which every row of every
class carries a gradient (_error, the 2-D cut of test_gpu_inplace_oracle._error) is evaluated on
the ops.trace2d outputs and on the oracle's trace of the same scene.  Before any gradient is
compared the two traces must hold the same rays in the same classes and order, the same
coordinates and the same error.  Then d error / d (segments, arcs, source rays) are compared with
test_gpu_trace2d._same_grad: identical non-finite entries, finite ones to test_backward_2d's bars.

What the cases reach that no other test does: the source gradient (pass 0 writing straight into
it with the source's own stride, its cast to a float32 source, the NaN a totally reflected link
hands to its source ray), the dead class with and without dead_ray_length, stopped and start-row
seeds on the geometry outputs, classes that are present but take no seed (null seed pointers),
max_passes = 1 (no child buffer), ray counts around the sweep's block size, scenes of one
primitive kind, empty but seeded classes, and all of that on the ordered (deterministic) sweep.
"""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import tracer
from test_gpu_trace2d import _gpu_scene, _oracle_system, _same_grad, _scene, _src2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("x_start", "y_start", "x_end", "y_end")
CLASSES = ("finished", "active", "stopped", "dead")
SEG_GEO = ("x_start", "y_start", "x_end", "y_end")
ARC_GEO = ("x_center", "y_center", "angle_start", "angle_end", "radius")
# The sweep's block size: k_backward2d is launched with __launch_bounds__(BLOCK) over
# cdiv(n, BLOCK) blocks, BLOCK = 256 (csrc/tfrt_common.h; block_size_in_the_sources() reads it
# back, and the CPU test beside this module holds the two equal).
BLOCK = 256
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "tensorflowraytrace_amd", "csrc")


def block_size_in_the_sources():
    """BLOCK as csrc/ defines it, provided k_backward2d is launched with it."""
    with open(os.path.join(CSRC, "tfrt_trace2d.hip")) as f:
        sweep = f.read()
    assert re.search(r"__launch_bounds__\(BLOCK\)\s+void\s+k_backward2d\(", sweep)
    with open(os.path.join(CSRC, "tfrt_common.h")) as f:
        return int(re.search(r"constexpr\s+int\s+BLOCK\s*=\s*(\d+)\s*;", f.read()).group(1))


def _error_columns(b, k):
    """Class k's part of the error, ray by ray (b: its (4, n) float64 block)."""
    w = torch.arange(1, 5, dtype=torch.float64, device=b.device)[:, None] * (0.3 + k)
    return 1e-2 * (w * b * b).sum(0) + (b[2:] * b[:2]).sum(0)


def _error(blocks, mode="all"):
    """The scalar of the classes' (4, n) float64 blocks.  "all": every class, every row; a class
    name: that class alone (the others take no seed at all); "active_start": only rows 0 and 1
    (the start points) of the active rays."""
    tot = 0.0
    for k, cls in enumerate(CLASSES):
        b = blocks.get(cls)
        if b is None:
            continue
        if mode == "active_start":
            if cls == "active":
                w = torch.arange(1, 3, dtype=torch.float64, device=b.device)[:, None] * (0.3 + k)
                tot = tot + 1e-2 * (w * b[:2] * b[:2]).sum() + (b[0] * b[1]).sum()
        elif mode in ("all", cls):
            tot = tot + _error_columns(b, k).sum()
    return tot


def _flags():
    from tensorflowraytrace_amd import _lib
    return _lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_STOPPED | _lib.COMPILE_DEAD


@functools.lru_cache(maxsize=None)
def _scene_for(seed, n_rays, kinds="both"):
    return _scene(np.random.default_rng(seed), n_rays, with_seg=kinds != "arc",
                  with_arc=kinds != "seg")


def _merged(sets, grads_of, kind, geo):
    """Per-field gradients gathered into the merged (optical, stop, target) primitive order."""
    parts = [torch.stack([grads_of[id(sets[f"{c}_{kind}"][f])] for f in geo], 1)
             for c in ("optical", "stop", "target") if sets.get(f"{c}_{kind}")]
    return torch.cat(parts) if parts else None


@functools.lru_cache(maxsize=None)
def _reference(seed, n_scene, kinds, n_rays, f32, passes, finite_tir, dead_len, mode):
    """The oracle's trace of the first n_rays rays of _scene_for(seed, n_scene, kinds) and the
    gradients of _error(mode) with respect to every float field of every boundary set and to the
    four source rows.  Computed once per case and shared; nobody writes to it."""
    sets, rays, wl = _scene_for(seed, n_scene, kinds)
    rays, wl = rays[:, :n_rays], wl[:n_rays]
    osets = {k: {f: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v)
                 for f, v in s.items()} for k, s in sets.items()}
    src = _src2(rays, wl, f32)
    src_leaves = [src[n].requires_grad_(True) for n in NAMES]
    ref = tracer.ray_trace(_oracle_system(osets), src, max_iterations=passes,
                           inherit=("wavelength", "ray_id"), finite_tir_gradient=finite_tir,
                           flags=dict(compile_dead_rays=True, compile_stopped_rays=True,
                                      dead_ray_length=dead_len))
    blocks = {c: torch.stack([ref[c][n] for n in NAMES]) for c in CLASSES
              if ref.get(c) and ref[c]["x_start"].shape[0]}
    loss = _error(blocks, mode)
    geo_leaves = [v for s in osets.values() for v in s.values() if v.dtype.is_floating_point]
    leaves = geo_leaves + src_leaves
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads_of = {id(l): (torch.zeros_like(l) if g is None else g) for l, g in zip(leaves, grads)}
    return types.SimpleNamespace(
        ids={c: ref[c]["ray_id"].numpy().astype(np.int64) for c in blocks},
        rays={c: b.detach().numpy() for c, b in blocks.items()},
        counts={c: (blocks[c].shape[1] if c in blocks else 0) for c in CLASSES},
        loss=float(loss.detach()),
        g_seg=_merged(osets, grads_of, "segments", SEG_GEO),
        g_arc=_merged(osets, grads_of, "arcs", ARC_GEO),
        g_src=torch.stack([grads_of[id(l)] for l in src_leaves]))


def _same_sets(out, ref, tol, tag):
    """Same rays in the same classes and order; coordinates to `tol` of the class's magnitude
    (test_forward_2d's measure).  A class the oracle leaves empty is empty on the device."""
    for cls in CLASSES:
        n = ref.counts[cls]
        assert out[cls].shape[1] == n, (tag, cls, out[cls].shape[1], n)
        if n:
            assert np.array_equal(out[cls + "_id"].cpu().numpy().astype(np.int64), ref.ids[cls]), \
                (tag, cls)
            want = ref.rays[cls]
            got = out[cls].detach().cpu().double().numpy()
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            assert err <= tol, f"{tag} {cls}: rel err {err:.2e}"


def _close(got, want, tol, what):
    """_same_grad; where the reference has no finite non-zero entry at all (its scale is 0) the
    device must give exact zeros in the same places.  Returns the number of non-finite entries."""
    w = want.double().cpu()
    fin = torch.isfinite(w)
    g = got.double().cpu()
    if fin.any() and float(w[fin].abs().max()) > 0.0:
        both = fin & torch.isfinite(g)
        print(f"{what}: rel err {float((g[both] - w[both]).abs().max() / w[fin].abs().max()):.2e}")
        return _same_grad(got, want, tol, what)
    assert torch.equal(~torch.isfinite(g), ~fin), f"{what}: non-finite pattern differs"
    assert not fin.any() or float(g[fin].abs().max()) == 0.0, f"{what}: the reference is zero"
    return int((~fin).sum())


def _sweep(scene_key, dtype, passes, finite_tir, dead_len, mode="all", n_rays=None,
           deterministic=False, tag="", f32_bars=None):
    """ops.trace2d of the scene with all four classes compiled and the gradients of _error(mode)
    with respect to (segments, arcs, source rays), checked against _reference.  Returns the
    device's gradients, the reference and the trace.

    Bars: test_forward_2d's for the rays (1e-9 float64 state, 1e-5 float32), test_backward_2d's
    for the gradients (1e-7, 1e-5).  f32_bars: {"segment" | "arc" | "source": bar} for the
    outputs of a float32-state case that were measured to need another one (F32_MEASURED)."""
    from tensorflowraytrace_amd import ops
    f32 = dtype == torch.float32
    set_tol, tol = (1e-5, 1e-5) if f32 else (1e-9, 1e-7)
    bars = dict(segment=tol, arc=tol, source=tol)
    if f32:
        bars.update(f32_bars or {})
    sets, rays, wl = _scene_for(*scene_key)
    n_rays = rays.shape[1] if n_rays is None else n_rays
    ref = _reference(*scene_key, n_rays, f32, passes, finite_tir, dead_len, mode)
    scene, seg, arc = _gpu_scene(sets, wl[:n_rays], requires_grad=True)
    scene.finite_tir_gradient = finite_tir
    scene.deterministic = deterministic
    src = torch.tensor(rays[:, :n_rays], dtype=dtype, device=DEV).requires_grad_(True)
    out = ops.trace2d(src, scene, max_passes=passes, dead_ray_length=dead_len, flags=_flags())
    _same_sets(out, ref, set_tol, tag)
    loss = _error({c: out[c].double() for c in CLASSES}, mode)
    print(f"{tag}: error {float(loss):.17g} oracle {ref.loss:.17g}")
    assert abs(float(loss) - ref.loss) <= 10 * tol * abs(ref.loss), tag
    leaves = [k["geo"] for k in (seg, arc) if k is not None] + [src]
    grads = list(torch.autograd.grad(loss, leaves))
    g_src = grads.pop()
    g_seg = grads.pop(0) if seg is not None else None
    g_arc = grads.pop(0) if arc is not None else None
    assert g_src.dtype == dtype and g_src.shape == src.shape
    assert (g_seg is None) == (ref.g_seg is None) and (g_arc is None) == (ref.g_arc is None)
    bad = 0
    if g_seg is not None:
        bad += _close(g_seg, ref.g_seg, bars["segment"], f"{tag} segment")
    if g_arc is not None:
        # (the oracle's arcs take no gradient through their angles either: they only gate hits)
        assert float(ref.g_arc[:, 2:4].abs().max()) == 0.0
        bad += _close(g_arc[:, [0, 1, 4]], ref.g_arc[:, [0, 1, 4]], bars["arc"], f"{tag} arc")
        assert float(g_arc[:, 2:4].abs().max()) == 0.0
    _close(g_src, ref.g_src, bars["source"], f"{tag} source")
    if not f32:
        # row by row: the start rows' own scale, not the larger one of the end rows
        for r, name in enumerate(NAMES):
            _close(g_src[r], ref.g_src[r], tol, f"{tag} source {name}")
    bad_cols = int((~torch.isfinite(g_src)).any(0).sum())
    assert bad_cols == int((~torch.isfinite(ref.g_src)).any(0).sum())
    return types.SimpleNamespace(g_seg=g_seg, g_arc=g_arc, g_src=g_src, ref=ref, out=out,
                                 poisoned=bad, poisoned_columns=bad_cols)


def _bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


# ------------------------------------------------------------ float32 state: the measured bars
# A float32 ray state rounds every pass's hit and child points to 2^-24; the sweep itself works in
# float64 either way.  In these scenes that rounding, not the sweep, sets the error of the
# outputs below, and it is beyond test_backward_2d's 1e-5.  Measured on an MI355X against the
# oracle, both kernels and the oracle reading the same float32-rounded source (largest error over
# an output / largest finite reference entry):
#
#   case, output                                  float64 state   float32 state
#   MIXED, 4 passes, reference TIR policy, source    1.2e-13         3.59e-5
#   MIXED, 4 passes, finite_tir_gradient, source     5.0e-14         1.52e-5
#   EDGE, first 255 / 256 / 257 rays, arc            4.8e-14         1.36e-5
#   EDGE, first 255 / 256 / 257 rays, source         5.7e-14         1.45e-5
#
# (dead_ray_length changes none of them; every other float32 output of this module stays below
# 3e-6 and keeps 1e-5.)  For scale: rounding only the oracle's own source to float32, once, moves
# these same outputs of the oracle by 2.9e-5, 1.2e-5, 4.5e-5 and 7.2e-5.  The bar is the measured
# float32 figure times 4 (the spread the float64 atomics' summation order can add is far inside).
F32_MEASURED = {
    ("MIXED", False): {"source": 4 * 3.59e-5},
    ("MIXED", True): {"source": 4 * 1.52e-5},
    "EDGE block": {"arc": 4 * 1.36e-5, "source": 4 * 1.45e-5},
}

# ------------------------------------------------------------------- 1. all classes, all outputs

MIXED = (5, 3000, "both")          # 2580 finished, 7893 active, 162 stopped, 31 dead at 4 passes


@pytest.mark.parametrize("dead_len", [None, 0.25])
@pytest.mark.parametrize("finite_tir", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_every_class_seeded_every_gradient_against_oracle_autograd(dtype, finite_tir, dead_len):
    """Every row of every class seeded; segment, arc and source gradients.  Under the reference's
    TIR policy the source columns whose chain reflects totally are NaN on both sides (256 of the
    3000 in the oracle); with finite_tir_gradient nothing is, and every source ray takes a
    gradient.  Float32 state: the source gradient's bar is the measured one (F32_MEASURED:
    float64 state 1.2e-13 / 5.0e-14, float32 state 3.59e-5 / 1.52e-5 without / with
    finite_tir_gradient; bar = 4 x the float32 figure)."""
    r = _sweep(MIXED, dtype, 4, finite_tir, dead_len, tag="all",
               f32_bars=F32_MEASURED["MIXED", finite_tir])
    assert all(r.ref.counts[c] > 0 for c in CLASSES), r.ref.counts
    assert (r.poisoned == 0) == finite_tir, r.poisoned
    assert (r.poisoned_columns == 0) == finite_tir, r.poisoned_columns
    if finite_tir:
        assert bool((r.ref.g_src != 0).any(0).all())
        assert bool((r.g_src != 0).any(0).all()), "a source ray took no gradient"


# -------------------------------------------------------------------- 2. one class seeded at a time

SMALL = (5, 700, "both")           # 599 / 1820 / 38 / 5 at 4 passes


@pytest.mark.parametrize("mode,dead_len", [
    ("finished", 0.25), ("active", 0.25), ("stopped", 0.25), ("dead", 0.25),
    ("active_start", 0.25), ("dead", None)])
def test_one_class_seeded_the_others_take_none(mode, dead_len):
    """The error reads one class only: the other three, present in the trace and holding rays,
    arrive in backward() as None (null seed pointers in the sweep).  "active_start": only the
    start rows of the active rays, the seed g_s of links that also have a child."""
    r = _sweep(SMALL, torch.float64, 4, True, dead_len, mode=mode, tag=mode)
    assert all(r.ref.counts[c] > 0 for c in CLASSES), r.ref.counts
    if mode in ("dead", "stopped"):
        cols = int((r.g_src != 0).any(0).sum())
        assert cols >= r.ref.counts[mode], (mode, cols, r.ref.counts[mode])


# ---------------------------------------------------------------------------- 3. pass-count edges

EDGE = (7, 321, "both")


@pytest.mark.parametrize("finite_tir", [False, True])
@pytest.mark.parametrize("passes,dead_len", [(1, 0.25), (6, None)])
def test_pass_count_edges(passes, dead_len, finite_tir):
    """max_passes = 1: pass 0 is also the last pass, it writes the source gradient without a
    child buffer, and the dead class is compiled, seeded and empty (23 / 287 / 11 / 0).
    max_passes = 6: 248 / 850 / 35 / 25, 95 source columns NaN under the reference's policy."""
    r = _sweep(EDGE, torch.float64, passes, finite_tir, dead_len, tag=f"P={passes}")
    if passes == 1:
        assert r.ref.counts["dead"] == 0 and r.out["dead"].shape[1] == 0
        assert r.poisoned_columns == 0           # (nothing reacts after the only projection)
    else:
        assert all(r.ref.counts[c] > 0 for c in CLASSES), r.ref.counts
        assert (r.poisoned_columns == 0) == finite_tir, r.poisoned_columns


# ----------------------------------------------------------------------------- 4. ray-count edges

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_ray_counts_around_the_wavefront_and_the_block(n_rays, dtype):
    """The first n rays of the pass-edge scene: one ray, a wavefront and a block of the sweep,
    each minus and plus one (the last block partly filled, or exactly full).  Float32 state at
    255 / 256 / 257 rays: the arc and source gradients' bars are the measured ones (F32_MEASURED:
    float64 state 4.8e-14 and 5.7e-14, float32 state 1.36e-5 and 1.45e-5; bar = 4 x the float32
    figure); up to 65 rays every output keeps 1e-5."""
    r = _sweep(EDGE, dtype, 4, True, None, n_rays=n_rays, tag=f"N={n_rays}",
               f32_bars=F32_MEASURED["EDGE block"] if n_rays >= BLOCK - 1 else None)
    assert sum(r.ref.counts.values()) >= n_rays


# --------------------------------------------------------------------------- 5. single-kind scenes

@pytest.mark.parametrize("finite_tir", [False, True])
@pytest.mark.parametrize("kinds", ["arc", "seg"])
def test_scenes_of_one_primitive_kind(kinds, finite_tir):
    """Arcs only (no segment tensor, no stop: the stopped class is seeded and empty) and segments
    only (no arc tensor)."""
    r = _sweep((5, 700, kinds), torch.float64, 4, finite_tir, 0.25, tag=kinds)
    assert (r.g_seg is None) == (kinds == "arc") and (r.g_arc is None) == (kinds == "seg")
    if kinds == "arc":
        assert r.ref.counts["stopped"] == 0
    assert sum(n > 0 for n in r.ref.counts.values()) >= 2, r.ref.counts


# --------------------------------------------------------------------------------- 6. ordered sums

@pytest.mark.parametrize("dead_len", [None, 0.25])
@pytest.mark.parametrize("finite_tir", [False, True])
def test_ordered_sweep_with_every_class_seeded(finite_tir, dead_len):
    """Case 1's float64 rows on Scene2DArgs(deterministic=True): the same bars against the
    oracle, primitive gradients bit-identical from run to run, and the source gradient -- written
    ray by ray, never summed -- bit-identical to the float64-atomic sweep's."""
    a = _sweep(MIXED, torch.float64, 4, finite_tir, dead_len, deterministic=True, tag="ordered")
    b = _sweep(MIXED, torch.float64, 4, finite_tir, dead_len, deterministic=True, tag="ordered")
    assert _bits(a.g_seg) == _bits(b.g_seg) and _bits(a.g_arc) == _bits(b.g_arc)
    assert _bits(a.g_src) == _bits(b.g_src)
    atomic = _sweep(MIXED, torch.float64, 4, finite_tir, dead_len, tag="atomic")
    assert _bits(a.g_src) == _bits(atomic.g_src), "the ordered sweep changed a source gradient"
    assert (a.poisoned == 0) == finite_tir, a.poisoned
