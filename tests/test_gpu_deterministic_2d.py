"""Ordered 2-D reverse sweeps (tfrt_scene2d.deterministic, OpticalEngine(2, ...,
deterministic=True)): the primitive and index gradients are bit-identical from run to run and for
any order of the source rays, agree with the float64-atomic default and with oracle autograd, keep
the reference's TIR NaN policy, drive the fused, graph-replayed 2-D step reproducibly, and keep
their headroom beyond 2^22 terms per entry."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_fused_2d import _folded, _trace as _trace_c
from test_gpu_index_gradients import _gpu_value_scene, _loss, _value_sets
from test_gpu_trace2d import _gpu_scene, _oracle_system, _same_grad, _scene, _src2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_trace2d.npz")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))
CLASSES = ("finished", "active", "stopped")
# ordered against atomic sums: both round, in different ways, to the float64 sum of the terms
ORDER_TOL = 1e-10


def _bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def _agree(got, want, what):
    """NaN exactly where the atomic sum is not finite; elsewhere within ORDER_TOL of the largest
    finite entry.  Returns the number of non-finite entries."""
    got, want = got.double().cpu(), want.double().cpu()
    bad = ~torch.isfinite(want)
    assert torch.equal(torch.isnan(got), bad), f"{what}: non-finite pattern differs"
    if (~bad).any():
        err = float((got[~bad] - want[~bad]).abs().max())
        assert err <= ORDER_TOL * float(want[~bad].abs().max()), f"{what}: {err:.3e}"
    return int(bad.sum())


def _gradients(mode, sets, rays, wl, dtype, deterministic, P=4, finite_tir=False):
    """ops.trace2d over the mixed scene and the gradients of _loss: [g_seg, g_arc] and, in "value"
    mode, the four index gradients."""
    from tensorflowraytrace_amd import _lib, ops
    if mode == "index":
        scene, seg, arc = _gpu_scene(sets, wl, requires_grad=True)
        scene.finite_tir_gradient = finite_tir
        leaves = [k["geo"] for k in (seg, arc) if k is not None]
    else:
        scene, merged = _gpu_value_scene(sets, finite_tir, geo_grad=True)
        seg, arc = merged["segments"], merged["arcs"]
        leaves = [seg["geo"], arc["geo"], seg["n_in"], seg["n_out"], arc["n_in"], arc["n_out"]]
    scene.deterministic = deterministic
    src = torch.tensor(rays, dtype=dtype, device=DEV)
    flags = _lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_STOPPED
    out = ops.trace2d(src, scene, max_passes=P, flags=flags)
    grads = torch.autograd.grad(_loss([out[c] for c in CLASSES]), leaves)
    torch.cuda.synchronize()
    return [g.detach() for g in grads]


@pytest.mark.parametrize("mode", ["index", "value"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_ordered_sweep_is_bit_identical_across_runs_and_ray_orders(mode, dtype):
    n = 200_000
    if mode == "index":
        sets, rays, wl = _scene(np.random.default_rng(21), n)
    else:
        sets, rays, wl = _value_sets(21, n)
    runs = [_gradients(mode, sets, rays, wl, dtype, True) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert _bits(a) == _bits(b), "ordered gradients differ between runs"
    # the same rays in another order (a ray's wavelength travels with it)
    perm = np.random.default_rng(22).permutation(n)
    permuted = _gradients(mode, sets, rays[:, perm], wl[perm], dtype, True)
    for k, (a, b) in enumerate(zip(runs[0], permuted)):
        assert _bits(a) == _bits(b), f"ordered gradient {k} depends on the order of the rays"
    # against the float64-atomic default, entry array by entry array
    atomic = _gradients(mode, sets, rays, wl, dtype, False)
    names = ["segment", "arc", "seg n_in", "seg n_out", "arc n_in", "arc n_out"]
    for a, b, what in zip(runs[0], atomic, names):
        _agree(a, b, what)
    assert float(torch.nan_to_num(runs[0][1], nan=0.0).abs().max()) > 0
    if mode == "value":
        assert any(float(torch.nan_to_num(g, nan=0.0).abs().max()) > 0 for g in runs[0][2:])


@pytest.mark.parametrize("finite_tir", [False, True])
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-7), (torch.float32, 1e-5)])
def test_ordered_sweep_against_oracle_autograd(dtype, tol, finite_tir):
    """test_gpu_trace2d.test_backward_2d with the ordered sweep."""
    from oracle import tracer
    from tensorflowraytrace_amd import ops
    rng = np.random.default_rng(5)
    sets, rays, wl = _scene(rng, 3000)
    scene, seg, arc = _gpu_scene(sets, wl, requires_grad=True)
    scene.finite_tir_gradient = finite_tir
    scene.deterministic = True
    src = torch.tensor(rays, dtype=dtype, device=DEV)
    out = ops.trace2d(src, scene, max_passes=4)
    loss = (out["finished"][2].double() ** 2).sum() + 0.3 * (out["active"][3].double()).sum()
    g_seg, g_arc = torch.autograd.grad(loss, [seg["geo"], arc["geo"]])

    osets = {k: {f: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v)
                 for f, v in s.items()} for k, s in sets.items()}
    ref = tracer.ray_trace(_oracle_system(osets), _src2(rays, wl, dtype == torch.float32),
                           max_iterations=4, inherit=("wavelength", "ray_id"),
                           finite_tir_gradient=finite_tir)
    rloss = (ref["finished"]["x_end"] ** 2).sum() + 0.3 * ref["active"]["y_end"].sum()
    leaves, segs, arcs = [], [], []
    for kind, geo, bucket in (("segments", ("x_start", "y_start", "x_end", "y_end"), segs),
                              ("arcs", ("x_center", "y_center", "radius"), arcs)):
        for cname in ("optical", "stop", "target"):
            s = osets.get(f"{cname}_{kind}")
            if s:
                bucket.append(len(geo))
                leaves += [s[f] for f in geo]
    grads = torch.autograd.grad(rloss, leaves, allow_unused=True)
    it = iter([torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)])
    r_seg = torch.cat([torch.stack([next(it) for _ in range(k)], 1) for k in segs])
    r_arc = torch.cat([torch.stack([next(it) for _ in range(k)], 1) for k in arcs])
    poisoned = _same_grad(g_seg, r_seg, tol, "segment")
    poisoned += _same_grad(g_arc[:, [0, 1, 4]], r_arc, tol, "arc")
    assert float(g_arc[:, 2:4].abs().max()) == 0.0
    assert (poisoned == 0) == finite_tir, poisoned


def _golden_sets(g, tag):
    sets = {}
    for key in g.files:
        if key.startswith(tag + "__"):
            _, name, field = key.split("__")
            sets.setdefault(name, {})[field] = torch.tensor(g[key])
    return sets


def test_ordered_sweep_keeps_the_tir_nan_policy_on_the_reference_cases():
    """prism / gtir of reference_trace2d.npz: NaN exactly where the atomic sums are not finite,
    the same values elsewhere; with finite_tir_gradient everything is finite in both modes."""
    g = np.load(GOLD)
    poisoned = 0
    for tag in ("prism", "gtir"):
        sets = _golden_sets(g, tag)
        rays, wl = g[tag + "_rays"], g[tag + "_wl"]
        for finite_tir in (False, True):
            got = _gradients("index", sets, rays, wl, torch.float64, True, finite_tir=finite_tir)
            want = _gradients("index", sets, rays, wl, torch.float64, False, finite_tir=finite_tir)
            assert len(got) == len(want) == 1
            for a, b in zip(got, want):
                bad = _agree(a, b, tag)
                if finite_tir:
                    assert bad == 0, f"{tag}: finite_tir_gradient left {bad} NaN"
                else:
                    poisoned += bad
    assert poisoned > 0          # (the cases do reflect totally)


# ----------------------------------------------------------------- the fused 2-D optimiser step
def _arc_scene(beam_points, permute=None):
    """examples/optimize_arc.py's scene on a deterministic engine; ``permute``: the source's rays
    in this order instead (a ManualSource with the same rays)."""
    import optimize_arc
    import tfrt.sources as sources
    s = optimize_arc.build(beam_points, deterministic=True)
    if permute is not None:
        system = s["system"]
        rays = system.sources
        src = sources.ManualSource(2)
        for f in ("x_start", "y_start", "x_end", "y_end", "wavelength"):
            src[f] = rays[f].detach().cpu().numpy()[permute]
        system.sources = [src]
        system.update()
    return s


def _steps(error, steps, beam_points=17_000, permute=None, fused=True):
    """`steps` steps of optimize_arc's optimiser (plain SGD); the errors, the parameter after
    every step and the first step's primitive gradient (fused path)."""
    import optimize_arc
    s = _arc_scene(beam_points, permute)
    assert s["system"].sources["x_start"].shape[0] >= 100_000
    opt = optimize_arc.make_optimizer(s, generic=not fused, rowwise=error == "rowwise")
    errors, params, g_prim = [], [], None
    for i in range(steps):
        errors.append(opt.single_step(None, lr_scale=1.0, momentum=0.0))
        params.append(s["parameter"].detach().clone())
        if i == 0 and fused:
            g_prim = opt._fused_step._state["g_prim"].clone()
    torch.cuda.synchronize()
    return [float(e) for e in errors], params, g_prim, opt


@pytest.mark.parametrize("error", ["goal", "rowwise"])
def test_fused_2d_step_is_bit_reproducible(error):
    a = _steps(error, 10)
    b = _steps(error, 10)
    fs = a[3]._fused_step
    assert fs is not None and fs.capture_error is None and fs.graph_replays > 0
    assert b[3]._fused_step.graph_replays == fs.graph_replays
    assert np.array(a[0]).tobytes() == np.array(b[0]).tobytes(), "error sums differ"
    for x, y in zip(a[1], b[1]):
        assert _bits(x) == _bits(y), "parameters differ"
    assert _bits(a[2]) == _bits(b[2])
    assert float((a[1][-1] - a[1][0]).abs().max()) > 0          # (the parameter does move)

    # the same rays in another order (the goal, y_end = 0 for every ray, is its own permutation)
    n = a[3].engine.optical_system.sources["x_start"].shape[0]
    perm = np.random.default_rng(5).permutation(n)
    p = _steps(error, 1, permute=perm)
    assert _bits(p[2]) == _bits(a[2]), "first-step primitive gradient depends on the ray order"
    assert _bits(p[1][0]) == _bits(a[1][0]), "first-step parameter depends on the ray order"

    # the generic path of the same deterministic engine (per-pass ordered sums)
    generic = _steps(error, 10, fused=False)
    assert generic[3]._fused_step is None
    np.testing.assert_allclose(a[0], generic[0], rtol=1e-11, atol=0)
    for x, y in zip(a[1], generic[1]):
        assert float((x - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))


def test_ordered_sum_keeps_its_headroom_beyond_2_22_terms_per_entry():
    """One arc and 4.32M rays x 2 passes (the goal sweep's bound: 8.6M terms per entry, so 38
    bits instead of 40): the ordered sum matches the float64-atomic one."""
    import optimize_arc
    s = optimize_arc.build(720_000)
    eng = s["engine"]
    src = eng.optical_system._amalgamated_sources
    block, scene, _ = eng._trace_inputs(src)
    N = block.shape[1]
    assert N > 2 ** 22
    seg, arc = scene.segments["geo"].detach(), scene.arcs["geo"].detach()
    from tfrt.optimizer import GoalError
    goal = GoalError(("y_end",), torch.zeros(N, dtype=torch.float64, device=DEV)).table(src)
    res = {}
    for det in (False, True):
        scene.deterministic = det
        t = _trace_c(block, scene, seg, arc, 2)
        res[det] = _folded(t, (3,), goal)
        counts = t["counts"].cpu().numpy()
        del t
    assert counts[0] > 2 ** 22          # rays that met the arc in the first pass (all of them)
    np.testing.assert_allclose(res[True][0].cpu().numpy()[:2], res[False][0].cpu().numpy()[:2],
                               rtol=1e-12)
    got, want = res[True][2], res[False][2]
    assert float(want[0, 4].abs()) > 0
    _agree(got, want, "arc")
    assert bool(torch.isfinite(got).all())
