"""The fused, graph-replayed optimiser step on 2-D engines (FusedStep with a GoalError) and its
one-launch reverse sweep tfrt_trace2d_backward_goal: against the generic path, against the
unfolded launch sequence (tfrt_goal_error3d + tfrt_trace2d_backward) and against oracle autograd."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import tracer
from test_gpu_trace2d import _gpu_scene, _oracle_system, _same_grad, _scene, _src2
from test_gpu_variants import _source2, _system2

pytestmark = pytest.mark.gpu
PI = math.pi
DEV = "cuda:0"
LR_SCALES = (1.0, 0.7, 0.5, 1.2, 0.9, 0.6, 1.0, 0.8)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))


# ------------------------------------------------------------------------------------ scenes
def _single_arc(ray_dtype, rays=200):
    """dev/optimize_single_arc.py: one parameter is the arc's x_center AND radius."""
    import optimize_arc
    s = optimize_arc.build(rays, ray_dtype=ray_dtype)
    n = s["system"].sources["x_start"].shape[0]
    from tfrt.optimizer import GoalError
    return s["engine"], [s["parameter"]], GoalError(("y_end",), torch.zeros(n, dtype=torch.float64,
                                                                            device=DEV))


def _segment_lens(ray_dtype):
    """A ParametricMultiSegmentBoundary lens (two layers, ThicknessConstraints)."""
    import tfrt.boundaries as boundaries
    import tfrt.distributions as distributions
    from tfrt.optimizer import GoalError
    k = 13
    ys = np.linspace(-1.1, 1.1, k)
    zero = distributions.ManualBasePointDistribution(2, points=np.stack([np.zeros(k), ys], 1))
    one = distributions.ManualBasePointDistribution(2, points=np.stack([np.ones(k), ys], 1))
    bump = 1 - (ys / 1.1) ** 2
    multi = boundaries.ParametricMultiSegmentBoundary(
        zero, one,
        [boundaries.ThicknessConstraint(0.0, "min"), boundaries.ThicknessConstraint(0.15, "min")],
        [True, False], initial_parameters=[-0.2 * bump - 0.05, 0.2 * bump],
        material_list=[{"mat_in": 1, "mat_out": 0}] * 2)
    system, eng, _ = _system2([multi], _source2(2000))
    eng.ray_dtype = ray_dtype
    n = system.sources["x_start"].shape[0]
    return eng, list(multi.parameters), GoalError(
        ("y_end",), torch.full((n,), 0.05, dtype=torch.float64, device=DEV))


def _mixed(ray_dtype):
    """Refracting arcs (radii are a parameter), a mirror polyline (start heights are another), a
    stop, a target wall and a target arc: every class occurs, totally reflected rays included."""
    import tfrt.boundaries as boundaries
    import tfrt.engine as engine
    import tfrt.materials as materials
    import tfrt.operation as operation
    import tfrt.sources as sources
    from tfrt.optimizer import GoalError
    rng = np.random.default_rng(7)
    sets, rays, wl = _scene(rng, 3000)
    radius = sets["optical_arcs"]["radius"].to(DEV).requires_grad_(True)
    heights = sets["optical_segments"]["y_start"].to(DEV).requires_grad_(True)
    made = {}
    for name, fields in sets.items():
        b = boundaries.ManualArcBoundary() if name.endswith("arcs") else \
            boundaries.ManualSegmentBoundary()
        for f, v in fields.items():
            b[f] = v
        made[name] = b
    made["optical_arcs"]["radius"] = radius
    made["optical_segments"]["y_start"] = heights
    src = sources.ManualSource(2)
    for i, f in enumerate(("x_start", "y_start", "x_end", "y_end")):
        src[f] = rays[i]
    src["wavelength"] = wl
    system = engine.OpticalSystem2D()
    for name, b in made.items():
        setattr(system, name, [b])
    system.sources = [src]
    system.materials = [{"n": materials.vacuum}, {"n": materials.acrylic},
                        {"n": materials.reflective}]
    eng = engine.OpticalEngine(2, [operation.StandardReaction()], ray_dtype=ray_dtype,
                               compile_dead_rays=True, compile_stopped_rays=True)
    eng.optical_system = system
    system.update()
    eng.validate_system()
    goal = torch.stack([0.5 * torch.tensor(rays[0]), torch.full((rays.shape[1],), 5.0)], 1)
    return eng, [radius, heights], GoalError(("x_end", "y_end"), goal.to(DEV))


SCENES = {"single_arc": _single_arc, "segment_lens": _segment_lens, "mixed": _mixed}


def _run(make, mode, ray_dtype, steps=8, momentum=None, accumulators=None):
    from tfrt.optimizer import SGD_Optimizer
    eng, params, erf = make(ray_dtype)
    opt = SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                        sgd_learning_rate=1.0, apply_momentum=momentum is not None,
                        fused=mode != "generic", graph=mode == "graph")
    errors, history = [], []
    for i in range(steps):
        m = 0.0 if momentum is None else momentum[i]
        e = opt.single_step(accumulators, lr_scale=LR_SCALES[i % len(LR_SCALES)], momentum=m)
        errors.append(float(e))
        history.append([p.detach().clone() for p in params])
    torch.cuda.synchronize()
    return errors, history, opt


def _compare(runs, err_rtol, param_atol):
    (e0, h0, _), rest = runs[0], runs[1:]
    for e, h, _ in rest:
        np.testing.assert_allclose(e, e0, rtol=err_rtol, atol=0)
        for a, b in zip(h, h0):
            for x, y in zip(a, b):
                assert float((x - y).abs().max()) <= param_atol


# float32 state: the trace is the same launch on both paths, but the parameters differ in their
# last bits (the primitive gradients are summed in another order), and a float32 ray that then
# rounds the other way changes the error in its 7th digit and a gradient entry by its share
TOLS = {torch.float64: (1e-11, 1e-12), torch.float32: (1e-6, 1e-7)}


@pytest.mark.parametrize("ray_dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_fused_2d_step_equals_the_generic_step(scene, ray_dtype):
    make = SCENES[scene]
    runs = [_run(make, mode, ray_dtype) for mode in ("generic", "eager", "graph")]
    generic, eager, graph = (r[2] for r in runs)
    assert generic._fused_step is None
    assert eager._fused_step is not None and eager._fused_step.graph_replays == 0
    fs = graph._fused_step
    assert fs is not None and fs.capture_error is None and not fs.untapped
    assert fs.graph_replays >= len(LR_SCALES) - 4
    assert all(np.isfinite(runs[0][0]))
    _compare(runs, *TOLS[ray_dtype])
    # the ray sets of the last fused step are published on demand, like the generic path's
    fin_g = generic.engine.finished_rays["y_end"]
    fin_f = graph.engine.finished_rays["y_end"]
    assert fin_g.shape == fin_f.shape and fin_g.shape[0] > 0


def test_fused_2d_momentum_and_accumulator_equal_the_generic_step():
    """Nesterov momentum with a phase change (0.6 -> 0.9: the same graph replays) and a CSR
    accumulator on one of the lens's two parameters."""
    k = 13
    acc = np.triu(np.ones((k, k))) * 0.5 + np.eye(k) * 0.5
    momentum = [0.6] * 4 + [0.9] * 4
    runs = []
    for mode in ("generic", "eager", "graph"):
        r = _run(_segment_lens, mode, torch.float64, momentum=momentum, accumulators=[acc, None])
        runs.append(r)
    fs = runs[2][2]._fused_step
    assert fs.capture_error is None and fs.graph_replays >= 4
    _compare(runs, 1e-11, 1e-12)


def test_momentum_phase_change_replays_one_graph():
    from tfrt.optimizer import SGD_Optimizer
    eng, params, erf = _single_arc(torch.float64)
    opt = SGD_Optimizer(eng, params, erf, 2, learning_rate=1.0, grad_clip=0.1,
                        sgd_learning_rate=1.0, apply_momentum=True)
    for _ in range(5):
        opt.single_step(None, momentum=0.8)
    g = opt._fused_step._graphs[1]
    replays = opt._fused_step.graph_replays
    for _ in range(3):
        opt.single_step(None, momentum=0.9, lr_scale=0.1)
    assert opt._fused_step._graphs[1] is g and opt._fused_step.graph_replays == replays + 3


# ------------------------------------------------------------------------------- the C ABI
def _trace(src, scene, seg, arc, P, L=1.0):
    """tfrt_trace2d_forward into fresh buffers; returns what both reverse routes need."""
    from tensorflowraytrace_amd import _lib, ops
    lib = _lib.lib()
    N, dt = src.shape[1], ops._DT[src.dtype]
    Ms = 0 if seg is None else seg.shape[0]
    Ma = 0 if arc is None else arc.shape[0]
    wsb = lib.tfrt_trace2d_workspace_bytes(N, Ms, Ma, P, dt)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    capN = max(N, 1)
    counts = torch.zeros(_lib.COUNTS_PER_PASS * (P + 1), dtype=torch.int32, device=DEV)
    fin = torch.zeros((4, capN), dtype=src.dtype, device=DEV)
    fid = torch.zeros(capN, dtype=torch.int32, device=DEV)
    ffc = torch.zeros(capN, dtype=torch.int32, device=DEV)
    outs = [ops._ray_out(fin, fid, ffc)] + [ops._ray_out(None, None, None)] * 3
    sc = scene.struct(seg, arc)
    flags = _lib.COMPILE_FINISHED
    _lib.check(lib.tfrt_trace2d_forward(
        ops._p(src), N, N, ctypes.byref(sc), L, 0.0, P, dt, flags, *[ctypes.byref(o) for o in outs],
        None, None, ops._p(counts), ops._p(ws), wsb, ops._stream(src)), "tfrt_trace2d_forward")
    return dict(src=src, sc=sc, seg=seg, arc=arc, P=P, L=L, dt=dt, N=N, ws=ws, wsb=wsb,
                counts=counts, fin=fin, fid=fid, out=outs[0], capN=capN, Ms=Ms, Ma=Ma)


def _folded(t, rows, goal):
    from tensorflowraytrace_amd import _lib, ops
    lib = _lib.lib()
    g_seg = torch.zeros((max(t["Ms"], 1), 4), dtype=torch.float64, device=DEV)
    g_arc = torch.zeros((max(t["Ma"], 1), 5), dtype=torch.float64, device=DEV)
    err = torch.zeros(3, dtype=torch.float64, device=DEV)
    tests = torch.zeros(1, dtype=torch.int64, device=DEV)
    gwb = lib.tfrt_trace2d_backward_goal_workspace_bytes(t["N"])
    gws = torch.zeros(gwb, dtype=torch.uint8, device=DEV)
    pending = _lib.GoalPending()
    fields = (ctypes.c_int32 * 4)(*(list(rows) + [0] * 4)[:4])
    st = ops._stream(t["src"])
    _lib.check(lib.tfrt_trace2d_backward_goal(
        ops._p(t["src"]), t["N"], t["N"], ctypes.byref(t["sc"]), t["L"], t["P"], t["dt"],
        ctypes.byref(t["out"]), fields, len(rows), ops._p(goal), goal.shape[1], 1, ops._p(err),
        ops._p(tests), ops._p(gws), gwb, ctypes.byref(pending),
        ops._p(g_seg) if t["Ms"] else None, ops._p(g_arc) if t["Ma"] else None,
        ops._p(t["counts"]), ops._p(t["ws"]), t["wsb"], st), "tfrt_trace2d_backward_goal")
    _lib.check(lib.tfrt_goal_finish(ctypes.byref(pending), st), "tfrt_goal_finish")
    torch.cuda.synchronize()
    return err, g_seg[:t["Ms"]], g_arc[:t["Ma"]], tests


def _unfolded(t, rows, goal):
    from tensorflowraytrace_amd import _lib, ops
    lib = _lib.lib()
    g_seg = torch.zeros((max(t["Ms"], 1), 4), dtype=torch.float64, device=DEV)
    g_arc = torch.zeros((max(t["Ma"], 1), 5), dtype=torch.float64, device=DEV)
    err = torch.zeros(3, dtype=torch.float64, device=DEV)
    tests = torch.zeros(1, dtype=torch.int64, device=DEV)
    g_fin = torch.zeros((4, t["capN"]), dtype=torch.float64, device=DEV)
    gwb = lib.tfrt_goal_error3d_workspace_bytes(t["capN"])
    gws = torch.zeros(gwb, dtype=torch.uint8, device=DEV)
    fields = (ctypes.c_int32 * 6)(*(list(rows) + [0] * 6)[:6])
    st = ops._stream(t["src"])
    _lib.check(lib.tfrt_goal_error3d(
        ops._p(t["fin"]), t["capN"], ops._p(t["fid"]), t["dt"], ops._p(t["counts"]), t["P"],
        fields, len(rows), ops._p(goal), goal.shape[1], 1, ops._p(g_fin), ops._p(err), None, 0,
        ops._p(tests), ops._p(gws), gwb, st), "tfrt_goal_error3d")
    _lib.check(lib.tfrt_trace2d_backward(
        ops._p(t["src"]), t["N"], t["N"], ctypes.byref(t["sc"]), t["L"], 0.0, t["P"], t["dt"],
        ops._p(g_fin), t["capN"], None, 0, None, 0, None, 0,
        ops._p(g_seg) if t["Ms"] else None, ops._p(g_arc) if t["Ma"] else None, None,
        ops._p(t["counts"]), ops._p(t["ws"]), t["wsb"], st), "tfrt_trace2d_backward")
    torch.cuda.synchronize()
    return err, g_seg[:t["Ms"]], g_arc[:t["Ma"]], tests


def _check_routes(t, rows, goal, grad_tol=1e-12):
    a = _folded(t, rows, goal)
    b = _unfolded(t, rows, goal)
    e1, e2 = a[0].cpu().numpy(), b[0].cpu().numpy()
    assert e1[1] == e2[1]                                        # terms
    np.testing.assert_allclose(e1[0], e2[0], rtol=1e-13, atol=0)
    assert int(a[3]) == int(b[3])                                # the trace's test count
    for x, y, what in ((a[1], b[1], "segment"), (a[2], b[2], "arc")):
        if x.numel() and float(torch.nan_to_num(y, nan=0.0).abs().max()) > 0:
            _same_grad(x, y, grad_tol, what)
        else:                               # (nothing reached these primitives: zeros on both sides)
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    again = _folded(t, rows, goal)
    assert again[0][0].cpu().numpy().tobytes() == e1[0].tobytes()   # bit-identical error
    return a, b


def _guide(n_rays, rng):
    """A mirrored light guide: two mirror walls (8 segments each) 2 apart and 30 long, a target
    wall at the far end; the rays bounce 10 to 19 times."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    xs = np.linspace(0.0, 30.0, 9)
    walls = dict(x_start=t(np.r_[xs[:-1], xs[1:]]), y_start=t(np.r_[np.full(8, -1.0), np.full(8, 1.0)]),
                 x_end=t(np.r_[xs[1:], xs[:-1]]), y_end=t(np.r_[np.full(8, -1.0), np.full(8, 1.0)]),
                 mat_in=torch.full((16,), 2, dtype=torch.int64),
                 mat_out=torch.zeros(16, dtype=torch.int64))
    sets = dict(optical_segments=walls,
                target_segments=dict(x_start=t([30.0]), y_start=t([-2.0]), x_end=t([30.0]),
                                     y_end=t([2.0])))
    ang = rng.uniform(0.6, 0.9, n_rays) * rng.choice([-1, 1], n_rays)
    y0 = rng.uniform(-0.5, 0.5, n_rays)
    rays = np.stack([np.full(n_rays, 0.5), y0, 0.5 + np.cos(ang), y0 + np.sin(ang)])
    return sets, rays, rng.uniform(450, 650, n_rays)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16])
@pytest.mark.parametrize("finite_tir", [False, True])
@pytest.mark.parametrize("P", [1, 2, 4])
def test_backward_goal_2d_equals_the_unfolded_sequence(P, finite_tir, dtype):
    rng = np.random.default_rng(100 + P)
    sets, rays, wl = _scene(rng, 3001)                    # (not a multiple of 64)
    scene, seg, arc = _gpu_scene(sets, wl)
    scene.finite_tir_gradient = finite_tir
    src = torch.tensor(rays, dtype=dtype, device=DEV)
    t = _trace(src, scene, seg["geo"], arc["geo"], P)
    goal = torch.tensor(rng.normal(size=(2, 3001)), dtype=torch.float64, device=DEV)
    a, _ = _check_routes(t, (2, 3), goal)
    assert float(a[0][1]) > 0
    one = goal[:1].contiguous()
    _check_routes(t, (1,), one)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("P", [12, 24])
def test_backward_goal_2d_over_long_chains(P, dtype):
    """P = 12 and 24 on the mirrored guide: chains longer than the 16 links a lane keeps in LDS
    re-walk the tape."""
    rng = np.random.default_rng(9)
    sets, rays, wl = _guide(2000, rng)
    scene, seg, _ = _gpu_scene(sets, wl)
    src = torch.tensor(rays, dtype=dtype, device=DEV)
    t = _trace(src, scene, seg["geo"], None, P)
    counts = t["counts"].cpu().numpy()
    assert counts[P * 8 + 1] > 100                       # finished chains ...
    assert counts[8 * 8:P * 8].reshape(-1, 8)[:, 1].sum() > 0   # ... of more than 8 links
    goal = torch.tensor(rng.normal(size=(1, 2000)), dtype=torch.float64, device=DEV)
    _check_routes(t, (3,), goal)
    _check_routes(t, (0, 1, 2, 3), goal.expand(4, 2000).contiguous())


def test_backward_goal_2d_edge_cases():
    rng = np.random.default_rng(3)
    # zero finished rays: one pass of the guide, where every ray meets a wall first
    sets, rays, wl = _guide(70, rng)
    scene, seg, _ = _gpu_scene(sets, wl)
    src = torch.tensor(rays, dtype=torch.float64, device=DEV)
    goal = torch.zeros((1, 70), dtype=torch.float64, device=DEV)
    for P in (0, 1):
        t = _trace(src, scene, seg["geo"], None, P)
        a, b = _check_routes(t, (3,), goal)
        assert float(a[0][1]) == 0 and math.isnan(float(a[0][2])) and float(a[0][0]) == 0
    # n_rays = 0
    sets, rays, wl = _scene(rng, 70)
    scene, seg, arc = _gpu_scene(sets, wl)
    t = _trace(src[:, :0].contiguous(), scene, seg["geo"], arc["geo"], 3)
    a = _folded(t, (3,), goal[:, :0].contiguous())
    assert float(a[0][0]) == 0 and float(a[0][1]) == 0
    assert float(a[1].abs().sum()) == 0 and float(a[2].abs().sum()) == 0


@pytest.mark.parametrize("finite_tir", [False, True])
def test_backward_goal_2d_against_oracle_autograd(finite_tir):
    rng = np.random.default_rng(5)
    sets, rays, wl = _scene(rng, 3000)
    scene, seg, arc = _gpu_scene(sets, wl)
    scene.finite_tir_gradient = finite_tir
    src = torch.tensor(rays, dtype=torch.float64, device=DEV)
    P = 4
    t = _trace(src, scene, seg["geo"], arc["geo"], P)
    goal = torch.tensor(rng.normal(size=(2, 3000)), dtype=torch.float64, device=DEV)
    err, g_seg, g_arc, _ = _folded(t, (2, 3), goal)

    osets = {k: {f: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v)
                 for f, v in s.items()} for k, s in sets.items()}
    ref = tracer.ray_trace(_oracle_system(osets), _src2(rays, wl, False), max_iterations=P,
                           inherit=("wavelength", "ray_id"), finite_tir_gradient=finite_tir)
    rf = ref["finished"]
    ids = rf["ray_id"].long()
    gl = goal.cpu()
    rloss = ((rf["x_end"] - gl[0, ids]) ** 2).sum() + ((rf["y_end"] - gl[1, ids]) ** 2).sum()
    np.testing.assert_allclose(float(err[0]), float(rloss.detach()), rtol=1e-9)
    leaves = []
    for kind, geo in (("segments", ("x_start", "y_start", "x_end", "y_end")),
                      ("arcs", ("x_center", "y_center", "radius"))):
        for cname in ("optical", "stop", "target"):
            s = osets.get(f"{cname}_{kind}")
            if s:
                leaves += [s[f] for f in geo]
    grads = torch.autograd.grad(rloss, leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
    it = iter(grads)
    segs = [torch.stack([next(it) for _ in range(4)], 1) for c in ("optical", "stop", "target")
            if osets.get(f"{c}_segments")]
    arcs = [torch.stack([next(it) for _ in range(3)], 1) for c in ("optical", "stop", "target")
            if osets.get(f"{c}_arcs")]
    poisoned = _same_grad(g_seg, torch.cat(segs), 1e-9, "segment")
    poisoned += _same_grad(g_arc[:, [0, 1, 4]], torch.cat(arcs), 1e-9, "arc")
    assert float(g_arc[:, 2:4].abs().max()) == 0.0
    assert (poisoned == 0) == finite_tir, poisoned


def test_single_arc_at_a_million_rays_against_the_per_pass_sequence():
    """Every lane of the single-arc scene adds into the same arc row: the wave-combined atomics
    give the per-pass sequence's gradient."""
    eng, params, erf = _single_arc(torch.float64, rays=166_667)      # x 6 wavelengths
    src = eng.optical_system._amalgamated_sources
    block, scene, _ = eng._trace_inputs(src)
    assert block.shape[1] > 1_000_000
    seg, arc = scene.segments["geo"].detach(), scene.arcs["geo"].detach()
    t = _trace(block, scene, seg, arc, 2)
    goal = erf.table(src)
    # (a million float64 terms per entry, added in another order: up to n * eps apart)
    a, b = _check_routes(t, (3,), goal, grad_tol=1e-10)
    assert float(a[0][1]) > 900_000
    assert float(a[2][0, 4].abs()) > 0


def test_optimize_arc_example_lowers_the_error_on_the_graph_path():
    import optimize_arc
    errors, s = optimize_arc.run(ray_count=50, steps=20, momentum=True, verbose=False)
    fs = s["optimizer"]._fused_step
    assert fs is not None and fs.capture_error is None and fs.graph_replays >= 15
    assert min(errors[-5:]) < 0.5 * errors[0], errors
