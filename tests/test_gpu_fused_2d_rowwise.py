"""A RowwiseError on the fused, graph-replayed 2-D step (FusedStep._enqueue_rowwise2d) and its two
launches tfrt_trace2d_rows / tfrt_trace2d_backward_rows: against the generic path, against the
GoalError route for the same error, against tfrt_trace2d_backward_goal and against oracle
autograd."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import tracer
from test_gpu_fused_2d import (LR_SCALES, SCENES, TOLS, _compare, _folded, _guide, _single_arc,
                               _segment_lens)
from test_gpu_trace2d import _gpu_scene, _oracle_system, _same_grad, _scene, _src2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fn(r):
    """Two terms per ray: an inherited field, a non-polynomial term of an angle."""
    slope = (r["y_end"] - r["y_start"]) / (r["x_end"] - r["x_start"])
    return torch.stack([(1 + r["wavelength"] / 1000) * r["y_end"] ** 2, torch.log1p(slope ** 2)], 1)


def _rowwise(make, fn=_fn):
    def build(ray_dtype):
        from tfrt.optimizer import RowwiseError
        eng, params, _ = make(ray_dtype)
        return eng, params, RowwiseError(fn)
    return build


def _run(make, mode, ray_dtype, steps=8, momentum=None, accumulators=None, setup=None):
    from tfrt.optimizer import SGD_Optimizer
    eng, params, erf = make(ray_dtype)
    if setup is not None:
        setup(eng)
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


# ------------------------------------------------------------------------- the optimiser
@pytest.mark.parametrize("ray_dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_fused_2d_rowwise_step_equals_the_generic_step(scene, ray_dtype):
    make = _rowwise(SCENES[scene])
    runs = [_run(make, mode, ray_dtype) for mode in ("generic", "eager", "graph")]
    generic, eager, graph = (r[2] for r in runs)
    assert generic._fused_step is None
    assert eager._fused_step is not None and eager._fused_step.steps == 8
    assert eager._fused_step.graph_replays == 0
    fs = graph._fused_step
    assert fs is not None and fs.steps == 8 and fs.graph_replays > 0
    assert fs.capture_error is None and not fs.untapped
    assert all(np.isfinite(runs[0][0]))
    _compare(runs, *TOLS[ray_dtype])
    # the ray sets of the last fused step are published on demand, like the generic path's
    fin_g = generic.engine.finished_rays["y_end"]
    fin_f = graph.engine.finished_rays["y_end"]
    assert fin_g.shape == fin_f.shape and fin_g.shape[0] > 0


def test_rowwise_2d_equals_the_goal_error_for_the_same_error():
    runs = [_run(_single_arc, "graph", torch.float64),
            _run(_rowwise(_single_arc, lambda r: r["y_end"] ** 2), "graph", torch.float64)]
    for r in runs:
        fs = r[2]._fused_step
        assert fs is not None and fs.capture_error is None and fs.graph_replays > 0
    (e0, h0, o0), (e1, h1, o1) = runs
    np.testing.assert_allclose(e1, e0, rtol=1e-13, atol=0)
    for a, b in zip(h0, h1):
        for x, y in zip(a, b):
            assert float((x - y).abs().max()) <= 1e-12
    # the same running test count as the goal route's
    assert int(o0._fused_step.tests_total) == int(o1._fused_step.tests_total) > 0


def test_fused_2d_rowwise_momentum_and_accumulator_equal_the_generic_step():
    k = 13
    acc = np.triu(np.ones((k, k))) * 0.5 + np.eye(k) * 0.5
    momentum = [0.6] * 4 + [0.9] * 4
    make = _rowwise(_segment_lens)
    runs = [_run(make, mode, torch.float64, momentum=momentum, accumulators=[acc, None])
            for mode in ("generic", "eager", "graph")]
    fs = runs[2][2]._fused_step
    assert fs.capture_error is None and fs.graph_replays >= 4
    _compare(runs, 1e-11, 1e-12)


def test_rowwise_2d_momentum_phase_change_replays_one_graph():
    from tfrt.optimizer import SGD_Optimizer
    eng, params, erf = _rowwise(_single_arc)(torch.float64)
    opt = SGD_Optimizer(eng, params, erf, 2, learning_rate=1.0, grad_clip=0.1,
                        sgd_learning_rate=1.0, apply_momentum=True)
    for _ in range(5):
        opt.single_step(None, momentum=0.8)
    g = opt._fused_step._graphs[1]
    replays = opt._fused_step.graph_replays
    for _ in range(3):
        opt.single_step(None, momentum=0.9, lr_scale=0.1)
    assert opt._fused_step._graphs[1] is g and opt._fused_step.graph_replays == replays + 3


def _with_custom_operation(eng):
    import tfrt.operation as operation

    class Passive(operation.RayOperation):
        """An operation with a main() of its own that adds no rays."""

        def main(self, engine, proj_result):
            return {}
    eng._operations = list(eng._operations) + [Passive()]
    assert eng._custom_ops()


def _with_ray_shard(eng):
    eng.ray_shard = (0, 1)


@pytest.mark.parametrize("setup", [_with_custom_operation, _with_ray_shard])
def test_rowwise_2d_with_a_custom_operation_or_ray_shards_stays_generic(setup):
    make = _rowwise(_segment_lens)
    runs = [_run(make, mode, torch.float64, setup=setup) for mode in ("generic", "graph")]
    assert runs[1][2]._fused_step is None
    assert all(np.isfinite(runs[0][0]))
    _compare(runs, *TOLS[torch.float64])      # (the generic sweep's atomics: last bits only)


def test_optimize_arc_example_rowwise_lowers_the_error_on_the_graph_path():
    import optimize_arc
    errors, s = optimize_arc.run(ray_count=50, steps=20, momentum=True, verbose=False,
                                 rowwise=True)
    fs = s["optimizer"]._fused_step
    assert fs is not None and fs.capture_error is None and fs.graph_replays >= 15
    assert min(errors[-5:]) < 0.5 * errors[0], errors


# ------------------------------------------------------------------------------- the C ABI
def _trace(src, scene, seg, arc, P, L=1.0):
    """tfrt_trace2d_forward into fresh buffers (the finished faces kept)."""
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
    _lib.check(lib.tfrt_trace2d_forward(
        ops._p(src), N, N, ctypes.byref(sc), L, 0.0, P, dt, _lib.COMPILE_FINISHED,
        *[ctypes.byref(o) for o in outs], None, None, ops._p(counts), ops._p(ws), wsb,
        ops._stream(src)), "tfrt_trace2d_forward")
    return dict(src=src, sc=sc, seg=seg, arc=arc, P=P, L=L, dt=dt, N=N, ws=ws, wsb=wsb,
                counts=counts, fin=fin, fid=fid, ffc=ffc, out=outs[0], capN=capN, Ms=Ms, Ma=Ma)


def _rows(t, pad=5):
    """tfrt_trace2d_rows into a block whose rows are `pad` entries longer than n_rays."""
    from tensorflowraytrace_amd import _lib, ops
    N = t["N"]
    rows = torch.full((4, N + pad), float("nan"), dtype=t["src"].dtype, device=DEV)
    face = torch.full((N + pad,), 7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().tfrt_trace2d_rows(
        ops._p(t["src"]), t["N"], N, t["P"], t["dt"], ctypes.byref(t["out"]), ops._p(rows),
        N + pad, ops._p(face), ops._p(t["counts"]), ops._p(t["ws"]), t["wsb"],
        ops._stream(t["src"])), "tfrt_trace2d_rows")
    torch.cuda.synchronize()
    return rows, face


def _backward_rows(t, terms, grad_rows):
    """tfrt_trace2d_backward_rows + tfrt_goal_finish; `terms` (n_terms, n_rays) error terms."""
    from tensorflowraytrace_amd import _lib, ops
    lib = _lib.lib()
    g_seg = torch.zeros((max(t["Ms"], 1), 4), dtype=torch.float64, device=DEV)
    g_arc = torch.zeros((max(t["Ma"], 1), 5), dtype=torch.float64, device=DEV)
    err = torch.zeros(3, dtype=torch.float64, device=DEV)
    tests = torch.zeros(1, dtype=torch.int64, device=DEV)
    gwb = lib.tfrt_trace2d_backward_goal_workspace_bytes(t["N"])
    gws = torch.zeros(gwb, dtype=torch.uint8, device=DEV)
    pending = _lib.GoalPending()
    st = ops._stream(t["src"])
    _lib.check(lib.tfrt_trace2d_backward_rows(
        ops._p(t["src"]), t["N"], t["N"], ctypes.byref(t["sc"]), t["L"], t["P"], t["dt"],
        ctypes.byref(t["out"]), ops._p(terms), terms.shape[0], terms.stride(0), terms.stride(1),
        None if grad_rows is None else ops._p(grad_rows),
        0 if grad_rows is None else grad_rows.shape[1], ops._p(err), ops._p(tests), ops._p(gws),
        gwb, ctypes.byref(pending), ops._p(g_seg) if t["Ms"] else None,
        ops._p(g_arc) if t["Ma"] else None, ops._p(t["counts"]), ops._p(t["ws"]), t["wsb"], st),
        "tfrt_trace2d_backward_rows")
    _lib.check(lib.tfrt_goal_finish(ctypes.byref(pending), st), "tfrt_goal_finish")
    torch.cuda.synchronize()
    return err, g_seg[:t["Ms"]], g_arc[:t["Ma"]], tests


def _bits(x):
    return x.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[x.element_size()])


def _check_rows_against_goal(t, goal_rows, goal):
    N, P = t["N"], t["P"]
    rows, face = _rows(t)
    counts = t["counts"].cpu().numpy()
    nf = int(counts[P * 8 + 1])
    fid = t["fid"][:nf].long()
    # the finished block scattered by finished_id, the source rays elsewhere, bit for bit
    want = t["src"].clone()
    want[:, fid] = t["fin"][:, :nf]
    assert torch.equal(_bits(rows[:, :N]), _bits(want))
    assert bool(torch.isnan(rows[:, N:].float()).all())          # nothing past n_rays
    want_face = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    want_face[fid] = t["ffc"][:nf]
    assert torch.equal(face[:N], want_face) and bool((face[N:] == 7).all())
    assert int((face[:N] >= 0).sum()) == nf
    # terms (out - goal)^2 and seeds 2 (out - goal) on the finished columns, NaN on the masked ones
    finished = face[:N] >= 0
    nan = torch.tensor(float("nan"), dtype=torch.float64, device=DEV)
    r = torch.stack([rows[k, :N].double() - goal[c] for c, k in enumerate(goal_rows)])
    terms = torch.where(finished, r ** 2, nan)
    g = torch.zeros((4, N + 3), dtype=torch.float64, device=DEV)
    for c, k in enumerate(goal_rows):
        g[k, :N] = 2.0 * r[c]
    g[:, :N] = torch.where(finished, g[:, :N], nan)
    err, g_seg, g_arc, tests = _backward_rows(t, terms, g)
    w_err, w_seg, w_arc, w_tests = _folded(t, goal_rows, goal)
    # the same terms in the same fixed order: the same error, bit for bit, and test count
    assert err.cpu().numpy().tobytes() == w_err.cpu().numpy().tobytes()
    assert int(tests) == int(w_tests)
    for x, y, what in ((g_seg, w_seg, "segment"), (g_arc, w_arc, "arc")):
        if x.numel() and float(torch.nan_to_num(y, nan=0.0).abs().max()) > 0:
            _same_grad(x, y, 1e-13, what)
        else:
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    # the (n_rays, n_terms) layout the optimiser passes gives the same sum; without seeds only the
    # NaN of totally reflected parent links can reach the gradients
    again = _backward_rows(t, terms.t().contiguous().t(), None)
    assert again[0].cpu().numpy().tobytes() == w_err.cpu().numpy().tobytes()
    for x in again[1:3]:
        assert float(torch.nan_to_num(x, nan=0.0).abs().sum()) == 0
    return nf


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16])
@pytest.mark.parametrize("finite_tir", [False, True])
@pytest.mark.parametrize("P", [1, 2, 4, 12, 24])
def test_rows_and_seeded_sweep_against_the_goal_kernel(P, finite_tir, dtype):
    rng = np.random.default_rng(200 + P)
    if P <= 4:
        sets, rays, wl = _scene(rng, 3001)                # (not a multiple of 64)
        scene, seg, arc = _gpu_scene(sets, wl)
        arc = arc["geo"]
        goal_rows = (2, 3)
    else:                                  # chains longer than a lane's 16 links in LDS
        sets, rays, wl = _guide(2001, rng)
        scene, seg, _ = _gpu_scene(sets, wl)
        arc = None
        goal_rows = (0, 1, 2, 3)
    scene.finite_tir_gradient = finite_tir
    src = torch.tensor(rays, dtype=dtype, device=DEV)
    t = _trace(src, scene, seg["geo"], arc, P)
    goal = torch.tensor(rng.normal(size=(len(goal_rows), src.shape[1])), dtype=torch.float64,
                        device=DEV)
    nf = _check_rows_against_goal(t, goal_rows, goal)
    if dtype != torch.float16:
        assert nf > 0


@pytest.mark.parametrize("finite_tir", [False, True])
def test_rows_route_against_oracle_autograd(finite_tir):
    """The rows route of a RowwiseError (tfrt_trace2d_rows -> fn on the columns, masked sum,
    autograd -> tfrt_trace2d_backward_rows) on the mixed scene, against oracle autograd of fn."""
    rng = np.random.default_rng(5)
    sets, rays, wl = _scene(rng, 3000)
    scene, seg, arc = _gpu_scene(sets, wl)
    scene.finite_tir_gradient = finite_tir
    src = torch.tensor(rays, dtype=torch.float64, device=DEV)
    P = 4
    t = _trace(src, scene, seg["geo"], arc["geo"], P)
    rows, face = _rows(t, pad=0)
    leaf = rows.detach().requires_grad_(True)
    fields = {name: leaf[k] for k, name in enumerate(("x_start", "y_start", "x_end", "y_end"))}
    fields["wavelength"] = torch.tensor(wl, dtype=torch.float64, device=DEV)
    e = _fn(fields)
    mask = (face >= 0).unsqueeze(1)
    g_rows, = torch.autograd.grad(e, [leaf], grad_outputs=mask.expand_as(e).double())
    out, g_seg, g_arc, _ = _backward_rows(t, e.detach().contiguous().t(), g_rows.contiguous())
    err = out[0]

    osets = {k: {f: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v)
                 for f, v in s.items()} for k, s in sets.items()}
    ref = tracer.ray_trace(_oracle_system(osets), _src2(rays, wl, False), max_iterations=P,
                           inherit=("wavelength", "ray_id"), finite_tir_gradient=finite_tir)
    rf = ref["finished"]
    rloss = _fn(rf).sum()
    assert int(mask.sum()) == rf["ray_id"].shape[0] > 0
    assert float(out[1]) == 2 * rf["ray_id"].shape[0]
    np.testing.assert_allclose(float(err), float(rloss.detach()), rtol=1e-9)
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


def test_rows_edge_cases():
    rng = np.random.default_rng(3)
    # no chain finishes (one pass of the guide: every ray meets a wall first), and P = 0
    sets, rays, wl = _guide(70, rng)
    scene, seg, _ = _gpu_scene(sets, wl)
    src = torch.tensor(rays, dtype=torch.float64, device=DEV)
    nan = torch.full((4, 70), float("nan"), dtype=torch.float64, device=DEV)
    for P in (0, 1):
        t = _trace(src, scene, seg["geo"], None, P)
        rows, face = _rows(t)
        assert torch.equal(rows[:, :70], src) and bool((face[:70] == -1).all())
        err, g_seg, _, _ = _backward_rows(t, nan[:2], nan)
        assert float(g_seg.abs().sum()) == 0
        assert float(err[0]) == 0 and float(err[1]) == 0 and math.isnan(float(err[2]))
    # n_rays = 0: nothing written
    t = _trace(src[:, :0].contiguous(), scene, seg["geo"], None, 3)
    rows, face = _rows(t)
    assert bool((face == 7).all()) and math.isnan(float(rows[0, 0]))
    err, g_seg, _, tests = _backward_rows(t, nan[:1, :0], None)
    assert float(err[0]) == 0 and float(err[1]) == 0 and float(g_seg.abs().sum()) == 0
