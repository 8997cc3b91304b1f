"""
FocusError on the GPU: tfrt_focus_error (clear, accumulate, solve, seed, finish) against the numpy
reference of tests/focus_error_reference.py, and the error on the optimiser's paths -- the fused,
replayed 3-D step against the generic one, a re-drawn source, the parameter gradient against the
oracle, a SumError, the fallbacks, 2-D, the example.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import focus_error_reference as fr
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float16}
COUNTS = (0, 1, 63, 64, 65, 1000, 20000)
LDS = 256                                   # ops.FOCUS_LDS_GROUPS (asserted below)
TWO_TRIPS = 512 * 4 * 256 + 37              # the second trip of both grid-stride loops


@functools.lru_cache(maxsize=None)
def _case(n, G, np_dtype, dim, masked, permuted):
    """The inputs and the reference of one case, computed once and shared (never written to)."""
    block, mask, group, perm = fr.rays(n, G, np_dtype, dim, permuted)
    ref = fr.focus_error(block.astype(np.float64) if np_dtype == np.float16 else block, group, G,
                         fr.DOMAIN, mask=mask if masked else None,
                         perm=perm if permuted else None)
    return block, mask, group, perm, ref


def _kernel(n, G, dtype, dim, masked, permuted, variant=0, pad=3):
    """tfrt_focus_error on a case: the block has ``pad`` spare columns; the gradient block starts
    out as NaN to show what is written."""
    from tensorflowraytrace_amd import ops
    block, mask, group, perm, _ = _case(n, G, NP_DTYPE[dtype], dim, masked, permuted)
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[:, :n] = torch.tensor(block, device=DEV)
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    err, _, acc, foci = ops.focus_error(
        rows[:, :n], torch.tensor(group, device=DEV), G, ops.focus_grid(fr.DOMAIN[:dim]),
        fr.MIN_DET, mask=torch.tensor(mask, device=DEV) if masked else None,
        perm=torch.tensor(perm, device=DEV) if permuted else None, dimension=dim,
        grad=grad[:, :n], variant=variant)
    torch.cuda.synchronize()
    return err.cpu().numpy(), grad.cpu().numpy(), acc.cpu().numpy(), foci.cpu().numpy()


def _check_focus(got, ref, n):
    err, grad, acc, foci = got
    assert np.array_equal(acc, ref["acc"])
    same = (foci.view(np.int64) == ref["table"].view(np.int64)) \
        | (np.isnan(foci) & np.isnan(ref["table"]))
    assert same.all(), f"foci that are not bit-equal: groups {np.nonzero(~same.all(axis=1))[0][:5]}"
    first = {}
    for row in range(grad.shape[0]):
        ok = grad[row, :n].view(np.int64) == ref["grad"][row].view(np.int64)
        if not ok.all():
            i = int(np.nonzero(~ok)[0][0])
            first[row] = (i, grad[row, i], ref["grad"][row, i])
    assert not first, f"gradient entries that are not bit-equal (index, kernel, reference): {first}"
    assert np.isnan(grad[:, n:]).all() and not np.isnan(grad[:, :n]).any()
    print(f"error {err[0]!r} reference {ref['error']!r} bound {fr.error_bound(ref):.3e}")
    assert err[1] == ref["terms"]
    assert abs(err[0] - ref["error"]) <= fr.error_bound(ref)
    if ref["terms"]:
        assert err[2] == err[0] / err[1]
    else:
        assert np.isnan(err[2]) and err[0] == 0.0


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("G", [3, LDS, LDS + 1])
def test_kernel_equals_the_reference(G, dtype, dim):
    """Every count, with and without mask and perm.  257 groups take the global atomics, fewer the
    table in LDS."""
    from tensorflowraytrace_amd import ops
    assert ops.FOCUS_LDS_GROUPS == LDS
    for n in COUNTS:
        for masked, permuted in ((False, False), (True, True)):
            ref = _case(n, G, NP_DTYPE[dtype], dim, masked, permuted)[4]
            _check_focus(_kernel(n, G, dtype, dim, masked, permuted), ref, n)


def test_the_second_trip_of_the_grid_stride_loops():
    """512 * 4 * 256 + 37 columns: the accumulate launch's 512 workgroups and the seed launch's
    2,048 each go round again."""
    ref = _case(TWO_TRIPS, 7, np.float32, 3, True, True)[4]
    assert ref["has"][-37:].sum() > 10
    _check_focus(_kernel(TWO_TRIPS, 7, torch.float32, 3, True, True), ref, TWO_TRIPS)


def test_both_accumulate_variants_and_repeated_calls_give_the_same_bits():
    ref = _case(20000, 64, np.float64, 3, True, True)[4]
    lds = _kernel(20000, 64, torch.float64, 3, True, True, variant=1)
    glb = _kernel(20000, 64, torch.float64, 3, True, True, variant=2)
    again = _kernel(20000, 64, torch.float64, 3, True, True, variant=0)
    _check_focus(lds, ref, 20000)
    for other in (glb, again):
        for a, b in zip(lds, other):
            assert a.tobytes() == b.tobytes()
    for G in (64, LDS + 1):
        a = _kernel(20000, G, torch.float32, 2, True, True)
        b = _kernel(20000, G, torch.float32, 2, True, True)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
    with pytest.raises(ValueError):
        _kernel(64, LDS + 1, torch.float64, 3, False, False, variant=1)


def test_float16_state_goes_through_the_same_dispatch():
    for dim in (2, 3):
        ref = _case(1025, 7, np.float16, dim, True, True)[4]
        assert ref["has"].sum() > 300
        _check_focus(_kernel(1025, 7, torch.float16, dim, True, True), ref, 1025)


def test_bad_arguments_are_refused_before_any_launch():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_focus_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_focus_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_focus_error_workspace_bytes(-1, 4) == 0
    assert L.tfrt_focus_error_workspace_bytes(0, 4) > 0
    t = torch.zeros(1 << 15, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, G=4, dim=3, x1=1.0, y1=1.0, z1=1.0, ws=1 << 17, stride=8, gstride=8, variant=0,
             group=p, dtype=1, pbits=40, n_source=8, acc=p, foci=p, min_det=1e-6):
        return L.tfrt_focus_error(p, stride, n, dtype, dim, None, group, n_source, None, G,
                                  0.0, x1, 0.0, y1, 0.0, z1, pbits, min_det, p, gstride, p, acc,
                                  foci, variant, p, ws, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(dim=1), dict(dim=4), dict(x1=0.0),
                dict(y1=float("nan")), dict(z1=-1.0), dict(stride=4), dict(gstride=4),
                dict(variant=3), dict(group=None), dict(n=1 << 31), dict(dtype=7),
                dict(G=LDS + 1, variant=1), dict(pbits=41), dict(pbits=0),
                dict(n=1 << 21, stride=1 << 21, gstride=1 << 21), dict(n_source=-1),
                dict(acc=None), dict(foci=None), dict(min_det=0.0)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    torch.cuda.synchronize()
    assert not t.any()                    # nothing was launched: nothing was written
    assert call(n=0) == 0
    torch.cuda.synchronize()


def test_reused_buffers_allocate_nothing():
    from tensorflowraytrace_amd import _lib, ops
    n, G = 20000, 64
    block, mask, group, perm, ref = _case(n, G, np.float32, 3, True, True)
    rows = torch.tensor(block, device=DEV)
    group, mask, perm = (torch.tensor(v, device=DEV) for v in (group, mask, perm))
    grad = torch.zeros((6, n), dtype=torch.float64, device=DEV)
    err = torch.zeros(3, dtype=torch.float64, device=DEV)
    acc = torch.zeros((G, 10), dtype=torch.int64, device=DEV)
    foci = torch.zeros((G, 4), dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.lib().tfrt_focus_error_workspace_bytes(n, G), dtype=torch.uint8,
                     device=DEV)
    grid = ops.focus_grid(fr.DOMAIN)

    def call():
        return ops.focus_error(rows, group, G, grid, fr.MIN_DET, mask=mask, perm=perm, grad=grad,
                               err=err, acc=acc, foci=foci, workspace=ws)
    call()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    got = call()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert got[0] is err and got[1] is grad and got[2] is acc and got[3] is foci
    assert np.array_equal(acc.cpu().numpy(), ref["acc"])


# ------------------------------------------------------------------------ the optimiser
# the target plane is x = 10; the lens' finished rays fill a disk of radius ~1.28 on it
BOX_LENS = ((9.0, 11.0), (-1.5, 1.5), (-1.5, 1.5))
MIN_DET_LENS = 1e-9


def _make(n_rays, mode, ray_dtype=torch.float64, random_rays=False, n_groups=37,
          sum_with_goal=False, **engine_kw):
    """The lens of tests/test_gpu_spot.py's ``_make`` with a FocusError over 37 groups."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype,
                                                    random_rays=random_rays, **engine_kw)
    groups = torch.arange(n_rays) % n_groups
    erf = focus = optimizer.FocusError(groups, BOX_LENS, min_det=MIN_DET_LENS)
    lr = 0.2 / n_rays            # (a sum over the rays, as the SpotError of tests/test_gpu_spot.py)
    if sum_with_goal:
        goal = optimizer.GoalError(("y_end", "z_end"), lambda src: -src["object_coords"][:, 1:])
        erf, lr = optimizer.SumError([focus, goal], reduce="mean"), 0.4
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source), focus


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def _finished_reference(eng, erf, n_groups=37):
    """The reference on the engine's finished rays, their source-ray indices and the labels."""
    fin = eng.finished_rays
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
    block = np.stack([fin[k].detach().cpu().numpy() for k in names])
    ids = eng.last_trace["finished_id"].cpu().numpy()
    return fr.focus_error(block, erf.labels.cpu().numpy(), n_groups, BOX_LENS,
                          min_det=MIN_DET_LENS, perm=ids), ids


def test_fused_step_equals_the_generic_step():
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    tests/test_gpu_spot.py's test of the same name; the step is one graph replay."""
    runs = {mode: _make(8192, mode) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 6) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert runs["generic"][0]._fused_step is None
    assert fs is not None and fs.in_place and fs.capture_error is None, fs and fs.capture_error
    assert fs.graph_replays > 0
    print("errors, generic:", out["generic"][0], "graph:", out["graph"][0])
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11
    assert abs(out["generic"][0][-1] - out["generic"][0][0]) > 1e-6 * out["generic"][0][0]
    # the records and the foci of the last replayed step can be read afterwards
    erf = runs["graph"][4]
    n_fin = runs["graph"][1].finished_rays["x_end"].shape[0]
    assert n_fin > 4000 and int(erf.last_acc[:, 0].sum()) == n_fin
    foci = erf.foci()
    assert foci.shape == (37, 3) and bool(torch.isfinite(foci).all())
    np.testing.assert_allclose(foci.cpu().numpy(), runs["generic"][4].foci().cpu().numpy(),
                               rtol=0, atol=1e-8)


def test_a_redrawn_source_keeps_its_labels_under_replay():
    """The source is re-drawn (and re-ordered) inside the graph at every step; the kernels look
    the labels up through the trace's order themselves: the records of the last replay equal the
    reference on that trace's finished rays, their source-ray indices and the labels."""
    opt, eng, lens, _, erf = _make(8192, "graph", random_rays=True)
    _steps(opt, lens, 5)
    fs = opt._fused_step
    # (five steps are one generic step, the eager warm-up and the capture: the first REPLAY is
    # the step after them, and a replay is what this test is about)
    for _ in range(4):
        if fs.graph_replays >= 2:
            break
        _steps(opt, lens, 1)
    assert fs is not None and fs.in_place and fs.graph_replays >= 2 and fs.capture_error is None
    acc = erf.last_acc.cpu().numpy().copy()
    foci = erf.foci().cpu().numpy().copy()
    ref, ids = _finished_reference(eng, erf)
    assert ref["terms"] > 4000 and len(set(ids.tolist())) == ids.shape[0]
    assert np.array_equal(acc, ref["acc"])
    assert np.array_equal(foci, ref["foci"])


def _torch_objective(block, label, n_groups):
    from test_focus_error_host import _torch_objective as objective
    return objective(block, label, n_groups, np.ones(n_groups, dtype=bool))


def test_parameter_gradient_equals_the_oracle():
    """4,096 rays, float64 state, one step: d error / d parameters on the generic path and on the
    fused step's fixed-shape path against the oracle's float64 trace composed with the plain torch
    objective (the foci differentiated through) under autograd, at the tolerance
    tests/test_gpu_spot.py uses for the same comparison."""
    tol = 1e-9
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    opt, eng, lens, (system, target, source), erf = _make(4096, "eager")
    grads, err_sum, n_terms = opt.raw_gradient()
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    src["focus_label"] = erf.labels.cpu().double()
    ref = tracer.ray_trace(osys, src, max_iterations=3,
                           inherit=("wavelength", "object_coords", "focus_label"))
    fin = ref["finished"]
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
    block = torch.stack([fin[k] for k in names])
    label = fin["focus_label"].long().numpy()
    assert n_terms == block.shape[1] > 2000
    # every finished ray ends inside the box, farther than 1e-6 from its faces
    for v, (lo, hi) in zip(block[3:].detach().numpy(), BOX_LENS):
        assert lo + 1e-6 < v.min() and v.max() < hi - 1e-6
    e = _torch_objective(block, label, 37)
    rg = torch.autograd.grad(e, q)
    e = e.detach()
    print(f"error {float(err_sum)!r} oracle {float(e)!r}")
    assert abs(float(err_sum) - float(e)) <= 10 * tol * float(e)

    def compare(got, what):
        for g, r in zip(got, rg):
            rel = float((g.cpu() - r).abs().max() / r.abs().max())
            print(f"{what}: parameter gradient rel err {rel:.2e}")
            assert rel < tol, what
    compare(grads, "generic")
    # (the generic trace above has shown that this source is traced in place)
    assert FusedStep.eligible(opt, (), {})
    fs = FusedStep(opt, graph=False)
    fused, err3 = fs._enqueue_gradient()
    torch.cuda.synchronize()
    assert fs.in_place
    compare(fused, "fused")
    assert abs(float(err3[0]) - float(e)) <= 10 * tol * float(e)
    assert float(err3[1]) == block.shape[1]


def test_float32_state_fused_equals_generic():
    """With float32 state the lever alpha / L inherits the direction's eps32 * max|coordinate| / L:
    the fused step is compared with the generic one, which runs the same kernels on the same
    float32 rows, not with the oracle -- at the tolerance tests/test_gpu_spot.py applies to float32
    state."""
    tol = 1e-5
    from tensorflowraytrace_amd.fused_step import FusedStep
    opt, eng, lens, _, erf = _make(4096, "eager", torch.float32)
    grads, err_sum, n_terms = opt.raw_gradient()
    assert FusedStep.eligible(opt, (), {})
    fs = FusedStep(opt, graph=False)
    fused, err3 = fs._enqueue_gradient()
    torch.cuda.synchronize()
    assert fs.in_place and float(err3[1]) == n_terms > 2000
    assert abs(float(err3[0]) - float(err_sum)) <= 10 * tol * float(err_sum)
    for g, f in zip(grads, fused):
        rel = float((g - f).abs().max() / g.abs().max())
        print(f"fused against generic: parameter gradient rel diff {rel:.2e}")
        assert rel < tol


def test_a_sum_with_a_goal_runs_fused_and_equals_the_generic_step():
    runs = {mode: _make(8192, mode, sum_with_goal=True) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 6) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert runs["generic"][0]._fused_step is None
    assert fs is not None and fs.in_place and fs.capture_error is None, fs and fs.capture_error
    assert fs.graph_replays > 0
    print("errors, generic:", out["generic"][0], "graph:", out["graph"][0])
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11
    fused, generic = (runs[m][0].error_function for m in ("graph", "generic"))
    np.testing.assert_allclose(fused.last_errors.cpu().numpy(), generic.last_errors.cpu().numpy(),
                               rtol=1e-10, atol=0)
    assert bool(torch.isfinite(runs["graph"][4].foci()).all())


@pytest.mark.parametrize("what", ["few_rays", "deterministic"])
def test_fallbacks_take_the_generic_path(what):
    n, kw = (2000, {}) if what == "few_rays" else (8192, dict(deterministic=True))
    runs = {mode: _make(n, mode, **kw) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 4) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert fs is None or fs.steps == 0
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11


def test_2d_engine_runs_on_the_generic_path_and_equals_the_reference():
    import tfrt.optimizer as optimizer
    from test_gpu_fused_2d import _segment_lens
    eng, params, _ = _segment_lens(torch.float64)
    eng.optical_system.update()
    eng.ray_trace(4)
    fin = eng.finished_rays
    x = fin["x_end"].detach().cpu().double().numpy()
    y = fin["y_end"].detach().cpu().double().numpy()
    n_source = eng.optical_system.sources["x_start"].shape[0]
    # a box around the finished rays' ends that leaves some of them outside
    box = ((float(x.min()) - 1.0, float(x.max()) + 1.0),
           (float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))))
    groups = np.arange(n_source) % 9
    erf = optimizer.FocusError(groups, box, min_det=MIN_DET_LENS)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    fin = eng.finished_rays
    block = np.stack([fin[k].detach().cpu().double().numpy()
                      for k in ("x_start", "y_start", "x_end", "y_end")])
    ids = eng.last_trace["finished_id"].cpu().numpy()
    ref = fr.focus_error(block, groups, 9, box, min_det=MIN_DET_LENS, perm=ids)
    assert 100 < ref["terms"] < block.shape[1] == n_terms
    assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
    assert np.array_equal(erf.foci().cpu().numpy(), ref["foci"], equal_nan=True)
    assert abs(float(err_sum) - ref["error"]) <= fr.error_bound(ref)
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_imaging_example_with_a_focus_error_lowers_its_error():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "imaging.py"), "--focus",
                          "--rays", "8192", "--steps", "8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("focus error: first")][-1]
    first, last = float(line.split()[3]), float(line.split()[5])
    assert last < first
    assert any(ln.startswith("foci of") and "spread" in ln for ln in out.stdout.splitlines())
