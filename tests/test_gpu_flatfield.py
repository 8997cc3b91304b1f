"""
FlatFieldError on the GPU: tfrt_flatfield_error (clear, FocusError's accumulate, fit, seed)
against the numpy reference of tests/flatfield_error_reference.py -- records equal as integers;
table, plane, gradient and error bit for bit --, and the error on the optimiser's paths: the
fused, replayed 3-D step against the generic one, a re-drawn source, a SumError with a FocusError,
the fallbacks, 2-D, the example, the parameter gradient against the oracle.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flatfield_error_reference as ff
from test_flatfield_error_host import check, has_plane, quantisation_difference, same_bits, \
    torch_objective
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
    return ff.case(n, G, np_dtype, dim, permuted, masked, plane=has_plane(n, G))


def _kernel(n, G, dtype, dim, masked, permuted, variant=0, pad=3):
    """tfrt_flatfield_error on a case: the block has ``pad`` spare columns; the gradient block
    starts out as NaN to show what is written."""
    from tensorflowraytrace_amd import ops
    block, mask, group, perm, _ = _case(n, G, NP_DTYPE[dtype], dim, masked, permuted)
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[:, :n] = torch.tensor(block, device=DEV)
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    err, _, acc, table, fit = ops.flatfield_error(
        rows[:, :n], torch.tensor(group, device=DEV), G, ops.focus_grid(ff.DOMAIN[:dim]),
        ff.AXIS3 if dim == 3 else ff.AXIS2, ff.MIN_DET,
        mask=torch.tensor(mask, device=DEV) if masked else None,
        perm=torch.tensor(perm, device=DEV) if permuted else None, dimension=dim,
        grad=grad[:, :n], variant=variant)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (err, grad, acc, table, fit)]


def _check_kernel(got, ref, n):
    err, grad, acc, table, fit = got
    assert np.isnan(grad[:, n:]).all() and not np.isnan(grad[:, :n]).any()
    print(f"error {err[0]!r} reference {ref['error']!r} terms {err[1]} used {fit[3]}")
    check([err, grad[:, :n], acc, table, fit], ref)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("G", [3, LDS, LDS + 1])
def test_kernel_equals_the_reference(G, dtype, dim):
    """Every count, with and without mask and perm.  257 groups take the global atomics, fewer the
    table in LDS; the counts below G have no plane."""
    from tensorflowraytrace_amd import ops
    assert ops.FOCUS_LDS_GROUPS == LDS
    for n in COUNTS:
        for masked, permuted in ((False, False), (True, True)):
            ref = _case(n, G, NP_DTYPE[dtype], dim, masked, permuted)[4]
            _check_kernel(_kernel(n, G, dtype, dim, masked, permuted), ref, n)


def test_the_third_trip_of_the_threads_over_the_groups():
    """2,100 groups: the 1,024 threads of the fit go round the groups three times."""
    ref = _case(5000, 2100, np.float64, 3, True, True)[4]
    assert ref["used"][2048:].sum() > 2
    _check_kernel(_kernel(5000, 2100, torch.float64, 3, True, True), ref, 5000)


def test_the_second_trip_of_the_grid_stride_loops():
    """512 * 4 * 256 + 37 columns: the accumulate launch's 512 workgroups and the seed launch's
    2,048 each go round again."""
    ref = _case(TWO_TRIPS, 7, np.float32, 3, True, True)[4]
    assert ref["has"][-37:].sum() > 10
    _check_kernel(_kernel(TWO_TRIPS, 7, torch.float32, 3, True, True), ref, TWO_TRIPS)


def test_both_accumulate_variants_and_repeated_calls_give_the_same_bits():
    ref = _case(20000, 64, np.float64, 3, True, True)[4]
    lds = _kernel(20000, 64, torch.float64, 3, True, True, variant=1)
    glb = _kernel(20000, 64, torch.float64, 3, True, True, variant=2)
    again = _kernel(20000, 64, torch.float64, 3, True, True, variant=0)
    _check_kernel(lds, ref, 20000)
    for other in (glb, again):
        for a, b in zip(lds, other):
            assert a.tobytes() == b.tobytes()
    for G in (64, LDS + 1):
        a = _kernel(20000, G, torch.float32, 2, True, True)
        b = _kernel(20000, G, torch.float32, 2, True, True)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
    with pytest.raises(ValueError):
        _kernel(1000, LDS + 1, torch.float64, 3, False, False, variant=1)


def test_float16_state_goes_through_the_same_dispatch():
    for dim in (2, 3):
        ref = _case(1025, 7, np.float16, dim, True, True)[4]
        assert ref["has"].sum() > 300
        _check_kernel(_kernel(1025, 7, torch.float16, dim, True, True), ref, 1025)


def test_bad_arguments_are_refused_before_any_launch():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_flatfield_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_flatfield_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_flatfield_error_workspace_bytes(-1, 4) == 0
    assert L.tfrt_flatfield_error_workspace_bytes(0, 4) > 0
    t = torch.zeros(1 << 15, dtype=torch.float64, device=DEV)
    p = t.data_ptr()
    assert p % 64 == 0

    def call(n=8, G=4, dim=3, x1=1.0, y1=1.0, z1=1.0, ws=1 << 17, stride=8, gstride=8, variant=0,
             group=p, dtype=1, pbits=40, n_source=8, acc=p, table=p, fit=p, min_det=1e-6,
             axis=(0.6, 0.0, 0.8)):
        return L.tfrt_flatfield_error(p, stride, n, dtype, dim, None, group, n_source, None, G,
                                      0.0, x1, 0.0, y1, 0.0, z1, pbits, min_det, *axis, p, gstride,
                                      p, acc, table, fit, variant, p, ws, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(dim=1), dict(dim=4), dict(x1=0.0),
                dict(y1=float("nan")), dict(z1=-1.0), dict(stride=4), dict(gstride=4),
                dict(variant=3), dict(group=None), dict(n=1 << 31), dict(dtype=7),
                dict(G=LDS + 1, variant=1), dict(pbits=41), dict(pbits=0),
                dict(n=1 << 21, stride=1 << 21, gstride=1 << 21), dict(n_source=-1),
                dict(acc=None), dict(table=None), dict(fit=None), dict(min_det=0.0),
                dict(table=p + 8), dict(table=p + 32), dict(axis=(0.0, 0.0, 0.0)),
                dict(axis=(1.0, 0.0, 1e-6)), dict(axis=(float("nan"), 0.0, 1.0)),
                dict(dim=2, axis=(0.6, 0.0, 0.8))):
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
    table = torch.zeros((G, 8), dtype=torch.float64, device=DEV)
    fit = torch.zeros(8, dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.lib().tfrt_flatfield_error_workspace_bytes(n, G), dtype=torch.uint8,
                     device=DEV)
    grid = ops.focus_grid(ff.DOMAIN)

    def call():
        return ops.flatfield_error(rows, group, G, grid, ff.AXIS3, ff.MIN_DET, mask=mask,
                                   perm=perm, grad=grad, err=err, acc=acc, table=table,
                                   fit_out=fit, workspace=ws)
    call()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    got = call()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert got[0] is err and got[1] is grad and got[2] is acc and got[3] is table \
        and got[4] is fit
    check([t.cpu().numpy() for t in got], ref)


# ------------------------------------------------------------------------ the optimiser
# the lens, the box and min_det of tests/test_gpu_focus.py
BOX_LENS = ((9.0, 11.0), (-1.5, 1.5), (-1.5, 1.5))
MIN_DET_LENS = 1e-9
AXIS_LENS = (1.0, 0.0, 0.0)


def _make(n_rays, mode, ray_dtype=torch.float64, random_rays=False, n_groups=37,
          sum_with_focus=False, **engine_kw):
    """The lens of tests/test_gpu_focus.py's ``_make`` with a FlatFieldError over 37 groups."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype,
                                                    random_rays=random_rays, **engine_kw)
    groups = torch.arange(n_rays) % n_groups
    erf = flat = optimizer.FlatFieldError(groups, BOX_LENS, axis=AXIS_LENS,
                                          min_det=MIN_DET_LENS)
    lr = 0.2 / n_rays            # (a sum over the rays, as the FocusError of tests/test_gpu_focus.py)
    if sum_with_focus:
        focus = optimizer.FocusError(groups, BOX_LENS, min_det=MIN_DET_LENS)
        erf, lr = optimizer.SumError([focus, flat], reduce="mean"), 0.2
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source), flat


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def _finished_reference(eng, erf, n_groups=37):
    """The reference on the engine's finished rays, their source-ray indices and the labels."""
    fin = eng.finished_rays
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
    block = np.stack([fin[k].detach().cpu().numpy() for k in names])
    ids = eng.last_trace["finished_id"].cpu().numpy()
    return ff.flatfield_error(block, erf.labels.cpu().numpy(), n_groups, BOX_LENS, AXIS_LENS,
                              min_det=MIN_DET_LENS, perm=ids), ids


def test_fused_step_equals_the_generic_step():
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    tests/test_gpu_focus.py's test of the same name; the step is one graph replay; the plane and
    the residuals of the last replayed step can be read afterwards."""
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
    erf = runs["graph"][4]
    n_fin = runs["graph"][1].finished_rays["x_end"].shape[0]
    assert n_fin > 4000 and int(erf.last_acc[:, 0].sum()) == n_fin
    plane = erf.plane()
    assert plane["valid"] and plane["groups_used"] == 37 and plane["axis"] == AXIS_LENS
    assert np.isfinite(plane["offset"])
    r = erf.residuals()
    assert r.shape == (37,) and bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0.0
    h = erf.heights()
    np.testing.assert_allclose((h - plane["offset"]).cpu().numpy(), r.cpu().numpy(), rtol=0,
                               atol=1e-12)
    np.testing.assert_allclose(r.cpu().numpy(), runs["generic"][4].residuals().cpu().numpy(),
                               rtol=0, atol=1e-8)


def test_a_redrawn_source_keeps_its_labels_under_replay():
    """The source is re-drawn (and re-ordered) inside the graph at every step; the kernels look
    the labels up through the trace's order themselves: the records, the table and the plane of
    the last replay equal the reference on that trace's finished rays."""
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
    table = erf.last_table.cpu().numpy().copy()
    fit = erf.last_fit.cpu().numpy().copy()
    ref, ids = _finished_reference(eng, erf)
    assert ref["terms"] > 4000 and len(set(ids.tolist())) == ids.shape[0] and ref["valid"]
    assert np.array_equal(acc, ref["acc"])
    assert same_bits(table, ref["table"]) and same_bits(fit, ref["fit"])


def test_a_sum_with_a_focus_error_runs_fused_and_equals_the_generic_step():
    runs = {mode: _make(8192, mode, sum_with_focus=True) for mode in ("generic", "graph")}
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
    focus, flat = fused.terms
    # both terms fill the same records
    assert torch.equal(focus.last_acc, flat.last_acc) and runs["graph"][4].plane()["valid"]
    assert torch.equal(focus.foci(), flat.foci())


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
    # the generic path's numbers are the reference's on the last trace
    opt, eng, _, _, erf = runs["graph"]
    _, err_sum, n_terms = opt.raw_gradient()
    ref, _ = _finished_reference(eng, erf)
    assert float(err_sum) == ref["error"] or \
        abs(float(err_sum) - ref["error"]) <= n_terms * ff.EPS * ref["error"]
    assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
    assert same_bits(erf.last_table.cpu().numpy(), ref["table"])


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
    erf = optimizer.FlatFieldError(groups, box, min_det=MIN_DET_LENS)
    assert erf.axis == (1.0, 0.0)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    fin = eng.finished_rays
    block = np.stack([fin[k].detach().cpu().double().numpy()
                      for k in ("x_start", "y_start", "x_end", "y_end")])
    ids = eng.last_trace["finished_id"].cpu().numpy()
    ref = ff.flatfield_error(block, groups, 9, box, (1.0, 0.0), min_det=MIN_DET_LENS, perm=ids)
    assert 100 < ref["terms"] < block.shape[1] == n_terms and ref["valid"]
    assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
    assert same_bits(erf.last_table.cpu().numpy(), ref["table"])
    assert same_bits(erf.last_fit.cpu().numpy(), ref["fit"])
    assert same_bits(erf.residuals().cpu().numpy(), ref["residuals"])
    assert abs(float(err_sum) - ref["error"]) <= n_terms * ff.EPS * ref["error"]
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_imaging_example_with_a_flat_field_lowers_the_spread_of_the_foci():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "imaging.py"),
                          "--flat-field", "--rays", "8192", "--steps", "8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines()
            if ln.startswith("spread of the foci along the axis: first")][-1]
    first, last = float(line.split()[8]), float(line.split()[10])
    assert last < first
    assert any(ln.startswith("plane of the foci: offset") for ln in out.stdout.splitlines())
    refused = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "imaging.py"),
                              "--flat-field", "--distortion"], capture_output=True, text=True,
                             timeout=600)
    assert refused.returncode == 2 and "--flat-field" in refused.stderr


def test_parameter_gradient_equals_the_oracle():
    """4,096 rays, float64 state, one step: d error / d parameters on the generic path and on the
    fused step's fixed-shape path against the oracle's float64 trace composed with the plain torch
    objective (the foci differentiated through ``torch.linalg.solve``) under autograd.  The
    tolerance is the 1e-9 of tests/test_gpu_focus.py's comparison, or 8 x the quantisation
    difference measured on the CPU between the numpy reference and the plain objective on the
    oracle's own finished rays, whichever is larger.  Measured: that difference is 3.938e-10 on
    the rays' gradient (1.426e-11 on the error), so the tolerance is 3.150e-09; the parameter
    gradients were off by 3.51e-10 and 2.92e-10 on both paths."""
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
    quant, quant_e = quantisation_difference(block.detach().numpy(), label, 37, BOX_LENS,
                                             AXIS_LENS, MIN_DET_LENS)
    tol = max(1e-9, 8 * quant)
    print(f"quantisation difference on the oracle's rays: gradient {quant:.3e} error "
          f"{quant_e:.3e}; tolerance {tol:.3e}")
    e = torch_objective(block, label, 37, np.ones(37, dtype=bool), AXIS_LENS)
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
