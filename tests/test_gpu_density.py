"""
DensityError on the GPU: tfrt_density_error (splat, bins, seed) against the numpy reference of
tests/density_error_reference.py, and the error on the optimiser's paths -- the fused, replayed 3-D
step against the generic one, the parameter gradient against the oracle, the fallbacks, 2-D.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import density_error_reference as dr
from test_density_error_host import _torch_objective
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}
COUNTS = (0, 1, 63, 64, 65, 1000, 4097)
ONE_FIELD = {(1, 1): 1, (4, 4): 4, (7, 3): 7, (64, 64): 64, (256, 256): 8192}    # bins with one field


@functools.lru_cache(maxsize=None)
def _reference(n, nx, ny, two, f32, masked):
    """The reference of one case, computed once and shared (never written to)."""
    x, y, mask = dr.points(n, np.float32 if f32 else np.float64)
    goal = dr.goal_of(nx, ny, two)
    return dr.density_error(x, y if two else None, goal, dr.DOMAIN if two else dr.DOMAIN[:1],
                            oob_weight=0.3, mask=mask if masked else None)


def _kernel(n, nx, ny, two, dtype, masked, variant=0, pad=3):
    """tfrt_density_error on the points of a case: the rows sit in a 6-row block (x in row 4, y in
    row 5) with ``pad`` spare columns; the gradient block starts out as NaN to show what is
    written."""
    from tensorflowraytrace_amd import ops
    x, y, mask = dr.points(n, NP_DTYPE[dtype])
    rows = torch.full((6, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[4, :n] = torch.tensor(x, device=DEV)
    rows[5, :n] = torch.tensor(y, device=DEV)
    goal = torch.tensor(dr.normalise(dr.goal_of(nx, ny, two)), device=DEV).contiguous()
    grid = ops.density_grid(dr.DOMAIN if two else dr.DOMAIN[:1], nx, ny if two else None)
    grad = torch.full((6, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    m = torch.tensor(mask, device=DEV) if masked else None
    err, grad, hq = ops.density_error(rows[:, :n], 4, 5 if two else -1, goal, grid, 0.3, mask=m,
                                      grad=grad[:, :n], variant=variant)
    torch.cuda.synchronize()
    return err.cpu().numpy(), grad.cpu().numpy(), hq.cpu().numpy(), (x, y, mask)


def _check(got, ref, two, masked):
    err, grad, hq, (x, y, mask) = got
    assert np.array_equal(hq, ref["Hq"])
    assert err[1] == 1.0 and err[0] == err[2]
    print(f"error {err[0]!r} reference {ref['error']!r} bound {dr.error_bound(ref):.3e}")
    assert abs(err[0] - ref["error"]) <= dr.error_bound(ref)
    tol = dr.gradient_bound(ref)
    gx, gy = grad[4], grad[5]
    print(f"gradient deviation {np.abs(gx - ref['grad_x']).max(initial=0.0):.3e} bound {tol:.3e}")
    assert np.abs(gx - ref["grad_x"]).max(initial=0.0) <= tol
    off = ~np.isfinite(x.astype(np.float64))
    if two:
        assert np.abs(gy - ref["grad_y"]).max(initial=0.0) <= tol
        off |= ~np.isfinite(y.astype(np.float64))
    else:
        assert np.isnan(gy).all()                # (one field: the entry owns one row)
    if masked:
        off |= mask < 0
    assert (gx[off] == 0.0).all() and (not two or (gy[off] == 0.0).all())
    assert np.isnan(grad[:4]).all()              # rows it does not own are never written


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nx,ny", dr.BINS, ids=lambda v: str(v))
def test_kernel_equals_the_reference(nx, ny, dtype):
    """Every count, two fields and one, with and without the mask.  (256, 256) takes the global
    atomics, every other grid the histogram in LDS."""
    f32 = dtype == torch.float32
    for n in COUNTS:
        for two in (True, False):
            bx, by = (nx, ny) if two else (ONE_FIELD[nx, ny], 1)
            for masked in (False, True):
                ref = _reference(n, bx, by, two, f32, masked)
                _check(_kernel(n, bx, by, two, dtype, masked), ref, two, masked)


@pytest.mark.parametrize("nx,ny", [(4, 4), (64, 64)])
def test_both_splat_variants_give_the_same_bits(nx, ny):
    ref = _reference(4097, nx, ny, True, False, True)
    lds = _kernel(4097, nx, ny, True, torch.float64, True, variant=1)
    glb = _kernel(4097, nx, ny, True, torch.float64, True, variant=2)
    _check(lds, ref, True, True)
    for a, b in zip(lds[:3], glb[:3]):
        assert a.tobytes() == b.tobytes()
    from tensorflowraytrace_amd import _lib
    with pytest.raises(_lib.TfrtError):
        _kernel(10, 256, 256, True, torch.float64, False, variant=1)


def test_contention_every_point_in_one_bin():
    """100,000 points in one bin of a 4 x 4 grid, at the same place: the exact integer sum."""
    from tensorflowraytrace_amd import ops
    n = 100_000
    (x0, x1), (y0, y1) = dr.DOMAIN
    px, py = x0 + 0.3 * (x1 - x0), y0 + 0.55 * (y1 - y0)
    rows = torch.empty((2, n), dtype=torch.float64, device=DEV)
    rows[0], rows[1] = px, py
    goal = torch.tensor(dr.normalise(dr.goal_of(4, 4)), device=DEV)
    grid = ops.density_grid(dr.DOMAIN, 4, 4)
    one = dr.density_error(np.array([px]), np.array([py]), dr.goal_of(4, 4), dr.DOMAIN)
    assert np.count_nonzero(one["Hq"]) == 4
    for variant in (1, 2):
        err, grad, hq = ops.density_error(rows, 0, 1, goal, grid, variant=variant)
        assert np.array_equal(hq.cpu().numpy(), one["Hq"] * n)
    # ... and all of it in ONE bin: a single bin takes every weight
    g1 = torch.ones((1, 1), dtype=torch.float64, device=DEV)
    err, grad, hq = ops.density_error(rows, 0, 1, g1, ops.density_grid(dr.DOMAIN, 1, 1))
    assert int(hq[0, 0]) == n * 2 ** 32 and float(err[0]) == 0.0
    assert not bool(grad.any())


def test_two_calls_give_the_same_bits():
    a = _kernel(4097, 64, 64, True, torch.float32, True)
    b = _kernel(4097, 64, 64, True, torch.float32, True)
    c = _kernel(4097, 256, 256, True, torch.float32, True)
    d = _kernel(4097, 256, 256, True, torch.float32, True)
    for p, q in ((a, b), (c, d)):
        for u, v in zip(p[:3], q[:3]):
            assert u.tobytes() == v.tobytes()


def test_bad_arguments():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_density_error_workspace_bytes(10, 0, 4) == 0
    assert L.tfrt_density_error_workspace_bytes(10, 512, 512) == 0
    assert L.tfrt_density_error_workspace_bytes(-1, 4, 4) == 0
    assert L.tfrt_density_error_workspace_bytes(0, 4, 4) > 0
    t = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, nx=4, ny=4, row_x=0, row_y=1, x1=1.0, sx=4.0, oob=0.0, ws=1 << 13, stride=8,
             variant=0, goal=p):
        return L.tfrt_density_error(p, stride, n, 1, None, row_x, row_y, goal, nx, ny, 0.0, x1, sx,
                                    0.0, 1.0, 4.0, oob, p, 8, p, p, variant, p, ws, None)
    for bad in (dict(n=-1), dict(nx=0), dict(nx=512, ny=512), dict(row_x=6), dict(row_y=0),
                dict(x1=0.0), dict(sx=0.0), dict(oob=-1.0), dict(stride=4), dict(variant=3),
                dict(goal=None), dict(row_y=-1), dict(n=1 << 31)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    assert call(n=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28


def _gauss16(gx, gy):
    return torch.exp(-(gx ** 2 + gy ** 2) / (2 * 0.5 ** 2))


def _make(n_rays, mode, ray_dtype=torch.float64, fields=("y_end", "z_end"), **engine_kw):
    """The lens of tests/test_gpu_rowwise.py's ``_make`` with a DensityError."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype, **engine_kw)
    erf = optimizer.DensityError(fields, _gauss16, DOMAIN_LENS, oob_weight=2.0 / n_rays, bins=16)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=0.05, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source)


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def test_fused_step_equals_the_generic_step():
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    tests/test_gpu_rowwise.py's fixed-shape-against-generic test; the step is one graph replay."""
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
    # the histogram of the last replayed step can be read afterwards: every finished ray inside
    # the domain carries weight 1
    erf = runs["graph"][0].error_function
    fin = runs["graph"][1].finished_rays
    y, z = fin["y_end"].double(), fin["z_end"].double()
    inside = int(((y.abs() <= 1.1) & (z.abs() <= 1.1)).sum())
    assert abs(int(erf.last_hq.sum()) - inside * 2 ** 32) <= 4 * inside


def test_goal_overwritten_in_place_is_seen_by_replays_and_another_goal_recaptures():
    opt, eng, lens, _ = _make(8192, "graph")
    _steps(opt, lens, 6)
    fs = opt._fused_step
    erf = opt.error_function
    assert fs.graph_replays > 0
    before, e_before = fs.graph_replays, float(opt.single_step(None))
    shifted = torch.roll(erf.goal, (3, -2), (0, 1))
    erf.goal.copy_(shifted)
    e_after = float(opt.single_step(None))
    assert fs.graph_replays == before + 2 and abs(e_after - e_before) > 1e-3 * e_before
    erf.goal = erf.goal.clone()                       # another buffer: not the captured one
    float(opt.single_step(None))
    assert fs.graph_replays == before + 2


@pytest.mark.parametrize("ray_dtype,tol", [(torch.float64, 1e-9), (torch.float32, 1e-5)],
                         ids=["f64", "f32"])
def test_parameter_gradient_equals_the_oracle(ray_dtype, tol):
    """4,096 rays, one step: d error / d parameters on the generic path and on the fused step's
    fixed-shape path against the oracle's float64 trace composed with the unquantised torch
    objective under autograd."""
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    opt, eng, lens, (system, target, source) = _make(4096, "eager", ray_dtype)
    erf = opt.error_function
    grads, err_sum, n_terms = opt.raw_gradient()
    assert n_terms == 1
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    if ray_dtype == torch.float32:
        for k in ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end"):
            src[k] = src[k].float().double()
    ref = tracer.ray_trace(osys, src, max_iterations=3, inherit=("wavelength", "object_coords"))
    y, z = ref["finished"]["y_end"], ref["finished"]["z_end"]
    # no finished ray within 1e-6 of a bin-centre line or of the domain's edge: floor and the
    # in / out decision are the same in float32 and float64
    for v, (lo, hi) in zip((y.detach().numpy(), z.detach().numpy()), DOMAIN_LENS):
        s = 16 / (hi - lo)
        u = (v - lo) * s - 0.5
        assert np.abs(u - np.round(u)).min() / s > 1e-6
        assert min(np.abs(v - lo).min(), np.abs(v - hi).min()) > 1e-6
    assert int(((y.abs() > 1.1) | (z.abs() > 1.1)).sum()) > 50       # the penalty takes part
    e = _torch_objective(y, z, erf.goal.cpu(), DOMAIN_LENS, erf.oob_weight)
    rg = torch.autograd.grad(e, q)
    e = e.detach()
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
    assert abs(float(err3[0]) - float(e)) <= 10 * tol * float(e) and float(err3[1]) == 1.0


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
    goal = dr.goal_of(9, 1, two=False)
    eng.optical_system.update()
    eng.ray_trace(4)
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    domain = ((float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))),)    # some rays outside
    erf = optimizer.DensityError(("y_end",), goal, domain, oob_weight=0.01)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    ref = dr.density_error(y, None, goal, domain, oob_weight=0.01)
    assert ref["n_penalised"] > 0 and ref["contributions"].sum() > 100
    assert np.array_equal(erf.last_hq.cpu().numpy(), ref["Hq"])
    assert abs(float(err_sum) - ref["error"]) <= dr.error_bound(ref)
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_illumination_example_with_a_density_error_lowers_the_error():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "illumination.py"),
                          "--density-error", "--rays", "8192", "--steps", "8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("density error: first")][-1]
    first, last = float(line.split()[3]), float(line.split()[6])
    assert last < first
