"""
DistortionError on the GPU: tfrt_distortion_error (clear, SpotError's accumulate, fit, seed)
against the numpy reference of tests/distortion_error_reference.py, and the error on the
optimiser's paths -- the fused, replayed 3-D step against the generic one, a re-drawn source, the
parameter gradient against the oracle, a SumError with a SpotError, the fallbacks, 2-D, the
example.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import direction_fields_reference as dfr
import distortion_error_reference as dr
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float16}
COUNTS = (0, 1, 63, 64, 65, 1000, 20000)
LDS = 1024                                  # ops.SPOT_LDS_GROUPS (asserted below)
TWO_TRIPS = 512 * 4 * 256 + 37              # the second trip of both grid-stride loops


@functools.lru_cache(maxsize=None)
def _case(n, G, np_dtype, two, fit, masked, permuted):
    """The inputs and the reference of one case, computed once and shared (never written to)."""
    x, y, mask, group, perm, points = dr.rays(n, G, np_dtype, permuted)
    points = points if two else np.ascontiguousarray(points[:, :1])
    ref = dr.distortion_error(x.astype(np.float64), y.astype(np.float64) if two else None, group,
                              G, points, dr.DOMAIN if two else dr.DOMAIN[:1], fit=fit,
                              oob_weight=dr.OOB, mask=mask if masked else None,
                              perm=perm if permuted else None)
    if n >= 1000:
        dr.assert_generator(ref)
    return x, y, mask, group, perm, points, ref


def _kernel(n, G, dtype, dim, two, fit, masked, permuted, variant=0, pad=3):
    """tfrt_distortion_error on a case: x and y are the end rows of a ``dim``-D block with ``pad``
    spare columns; the gradient block starts out as NaN to show what is written."""
    from tensorflowraytrace_amd import ops
    x, y, mask, group, perm, points, _ = _case(n, G, NP_DTYPE[dtype], two, fit, masked, permuted)
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[dim, :n] = torch.tensor(x, device=DEV)
    rows[dim + 1, :n] = torch.tensor(y, device=DEV)
    g = torch.tensor(group, device=DEV)
    grid = ops.spot_grid(dr.DOMAIN if two else dr.DOMAIN[:1], ops.spot_qbits(g.numel()))
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    err, _, acc, fit_out, residual = ops.distortion_error(
        rows[:, :n], dim, dim + 1 if two else -1, g, G, torch.tensor(points, device=DEV), grid,
        fit=fit, oob_weight=dr.OOB, mask=torch.tensor(mask, device=DEV) if masked else None,
        perm=torch.tensor(perm, device=DEV) if permuted else None, grad=grad[:, :n],
        variant=variant, dimension=dim)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (err, grad, acc, fit_out, residual))


def _bits_equal(a, b):
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _check(got, ref, n, want_grad):
    """``want_grad``: {row: reference gradient row}; every other row must be untouched."""
    err, grad, acc, fit_out, residual = got
    assert np.array_equal(acc, ref["acc"])
    assert _bits_equal(fit_out, ref["fit_out"]).all(), (fit_out, ref["fit_out"])
    same = _bits_equal(residual, ref["residual"])
    assert same.all(), f"residuals not bit-equal: groups {np.nonzero(~same.all(axis=1))[0][:5]}"
    first = {}
    for row in range(grad.shape[0]):
        if row not in want_grad:
            assert np.isnan(grad[row]).all(), row
            continue
        ok = grad[row, :n].view(np.int64) == want_grad[row].view(np.int64)
        if not ok.all():
            i = int(np.nonzero(~ok)[0][0])
            first[row] = (i, grad[row, i], want_grad[row][i])
    assert not first, f"gradient entries that are not bit-equal (index, kernel, reference): {first}"
    assert np.isnan(grad[:, n:]).all()
    print(f"error {err[0]!r} reference {ref['error']!r} bound {dr.error_bound(ref):.3e}")
    assert err[1] == ref["terms"]
    assert abs(err[0] - ref["error"]) <= dr.error_bound(ref)
    if ref["terms"]:
        assert err[2] == err[0] / err[1]
    else:
        assert np.isnan(err[2]) and err[0] == 0.0


def _rows_of(ref, dim):
    want = {dim: ref["grad_x"]}
    if ref["grad_y"] is not None:
        want[dim + 1] = ref["grad_y"]
    return want


@pytest.mark.parametrize("fit", ["scale", "affine"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("G", [3, LDS, LDS + 1, 2049])
def test_kernel_equals_the_reference(G, dtype, dim, fit):
    """Every count, two fields and one, with and without mask and perm.  1,025 groups take the
    global atomics, fewer the table in LDS; with 2,049 the fit's per-thread loop takes a third
    trip."""
    from tensorflowraytrace_amd import ops
    assert ops.SPOT_LDS_GROUPS == LDS and ops.DISTORTION_BLOCK == dr.BLOCK == 1024
    for n in COUNTS:
        for two in (True, False):
            for masked, permuted in ((False, False), (True, True)):
                ref = _case(n, G, NP_DTYPE[dtype], two, fit, masked, permuted)[6]
                _check(_kernel(n, G, dtype, dim, two, fit, masked, permuted), ref, n,
                       _rows_of(ref, dim))


def test_the_second_trip_of_the_grid_stride_loops():
    """512 * 4 * 256 + 37 columns: the accumulate launch's 512 workgroups and the seed launch's
    2,048 each go round again."""
    ref = _case(TWO_TRIPS, 7, np.float32, True, "affine", True, True)[6]
    assert ref["inside"][-37:].sum() > 10
    _check(_kernel(TWO_TRIPS, 7, torch.float32, 3, True, "affine", True, True), ref, TWO_TRIPS,
           _rows_of(ref, 3))


def test_both_accumulate_variants_and_repeated_calls_give_the_same_bytes():
    ref = _case(20000, 64, np.float64, True, "affine", True, True)[6]
    lds = _kernel(20000, 64, torch.float64, 3, True, "affine", True, True, variant=1)
    glb = _kernel(20000, 64, torch.float64, 3, True, "affine", True, True, variant=2)
    again = _kernel(20000, 64, torch.float64, 3, True, "affine", True, True, variant=0)
    _check(lds, ref, 20000, _rows_of(ref, 3))
    for other in (glb, again):
        for a, b in zip(lds, other):
            assert a.tobytes() == b.tobytes()
    for G in (64, 2049):
        a = _kernel(20000, G, torch.float32, 2, True, "scale", True, True)
        b = _kernel(20000, G, torch.float32, 2, True, "scale", True, True)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
    with pytest.raises(ValueError):
        _kernel(64, LDS + 1, torch.float64, 3, True, "scale", False, False, variant=1)


def test_float16_state_goes_through_the_same_dispatch():
    for dim in (2, 3):
        ref = _case(1025, 7, np.float16, True, "scale", True, True)[6]
        assert ref["n_inside"] > 300 and ref["valid"]
        _check(_kernel(1025, 7, torch.float16, dim, True, "scale", True, True), ref, 1025,
               _rows_of(ref, dim))


@pytest.mark.parametrize("fit", ["scale", "affine"])
def test_a_direction_field_is_chained_onto_every_row(fit):
    """(y_dir, z_dir) of a 3-D block: the centroids are mean direction cosines, and the seed
    writes all six rows of every column through the chain rule of direction_fields.h."""
    from tensorflowraytrace_amd import ops
    n, G, codes = 1000, 7, (7, 8)
    block = dfr.rays(n, np.float64)
    rng = np.random.default_rng(3)
    group = rng.integers(0, G - 1, n + 3).astype(np.int32)
    mask = np.where(np.arange(n) % 5 == 4, -1, 0).astype(np.int32)
    points = dr.object_points(G)
    vals, d, L, ok = dfr.field_values(block, codes)
    ref = dr.distortion_error(vals[0], vals[1], group, G, points, dfr.DOMAIN, fit=fit,
                              oob_weight=dr.OOB, mask=mask)
    assert ref["valid"] and ref["n_inside"] > 200 and ref["n_penalised"] > 50
    counts = ref["inside"] | ref["outside"]
    want = np.where(counts[None, :], dfr.chain([ref["grad_x"], ref["grad_y"]], codes, d, L, ok),
                    0.0)
    grad = torch.full((6, n + 3), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.tensor(group, device=DEV)
    out = ops.distortion_error(
        torch.tensor(block, device=DEV), 7, 8, g, G, torch.tensor(points, device=DEV),
        ops.spot_grid(dfr.DOMAIN, ops.spot_qbits(g.numel())), fit=fit, oob_weight=dr.OOB,
        mask=torch.tensor(mask, device=DEV), grad=grad[:, :n], dimension=3)
    torch.cuda.synchronize()
    got = (out[0].cpu().numpy(), grad.cpu().numpy()) + tuple(t.cpu().numpy() for t in out[2:])
    _check(got, ref, n, {row: want[row] for row in range(6)})


def test_an_invalid_fit_gives_zero_gradients_and_keeps_the_penalties():
    """One used group (scale) and collinear object points (affine): no valid fit; the rays inside
    get zeros, the rays outside keep their penalty and its gradient."""
    from tensorflowraytrace_amd import ops
    n, G = 1000, 7
    x, y, mask, group, perm, points, _ = _case(n, G, np.float64, True, "scale", False, False)
    line = np.stack([points[:, 0], 2.0 * points[:, 0]], axis=1)
    for fit, grp, pts in (("scale", np.zeros_like(group), points), ("affine", group, line)):
        ref = dr.distortion_error(x, y, grp, G, pts, dr.DOMAIN, fit=fit, oob_weight=dr.OOB)
        assert not ref["valid"] and ref["n_inside"] > 500 and ref["n_penalised"] > 20
        assert not ref["grad_x"][ref["inside"]].any() and ref["grad_x"][ref["outside"]].any()
        rows = torch.zeros((6, n), dtype=torch.float64, device=DEV)
        rows[4], rows[5] = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
        g = torch.tensor(grp, device=DEV)
        grad = torch.full((6, n), float("nan"), dtype=torch.float64, device=DEV)
        out = ops.distortion_error(rows, 4, 5, g, G, torch.tensor(pts, device=DEV),
                                   ops.spot_grid(dr.DOMAIN, ops.spot_qbits(g.numel())), fit=fit,
                                   oob_weight=dr.OOB, grad=grad)
        torch.cuda.synchronize()
        got = tuple(t.cpu().numpy() for t in out)
        _check(got, ref, n, _rows_of(ref, 4))
        assert got[3][6] == 0.0 and np.isnan(got[3][:6]).all()
        assert not got[4][ref["acc"][:, 0] > 0].any()


def test_bad_arguments_are_refused_before_any_launch():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_distortion_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_distortion_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_distortion_error_workspace_bytes(-1, 4) == 0
    assert L.tfrt_distortion_error_workspace_bytes(0, 4) > 0
    t = torch.zeros(1 << 15, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, G=4, dim=3, fx=4, fy=5, x1=1.0, qsx=4.0, oob=0.0, ws=1 << 17, stride=8,
             gstride=8, variant=0, group=p, qbits=40, n_source=8, points=p, fit=0, min_cond=1e-9,
             fit_out=p, residual=p, acc=p, err=p, dtype=1):
        return L.tfrt_distortion_error(p, stride, n, dtype, dim, None, fx, fy, group, n_source,
                                       None, G, points, fit, min_cond, 0.0, x1, qsx, 0.0, 1.0, 4.0,
                                       qbits, oob, p, gstride, err, fit_out, residual, acc, variant,
                                       p, ws, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(dim=1), dict(dim=4), dict(fx=9),
                dict(fy=4), dict(dim=2, fx=6), dict(x1=0.0), dict(qsx=0.0), dict(oob=-1.0),
                dict(stride=4), dict(gstride=4), dict(variant=3), dict(group=None),
                dict(n=1 << 31), dict(qbits=53), dict(qbits=0), dict(dtype=7),
                dict(n=1 << 22, stride=1 << 22, gstride=1 << 22), dict(G=LDS + 1, variant=1),
                dict(n_source=-1), dict(points=None), dict(fit=2), dict(fit=-1),
                dict(min_cond=-1.0), dict(min_cond=float("nan")), dict(fit_out=None),
                dict(residual=None), dict(residual=p + 8), dict(acc=None), dict(err=None)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    torch.cuda.synchronize()
    assert not t.any()                    # nothing was launched: nothing was written
    assert call(n=0) == 0
    torch.cuda.synchronize()


def test_reused_buffers_allocate_nothing():
    from tensorflowraytrace_amd import _lib, ops
    n, G = 20000, 64
    x, y, mask, group, perm, points, ref = _case(n, G, np.float32, True, "affine", True, True)
    rows = torch.zeros((6, n), dtype=torch.float32, device=DEV)
    rows[4], rows[5] = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    group, mask, perm, points = (torch.tensor(v, device=DEV) for v in (group, mask, perm, points))
    grad = torch.zeros((6, n), dtype=torch.float64, device=DEV)
    err = torch.zeros(3, dtype=torch.float64, device=DEV)
    acc = torch.zeros((G, 4), dtype=torch.int64, device=DEV)
    fit_out = torch.zeros(8, dtype=torch.float64, device=DEV)
    residual = torch.zeros((G, 2), dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.lib().tfrt_distortion_error_workspace_bytes(n, G), dtype=torch.uint8,
                     device=DEV)
    grid = ops.spot_grid(dr.DOMAIN, ops.spot_qbits(group.numel()))

    def call():
        return ops.distortion_error(rows, 4, 5, group, G, points, grid, fit="affine",
                                    oob_weight=dr.OOB, mask=mask, perm=perm, grad=grad, err=err,
                                    acc=acc, fit_out=fit_out, residual=residual, workspace=ws)
    call()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    got = call()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert got[0] is err and got[1] is grad and got[2] is acc and got[3] is fit_out \
        and got[4] is residual
    assert np.array_equal(acc.cpu().numpy(), ref["acc"])
    assert _bits_equal(fit_out.cpu().numpy(), ref["fit_out"]).all()


# ------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28
CELLS = 6                                    # the object: a 6 x 6 grid of cells over +-0.2


def _cells(object_yz):
    """(labels, points): the cell of every start point on the 6 x 6 grid over +-0.2 and the
    (36, 2) cell centres."""
    c = np.clip(np.floor((object_yz + 0.2) / 0.4 * CELLS), 0, CELLS - 1).astype(np.int64)
    centre = -0.2 + (np.arange(CELLS) + 0.5) * (0.4 / CELLS)
    g = np.arange(CELLS * CELLS)
    return c[:, 0] * CELLS + c[:, 1], np.stack([centre[g // CELLS], centre[g % CELLS]], axis=1)


def _make(n_rays, mode, ray_dtype=torch.float64, random_rays=False, fit="scale", with_spot=False,
          **engine_kw):
    """The lens of tests/test_gpu_spot.py's ``_make`` with a DistortionError over the 36 cells of
    the object."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype,
                                                    random_rays=random_rays, **engine_kw)
    start = system._amalgamated_sources["object_coords"].detach().cpu().double().numpy()[:, 1:]
    labels, points = _cells(start)
    erf = dist = optimizer.DistortionError(("y_end", "z_end"), labels, points, DOMAIN_LENS, fit=fit,
                                           oob_weight=2.0 / n_rays, n_groups=CELLS * CELLS)
    lr = 0.2 / n_rays            # (a sum over the rays, as the SpotError of tests/test_gpu_spot.py)
    if with_spot:
        spot = optimizer.SpotError(("y_end", "z_end"), labels, DOMAIN_LENS,
                                   oob_weight=2.0 / n_rays, n_groups=CELLS * CELLS)
        erf, lr = optimizer.SumError([spot, dist], reduce="mean"), 0.4
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source), dist


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def _finished_reference(eng, erf):
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].cpu().numpy()
    return dr.distortion_error(fin["y_end"].detach().cpu().double().numpy(),
                               fin["z_end"].detach().cpu().double().numpy(),
                               erf.labels.cpu().numpy(), erf.n_groups, erf.points.cpu().numpy(),
                               DOMAIN_LENS, fit=erf.fit, min_cond=erf.min_cond,
                               oob_weight=erf.oob_weight, perm=ids), ids


@pytest.mark.parametrize("fit", ["scale", "affine"])
def test_fused_step_equals_the_generic_step(fit):
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    tests/test_gpu_focus.py's test of the same name; the step is one graph replay."""
    runs = {mode: _make(8192, mode, fit=fit) for mode in ("generic", "graph")}
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
    # the records, the fit and the residuals of the last replayed step can be read afterwards
    erf = runs["graph"][4]
    fp = erf.fit_parameters()
    print("fit:", fp)
    assert fp["valid"] and fp["groups_used"] >= 30 and int(erf.last_acc[:, 0].sum()) > 4000
    assert erf.centroids().shape == erf.residuals().shape == (36, 2)
    other = runs["generic"][4].fit_parameters()
    np.testing.assert_allclose(fp["matrix"].numpy(), other["matrix"].numpy(), rtol=0, atol=1e-8)
    if fit == "scale":
        assert fp["magnification"] < 0.0                  # a real image: inverted


def test_a_redrawn_source_keeps_its_labels_under_replay():
    """The source is re-drawn (and re-ordered) inside the graph at every step; the kernels look
    the labels up through the trace's order themselves: the records, the fit and the residuals of
    the last replay equal the reference on that trace's finished rays."""
    opt, eng, lens, _, erf = _make(8192, "graph", random_rays=True)
    _steps(opt, lens, 5)
    fs = opt._fused_step
    for _ in range(4):
        if fs.graph_replays >= 2:
            break
        _steps(opt, lens, 1)
    assert fs is not None and fs.in_place and fs.graph_replays >= 2 and fs.capture_error is None
    acc = erf.last_acc.cpu().numpy().copy()
    fit_out = erf.last_fit.cpu().numpy().copy()
    residual = erf.last_residual.cpu().numpy().copy()
    ref, ids = _finished_reference(eng, erf)
    assert ref["n_inside"] > 4000 and len(set(ids.tolist())) == ids.shape[0]
    assert np.array_equal(acc, ref["acc"])
    assert _bits_equal(fit_out, ref["fit_out"]).all()
    assert _bits_equal(residual, ref["residual"]).all()


@pytest.mark.parametrize("fit", ["scale", "affine"])
def test_parameter_gradient_equals_the_oracle(fit):
    """4,096 rays, float64 state, one step: d error / d parameters on the generic path and on the
    fused step's fixed-shape path against the oracle's float64 trace composed with the plain torch
    objective (centroids and fit differentiated through) under autograd, at the tolerance
    tests/test_gpu_spot.py uses for the same comparison."""
    tol = 1e-9
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    from test_distortion_error_host import _torch_objective
    opt, eng, lens, (system, target, source), erf = _make(4096, "eager", fit=fit)
    grads, err_sum, n_terms = opt.raw_gradient()
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    src["cell_label"] = erf.labels.cpu().double()
    ref = tracer.ray_trace(osys, src, max_iterations=3,
                           inherit=("wavelength", "object_coords", "cell_label"))
    y, z = ref["finished"]["y_end"], ref["finished"]["z_end"]
    label = ref["finished"]["cell_label"].long()
    assert n_terms == 2 * y.shape[0] and y.shape[0] > 2000
    for v, (lo, hi) in zip((y.detach().numpy(), z.detach().numpy()), DOMAIN_LENS):
        assert min(np.abs(v - lo).min(), np.abs(v - hi).min()) > 1e-6
    e = _torch_objective(torch.stack([y, z]), label, erf.points.cpu(), DOMAIN_LENS,
                         erf.oob_weight, fit)
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
    assert FusedStep.eligible(opt, (), {})
    fs = FusedStep(opt, graph=False)
    fused, err3 = fs._enqueue_gradient()
    torch.cuda.synchronize()
    assert fs.in_place
    compare(fused, "fused")
    assert abs(float(err3[0]) - float(e)) <= 10 * tol * float(e)
    assert float(err3[1]) == 2 * y.shape[0]


def test_float32_state_fused_equals_generic():
    """float32 state: the fused step against the generic one, which runs the same kernels on the
    same float32 rows, at the tolerance tests/test_gpu_focus.py applies to float32 state."""
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


def test_a_sum_with_a_spot_error_runs_fused_and_equals_the_generic_step():
    runs = {mode: _make(8192, mode, with_spot=True) for mode in ("generic", "graph")}
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
    assert runs["graph"][4].fit_parameters()["valid"]


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
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    n_source = eng.optical_system.sources["x_start"].shape[0]
    domain = ((float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))),)    # some rays outside
    groups = np.arange(n_source) * 9 // n_source                           # neighbours together
    points = np.linspace(-1.0, 1.0, 9)[:, None]
    erf = optimizer.DistortionError(("y_end",), groups, points, domain, fit="affine",
                                    oob_weight=0.01)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    ids = eng.last_trace["finished_id"].cpu().numpy()
    ref = dr.distortion_error(y, None, groups, 9, points, domain, fit="affine", oob_weight=0.01,
                              perm=ids)
    assert ref["n_penalised"] > 0 and ref["n_inside"] > 100 and n_terms == y.shape[0]
    assert ref["valid"] and ref["groups_used"] >= 3
    assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
    assert _bits_equal(erf.last_fit.cpu().numpy(), ref["fit_out"]).all()
    assert abs(float(err_sum) - ref["error"]) <= dr.error_bound(ref)
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_imaging_example_with_a_distortion_error_lowers_its_error():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "imaging.py"),
                          "--distortion", "scale", "--rays", "8192", "--steps", "8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("combined error: first")][-1]
    first, last = float(line.split()[3]), float(line.split()[5])
    assert last < first
    assert any(ln.startswith("fitted magnification") for ln in out.stdout.splitlines())
