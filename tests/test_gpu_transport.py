"""
TransportError on the GPU: tfrt_transport_error (keys, radix sort, sorted keys, ranks, seed,
finish) against the numpy reference of tests/transport_error_reference.py -- ranks equal as
integers, gradients bit for bit, the error within ``error_bound`` --, and the error on the
optimiser's paths: the fused, replayed 3-D step against the generic one, ``set_goal`` under
replays, the parameter gradient against the oracle, the fallbacks, 2-D, the example.

float32 (and float16) ray state is covered at kernel level only (the values are upcast and fed to
the reference, so the keys are the same).  Against the oracle it is not: two rays closer in projection
than float32 resolution may swap ranks between a float32 and a float64 trace, and each swap moves
a target by one quantile step -- such a comparison would measure the scene, not the code.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import transport_error_reference as ref
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float16: np.float16, torch.float32: np.float32, torch.float64: np.float64}
# a wave edge, a sort tile edge (4 x 256 items), a second column segment of 32 tiles (32,769), the
# switch to 8 items per thread (128 Ki)
COUNTS = (1, 64, 65, 1023, 1025, 32769, 131073)
SHAPES = ((1, 2), (1, 1024), (3, 2), (3, 1024), (8, 2), (8, 1024))          # (K, Q); K = 1: one field
# the large counts take every family at (3, 1024) and the other shapes on one family each
BIG_SHAPES = {"uniform": SHAPES, "ties": ((1, 2), (3, 1024)), "outside": ((3, 1024), (8, 2))}


def _shapes(n, family):
    return SHAPES if n <= 1025 else BIG_SHAPES.get(family, ((3, 1024),))


@functools.lru_cache(maxsize=None)
def _tables(K, Q):
    from tensorflowraytrace_amd import ops
    two = K > 1
    cs = ops.transport_directions(K, 2 if two else 1)
    goal = ref.goal_of(16, 12, two)
    domain = ref.DOMAIN if two else ref.DOMAIN[:1]
    return cs, ops.transport_tables(goal, domain, cs, Q), domain


def _points(family, n, dtype):
    """The family's points rounded to the ray state's ``dtype``."""
    x, y, mask = ref.points(family, n, seed=n)
    return x.astype(NP_DTYPE[dtype]), y.astype(NP_DTYPE[dtype]), mask


@functools.lru_cache(maxsize=None)
def _reference(family, n, K, Q, dtype):
    """The reference of one case -- of the values as the state's ``dtype`` holds them, upcast --,
    computed once and shared (never written to)."""
    cs, tables, domain = _tables(K, Q)
    x, y, mask = _points(family, n, dtype)
    return ref.transport_error(x.astype(np.float64), y.astype(np.float64) if K > 1 else None,
                               tables, cs, domain, mask)


def _kernel(family, n, K, Q, dtype, pad=3):
    """tfrt_transport_error on the points of a case: the rows sit in a 6-row block (x in row 4, y
    in row 5) with ``pad`` spare columns; the gradient block starts out as NaN to show what is
    written."""
    from tensorflowraytrace_amd import ops
    cs, tables, domain = _tables(K, Q)
    x, y, mask = _points(family, n, dtype)
    rows = torch.full((6, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[4, :n] = torch.tensor(x, device=DEV)
    rows[5, :n] = torch.tensor(y, device=DEV)
    grad = torch.full((6, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    m = torch.tensor(mask, device=DEV) if mask is not None else None
    err, grad, rank2 = ops.transport_error(
        rows[:, :n], 4, 5 if K > 1 else -1, torch.tensor(tables, device=DEV),
        ops.transport_grid(domain), torch.tensor(cs, device=DEV), mask=m, dimension=3,
        grad=grad[:, :n])
    torch.cuda.synchronize()
    return err.cpu().numpy(), grad.cpu().numpy(), rank2.cpu().numpy()


def _check(got, want, two):
    err, grad, rank2 = got
    assert np.array_equal(rank2.astype(np.int64), want["rank2"])
    assert np.array_equal(grad[4], want["grad_x"])
    if two:
        assert np.array_equal(grad[5], want["grad_y"])
    else:
        assert np.isnan(grad[5]).all()               # (one field: the entry owns one row)
    assert np.isnan(grad[:4]).all()                  # rows it does not own are never written
    total, terms, mean = want["error"]
    bound = ref.error_bound(want)
    print(f"error {err[0]!r} reference {total!r} bound {bound:.3e}")
    assert err[1] == terms and abs(err[0] - total) <= bound
    if terms == 0:
        assert err[0] == 0.0 and np.isnan(err[2]) and not grad[4].any()
    else:
        assert abs(err[2] - mean) <= bound / terms


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", COUNTS)
def test_kernel_equals_the_reference(n, dtype):
    """Every family; every (K, Q) up to 1,025 columns, a selection above."""
    for family in ref.FAMILIES:
        for K, Q in _shapes(n, family):
            want = _reference(family, n, K, Q, dtype)
            _check(_kernel(family, n, K, Q, dtype), want, K > 1)
            if family == "all_invalid":
                assert want["n_valid"] == 0
            if family == "one_valid":
                assert want["n_valid"] == 1


def test_float16_state_goes_through_the_same_dispatch():
    """float16 columns (finite in the domain; many share a value, so ties abound) against the
    reference of the upcast values."""
    for family, K in (("uniform", 3), ("masked", 1), ("nonfinite", 8)):
        want = _reference(family, 1025, K, 1024, torch.float16)
        _check(_kernel(family, 1025, K, 1024, torch.float16), want, K > 1)
        assert (want["rank2"] % 2 == 0).any()          # counts of two and more: ties


def test_a_padded_stride_changes_nothing():
    for n, K in ((1025, 3), (65, 1)):
        a = _kernel("masked", n, K, 1024, torch.float64, pad=0)
        b = _kernel("masked", n, K, 1024, torch.float64, pad=61)
        for u, v in zip(a, b):
            assert u[..., :n].tobytes() == v[..., :n].tobytes()


def test_two_calls_give_the_same_bits():
    for case in (("uniform", 32769, 8, 1024, torch.float32), ("ties", 1025, 3, 2, torch.float64),
                 ("outside", 131073, 3, 1024, torch.float64)):
        for u, v in zip(_kernel(*case), _kernel(*case)):
            assert u.tobytes() == v.tobytes()


def test_reused_buffers_allocate_nothing():
    from tensorflowraytrace_amd import _lib, ops
    cs, tables, domain = _tables(3, 1024)
    n = 5000
    x, y, mask = _points("masked", n, torch.float64)
    rows = torch.tensor(np.stack([x, y]), device=DEV)
    T, A = torch.tensor(tables, device=DEV), torch.tensor(cs, device=DEV)
    m = torch.tensor(mask, device=DEV)
    grad = torch.zeros((2, n), dtype=torch.float64, device=DEV)
    err = torch.zeros(3, dtype=torch.float64, device=DEV)
    rank2 = torch.zeros((3, n), dtype=torch.int32, device=DEV)
    ws = torch.empty(_lib.lib().tfrt_transport_error_workspace_bytes(n, 3), dtype=torch.uint8,
                     device=DEV)
    grid = ops.transport_grid(domain)
    ops.transport_error(rows, 0, 1, T, grid, A, mask=m, grad=grad, err=err, rank2=rank2,
                        workspace=ws)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    out = ops.transport_error(rows, 0, 1, T, grid, A, mask=m, grad=grad, err=err, rank2=rank2,
                              workspace=ws)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert out[0] is err and out[1] is grad and out[2] is rank2
    want = _reference("masked", n, 3, 1024, torch.float64)
    assert np.array_equal(rank2.cpu().numpy().astype(np.int64), want["rank2"])


def test_bad_arguments():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_transport_error_workspace_bytes(-1, 8) == 0
    assert L.tfrt_transport_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_transport_error_workspace_bytes(10, 65) == 0
    assert L.tfrt_transport_error_workspace_bytes((1 << 30) + 1, 8) == 0
    assert L.tfrt_transport_error_workspace_bytes(0, 1) > 0
    big = L.tfrt_transport_error_workspace_bytes(8, 2)
    t = torch.zeros(max(big, 1 << 12) // 8 + 1, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, dtype=1, dim=3, row_x=4, row_y=5, x0=0.0, ix=1.0, iy=1.0, cs=p, tables=p, Q=4,
             K=2, stride=8, gstride=8, err=p, rank2=p, ws=p, wsb=big):
        return L.tfrt_transport_error(p, stride, n, dtype, dim, None, row_x, row_y, x0, ix, 0.0, iy,
                                      cs, tables, Q, K, p, gstride, err, rank2, ws, wsb, None)
    for bad in (dict(n=-1), dict(n=(1 << 30) + 1), dict(dtype=7), dict(dim=4), dict(dim=1),
                dict(row_x=6), dict(row_x=-1), dict(row_y=4), dict(row_y=6), dict(dim=2, row_y=5),
                dict(x0=float("nan")), dict(ix=0.0), dict(ix=float("inf")), dict(iy=-1.0),
                dict(cs=None), dict(tables=None), dict(Q=1), dict(Q=65537), dict(K=0), dict(K=65),
                dict(row_y=-1, K=2), dict(stride=4), dict(gstride=4), dict(err=None),
                dict(rank2=None), dict(ws=None)):
        assert call(**bad) == -1, bad
    assert call(wsb=8) == -2
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert float(t[0]) == 0.0 and float(t[1]) == 0.0 and np.isnan(float(t[2]))   # err of no column


# ------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28
DIRECTIONS = 4


def _gauss16(gx, gy):
    return torch.exp(-(gx ** 2 + gy ** 2) / (2 * 0.5 ** 2))


def _make(n_rays, mode, ray_dtype=torch.float64, **engine_kw):
    """The lens of tests/test_gpu_density.py's ``_make`` with a TransportError.  The error is a sum
    over n_rays * K terms: the learning rate is per term."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype, **engine_kw)
    erf = optimizer.TransportError(("y_end", "z_end"), _gauss16, DOMAIN_LENS, bins=16,
                                   directions=DIRECTIONS, knots=256)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3,
                                  learning_rate=2.0 / (n_rays * DIRECTIONS), grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source)


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def test_fused_step_equals_the_generic_step():
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    tests/test_gpu_density.py's test of the same name -- the mid-rank gives every ray the same
    gradient bits on both paths, whatever order its column stands in --; the step is one graph
    replay."""
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
    # the ranks of the last replayed step can be read afterwards: every finished ray has one
    erf = runs["graph"][0].error_function
    n_fin = runs["graph"][1].finished_rays["y_end"].shape[0]
    assert tuple(erf.last_rank2.shape) == (DIRECTIONS, 8192) and erf.last_count == n_fin
    assert runs["generic"][0].error_function.last_count == n_fin
    assert runs["generic"][0].last_error_terms == DIRECTIONS * n_fin


def test_set_goal_is_seen_by_replays_without_a_recapture():
    opt, eng, lens, _ = _make(8192, "graph")
    _steps(opt, lens, 6)
    fs, erf = opt._fused_step, opt.error_function
    assert fs.graph_replays > 0
    before, e_before = fs.graph_replays, float(opt.single_step(None))
    gx, gy = torch.meshgrid(*(torch.linspace(-1.1, 1.1, 33, dtype=torch.float64)[1::2],) * 2,
                            indexing="xy")
    ptr = erf.tables.data_ptr()
    erf.set_goal(torch.exp(-((gx - 0.5) ** 2 + (gy + 0.4) ** 2) / (2 * 0.2 ** 2)))
    e_after = float(opt.single_step(None))
    assert erf.tables.data_ptr() == ptr
    assert fs.graph_replays == before + 2 and abs(e_after - e_before) > 1e-3 * e_before


def _torch_transport(x, y, erf):
    """The objective over torch tensors under autograd, the ranks from ``torch.searchsorted`` on
    the tensors' own keys; the targets are constants."""
    tables = erf.tables.cpu()
    x0, ix, y0, iy = erf.grid
    xi, eta = (x - x0) * ix, (y - y0) * iy
    n, Q = x.shape[0], erf.knots
    total = torch.zeros((), dtype=torch.float64)
    for k, (c, s) in enumerate(erf.directions):
        p = float(c) * xi + float(s) * eta
        lo, scale = ref.key_map(float(c), float(s))
        key = torch.clamp(torch.floor((p.detach() - lo) * scale), 0.0,
                          float(ref.KEY_INVALID - 1)).long()
        sk = torch.sort(key).values
        r2 = torch.searchsorted(sk, key, right=False) + torch.searchsorted(sk, key, right=True)
        z = ((r2.double() * 0.5) / float(n)) * float(Q)
        fm = torch.clamp(torch.floor(z), max=float(Q - 1))
        m = fm.long()
        t = tables[k][m] + (z - fm) * (tables[k][m + 1] - tables[k][m])
        total = total + ((p - t) ** 2).sum()
    return total


def test_parameter_gradient_equals_the_oracle():
    """4,096 rays of float64 state, one step: d error / d parameters on the generic path and on the
    fused step's fixed-shape path against the oracle's float64 trace composed with the torch
    objective under autograd, at DensityError's tolerance."""
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    tol = 1e-9
    opt, eng, lens, (system, target, source) = _make(4096, "eager")
    erf = opt.error_function
    grads, err_sum, n_terms = opt.raw_gradient()
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    out = tracer.ray_trace(osys, src, max_iterations=3, inherit=("wavelength", "object_coords"))
    y, z = out["finished"]["y_end"], out["finished"]["z_end"]
    assert n_terms == DIRECTIONS * y.shape[0] and y.shape[0] > 3000
    assert int(((y.abs() > 1.1) | (z.abs() > 1.1)).sum()) > 50      # rays outside the domain take part
    e = _torch_transport(y, z, erf)
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
    assert abs(float(err3[0]) - float(e)) <= 10 * tol * float(e)
    assert float(err3[1]) == n_terms


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
    goal = ref.goal_of(9, 1, two=False)
    eng.optical_system.update()
    eng.ray_trace(4)
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    domain = ((float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))),)    # some rays outside
    erf = optimizer.TransportError(("y_end",), goal, domain, knots=64)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02 / y.shape[0],
                                  grad_clip=0.05, sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    want = ref.transport_error(y, None, erf.tables.cpu().numpy(), erf.directions, domain)
    assert want["n_valid"] == y.shape[0] == n_terms > 100
    assert np.array_equal(erf.last_rank2.cpu().numpy().astype(np.int64), want["rank2"])
    assert abs(float(err_sum) - want["error"][0]) <= ref.error_bound(want)
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_illumination_example_with_a_transport_error_lowers_the_error():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "illumination.py"),
                          "--transport-error", "--rays", "8192", "--steps", "8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("transport error: first")][-1]
    first, last = float(line.split()[3]), float(line.split()[6])
    assert last < first
