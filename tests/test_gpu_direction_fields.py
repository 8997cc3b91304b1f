"""
The direction fields (x_dir, y_dir, z_dir) of DensityError and SpotError on the GPU:
tfrt_density_error_fields / tfrt_spot_error_fields against the numpy reference of
tests/direction_fields_reference.py, position codes against the old entries, and the errors on the
optimiser's paths -- the fused, replayed 3-D step against the generic one, the parameter gradient
against the oracle, the fallbacks, 2-D, the example.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import density_error_reference as dr
import direction_fields_reference as df
import spot_error_reference as sr
from test_direction_fields_host import CASES, IDS, OOB, _density_grad_check
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}
COUNTS = (0, 1, 63, 64, 65, 1000, 20000)
# the splat's / accumulate's grid holds 512 workgroups of 4 * 256 columns: one more trip
OVER_THE_GRID = 512 * 4 * 256 + 37


def _mask(n):
    return np.where(np.arange(n) % 5 == 4, -1, np.arange(n) % 7).astype(np.int32)


def _labels(n, G):
    """(group of n + 3 source rays with -1 and G among the labels, perm with one entry below 0
    and one past the source)."""
    rng = np.random.default_rng(n + G)
    group = rng.integers(0, G, n + 3).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    if n > 12:
        group[3], group[7] = -1, G
        perm[5], perm[11] = -1, n + 3
    return group, perm


@functools.lru_cache(maxsize=None)
def _density_reference(n, f32, dim, codes, domain, bins, masked):
    """The reference of one case, computed once and shared (never written to)."""
    two = len(codes) == 2
    block = df.rays(n, np.float32 if f32 else np.float64, dimension=dim)
    goal = dr.goal_of(bins[0], bins[1] if two else 1, two)
    return df.density(block, codes, goal, domain, OOB, mask=_mask(n) if masked else None)


@functools.lru_cache(maxsize=None)
def _spot_reference(n, f32, dim, codes, domain, G, masked, permuted):
    block = df.rays(n, np.float32 if f32 else np.float64, dimension=dim)
    group, perm = _labels(n, G)
    return df.spot(block, codes, group, G, domain, OOB, mask=_mask(n) if masked else None,
                   perm=perm if permuted else None)


def _density_kernel(n, dtype, dim, codes, domain, bins, masked, variant=0, pad=3, fields=True):
    """tfrt_density_error_fields on the generator's block with ``pad`` spare columns; the gradient
    block starts out as NaN to show what is written.  ``fields`` false: the old entry."""
    from tensorflowraytrace_amd import ops
    two = len(codes) == 2
    nx, ny = bins[0], (bins[1] if two else 1)
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[:, :n] = torch.tensor(df.rays(n, NP_DTYPE[dtype], dimension=dim), device=DEV)
    goal = torch.tensor(dr.normalise(dr.goal_of(nx, ny, two)), device=DEV).contiguous()
    grid = ops.density_grid(domain, nx, ny if two else None)
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    m = torch.tensor(_mask(n), device=DEV) if masked else None
    err, _, hq = ops.density_error(rows[:, :n], codes[0], codes[1] if two else -1, goal, grid, OOB,
                                   mask=m, grad=grad[:, :n], variant=variant,
                                   dimension=dim if fields else None)
    torch.cuda.synchronize()
    return err.cpu().numpy(), grad.cpu().numpy(), hq.cpu().numpy()


def _spot_kernel(n, dtype, dim, codes, domain, G, masked, permuted, variant=0, pad=3, fields=True):
    from tensorflowraytrace_amd import ops
    two = len(codes) == 2
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[:, :n] = torch.tensor(df.rays(n, NP_DTYPE[dtype], dimension=dim), device=DEV)
    group, perm = _labels(n, G)
    g = torch.tensor(group, device=DEV)
    qbits = ops.spot_qbits(g.numel())
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    m = torch.tensor(_mask(n), device=DEV) if masked else None
    p = torch.tensor(perm, device=DEV) if permuted else None
    err, _, acc = ops.spot_error(rows[:, :n], codes[0], codes[1] if two else -1, g, G,
                                 ops.spot_grid(domain, qbits), OOB, mask=m, perm=p,
                                 grad=grad[:, :n], variant=variant,
                                 dimension=dim if fields else None)
    torch.cuda.synchronize()
    return err.cpu().numpy(), grad.cpu().numpy(), acc.cpu().numpy()


def _check_density(got, ref, n, codes, dim):
    err, grad, hq = got
    assert np.array_equal(hq, ref["Hq"])
    assert err[1] == 1.0 and err[0] == err[2]
    print(f"error {err[0]!r} reference {ref['error']!r} bound {dr.error_bound(ref):.3e}")
    assert abs(err[0] - ref["error"]) <= dr.error_bound(ref)
    assert np.isnan(grad[:, n:]).all() and not np.isnan(grad[:, :n]).any()
    if n:
        _density_grad_check(grad[:, :n], ref, codes, dim)


def _check_spot(got, ref, n):
    err, grad, acc = got
    assert np.array_equal(acc, ref["acc"])
    print(f"error {err[0]!r} reference {ref['error']!r} bound {sr.error_bound(ref):.3e}")
    assert abs(err[0] - ref["error"]) <= sr.error_bound(ref)
    assert err[1] == ref["terms"]
    if ref["terms"]:
        assert err[2] == err[0] / err[1]
    else:
        assert np.isnan(err[2]) and err[0] == 0.0
    assert np.isnan(grad[:, n:]).all()
    same = grad[:, :n].view(np.int64) == ref["grad"].view(np.int64)
    if not same.all():
        r, i = (int(v[0]) for v in np.nonzero(~same))
        raise AssertionError(f"gradient entry not bit-equal (row, column, kernel, reference): "
                             f"{r}, {i}, {grad[r, i]!r}, {ref['grad'][r, i]!r}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_density_kernel_equals_the_reference(case, dtype):
    """Every count, with and without the mask, bins (7, 3); one, two and mixed fields, 2-D and
    3-D."""
    _, dim, codes, domain = case
    f32 = dtype == torch.float32
    for n in COUNTS:
        if n >= 64 and codes == (7, 8):
            df.assert_generator(n, df.rays(n, NP_DTYPE[dtype]), codes, domain)
        for masked in (False, True):
            ref = _density_reference(n, f32, dim, codes, domain, (7, 3), masked)
            _check_density(_density_kernel(n, dtype, dim, codes, domain, (7, 3), masked), ref, n,
                           codes, dim)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_spot_kernel_equals_the_reference(case, dtype):
    """Every count, with and without the mask and perm; 3 groups take the table in LDS, 1,025 the
    global atomics."""
    _, dim, codes, domain = case
    f32 = dtype == torch.float32
    for n in COUNTS:
        for G in (3, 1025):
            for masked, permuted in ((False, False), (True, True)):
                ref = _spot_reference(n, f32, dim, codes, domain, G, masked, permuted)
                _check_spot(_spot_kernel(n, dtype, dim, codes, domain, G, masked, permuted), ref, n)


def test_more_than_4096_bins_take_the_global_atomics():
    for n in (1000, 20000):
        ref = _density_reference(n, True, 3, (7, 8), df.DOMAIN, (80, 60), True)
        _check_density(_density_kernel(n, torch.float32, 3, (7, 8), df.DOMAIN, (80, 60), True),
                       ref, n, (7, 8), 3)


def test_a_second_trip_of_the_grid_stride_loop():
    n = OVER_THE_GRID
    df.assert_generator(n, df.rays(n, np.float32), (7, 8), df.DOMAIN)
    ref = _density_reference(n, True, 3, (7, 8), df.DOMAIN, (7, 3), True)
    _check_density(_density_kernel(n, torch.float32, 3, (7, 8), df.DOMAIN, (7, 3), True), ref, n,
                   (7, 8), 3)
    ref = _spot_reference(n, True, 3, (7, 8), df.DOMAIN, 3, True, True)
    _check_spot(_spot_kernel(n, torch.float32, 3, (7, 8), df.DOMAIN, 3, True, True), ref, n)


def test_variants_and_repeated_calls_give_the_same_bits():
    args = (20000, torch.float32, 3, (7, 8), df.DOMAIN)
    base = _density_kernel(*args, (7, 3), True)
    for other in (_density_kernel(*args, (7, 3), True, variant=1),
                  _density_kernel(*args, (7, 3), True, variant=2),
                  _density_kernel(*args, (7, 3), True)):
        for a, b in zip(base, other):
            assert a.tobytes() == b.tobytes()
    base = _spot_kernel(*args, 37, True, True)
    for other in (_spot_kernel(*args, 37, True, True, variant=1),
                  _spot_kernel(*args, 37, True, True, variant=2),
                  _spot_kernel(*args, 37, True, True)):
        for a, b in zip(base, other):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dim,codes", [(3, (4, 5)), (3, (1,)), (3, (5, 0)), (2, (3,)), (2, (2, 1))])
def test_position_codes_equal_the_old_entries_bit_for_bit(dim, codes):
    """Codes below 2d through the new entries: error, gradient block (what is written and what is
    left alone) and histogram / records are the old entries'."""
    domain = ((-1.5, 1.0), (-1.0, 1.5))[:len(codes)]
    for n in (65, 20000):
        for dtype in (torch.float32, torch.float64):
            new = _density_kernel(n, dtype, dim, codes, domain, (7, 3), True)
            old = _density_kernel(n, dtype, dim, codes, domain, (7, 3), True, fields=False)
            for a, b in zip(new, old):
                assert a.tobytes() == b.tobytes()
            written = ~np.isnan(new[1]).all(axis=1)
            assert sorted(np.nonzero(written)[0]) == sorted(codes)
            new = _spot_kernel(n, dtype, dim, codes, domain, 37, True, True)
            old = _spot_kernel(n, dtype, dim, codes, domain, 37, True, True, fields=False)
            for a, b in zip(new, old):
                assert a.tobytes() == b.tobytes()
            assert int(new[2][:, 0].sum()) > n / 8


def test_bad_arguments():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    t = torch.zeros(1 << 15, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def density(dim=3, fx=7, fy=8, ny=4, n=8, new=True):
        head = (p, 8, n, 1) + ((dim,) if new else ())
        fn = L.tfrt_density_error_fields if new else L.tfrt_density_error
        return fn(*head, None, fx, fy, p, 4, ny, 0.0, 1.0, 4.0, 0.0, 1.0, 4.0, 0.0, p, 8, p, p, 0,
                  p, 1 << 17, None)

    def spot(dim=3, fx=7, fy=8, n=8):
        return L.tfrt_spot_error_fields(p, 8, n, 1, dim, None, fx, fy, p, 8, None, 4, 0.0, 1.0,
                                        4.0, 0.0, 1.0, 4.0, 40, 0.0, p, 8, p, p, 0, p, 1 << 17,
                                        None)
    for call in (density, spot):
        for bad in (dict(dim=1), dict(dim=4), dict(fx=9), dict(fy=9), dict(dim=2, fy=6),
                    dict(fx=8, fy=8)):
            assert call(**bad) == -1, (call.__name__, bad)
        assert call(n=0) == 0 and call(n=0, dim=2, fx=4, fy=5) == 0
    # one field wants ny == 1; a second field with ny == 1 is what it is today
    assert density(fy=-1, ny=4) == density(fx=4, fy=-1, ny=4, new=False) == -1
    assert density(n=0, fx=4, fy=5, ny=1) == density(n=0, fx=4, fy=5, ny=1, new=False) == 0
    assert density(n=0, fx=7, fy=8, ny=1) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ the optimiser
FIELDS = ("y_dir", "z_dir")


def _directions_of(fin):
    block = np.stack([fin[f].detach().cpu().double().numpy()
                      for f in ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")])
    return block, df.directions(block)


def _edge(v, q):
    """About the q-quantile of v, in the middle of the widest gap between neighbouring samples
    nearby: no sample lies close to it."""
    v = np.sort(v)
    at = int(q * (v.shape[0] - 1))
    j = at + int(np.argmax(np.diff(v[at:at + 50])))
    return float(0.5 * (v[j] + v[j + 1]))


def _scene(n_rays, ray_dtype=torch.float64, **engine_kw):
    """The lens of tests/test_gpu_spot.py, traced once: the domain lies between the 10 % and the
    90 % quantiles of the finished rays' directions, so that some rays are penalised."""
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype, **engine_kw)
    system.update()
    eng.ray_trace(3)
    _, (d, L, ok) = _directions_of(eng.finished_rays)
    assert ok.all()
    domain = tuple((_edge(d[a], 0.1), _edge(d[a], 0.9)) for a in (1, 2))
    return eng, system, lens, target, source, domain


def _make(kind, n_rays, mode, ray_dtype=torch.float64, fields=FIELDS, **engine_kw):
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source, domain = _scene(n_rays, ray_dtype, **engine_kw)
    if fields != FIELDS:
        domain = ((-1.1, 1.1), (-1.1, 1.1))           # positions: tests/test_gpu_density.py's
    if kind == "spot":
        erf = optimizer.SpotError(fields, torch.arange(n_rays) % 37, domain,
                                  oob_weight=2.0 / n_rays)
        # (a direction is a position over the length of the last link, ~10 in this scene: the
        # residuals and their derivatives are a tenth of tests/test_gpu_spot.py's, the step size
        # that moves the lens as far a hundred times its)
        lr = 20.0 / n_rays
    else:
        (y0, y1), (z0, z1) = domain

        def goal(gy, gz):
            return torch.exp(-(((gy - 0.5 * (y0 + y1)) / (y1 - y0)) ** 2
                               + ((gz - 0.5 * (z0 + z1)) / (z1 - z0)) ** 2) / (2 * 0.25 ** 2))
        erf = optimizer.DensityError(fields, goal, domain, oob_weight=2.0 / n_rays, bins=16)
        lr = 0.05
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source), domain


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


@pytest.mark.parametrize("kind", ["spot", "density"])
def test_fused_step_equals_the_generic_step(kind):
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    the position fields' tests; the step is one graph replay."""
    runs = {mode: _make(kind, 8192, mode) for mode in ("generic", "graph")}
    assert runs["generic"][4] == runs["graph"][4]
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
    # what the last replayed step left: the rays whose direction lies in the domain
    erf = runs["graph"][0].error_function
    _, (d, L, ok) = _directions_of(runs["graph"][1].finished_rays)
    (y0, y1), (z0, z1) = runs["graph"][4]
    inside = int((ok & (d[1] >= y0) & (d[1] <= y1) & (d[2] >= z0) & (d[2] <= z1)).sum())
    assert 2000 < inside < 8192 - 500
    if kind == "spot":
        assert int(erf.last_acc[:, 0].sum()) == inside
        c = erf.centroids()
        assert c.shape == (37, 2) and bool(torch.isfinite(c).all()) and float(c.abs().max()) < 1
    else:
        assert abs(int(erf.last_hq.sum()) - inside * 2 ** 32) <= 4 * inside


@pytest.mark.parametrize("fields", [FIELDS, ("y_end", "z_end")], ids=["direction", "position"])
def test_histogram_is_cleared_at_every_replay_of_a_redrawn_source(fields):
    """The source is re-drawn inside the graph at every step: after several replays the histogram
    holds the weight of ONE step's rays (a memset node in the place of the clearing launch left
    2**46 in every bin under them)."""
    opt, eng, lens, _, domain = _make("density", 8192, "graph", fields=fields, random_rays=True)
    _steps(opt, lens, 9)
    fs = opt._fused_step
    assert fs is not None and fs.in_place and fs.graph_replays >= 3 and fs.capture_error is None
    block, (d, L, ok) = _directions_of(eng.finished_rays)
    y, z = (d[1], d[2]) if fields == FIELDS else (block[4], block[5])
    (y0, y1), (z0, z1) = domain
    inside = int((ok & (y >= y0) & (y <= y1) & (z >= z0) & (z <= z1)).sum())
    assert inside > 2000
    assert abs(int(opt.error_function.last_hq.sum()) - inside * 2 ** 32) <= 4 * inside


@pytest.mark.parametrize("ray_dtype,tol", [(torch.float64, 1e-9), (torch.float32, 1e-5)],
                         ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["spot", "density"])
def test_parameter_gradient_equals_the_oracle(kind, ray_dtype, tol):
    """4,096 rays, one step: d error / d parameters on the generic path and on the fused step's
    fixed-shape path against the oracle's float64 trace composed with a plain torch objective over
    (end - start) / |end - start| under autograd.  With float32 state the subtraction cancels: the
    project's 1e-5 times max(1, max|coordinate| / min L) of the oracle's finished rays."""
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    from test_density_error_host import _torch_objective as density_objective
    from test_spot_error_host import _torch_objective as spot_objective
    opt, eng, lens, (system, target, source), domain = _make(kind, 4096, "eager", ray_dtype)
    erf = opt.error_function
    grads, err_sum, n_terms = opt.raw_gradient()
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    geo = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
    if ray_dtype == torch.float32:
        for k in geo:
            src[k] = src[k].float().double()
    if kind == "spot":
        src["spot_label"] = erf.labels.cpu().double()
    ref = tracer.ray_trace(osys, src, max_iterations=3,
                           inherit=("wavelength", "object_coords") + (("spot_label",) if kind == "spot" else ()))
    fin = ref["finished"]
    e3 = torch.stack([fin[k] for k in geo[3:]]) - torch.stack([fin[k] for k in geo[:3]])
    length = torch.sqrt((e3 * e3).sum(dim=0))
    dy, dz = e3[1] / length, e3[2] / length
    if ray_dtype == torch.float32:
        top = max(float(fin[k].detach().abs().max()) for k in geo)
        tol = tol * max(1.0, top / float(length.detach().min()))
    # no finished ray within 1e-6 of the domain's edge: the in / out decision is the same in
    # float32 and float64
    for v, (lo, hi) in zip((dy.detach().numpy(), dz.detach().numpy()), domain):
        assert min(np.abs(v - lo).min(), np.abs(v - hi).min()) > 1e-6
        assert int(((v < lo) | (v > hi)).sum()) > 50                 # the penalty takes part
        if kind == "density":
            # nor within 1e-7 of a bin-centre line, where the gradient has a kink (positions in
            # float32 and float64 state differ by up to ~1e-6, a direction is that over L ~ 10)
            s = 16 / (hi - lo)
            u = (v - lo) * s - 0.5
            assert np.abs(u - np.round(u)).min() / s > 1e-7
    if kind == "spot":
        assert n_terms == 2 * dy.shape[0]
        e = spot_objective(dy, dz, fin["spot_label"].long(), 37, domain, erf.oob_weight)
    else:
        assert n_terms == 1
        e = density_objective(dy, dz, erf.goal.cpu(), domain, erf.oob_weight)
    rg = torch.autograd.grad(e, q)
    e = e.detach()
    print(f"error {float(err_sum)!r} oracle {float(e)!r} tolerance {tol:.3g}")
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


@pytest.mark.parametrize("kind", ["spot", "density"])
def test_few_rays_take_the_generic_path_and_equal_the_reference(kind):
    opt, eng, lens, _, domain = _make(kind, 2000, "graph")
    errs, _ = _steps(opt, lens, 2)
    fs = opt._fused_step
    assert fs is None or fs.steps == 0
    grads, err_sum, n_terms = opt.raw_gradient()
    erf = opt.error_function
    block, _ = _directions_of(eng.finished_rays)
    if kind == "spot":
        ids = eng.last_trace["finished_id"].cpu().numpy()
        ref = df.spot(block, (7, 8), erf.labels.cpu().numpy(), 37, domain, erf.oob_weight, perm=ids)
        assert ref["n_inside"] > 500 and ref["n_penalised"] > 100
        assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
        assert abs(float(err_sum) - ref["error"]) <= sr.error_bound(ref)
    else:
        ref = df.density(block, (7, 8), erf.goal.cpu().numpy(), domain, erf.oob_weight)
        assert ref["inside"].sum() > 500 and ref["n_penalised"] > 100
        assert np.array_equal(erf.last_hq.cpu().numpy(), ref["Hq"])
        assert abs(float(err_sum) - ref["error"]) <= dr.error_bound(ref)
    assert np.isfinite(errs).all() and any(float(g.abs().max()) > 0 for g in grads)


@pytest.mark.parametrize("kind", ["spot", "density"])
def test_2d_engine_runs_on_the_generic_path_and_equals_the_reference(kind):
    import tfrt.optimizer as optimizer
    from test_gpu_fused_2d import _segment_lens
    eng, params, _ = _segment_lens(torch.float64)
    geo = ("x_start", "y_start", "x_end", "y_end")

    def block_of():
        return np.stack([eng.finished_rays[f].detach().cpu().double().numpy() for f in geo])
    eng.optical_system.update()
    eng.ray_trace(4)
    d, _, ok = df.directions(block_of())
    assert ok.all()
    domain = ((_edge(d[1], 0.1), _edge(d[1], 0.9)),)                       # some rays outside
    n_source = eng.optical_system.sources["x_start"].shape[0]
    groups = np.arange(n_source) % 9
    goal = dr.goal_of(9, 1, two=False)
    if kind == "spot":
        erf = optimizer.SpotError(("y_dir",), groups, domain, oob_weight=0.01)
    else:
        erf = optimizer.DensityError(("y_dir",), goal, domain, oob_weight=0.01)
    assert erf.rows_for(2) == [5]
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    block = block_of()
    if kind == "spot":
        ids = eng.last_trace["finished_id"].cpu().numpy()
        ref = df.spot(block, (5,), groups, 9, domain, oob_weight=0.01, perm=ids)
        assert ref["n_penalised"] > 0 and ref["n_inside"] > 100 and n_terms == block.shape[1]
        assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
        assert abs(float(err_sum) - ref["error"]) <= sr.error_bound(ref)
    else:
        ref = df.density(block, (5,), goal, domain, oob_weight=0.01)
        assert ref["n_penalised"] > 0 and ref["contributions"].sum() > 100
        assert np.array_equal(erf.last_hq.cpu().numpy(), ref["Hq"])
        assert abs(float(err_sum) - ref["error"]) <= dr.error_bound(ref)
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)
    with pytest.raises(ValueError):
        optimizer.SpotError(("z_dir",), groups, domain)(eng)


@pytest.mark.parametrize("density", [False, True], ids=["spot", "density"])
def test_collimator_example_lowers_its_error(density):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "collimator.py"),
                          "--rays", "8192", "--steps", "8"] + (["--density-error"] if density else []),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    name = "density error" if density else "rms angular spot"
    line = [ln for ln in out.stdout.splitlines() if ln.startswith(name + ": first")][-1]
    words = line[len(name) + 1:].split()
    first, last = float(words[1]), float(words[3])
    assert last < first
