"""
Weighted DensityError and SpotError on the GPU: tfrt_density_error_weighted and
tfrt_spot_error_weighted against the numpy / Python-integer reference of
tests/weighted_errors_reference.py, and the weighted errors on the optimiser's paths -- the fused,
replayed 3-D step against the generic one, weights overwritten in place, a re-drawn source, the
parameter gradient against the oracle, the fallbacks, 2-D, the imaging example.

A DensityError's gradient inside the domain is made from the pulls D, whose sums over the bins the
kernel forms in its own fixed order: it is compared bit for bit with the reference evaluated on
the kernel's own pulls (tfrt_density_error_weighted leaves them in the workspace) and within
``gradient_bound`` of the reference's pulls.  Every other gradient entry is compared bit for bit.
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
import weighted_errors_reference as wr
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}
COUNTS = (0, 1, 63, 64, 65, 1000, 4097)
OOB = 0.3
T = 512                                   # ops.SPOT_WEIGHTED_LDS_GROUPS
SPOT_GROUPS = (1, 3, T, T + 1)
DENSITY_BINS = ((1,), (7, 5), (64, 64), (4097,))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_the_threshold_is_the_exported_one():
    from tensorflowraytrace_amd import ops
    assert ops.SPOT_WEIGHTED_LDS_GROUPS == T


# ------------------------------------------------------------------------------ spot kernels
@functools.lru_cache(maxsize=None)
def _spot_reference(n, G, two, f32, masked, permuted):
    """The reference of one case, computed once and shared (never written to)."""
    x, y, mask, group, perm, weight, _ = wr.spot_inputs(n, np.float32 if f32 else np.float64,
                                                        n_groups=G)
    return wr.spot_error(x, y if two else None, group, G, sr.DOMAIN if two else sr.DOMAIN[:1],
                         weight, OOB, mask=mask if masked else None,
                         perm=perm if permuted else None)


def _spot_kernel(n, G, two, dtype, masked, permuted, variant=0, pad=3):
    """tfrt_spot_error_weighted on the points of a case: the rows sit in a 6-row block (x in row
    4, y in row 5) with ``pad`` spare columns; the gradient block starts out as NaN."""
    from tensorflowraytrace_amd import ops
    x, y, mask, group, perm, weight, wbits = wr.spot_inputs(n, NP_DTYPE[dtype], n_groups=G)
    rows = torch.full((6, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[4, :n] = torch.tensor(x, device=DEV)
    rows[5, :n] = torch.tensor(y, device=DEV)
    qbits = ops.spot_qbits(group.shape[0])
    assert wbits == ops.spot_wbits(group.shape[0])
    grid = ops.spot_grid(sr.DOMAIN if two else sr.DOMAIN[:1], qbits)
    grad = torch.full((6, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    err, grad, acc = ops.spot_error(
        rows[:, :n], 4, 5 if two else -1, torch.tensor(group, device=DEV), G, grid, OOB,
        mask=torch.tensor(mask, device=DEV) if masked else None,
        perm=torch.tensor(perm, device=DEV) if permuted else None, grad=grad[:, :n],
        variant=variant, weights=torch.tensor(weight, device=DEV))
    torch.cuda.synchronize()
    return err.cpu().numpy(), grad.cpu().numpy(), acc.cpu().numpy()


def _check_spot(got, ref, two):
    err, grad, acc = got
    assert acc.shape[1] == 8 and np.array_equal(acc, ref["acc"])
    assert np.array_equal(_bits(grad[4]), _bits(ref["grad_x"]))
    if two:
        assert np.array_equal(_bits(grad[5]), _bits(ref["grad_y"]))
    else:
        assert np.isnan(grad[5]).all()           # (one field: the entry owns one row)
    assert np.isnan(grad[:4]).all()              # rows it does not own are never written
    print(f"error {err[0]!r} reference {ref['error']!r} bound {sr.error_bound(ref):.3e}")
    assert abs(err[0] - ref["error"]) <= sr.error_bound(ref)
    assert err[1] == ref["terms"]
    if ref["terms"] > 0:
        assert err[2] == err[0] / err[1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("G", SPOT_GROUPS)
def test_spot_kernel_equals_the_reference(G, dtype):
    """Every count, two fields and one, with and without mask and perm.  G = T + 1 takes the
    global atomics, every other G the table in LDS."""
    f32 = dtype == torch.float32
    for n in COUNTS:
        for two in (True, False):
            for masked, permuted in ((False, False), (True, True)):
                ref = _spot_reference(n, G, two, f32, masked, permuted)
                if two and not f32:
                    x, y, mask, group, perm, weight, wbits = wr.spot_inputs(n, n_groups=G)
                    wr.guard(n, ref["inside"], weight, perm if permuted else None,
                             wr.special_weights(wbits))
                _check_spot(_spot_kernel(n, G, two, dtype, masked, permuted), ref, two)


@pytest.mark.parametrize("G", (3, T))
def test_both_accumulate_variants_and_two_calls_give_the_same_bits(G):
    ref = _spot_reference(4097, G, True, False, True, True)
    lds = _spot_kernel(4097, G, True, torch.float64, True, True, variant=1)
    glb = _spot_kernel(4097, G, True, torch.float64, True, True, variant=2)
    again = _spot_kernel(4097, G, True, torch.float64, True, True, variant=1)
    _check_spot(lds, ref, True)
    for a, b, c in zip(lds, glb, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_spot_contention_every_ray_at_one_place_in_one_group():
    """100,000 columns at one place in one group, each with the weight 3 * 2**-wbits: the exact
    integer record, from the table in LDS and from the global atomics."""
    from tensorflowraytrace_amd import ops
    n = 100_000
    (x0, x1), (y0, y1) = sr.DOMAIN
    px, py = x0 + 0.3 * (x1 - x0), y0 + 0.55 * (y1 - y0)
    rows = torch.empty((2, n), dtype=torch.float64, device=DEV)
    rows[0], rows[1] = px, py
    group = np.zeros(n, dtype=np.int32)
    qbits, wbits = ops.spot_qbits(n), ops.spot_wbits(n)
    weight = np.full(n, 3 * np.ldexp(1.0, -wbits))
    one = wr.spot_error(np.array([px]), np.array([py]), group, 2, sr.DOMAIN, weight,
                        qbits=qbits, wbits=wbits)
    assert one["acc"][0, 0] == 3 and one["acc"][0, 5] == 1
    grid = ops.spot_grid(sr.DOMAIN, qbits)
    for variant in (1, 2):
        _, _, acc = ops.spot_error(rows, 0, 1, torch.tensor(group, device=DEV), 2, grid,
                                   variant=variant, weights=torch.tensor(weight, device=DEV))
        assert np.array_equal(acc.cpu().numpy(), one["acc"] * n)


def test_spot_bad_arguments():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_spot_error_weighted_workspace_bytes(10, 0) == 0
    assert L.tfrt_spot_error_weighted_workspace_bytes(0, 4) > 0
    t = torch.zeros(1 << 15, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, G=4, x1=1.0, ws=1 << 17, stride=8, variant=0, weight=p, wbits=20, qbits=40,
             dimension=3, row_x=0):
        return L.tfrt_spot_error_weighted(p, stride, n, 1, dimension, None, row_x, 1, p, weight,
                                          wbits, 8, None, G, 0.0, x1, 4.0, 0.0, 1.0, 4.0, qbits,
                                          0.0, p, stride, p, p, variant, p, ws, None)
    # n over the overflow bound 2^(62 - wbits - ceil(qbits / 2)) = 2^16 with wbits 20, qbits 52:
    # refused before anything is read (the buffers hold far fewer columns)
    for bad in (dict(wbits=0), dict(wbits=21), dict(weight=None), dict(G=T + 1, variant=1),
                dict(n=1 << 16, stride=1 << 16, qbits=52), dict(dimension=4), dict(row_x=9),
                dict(x1=0.0), dict(variant=3), dict(stride=4)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    assert call(n=(1 << 16) - 1, stride=1 << 16, qbits=52, G=1, ws=8) == -2   # (under the bound)
    assert call(n=0) == 0 and call(G=T, variant=1, n=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ density kernels
def _density_case(n, bins, f32, masked, permuted):
    two = len(bins) == 2
    x, y, mask, perm, weight = wr.density_inputs(n, np.float32 if f32 else np.float64)
    goal = dr.goal_of(bins[0], bins[1]) if two else dr.goal_of(bins[0], 1, False)
    dom = dr.DOMAIN if two else dr.DOMAIN[:1]
    kw = dict(mask=mask if masked else None, perm=perm if permuted else None)
    return two, x, y, mask, perm, weight, goal, dom, kw


@functools.lru_cache(maxsize=None)
def _density_reference(n, bins, f32, masked, permuted):
    two, x, y, mask, perm, weight, goal, dom, kw = _density_case(n, bins, f32, masked, permuted)
    return wr.density_error(x, y if two else None, goal, dom, weight, OOB, **kw)


def _density_kernel(n, bins, dtype, masked, permuted, variant=0, pad=3):
    from tensorflowraytrace_amd import ops
    f32 = dtype == torch.float32
    two, x, y, mask, perm, weight, goal, dom, kw = _density_case(n, bins, f32, masked, permuted)
    rows = torch.full((6, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[4, :n] = torch.tensor(x, device=DEV)
    rows[5, :n] = torch.tensor(y, device=DEV)
    g = torch.tensor(dr.normalise(goal), device=DEV).contiguous()
    grid = ops.density_grid(dom, g.shape[-1], g.shape[0] if two else None)
    grad = torch.full((6, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    wsb = ops._lib.lib().tfrt_density_error_workspace_bytes(n, g.shape[-1], g.shape[0] if two else 1)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    err, grad, hq = ops.density_error(
        rows[:, :n], 4, 5 if two else -1, g, grid, OOB,
        mask=torch.tensor(mask, device=DEV) if masked else None,
        perm=torch.tensor(perm, device=DEV) if permuted else None, grad=grad[:, :n],
        variant=variant, workspace=ws, weights=torch.tensor(weight, device=DEV))
    torch.cuda.synchronize()
    pulls = ws[:8 * g.numel()].view(torch.float64).cpu().numpy()
    return err.cpu().numpy(), grad.cpu().numpy(), hq.cpu().numpy(), pulls


def _check_density(got, ref, case):
    err, grad, hq, pulls = got
    two, x, y, mask, perm, weight, goal, dom, kw = case
    assert np.array_equal(hq, ref["Hq"])
    assert err[1] == 1.0 and err[0] == err[2]
    print(f"error {err[0]!r} reference {ref['error']!r} bound {dr.error_bound(ref):.3e}")
    assert abs(err[0] - ref["error"]) <= dr.error_bound(ref)
    own = wr.density_error(x, y if two else None, goal, dom, weight, OOB, pulls=pulls, **kw)
    tol = dr.gradient_bound(ref)
    assert np.abs(pulls - ref["D"].reshape(-1)).max(initial=0.0) <= tol
    assert np.array_equal(_bits(grad[4]), _bits(own["grad_x"]))
    assert np.abs(grad[4] - ref["grad_x"]).max(initial=0.0) <= tol
    rest = ~ref["inside"]                        # (outside, or not counting: no pull takes part)
    assert np.array_equal(_bits(grad[4][rest]), _bits(ref["grad_x"][rest]))
    if two:
        assert np.array_equal(_bits(grad[5]), _bits(own["grad_y"]))
        assert np.abs(grad[5] - ref["grad_y"]).max(initial=0.0) <= tol
        assert np.array_equal(_bits(grad[5][rest]), _bits(ref["grad_y"][rest]))
    else:
        assert np.isnan(grad[5]).all()
    assert (grad[4][~ref["counts"]] == 0.0).all()
    assert np.isnan(grad[:4]).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("bins", DENSITY_BINS, ids=lambda v: str(v))
def test_density_kernel_equals_the_reference(bins, dtype):
    """Every count, with and without mask and perm.  4,097 bins take the global atomics, every
    other grid the histogram in LDS ((64, 64) is the largest that does)."""
    f32 = dtype == torch.float32
    for n in COUNTS:
        for masked, permuted in ((False, False), (True, True)):
            ref = _density_reference(n, bins, f32, masked, permuted)
            case = _density_case(n, bins, f32, masked, permuted)
            if not f32:
                wr.guard(n, ref["inside"] & (ref["w"] > 0), case[5], case[4] if permuted else None,
                         wr.special_weights(20))
            _check_density(_density_kernel(n, bins, dtype, masked, permuted), ref, case)


@pytest.mark.parametrize("bins", [(7, 5), (64, 64)], ids=lambda v: str(v))
def test_both_splat_variants_and_two_calls_give_the_same_bits(bins):
    ref = _density_reference(4097, bins, False, True, True)
    lds = _density_kernel(4097, bins, torch.float64, True, True, variant=1)
    glb = _density_kernel(4097, bins, torch.float64, True, True, variant=2)
    again = _density_kernel(4097, bins, torch.float64, True, True, variant=1)
    _check_density(lds, ref, _density_case(4097, bins, False, True, True))
    for a, b, c in zip(lds, glb, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_density_bad_arguments():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    t = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, nx=4, ny=4, ws=1 << 13, stride=8, variant=0, weight=p, n_source=8, dimension=3):
        return L.tfrt_density_error_weighted(p, stride, n, 1, dimension, None, 0, 1, p, weight,
                                             n_source, None, nx, ny, 0.0, 1.0, 4.0, 0.0, 1.0, 4.0,
                                             0.0, p, 8, p, p, variant, p, ws, None)
    for bad in (dict(weight=None), dict(n_source=-1), dict(n_source=1 << 31), dict(dimension=1),
                dict(nx=512, ny=512), dict(variant=3), dict(stride=4), dict(n=-1)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    assert call(n=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ direction fields
@pytest.mark.parametrize("dimension,codes", [(3, (4, 8)), (2, (3, 5))], ids=["3d", "2d"])
def test_a_position_with_a_direction(dimension, codes):
    """y_end with z_dir (3-D) / y_dir (2-D), weighted, both errors: records and histogram as
    integers, all 2 * dimension gradient rows bit for bit (a DensityError's from its own pulls)."""
    from tensorflowraytrace_amd import ops
    n, G = 1000, 7
    block = df.rays(n, dimension=dimension)
    domain = ((-2.0, 2.5), df.DOMAIN[1] if dimension == 3 else df.DOMAIN[0])
    df.assert_generator(n, block, codes, domain)
    rng = np.random.default_rng(9)
    group = rng.integers(0, G, n + 3).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    perm[20], perm[22] = -1, n + 3
    wbits = wr.wbits_of(n + 3)
    weight = wr.weights(n + 3, wbits)
    mask = np.where(np.arange(n) % 5 == 4, -1, 0).astype(np.int32)
    vals, d, L, ok = df.field_values(block, codes)
    rows = torch.tensor(block, device=DEV)
    tw, tp, tm = (torch.tensor(a, device=DEV) for a in (weight, perm, mask))

    ref = wr.spot_error(vals[0], vals[1], group, G, domain, weight, OOB, mask=mask, perm=perm)
    want = np.where((ref["inside"] | ref["outside"])[None, :],
                    df.chain([ref["grad_x"], ref["grad_y"]], codes, d, L, ok), 0.0)
    grad = torch.full((2 * dimension, n), float("nan"), dtype=torch.float64, device=DEV)
    grid = ops.spot_grid(domain, ops.spot_qbits(n + 3))
    err, grad, acc = ops.spot_error(rows, codes[0], codes[1], torch.tensor(group, device=DEV), G,
                                    grid, OOB, mask=tm, perm=tp, grad=grad, dimension=dimension,
                                    weights=tw)
    assert ref["n_inside"] > n // 8 and np.array_equal(acc.cpu().numpy(), ref["acc"])
    assert np.array_equal(_bits(grad.cpu().numpy()), _bits(want))
    assert abs(float(err[0]) - ref["error"]) <= sr.error_bound(ref)

    goal = dr.goal_of(7, 5)
    g = torch.tensor(dr.normalise(goal), device=DEV).contiguous()
    ws = torch.zeros(ops._lib.lib().tfrt_density_error_workspace_bytes(n, 7, 5),
                     dtype=torch.uint8, device=DEV)
    grad = torch.full((2 * dimension, n), float("nan"), dtype=torch.float64, device=DEV)
    err, grad, hq = ops.density_error(rows, codes[0], codes[1], g, ops.density_grid(domain, 7, 5),
                                      OOB, mask=tm, perm=tp, grad=grad, dimension=dimension,
                                      workspace=ws, weights=tw)
    ref = wr.density_error(vals[0], vals[1], goal, domain, weight, OOB, mask=mask, perm=perm)
    own = wr.density_error(vals[0], vals[1], goal, domain, weight, OOB, mask=mask, perm=perm,
                           pulls=ws[:8 * 35].view(torch.float64).cpu().numpy())
    want = np.where(own["counts"][None, :],
                    df.chain([own["grad_x"], own["grad_y"]], codes, d, L, ok), 0.0)
    assert np.array_equal(hq.cpu().numpy(), ref["Hq"]) and int(ref["inside"].sum()) > n // 8
    assert np.array_equal(_bits(grad.cpu().numpy()), _bits(want))
    assert abs(float(err[0]) - ref["error"]) <= dr.error_bound(ref)


# ------------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28
N_GROUPS = 37


def _lens_weights(n_rays, seed=3):
    """One weight per source ray in (0.05, 1], the maximum exactly 1; ray 5 carries no power and
    ray 7 one that quantises to 0."""
    w = 0.05 + 0.95 * np.random.default_rng(seed).random(n_rays)
    w[5], w[7], w[11] = 0.0, 2.0 ** -40, 1.0
    return w


def _gauss16(gx, gy):
    return torch.exp(-(gx ** 2 + gy ** 2) / (2 * 0.5 ** 2))


def _make(kind, n_rays, mode, ray_dtype=torch.float64, random_rays=False, weights="lens",
          **engine_kw):
    """The lens of tests/test_gpu_spot.py's and tests/test_gpu_density.py's ``_make`` with a
    weighted SpotError over 37 groups / a weighted DensityError on 16 x 16 bins."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype,
                                                    random_rays=random_rays, **engine_kw)
    if isinstance(weights, str):
        weights = _lens_weights(n_rays)
    if kind == "spot":
        erf = optimizer.SpotError(("y_end", "z_end"), torch.arange(n_rays) % N_GROUPS, DOMAIN_LENS,
                                  oob_weight=2.0 / n_rays, weights=weights)
        lr = 0.2 / n_rays
    else:
        erf = optimizer.DensityError(("y_end", "z_end"), _gauss16, DOMAIN_LENS,
                                     oob_weight=2.0 / n_rays, bins=16, weights=weights)
        lr = 0.05
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source)


def _steps(opt, lens, steps):
    errs, params = [], []
    for _ in range(steps):
        errs.append(float(opt.single_step(None)))
        params.append([p.detach().cpu().clone() for p in lens.parameters])
    return errs, params


def _reference_of_last_step(kind, eng, erf):
    """The reference on the finished rays of the engine's last trace, their source-ray indices and
    the error's own buffers."""
    fin = eng.finished_rays
    y, z = fin["y_end"].detach().cpu().numpy(), fin["z_end"].detach().cpu().numpy()
    ids = eng.last_trace["finished_id"].cpu().numpy()
    w = erf.weights.cpu().numpy()
    if kind == "spot":
        return wr.spot_error(y, z, erf.labels.cpu().numpy(), N_GROUPS, DOMAIN_LENS, w,
                             oob_weight=erf.oob_weight, perm=ids)
    return wr.density_error(y, z, erf.goal.cpu().numpy(), DOMAIN_LENS, w,
                            oob_weight=erf.oob_weight, perm=ids)


def _table(kind, erf):
    return (erf.last_acc if kind == "spot" else erf.last_hq).cpu().numpy().copy()


@pytest.mark.parametrize("kind", ["spot", "density"])
def test_fused_step_equals_the_generic_step(kind):
    """8,192 rays (traced in place), 6 steps: the same errors and parameters (after 3 steps and
    after 6) at the tolerances of the unweighted tests; the step is one graph replay; the records
    / the histogram of either path are, as integers, the reference's on that path's own finished
    rays -- and each other's when the parameters agree to the bit."""
    runs = {mode: _make(kind, 8192, mode) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 6) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert runs["generic"][0]._fused_step is None
    assert fs is not None and fs.in_place and fs.capture_error is None, fs and fs.capture_error
    assert fs.graph_replays > 0
    print("errors, generic:", out["generic"][0], "graph:", out["graph"][0])
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for step in (2, 5):
        for a, b in zip(out["graph"][1][step], out["generic"][1][step]):
            assert float((a - b).abs().max()) <= 1e-11
    assert abs(out["generic"][0][-1] - out["generic"][0][0]) > 1e-6 * out["generic"][0][0]
    tables = {}
    for mode, (opt, eng, lens, _) in runs.items():
        erf = opt.error_function
        ref = _reference_of_last_step(kind, eng, erf)
        tables[mode] = _table(kind, erf)
        assert int(ref["inside"].sum()) > 4000
        assert np.array_equal(tables[mode], ref["acc" if kind == "spot" else "Hq"]), mode
    if kind == "spot":
        erf = runs["graph"][0].error_function
        assert tables["graph"].shape == (N_GROUPS, 8)
        assert erf.centroids().shape == (N_GROUPS, 2) and bool(torch.isfinite(erf.centroids()).all())
    # (before the last step's update: the parameters the last traces ran with)
    if all(torch.equal(a, b) for a, b in zip(out["graph"][1][4], out["generic"][1][4])):
        assert np.array_equal(tables["graph"], tables["generic"])


@pytest.mark.parametrize("kind", ["spot", "density"])
def test_weights_overwritten_in_place_are_seen_by_replays_and_other_weights_recapture(kind):
    opt, eng, lens, _ = _make(kind, 8192, "graph")
    _steps(opt, lens, 6)
    fs = opt._fused_step
    erf = opt.error_function
    assert fs.graph_replays > 0
    before, e_before = fs.graph_replays, float(opt.single_step(None))
    ramp = torch.linspace(1.0, 0.01, 8192, dtype=torch.float64, device=erf.weights.device)
    erf.weights.copy_(ramp * ramp)
    e_after = float(opt.single_step(None))
    assert fs.graph_replays == before + 2 and abs(e_after - e_before) > 1e-3 * e_before
    ref = _reference_of_last_step(kind, eng, erf)
    assert np.array_equal(_table(kind, erf), ref["acc" if kind == "spot" else "Hq"])
    erf.weights = erf.weights.clone()                 # another buffer: not the captured one
    float(opt.single_step(None))
    assert fs.graph_replays == before + 2


@pytest.mark.parametrize("kind", ["spot", "density"])
def test_a_redrawn_source_keeps_its_weights_under_replay(kind):
    """The source is re-drawn (and re-ordered) inside the graph at every step; the kernel looks the
    weights up through the trace's order itself: the table of the last replay equals the reference
    on that trace's finished rays, their source-ray indices and the weights."""
    opt, eng, lens, _ = _make(kind, 8192, "graph", random_rays=True)
    _steps(opt, lens, 5)
    fs = opt._fused_step
    erf = opt.error_function
    for _ in range(4):
        if fs.graph_replays >= 2:
            break
        _steps(opt, lens, 1)
    assert fs is not None and fs.in_place and fs.graph_replays >= 2 and fs.capture_error is None
    table = _table(kind, erf)
    ids = eng.last_trace["finished_id"].cpu().numpy()
    ref = _reference_of_last_step(kind, eng, erf)
    assert int(ref["inside"].sum()) > 4000 and len(set(ids.tolist())) == ids.shape[0]
    assert np.array_equal(table, ref["acc" if kind == "spot" else "Hq"])


def _spot_objective(y, z, label, wr_, n_groups, domain, oob):
    """sum wr |x - c_w|^2 + sum wr * penalty as differentiable float64 torch code, the weighted
    centroid differentiated through; ``wr_``: the QUANTISED weight per ray (0: in no spot)."""
    (x0, x1), (y0, y1) = domain
    ok = torch.isfinite(y) & torch.isfinite(z) & (label >= 0) & (label < n_groups) & (wr_ > 0)
    out = (y < x0) | (y > x1) | (z < y0) | (z > y1)
    inside, outside = ok & ~out, ok & out
    yo, zo = y[outside], z[outside]
    ex = torch.clamp(x0 - yo, min=0) + torch.clamp(yo - x1, min=0)
    ey = torch.clamp(y0 - zo, min=0) + torch.clamp(zo - y1, min=0)
    e = ((oob * (ex ** 2 + ey ** 2)) * wr_[outside]).sum()
    li, wi = label[inside], wr_[inside]
    W = torch.zeros(n_groups, dtype=torch.float64).index_add(0, li, wi)
    W = torch.where(W > 0, W, torch.ones_like(W))
    for v in (y[inside], z[inside]):
        mean = torch.zeros(n_groups, dtype=torch.float64).index_add(0, li, wi * v) / W
        e = e + (wi * (v - mean[li]) ** 2).sum()
    return e


def _density_objective(x, y, w, g, domain, oob):
    """The unquantised weighted soft histogram against the goal, float64 torch code."""
    (x0, x1), (y0, y1) = domain
    ny, nx = g.shape
    sx, sy = nx / (x1 - x0), ny / (y1 - y0)
    ok = torch.isfinite(x) & torch.isfinite(y)
    out = (x < x0) | (x > x1) | (y < y0) | (y > y1)
    inside, outside = ok & ~out, ok & out
    xo, yo = x[outside], y[outside]
    ex = torch.clamp(x0 - xo, min=0) + torch.clamp(xo - x1, min=0)
    ey = torch.clamp(y0 - yo, min=0) + torch.clamp(yo - y1, min=0)
    penalty = ((oob * (ex ** 2 + ey ** 2)) * w[outside]).sum()
    xi, yi, wi = x[inside], y[inside], w[inside]

    def axis(v, lo, scale, nb):
        u = (v - lo) * scale - 0.5
        f = torch.floor(u.detach())
        i0 = f.long()
        return i0.clamp(0, nb - 1), (i0 + 1).clamp(0, nb - 1), u - f
    ia, ib, tx = axis(xi, x0, sx, nx)
    ja, jb, ty = axis(yi, y0, sy, ny)
    H = torch.zeros(nx * ny, dtype=torch.float64)
    for k, b in ((ja * nx + ia, (1 - ty) * (1 - tx)), (ja * nx + ib, (1 - ty) * tx),
                 (jb * nx + ia, ty * (1 - tx)), (jb * nx + ib, ty * tx)):
        H = H.index_add(0, k, b * wi)
    s = torch.linalg.norm(H)
    return ((H / s - g.reshape(-1)) ** 2).sum() + penalty


@pytest.mark.parametrize("ray_dtype,tol", [(torch.float64, 1e-9), (torch.float32, 1e-5)],
                         ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["spot", "density"])
def test_parameter_gradient_equals_the_oracle(kind, ray_dtype, tol):
    """4,096 rays, one step: d error / d parameters on the generic path and on the fused step's
    fixed-shape path against the oracle's float64 trace composed with the plain torch objective
    under autograd -- for a SpotError with the QUANTISED weights wr."""
    from tensorflowraytrace_amd import ops
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    opt, eng, lens, (system, target, source) = _make(kind, 4096, "eager", ray_dtype)
    erf = opt.error_function
    grads, err_sum, n_terms = opt.raw_gradient()
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    if ray_dtype == torch.float32:
        for k in ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end"):
            src[k] = src[k].float().double()
    w = erf.weights.cpu()
    if kind == "spot":
        wbits = ops.spot_wbits(4096)
        w = torch.round(w * 2.0 ** wbits) * 2.0 ** -wbits
        src["spot_label"] = erf.labels.cpu().double()
    src["ray_weight"] = w
    ref = tracer.ray_trace(osys, src, max_iterations=3,
                           inherit=("wavelength", "object_coords", "spot_label", "ray_weight")
                           if kind == "spot" else ("wavelength", "object_coords", "ray_weight"))
    y, z = ref["finished"]["y_end"], ref["finished"]["z_end"]
    wf = ref["finished"]["ray_weight"]
    for v, (lo, hi) in zip((y.detach().numpy(), z.detach().numpy()), DOMAIN_LENS):
        assert min(np.abs(v - lo).min(), np.abs(v - hi).min()) > 1e-6
        if kind == "density":
            s = 16 / (hi - lo)
            u = (v - lo) * s - 0.5
            assert np.abs(u - np.round(u)).min() / s > 1e-6
    assert int(((y.abs() > 1.1) | (z.abs() > 1.1)).sum()) > 50       # the penalty takes part
    if kind == "spot":
        assert n_terms == 2 * y.shape[0]
        e = _spot_objective(y, z, ref["finished"]["spot_label"].long(), wf, N_GROUPS, DOMAIN_LENS,
                            erf.oob_weight)
    else:
        assert n_terms == 1
        e = _density_objective(y, z, wf, erf.goal.cpu(), DOMAIN_LENS, erf.oob_weight)
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
    assert float(err3[1]) == n_terms


@pytest.mark.parametrize("kind", ["spot", "density"])
def test_all_ones_weights_give_the_unweighted_fused_step(kind):
    """Not bit-equal -- the weighted centroid is formed by other roundings --, but within the
    tolerances of the oracle comparison with float64 ray state (1e-9 relative)."""
    runs = {name: _make(kind, 8192, "graph", weights=w)
            for name, w in (("plain", None), ("ones", np.ones(8192)))}
    out = {name: _steps(r[0], r[2], 6) for name, r in runs.items()}
    for name, r in runs.items():
        assert r[0]._fused_step is not None and r[0]._fused_step.graph_replays > 0
    np.testing.assert_allclose(out["ones"][0], out["plain"][0], rtol=1e-9, atol=0)
    for a, b in zip(out["ones"][1][-1], out["plain"][1][-1]):
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max())
    if kind == "spot":
        acc, plain = runs["ones"][0].error_function.last_acc, runs["plain"][0].error_function.last_acc
        assert torch.equal(acc[:, 5], plain[:, 0])


@pytest.mark.parametrize("what", ["few_rays", "deterministic"])
@pytest.mark.parametrize("kind", ["spot", "density"])
def test_fallbacks_take_the_generic_path_and_equal_the_reference(kind, what):
    n, kw = (2000, {}) if what == "few_rays" else (8192, dict(deterministic=True))
    opt, eng, lens, _ = _make(kind, n, "graph", **kw)
    errs, _ = _steps(opt, lens, 3)
    fs = opt._fused_step
    assert fs is None or fs.steps == 0
    grads, err_sum, n_terms = opt.raw_gradient()
    erf = opt.error_function
    ref = _reference_of_last_step(kind, eng, erf)
    assert int(ref["inside"].sum()) > n // 2
    assert np.array_equal(_table(kind, erf), ref["acc" if kind == "spot" else "Hq"])
    bound = sr.error_bound(ref) if kind == "spot" else dr.error_bound(ref)
    assert abs(float(err_sum) - ref["error"]) <= bound
    assert all(np.isfinite(errs)) and any(float(g.abs().max()) > 0 for g in grads)


@pytest.mark.parametrize("kind", ["spot", "density"])
def test_2d_engine_runs_on_the_generic_path_and_equals_the_reference(kind):
    import tfrt.optimizer as optimizer
    from test_gpu_fused_2d import _segment_lens
    eng, params, _ = _segment_lens(torch.float64)
    eng.optical_system.update()
    eng.ray_trace(4)
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    n_source = eng.optical_system.sources["x_start"].shape[0]
    domain = ((float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))),)    # some rays outside
    weights = _lens_weights(n_source)
    groups = np.arange(n_source) % 9
    goal = dr.goal_of(9, 1, two=False)
    if kind == "spot":
        erf = optimizer.SpotError(("y_end",), groups, domain, oob_weight=0.01, weights=weights)
    else:
        erf = optimizer.DensityError(("y_end",), goal, domain, oob_weight=0.01, weights=weights)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    ids = eng.last_trace["finished_id"].cpu().numpy()
    w = erf.weights.cpu().numpy()
    if kind == "spot":
        ref = wr.spot_error(y, None, groups, 9, domain, w, oob_weight=0.01, perm=ids)
        assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"]) and n_terms == y.shape[0]
        assert abs(float(err_sum) - ref["error"]) <= sr.error_bound(ref)
    else:
        ref = wr.density_error(y, None, goal, domain, w, oob_weight=0.01, perm=ids)
        assert np.array_equal(erf.last_hq.cpu().numpy(), ref["Hq"])
        assert abs(float(err_sum) - ref["error"]) <= dr.error_bound(ref)
    assert ref["n_penalised"] > 0 and int(ref["inside"].sum()) > 100
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_imaging_example_with_an_apodised_pupil_shrinks_the_weighted_spots():
    """A fresh child process: the weighted RMS spot, which the example forms from ``last_acc``,
    is smaller after the steps than before."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "imaging.py"),
                          "--apodize", "0.5", "--rays", "20000", "--steps", "20"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("rms spot: first")][-1]
    first, last = float(line.split()[3]), float(line.split()[5])
    assert last < first
