"""
MixingError on the GPU: tfrt_mixing_error (clear, splat, margins, pulls, finish, seed) against the
numpy reference of tests/mixing_error_reference.py bit for bit, and the error on the optimiser's
paths -- the fused, replayed 3-D step against the generic one, in-place changes of labels and
weights under a replayed graph, a SumError with a DensityError, the parameter gradient against
the oracle, the fallbacks, 2-D, the example.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import direction_fields_reference as dfr
import mixing_error_reference as mr
import weighted_errors_reference as wr
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 63, 64, 65, 1000, 4097)
LDS_CELLS = 4096                            # ops.MIXING_LDS_CELLS (asserted below)
# (G, nx, ny, bins with one field, the group left empty): a degenerate group count; the last size
# with the table in LDS (4,096 cells) and the first two on global atomics; several trips of every
# per-thread loop; nx = 7 with a group left empty; one bin
SHAPES = ((1, 8, 6, 8, None), (4, 32, 32, 1024, None), (4, 33, 32, 1025, None),
          (5, 32, 32, 1024, None), (4, 64, 64, 4096, None), (3, 7, 3, 7, 1), (2, 1, 1, 1, None))
EMPTY = {(G, nx, ny): e for G, nx, ny, _, e in SHAPES}


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _inputs(n, G, nx, ny, f32):
    return mr.inputs(n, np.float32 if f32 else np.float64, n_groups=G, empty=EMPTY.get((G, nx, ny)))


@functools.lru_cache(maxsize=None)
def _reference(n, G, nx, ny, two, f32, indexed, weighted):
    """The reference of one case, computed once and shared (never written to).  ``indexed``: with
    the mask and the perm."""
    x, y, mask, perm, weight, group = _inputs(n, G, nx, ny, f32)
    ref = mr.mixing_error(x, y if two else None, group, G, (nx, ny) if two else (nx,),
                          mr.DOMAIN if two else mr.DOMAIN[:1], oob_weight=mr.OOB,
                          mask=mask if indexed else None, perm=perm if indexed else None,
                          weight=weight if weighted else None)
    if weighted:
        wr.guard(n, ref["inside"], weight, perm if indexed else None, wr.special_weights(20))
    return ref


def _kernel(n, G, nx, ny, two, dtype, dim, indexed, weighted, variant=0, pad=3):
    """tfrt_mixing_error on the points of a case: x and y sit in the last two rows of a
    (2 * dim, n + pad) geometry block (one field: x in the last row but one); the gradient block
    starts out as NaN to show what is written."""
    from tensorflowraytrace_amd import ops
    x, y, mask, perm, weight, group = _inputs(n, G, nx, ny, dtype == torch.float32)
    rx, ry = 2 * dim - 2, 2 * dim - 1
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[rx, :n] = torch.tensor(x, device=DEV)
    rows[ry, :n] = torch.tensor(y, device=DEV)
    domain = mr.DOMAIN if two else mr.DOMAIN[:1]
    grid = ops.density_grid(domain, nx, ny if two else None)
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    out = ops.mixing_error(rows[:, :n], rx, ry if two else -1, torch.tensor(group, device=DEV), G,
                           (nx, ny) if two else (nx,), grid, mr.OOB,
                           mask=torch.tensor(mask, device=DEV) if indexed else None,
                           perm=torch.tensor(perm, device=DEV) if indexed else None,
                           grad=grad[:, :n], variant=variant, dimension=dim,
                           weights=torch.tensor(weight, device=DEV) if weighted else None)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out] + [grad.cpu().numpy()]


def _check(got, ref, n, dim, two):
    err, grad, hq, pull, group_errors, used, block = got
    assert np.array_equal(hq, ref["Hq"])
    assert _bits_equal(pull, ref["D"])
    assert _bits_equal(group_errors, ref["group_errors"])
    assert _bits_equal(err, [ref["error"], 1.0, ref["error"]]), (err, ref["error"])
    assert used[0] == ref["groups_used"] and used[1] == ref["N"]
    rx, ry = 2 * dim - 2, 2 * dim - 1
    assert _bits_equal(grad[rx], ref["grad_x"])
    if two:
        assert _bits_equal(grad[ry], ref["grad_y"])
    off = ~ref["counts"]
    assert not grad[rx][off].any() and (not two or not grad[ry][off].any())
    # rows not named and the spare columns are never written
    named = [rx, ry] if two else [rx]
    assert np.isnan(np.delete(block, named, axis=0)).all() and np.isnan(block[:, n:]).all()


@pytest.mark.parametrize("dim", [3, 2], ids=["3d", "2d"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"G{s[0]}-{s[1]}x{s[2]}")
def test_kernel_equals_the_reference(shape, dtype, dim):
    """Every count, two fields and one, with and without mask and perm (entries of perm below 0 and
    past the source, labels of -1 and G), with and without weights (the special weights)."""
    from tensorflowraytrace_amd import ops
    assert ops.MIXING_LDS_CELLS == LDS_CELLS
    G, nx, ny, one, _ = shape
    f32 = dtype == torch.float32
    for n in COUNTS:
        for two in (True, False):
            bx, by = (nx, ny) if two else (one, 1)
            for indexed in (False, True):
                for weighted in (False, True):
                    ref = _reference(n, G, bx, by, two, f32, indexed, weighted)
                    _check(_kernel(n, G, bx, by, two, dtype, dim, indexed, weighted), ref, n, dim,
                           two)
    if G == 3:
        big = _reference(4097, G, nx, ny, True, f32, True, False)
        assert big["groups_used"] == 2 and np.isnan(big["group_errors"][1])
        assert not big["D"][1].any() and big["n_penalised"] > 100


@pytest.mark.parametrize("G,nx,ny", [(4, 32, 32), (1, 8, 6), (3, 7, 3)])
def test_both_splat_variants_and_repeated_calls_give_the_same_bytes(G, nx, ny):
    ref = _reference(4097, G, nx, ny, True, False, True, True)
    lds = _kernel(4097, G, nx, ny, True, torch.float64, 3, True, True, variant=1)
    glb = _kernel(4097, G, nx, ny, True, torch.float64, 3, True, True, variant=2)
    again = _kernel(4097, G, nx, ny, True, torch.float64, 3, True, True, variant=0)
    _check(lds, ref, 4097, 3, True)
    for a, b, c in zip(lds, glb, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    with pytest.raises(ValueError):
        _kernel(10, 4, 33, 32, True, torch.float64, 3, False, False, variant=1)


def test_two_runs_on_global_atomics_give_the_same_bytes():
    a = _kernel(4097, 4, 64, 64, True, torch.float32, 3, True, True)
    b = _kernel(4097, 4, 64, 64, True, torch.float32, 3, True, True)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("dim,codes", [(3, (7, 8)), (3, (8,)), (3, (4, 8)), (2, (3, 5)), (2, (5,))],
                         ids=["3d-dirs", "3d-one", "3d-mixed", "2d-mixed", "2d-one"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_direction_and_mixed_fields_are_chained_onto_every_row(dim, codes, weighted):
    """Direction cosines of the last link (and a position with a direction): the histogram, the
    pulls and all 2 * dim gradient rows bit for bit; the spare columns stay untouched."""
    from tensorflowraytrace_amd import ops
    n, G, pad = 1000, 3, 3
    two = len(codes) == 2
    block = dfr.rays(n, np.float64, dimension=dim)
    domain = tuple(dfr.DOMAIN[i] if c >= 2 * dim else (-0.5, 2.5) for i, c in enumerate(codes))
    bins = (8, 6) if two else (7,)
    rng = np.random.default_rng(4)
    perm = rng.permutation(n).astype(np.int32)
    perm[20], perm[22] = -1, n + 3
    group = mr.labels_for(n + 3, G)
    weight = wr.weights(n + 3, 20) if weighted else None
    ref = mr.fields(block, codes, group, G, bins, domain, oob_weight=mr.OOB, perm=perm,
                    weight=weight)
    assert ref["inside"].sum() > 150 and ref["n_penalised"] > 50 and ref["groups_used"] == G
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=torch.float64, device=DEV)
    rows[:, :n] = torch.tensor(block, device=DEV)
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    grid = ops.density_grid(domain, bins[0], bins[1] if two else None)
    out = ops.mixing_error(rows[:, :n], codes[0], codes[1] if two else -1,
                           torch.tensor(group, device=DEV), G, bins, grid, mr.OOB,
                           perm=torch.tensor(perm, device=DEV), grad=grad[:, :n], dimension=dim,
                           weights=None if weight is None else torch.tensor(weight, device=DEV))
    torch.cuda.synchronize()
    err, g, hq, pull, ge, used = [o.cpu().numpy() for o in out]
    assert np.array_equal(hq, ref["Hq"]) and _bits_equal(pull, ref["D"])
    assert _bits_equal(ge, ref["group_errors"])
    assert _bits_equal(err, [ref["error"], 1.0, ref["error"]])
    assert _bits_equal(g, ref["grad"])
    assert np.isnan(grad.cpu().numpy()[:, n:]).all()
    assert np.abs(ref["grad"][:dim]).max() > 0            # the start rows carry gradient


def test_bad_arguments_are_refused_before_any_launch():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    ws = L.tfrt_mixing_error_workspace_bytes
    assert ws(10, 0, 4, 4) == 0 and ws(10, 1025, 4, 4) == 0 and ws(10, 4, 512, 512) == 0
    assert ws(10, 32, 256, 256) == 0 and ws(-1, 4, 4, 4) == 0 and ws(0, 4, 4, 4) > 0
    t = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, G=4, nx=4, ny=4, fx=4, fy=5, x1=1.0, sx=4.0, oob=0.0, wsb=1 << 13, stride=8,
             variant=0, group=p, dim=3, n_source=8, pull=p):
        return L.tfrt_mixing_error(p, stride, n, 1, dim, None, fx, fy, group, n_source, None, G,
                                   None, nx, ny, 0.0, x1, sx, 0.0, 1.0, 4.0, oob, p, 8, p, p, p,
                                   pull, p, variant, p, wsb, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=1025), dict(nx=0), dict(nx=512, ny=512),
                dict(G=32, nx=256, ny=256), dict(fx=9), dict(fy=4), dict(x1=0.0), dict(sx=0.0),
                dict(oob=-1.0), dict(stride=4), dict(variant=3), dict(group=None), dict(dim=4),
                dict(fy=-1), dict(n=1 << 31), dict(n_source=-1), dict(pull=None),
                dict(G=4, nx=33, ny=32, variant=1)):
        assert call(**bad) == -1, bad
    assert call(wsb=8) == -2
    assert call(n=0) == 0
    torch.cuda.synchronize()


def test_reused_buffers_allocate_nothing():
    from tensorflowraytrace_amd import _lib, ops
    n, G, nx, ny = 1000, 4, 8, 6
    x, y, mask, perm, weight, group = _inputs(n, G, nx, ny, False)
    ref = _reference(n, G, nx, ny, True, False, True, True)
    rows = torch.tensor(np.stack([x, y]), device=DEV)
    dev = dict(mask=torch.tensor(mask, device=DEV), perm=torch.tensor(perm, device=DEV),
               weights=torch.tensor(weight, device=DEV))
    lab = torch.tensor(group, device=DEV)
    grid = ops.density_grid(mr.DOMAIN, nx, ny)
    bufs = dict(grad=torch.zeros((2, n), dtype=torch.float64, device=DEV),
                err=torch.zeros(3, dtype=torch.float64, device=DEV),
                hq=torch.zeros((G, ny, nx), dtype=torch.int64, device=DEV),
                pull=torch.zeros((G, ny, nx), dtype=torch.float64, device=DEV),
                group_errors=torch.zeros(G, dtype=torch.float64, device=DEV),
                used_out=torch.zeros(2, dtype=torch.float64, device=DEV),
                workspace=torch.zeros(_lib.lib().tfrt_mixing_error_workspace_bytes(n, G, nx, ny),
                                      dtype=torch.uint8, device=DEV))
    ops.mixing_error(rows, 0, 1, lab, G, (nx, ny), grid, mr.OOB, **dev, **bufs)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    got = ops.mixing_error(rows, 0, 1, lab, G, (nx, ny), grid, mr.OOB, **dev, **bufs)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert got[2] is bufs["hq"] and got[3] is bufs["pull"]
    assert np.array_equal(bufs["hq"].cpu().numpy(), ref["Hq"])
    assert _bits_equal(bufs["pull"].cpu().numpy(), ref["D"])


# ------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28
BINS = (16, 12)


def _gauss16(gx, gy):
    return torch.exp(-(gx ** 2 + gy ** 2) / (2 * 0.5 ** 2))


def _quadrants(object_yz):
    """The quadrant of the object plane a source ray starts in: 0 .. 3."""
    return (object_yz[:, 0] > 0).astype(np.int64) * 2 + (object_yz[:, 1] > 0).astype(np.int64)


def _make(n_rays, mode, ray_dtype=torch.float64, weighted=False, with_density=False, weights=None,
          density_alone=False, **engine_kw):
    """The lens of tests/test_gpu_density.py's ``_make`` with a MixingError whose groups are the
    quadrants of the source."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype, **engine_kw)
    start = system._amalgamated_sources["object_coords"].detach().cpu().double().numpy()[:, 1:]
    labels = _quadrants(start)
    power = None
    if weighted:
        power = 0.25 + 0.75 * np.random.default_rng(2).random(labels.shape[0])
    erf = mix = optimizer.MixingError(("y_end", "z_end"), labels, DOMAIN_LENS, BINS,
                                      oob_weight=2.0 / n_rays, n_groups=4, weights=power)
    lr = 0.05
    if with_density:
        dens = optimizer.DensityError(("y_end", "z_end"), _gauss16, DOMAIN_LENS,
                                      oob_weight=2.0 / n_rays, bins=16)
        erf = optimizer.SumError([dens] if density_alone else [dens, mix], weights=weights)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source), mix


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def _finished_reference(eng, erf):
    """The reference on the engine's finished rays with the term's CURRENT labels and weights."""
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].cpu().numpy()
    dim = eng.dimension
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end") if dim == 3 \
        else ("x_start", "y_start", "x_end", "y_end")
    block = np.stack([fin[f].detach().cpu().double().numpy() for f in names])
    return mr.fields(block, tuple(erf.rows_for(dim)), erf.labels.cpu().numpy(), erf.n_groups,
                     erf.bins, erf.domain, oob_weight=erf.oob_weight, perm=ids,
                     weight=None if erf.weights is None else erf.weights.cpu().numpy())


def _assert_last_evaluation(erf, ref):
    assert np.array_equal(erf.last_hq.cpu().numpy(), ref["Hq"])
    assert _bits_equal(erf.last_pull.cpu().numpy(), ref["D"])
    assert _bits_equal(erf.group_errors().cpu().numpy(), ref["group_errors"])
    assert erf.groups_used == ref["groups_used"]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_fused_step_equals_the_generic_step(weighted):
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    tests/test_gpu_centroid.py's test of the same name; the step is one graph replay, and the last
    replayed step's Hq and D are the reference's on that trace's finished rays."""
    runs = {mode: _make(8192, mode, weighted=weighted) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 6) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert runs["generic"][0]._fused_step is None
    assert fs is not None and fs.in_place and fs.capture_error is None, fs and fs.capture_error
    assert fs.graph_replays > 0
    print("errors, generic:", out["generic"][0], "graph:", out["graph"][0])
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11
    assert out["generic"][0][-1] != out["generic"][0][0] and out["generic"][0][0] > 0.0
    erf, other = runs["graph"][4], runs["generic"][4]
    assert erf.groups_used == other.groups_used == 4
    assert erf.shares().shape == (4, BINS[1], BINS[0]) and erf.pooled().shape == (BINS[1], BINS[0])
    assert erf.group_errors().shape == (4,)
    ref = _finished_reference(runs["graph"][1], erf)
    assert ref["inside"].sum() > 4000 and ref["n_penalised"] > 50
    _assert_last_evaluation(erf, ref)


def test_replays_see_in_place_changes_of_labels_and_weights():
    """Overwriting the labels and the weights in place between replays: the next replay of the
    same graph object reads the new values -- the reference's tables for them."""
    opt, eng, lens, _, erf = _make(8192, "graph", weighted=True)
    _steps(opt, lens, 5)
    fs = opt._fused_step
    for _ in range(4):
        if fs.graph_replays >= 1:
            break
        _steps(opt, lens, 1)
    assert fs is not None and fs.in_place and fs.graph_replays >= 1 and fs.capture_error is None
    graph, replays, key = fs._graphs[1], fs.graph_replays, erf.graph_key()
    before = erf.last_hq.cpu().numpy().copy()
    n = erf.labels.numel()
    erf.labels.copy_((torch.arange(n, device=DEV, dtype=torch.int32) * 7) % 4)
    erf.labels[::5] = 3
    erf.labels[11] = -1
    erf.weights.copy_(torch.linspace(1.0, 0.125, n, dtype=torch.float64, device=DEV))
    assert erf.graph_key() == key
    _steps(opt, lens, 1)
    assert fs._graphs[1] is graph and fs.graph_replays == replays + 1
    _assert_last_evaluation(erf, _finished_reference(eng, erf))
    assert np.abs(erf.last_hq.cpu().numpy() - before).max() > 2 ** 32
    erf.labels = erf.labels.clone()                   # another buffer: not the captured one
    assert erf.graph_key() != key


def test_a_sum_with_a_density_error_runs_fused_and_equals_the_generic_step():
    runs = {mode: _make(8192, mode, with_density=True) for mode in ("generic", "graph")}
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
    assert runs["graph"][4].groups_used == 4


def test_a_weight_of_zero_steps_as_the_density_error_alone():
    """SumError([density, mixing], weights=[1, 0]) steps as the DensityError of the same sum
    alone: the same parameters at the fused test's tolerance; the term is still evaluated."""
    off = _make(8192, "graph", with_density=True, weights=[1.0, 0.0])
    alone = _make(8192, "graph", with_density=True, density_alone=True)
    a, b = _steps(off[0], off[2], 6), _steps(alone[0], alone[2], 6)
    assert off[0]._fused_step is not None and off[0]._fused_step.graph_replays > 0
    np.testing.assert_allclose(a[0], b[0], rtol=1e-10, atol=0)
    for u, v in zip(a[1], b[1]):
        assert float((u - v).abs().max()) <= 1e-11
    triples = off[0].error_function.last_errors.cpu().numpy()
    assert triples[1, 0] > 0.0 and off[4].groups_used == 4
    assert float(off[0].error_function.last_coefficients[1]) == 0.0


@pytest.mark.parametrize("ray_dtype,tol", [(torch.float64, 1e-9), (torch.float32, 1e-5)],
                         ids=["f64", "f32"])
def test_parameter_gradient_equals_the_oracle(ray_dtype, tol):
    """2,048 rays, one step, weighted: d error / d parameters on the generic path against the
    oracle's float64 trace composed with the plain float definition in torch, in which m, n_g and
    N ARE differentiated, under autograd -- the check of "no derivative of m, n_g or N is needed"
    -- at the tolerances tests/test_gpu_density.py uses for the same comparison."""
    from oracle import tracer
    opt, eng, lens, (system, target, source), erf = _make(2048, "eager", ray_dtype, weighted=True)
    grads, err_sum, n_terms = opt.raw_gradient()
    assert n_terms == 1
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    if ray_dtype == torch.float32:
        for k in ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end"):
            src[k] = src[k].float().double()
    src["die_label"] = erf.labels.cpu().double()
    src["die_power"] = erf.weights.cpu().double()
    ref = tracer.ray_trace(osys, src, max_iterations=3,
                           inherit=("wavelength", "object_coords", "die_label", "die_power"))
    fin = ref["finished"]
    y, z = fin["y_end"], fin["z_end"]
    # no finished ray within 1e-6 of a bin-centre line or of the domain's edge: floor and the
    # in / out decision are the same in float32 and float64
    for v, (lo, hi), nb in zip((y.detach().numpy(), z.detach().numpy()), DOMAIN_LENS, BINS):
        s = nb / (hi - lo)
        u = (v - lo) * s - 0.5
        assert np.abs(u - np.round(u)).min() / s > 1e-6
        assert min(np.abs(v - lo).min(), np.abs(v - hi).min()) > 1e-6
    assert int(((y.abs() > 1.1) | (z.abs() > 1.1)).sum()) > 20       # the penalty takes part
    e = mr.plain_torch(y, z, fin["die_label"].long(), 4, BINS, DOMAIN_LENS, erf.oob_weight,
                       w=fin["die_power"])
    rg = torch.autograd.grad(e, q)
    e = e.detach()
    print(f"error {float(err_sum)!r} oracle {float(e)!r}")
    assert float(e) > 0.0 and abs(float(err_sum) - float(e)) <= 10 * tol * float(e)
    for g, r in zip(grads, rg):
        rel = float((g.cpu() - r).abs().max() / r.abs().max())
        print(f"generic: parameter gradient rel err {rel:.2e}")
        assert rel < tol


@pytest.mark.parametrize("what", ["few_rays", "deterministic"])
def test_fallbacks_take_the_generic_path_and_equal_the_reference(what):
    n, kw = (2000, {}) if what == "few_rays" else (8192, dict(deterministic=True))
    runs = {mode: _make(n, mode, weighted=True, **kw) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 4) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert fs is None or fs.steps == 0
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11
    opt, eng, _, _, erf = runs["graph"]
    ref = _finished_reference(eng, erf)
    assert ref["inside"].sum() > n // 2 and ref["groups_used"] == 4
    _assert_last_evaluation(erf, ref)
    assert out["graph"][0][-1] == ref["error"]


@pytest.mark.parametrize("fields", [("y_end",), ("x_dir", "y_dir")], ids=["y_end", "dirs"])
def test_2d_engine_runs_on_the_generic_path_and_equals_the_reference(fields):
    import tfrt.optimizer as optimizer
    from test_gpu_fused_2d import _segment_lens
    eng, params, _ = _segment_lens(torch.float64)
    eng.optical_system.update()
    eng.ray_trace(4)
    n_source = eng.optical_system.sources["x_start"].shape[0]
    groups = np.arange(n_source) % 3
    if len(fields) == 1:
        y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
        domain = ((float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))),)   # some rays outside
        bins = 9
    else:
        domain, bins = ((0.0, 1.0), (-0.2, 0.2)), (4, 5)
    erf = optimizer.MixingError(fields, groups, domain, bins, oob_weight=0.01)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    ref = _finished_reference(eng, erf)
    assert ref["inside"].sum() > 100 and n_terms == 1 and ref["groups_used"] == 3
    if len(fields) == 1:
        assert ref["n_penalised"] > 0
    _assert_last_evaluation(erf, ref)
    assert float(err_sum) == ref["error"] and ref["error"] > 0.0
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_colour_mixing_example_lowers_the_largest_group_error():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "colour_mixing.py"),
                          "--rays", "20000", "--steps", "10"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("max group error: first")][-1]
    first, last = float(line.split()[4]), float(line.split()[6])
    assert last < first
