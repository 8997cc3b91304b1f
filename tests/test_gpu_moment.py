"""
MomentError on the GPU: tfrt_moment_error (clear, SpotError's accumulate, the centres, pass 2,
table, seed) against the numpy reference of tests/moment_error_reference.py, and the error on the
optimiser's paths -- the fused, replayed 3-D step against the generic one, in-place changes of the
target covariance and of the labels under replay, the parameter gradient against the oracle, a
SumError with a SpotError, the fallbacks, 2-D, the example.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import direction_fields_reference as dfr
import moment_error_reference as mr
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}
COUNTS = (0, 1, 65, 3000)
LDS = 256                                   # ops.MOMENT_LDS_GROUPS (asserted below)
SEED_BLOCK = 256                            # the lanes of a workgroup of the seed launch
MODES = ("covariance", "round")


def _mode(mode, G, two):
    return dict(shape="round") if mode == "round" else dict(covariance=mr.targets_for(G, two))


@functools.lru_cache(maxsize=None)
def _case(n, G, np_dtype, two, mode, masked, permuted):
    """The inputs and the reference of one case, computed once and shared (never written to)."""
    x, y, mask, group, perm = mr.rays(n, G, np_dtype)
    kw = _mode(mode, G, two)
    ref = mr.moment_error(x.astype(np.float64), y.astype(np.float64) if two else None, group, G,
                          mr.DOMAIN if two else mr.DOMAIN[:1], oob_weight=mr.OOB,
                          mask=mask if masked else None, perm=perm if permuted else None, **kw)
    return x, y, mask, group, perm, kw, ref


def _on_device(kw):
    return {k: torch.tensor(v, device=DEV) if isinstance(v, np.ndarray) else v
            for k, v in kw.items()}


def _kernel(n, G, dtype, dim, two, mode, masked, permuted, variant=0, pad=3):
    """tfrt_moment_error on a case: x and y are the end rows of a ``dim``-D block with ``pad``
    spare columns; the gradient block starts out as NaN to show what is written."""
    from tensorflowraytrace_amd import ops
    x, y, mask, group, perm, kw, _ = _case(n, G, NP_DTYPE[dtype], two, mode, masked, permuted)
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[dim, :n] = torch.tensor(x, device=DEV)
    rows[dim + 1, :n] = torch.tensor(y, device=DEV)
    g = torch.tensor(group, device=DEV)
    mbits = ops.moment_mbits(g.numel())
    grid = ops.spot_grid(mr.DOMAIN if two else mr.DOMAIN[:1], mbits)
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    out = ops.moment_error(
        rows[:, :n], dim, dim + 1 if two else -1, g, G, grid, oob_weight=mr.OOB,
        mask=torch.tensor(mask, device=DEV) if masked else None,
        perm=torch.tensor(perm, device=DEV) if permuted else None, grad=grad[:, :n],
        variant=variant, dimension=dim, **_on_device(kw))
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), grad.cpu().numpy()) + tuple(t.cpu().numpy() for t in out[2:])


def _bits_equal(a, b):
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _check(got, ref, n, want_grad):
    """``want_grad``: {row: reference gradient row}; every other row must be untouched.  Both
    records equal as integers; centres, covariances, D, the gradient and the error triple bit for
    bit (the reference restates the order of the sums over the groups and over the penalties)."""
    err, grad, acc, mom, group_rows, cov, used = got
    assert np.array_equal(acc, ref["acc"])
    assert np.array_equal(mom, ref["mom"])
    same = _bits_equal(group_rows, ref["group_rows"])
    assert same.all(), f"group rows not bit-equal: groups {np.nonzero(~same.all(axis=1))[0][:5]}"
    same = _bits_equal(cov, ref["cov"])
    assert same.all(), f"C, D not bit-equal: groups {np.nonzero(~same.all(axis=1))[0][:5]}"
    assert used.tolist() == [ref["groups_used"], int(ref["rays"].sum())]
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
    print(f"error {err[0]!r} reference {ref['error']!r}")
    want = np.array([ref["error"], ref["terms"], ref["mean"]])
    assert _bits_equal(err, want).all(), (err, want)
    if not ref["terms"]:
        assert np.isnan(err[2]) and err[0] == 0.0


def _rows_of(ref, dim):
    want = {dim: ref["grad_x"]}
    if ref["grad_y"] is not None:
        want[dim + 1] = ref["grad_y"]
    return want


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("G", [1, 7, LDS, LDS + 1, 2049])
def test_kernel_equals_the_reference(G, dtype, dim):
    """Every count, two fields and one, both modes, with and without mask and perm.  257 groups
    take the global atomics, fewer the tables in LDS; with 2,049 the
    table's per-thread loop takes a third trip."""
    from tensorflowraytrace_amd import ops
    assert ops.MOMENT_LDS_GROUPS == LDS == mr.LDS_GROUPS and ops.DISTORTION_BLOCK == 1024
    for n in COUNTS:
        for two, mode in ((True, "covariance"), (True, "round"), (False, "covariance")):
            for masked, permuted in ((False, False), (True, True)):
                ref = _case(n, G, NP_DTYPE[dtype], two, mode, masked, permuted)[6]
                _check(_kernel(n, G, dtype, dim, two, mode, masked, permuted), ref, n,
                       _rows_of(ref, dim))
    ref = _case(3000, G, NP_DTYPE[dtype], True, "covariance", True, True)[6]
    assert ref["inside"].sum() > 1000 and ref["outside"].sum() > 150 and ref["error"] > 0.0
    if G == 7:
        assert 0 < ref["groups_used"] < int(ref["rays"].sum()) < G


def test_the_second_trip_of_the_grid_stride_loops():
    """One column more than a full grid of each launch -- the full grids of the accumulate
    launches and of the seed launch hold the same number of columns --: the first lane of each
    goes round again."""
    from tensorflowraytrace_amd import _build, ops
    # the constants the kernels are built with: ops states them, the sources are read here
    text = "".join(open(os.path.join(_build.CSRC, f)).read()
                   for f in ("tfrt_common.h", "spot_records.h", "tfrt_moment.hip"))
    for line in (f"constexpr int SPOT_MAX_GRID = {ops.SPOT_MAX_GRID};",
                 "constexpr int SPOT_RAYS_PER_BLOCK = 4 * BLOCK;",
                 f"constexpr int BLOCK = {SEED_BLOCK};",
                 f"constexpr int MOMENT_LDS_GROUPS = {LDS};",
                 f"constexpr int MOMENT_SEED_MAX_GRID = {ops.MOMENT_SEED_MAX_GRID};"):
        assert line in text, line
    n = ops.SPOT_MAX_GRID * ops.SPOT_RAYS_PER_BLOCK + 1
    assert n == ops.MOMENT_SEED_MAX_GRID * SEED_BLOCK + 1 == mr.SEED_CAPACITY + 1
    ref = _case(n, 7, np.float32, True, "round", True, True)[6]
    _check(_kernel(n, 7, torch.float32, 3, True, "round", True, True), ref, n, _rows_of(ref, 3))
    # (the global-atomics variant's pass 2 has the same grid)
    got = _kernel(n, 7, torch.float32, 3, True, "round", True, True, variant=2)
    _check(got, ref, n, _rows_of(ref, 3))


def test_both_accumulate_variants_and_repeated_calls_give_the_same_bytes():
    for mode in MODES:
        args = (3000, 64, torch.float64, 3, True, mode, True, True)
        ref = _case(3000, 64, np.float64, True, mode, True, True)[6]
        lds = _kernel(*args, variant=1)
        _check(lds, ref, 3000, _rows_of(ref, 3))
        for variant in (2, 0):
            for a, b in zip(lds, _kernel(*args, variant=variant)):
                assert a.tobytes() == b.tobytes(), variant
        a = _kernel(3000, 2049, torch.float32, 2, True, mode, True, True)
        b = _kernel(3000, 2049, torch.float32, 2, True, mode, True, True)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
    with pytest.raises(ValueError):
        _kernel(64, LDS + 1, torch.float64, 3, True, "round", False, False, variant=1)


def test_a_padded_stride_changes_nothing():
    for mode in MODES:
        a = _kernel(1000, 7, torch.float32, 3, True, mode, True, True, pad=0)
        b = _kernel(1000, 7, torch.float32, 3, True, mode, True, True, pad=29)
        for u, v in zip(a, b):
            if u.ndim == 2 and u.shape[1] != v.shape[1]:
                assert u[:, :1000].tobytes() == v[:, :1000].tobytes()      # (the gradient block)
            else:
                assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("dim,codes,mode", [
    (d, c, m) for d, c in [(3, (7, 8)), (3, (8,)), (3, (4, 8)), (2, (3, 5)), (2, (5,))]
    for m in MODES if m == "covariance" or len(c) == 2])
def test_direction_and_mixed_fields_are_chained_onto_every_row(dim, codes, mode):
    """Direction and mixed codes of 2-D and 3-D blocks: the covariance of direction cosines (a
    divergence), of a position and a direction (a beam matrix in phase space); the seed writes all
    2 d rows of every column through direction_fields.h."""
    from tensorflowraytrace_amd import ops
    n, G = 1000, 7
    block = dfr.rays(n, np.float64, dimension=dim)
    rng = np.random.default_rng(3)
    group = rng.integers(-1, G - 1, n + 3).astype(np.int32)
    mask = np.where(np.arange(n) % 5 == 4, -1, 0).astype(np.int32)
    two = len(codes) == 2
    domain = tuple(dfr.DOMAIN[i] if c >= 2 * dim else (-0.5, 2.5) for i, c in enumerate(codes))
    kw = _mode(mode, G, two)
    if mode == "covariance":
        kw["covariance"] = kw["covariance"] * 0.1
    ref = mr.fields(block, codes, group, G, domain, oob_weight=mr.OOB, mask=mask, **kw)
    assert ref["inside"].sum() > 150 and ref["outside"].sum() > 50 and ref["groups_used"] >= 3
    grad = torch.full((2 * dim, n + 3), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.tensor(group, device=DEV)
    grid = ops.spot_grid(domain, ops.moment_mbits(g.numel()))
    out = ops.moment_error(torch.tensor(block, device=DEV), codes[0], codes[1] if two else -1,
                           g, G, grid, oob_weight=mr.OOB, mask=torch.tensor(mask, device=DEV),
                           grad=grad[:, :n], dimension=dim, **_on_device(kw))
    torch.cuda.synchronize()
    got = (out[0].cpu().numpy(), grad.cpu().numpy()) + tuple(t.cpu().numpy() for t in out[2:])
    _check(got, ref, n, {row: ref["grad"][row] for row in range(2 * dim)})


def test_bad_arguments_are_refused_before_any_launch():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_moment_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_moment_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_moment_error_workspace_bytes(-1, 4) == 0
    assert L.tfrt_moment_error_workspace_bytes(0, 4) > 0
    t = torch.zeros(1 << 15, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, G=4, dim=3, fx=4, fy=5, x1=1.0, msx=4.0, oob=0.0, ws=1 << 17, stride=8,
             gstride=8, variant=0, group=p, mbits=40, n_source=8, mode=0, target=p, used=p,
             rows=p, cov=p, acc=p, mom=p, err=p, dtype=1):
        return L.tfrt_moment_error(p, stride, n, dtype, dim, None, fx, fy, group, n_source, None,
                                   G, mode, target, 0.0, x1, msx, 0.0, 1.0, 4.0, mbits, oob, p,
                                   gstride, err, used, rows, cov, acc, mom, variant, p, ws, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(dim=1), dict(dim=4), dict(fx=9),
                dict(fy=4), dict(dim=2, fx=6), dict(x1=0.0), dict(msx=0.0), dict(oob=-1.0),
                dict(stride=4), dict(gstride=4), dict(variant=3), dict(variant=-1),
                dict(group=None), dict(n=1 << 31), dict(mbits=42), dict(mbits=39), dict(mbits=0),
                dict(dtype=7), dict(n=1 << 21, stride=1 << 21, gstride=1 << 21),
                dict(G=LDS + 1, variant=1), dict(n_source=-1),
                dict(target=None), dict(mode=1), dict(mode=2), dict(mode=1, target=None, fy=-1),
                dict(used=None), dict(rows=None), dict(rows=p + 8), dict(cov=None),
                dict(acc=None), dict(mom=None), dict(err=None)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    assert call(ws=8, mode=1, target=None) == -2
    torch.cuda.synchronize()
    assert not t.any()                    # nothing was launched: nothing was written
    assert call(n=0) == 0
    assert call(n=0, mode=1, target=None) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", MODES)
def test_reused_buffers_allocate_nothing(mode):
    from tensorflowraytrace_amd import _lib, ops
    n, G = 3000, 64
    x, y, mask, group, perm, kw, ref = _case(n, G, np.float32, True, mode, True, True)
    rows = torch.zeros((6, n), dtype=torch.float32, device=DEV)
    rows[4], rows[5] = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    group, mask, perm = (torch.tensor(v, device=DEV) for v in (group, mask, perm))
    kw = _on_device(kw)
    held = dict(grad=torch.zeros((6, n), dtype=torch.float64, device=DEV),
                err=torch.zeros(3, dtype=torch.float64, device=DEV),
                acc=torch.zeros((G, 4), dtype=torch.int64, device=DEV),
                mom=torch.zeros((G, 9), dtype=torch.int64, device=DEV),
                group_rows=torch.zeros((G, 8), dtype=torch.float64, device=DEV),
                cov=torch.zeros((G, 6), dtype=torch.float64, device=DEV),
                used_out=torch.zeros(2, dtype=torch.float64, device=DEV),
                workspace=torch.empty(_lib.lib().tfrt_moment_error_workspace_bytes(n, G),
                                      dtype=torch.uint8, device=DEV))
    grid = ops.spot_grid(mr.DOMAIN, ops.moment_mbits(group.numel()))

    def call():
        return ops.moment_error(rows, 4, 5, group, G, grid, oob_weight=mr.OOB, mask=mask,
                                perm=perm, **held, **kw)
    call()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    got = call()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    for t, name in zip(got, ("err", "grad", "acc", "mom", "group_rows", "cov", "used_out")):
        assert t is held[name]
    assert np.array_equal(held["acc"].cpu().numpy(), ref["acc"])
    assert np.array_equal(held["mom"].cpu().numpy(), ref["mom"])
    assert _bits_equal(held["cov"].cpu().numpy(), ref["cov"]).all()


# ------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28
CELLS = 6                                    # the object: a 6 x 6 grid of cells over +-0.2
G_CELLS = CELLS * CELLS


def _cells(object_yz):
    """The cell of every start point on the 6 x 6 grid over +-0.2."""
    c = np.clip(np.floor((object_yz + 0.2) / 0.4 * CELLS), 0, CELLS - 1).astype(np.int64)
    return c[:, 0] * CELLS + c[:, 1]


def _make(n_rays, mode, kind="covariance", ray_dtype=torch.float64, with_spot=False, weights=None,
          spot_alone=False, **engine_kw):
    """The lens of tests/test_gpu_centroid.py's ``_make`` with a MomentError over the 36 cells of
    the object.  ``kind`` "covariance": every cell's target is HALF its covariance under the
    starting lens (from one evaluation, written into the term's buffer in place), so that D is no
    difference of nearly equal numbers; cell 5's ``txy`` is free; "round": ``shape="round"``."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype, **engine_kw)
    start = system._amalgamated_sources["object_coords"].detach().cpu().double().numpy()[:, 1:]
    labels = _cells(start)
    kw = dict(shape="round") if kind == "round" else dict(covariance=np.ones((G_CELLS, 3)))
    erf = mom = optimizer.MomentError(("y_end", "z_end"), labels, DOMAIN_LENS,
                                      oob_weight=2.0 / n_rays, n_groups=G_CELLS, **kw)
    lr = 0.2 / n_rays            # (a sum over the rays, as the SpotError of tests/test_gpu_spot.py)
    if with_spot:
        spot = optimizer.SpotError(("y_end", "z_end"), labels, DOMAIN_LENS,
                                   oob_weight=2.0 / n_rays, n_groups=G_CELLS)
        erf = optimizer.SumError([spot] if spot_alone else [spot, mom], weights=weights,
                                 reduce="mean")
        lr = 0.4
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    if kind == "covariance":
        probe = optimizer.SGD_Optimizer(eng, lens.parameters, mom, 3, learning_rate=lr,
                                        grad_clip=1e9, fused=False)
        probe.suppress_warnings = True
        probe.raw_gradient()                          # (the generic path; no parameter moves)
        half = 0.5 * mom.covariances().clone()
        half[5, 1] = float("nan")
        mom.covariance.copy_(half)
    return opt, eng, lens, (system, target, source), mom


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def _finished_reference(eng, erf):
    """The reference on the engine's finished rays with the term's CURRENT labels and target."""
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].cpu().numpy()
    dim = eng.dimension
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end") if dim == 3 \
        else ("x_start", "y_start", "x_end", "y_end")
    block = np.stack([fin[f].detach().cpu().double().numpy() for f in names])
    kw = dict(shape="round") if erf.covariance is None else \
        dict(covariance=erf.covariance.cpu().numpy())
    return mr.fields(block, tuple(erf.rows_for(dim)), erf.labels.cpu().numpy(), erf.n_groups,
                     erf.domain, oob_weight=erf.oob_weight, perm=ids, **kw), ids


def _assert_last_evaluation(erf, ref):
    assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
    assert np.array_equal(erf.last_mom.cpu().numpy(), ref["mom"])
    assert _bits_equal(erf.last_cov.cpu().numpy(), ref["cov"]).all()
    assert _bits_equal(erf.last_rows.cpu().numpy(), ref["group_rows"]).all()
    assert erf.groups_used == ref["groups_used"]


@pytest.mark.parametrize("kind", MODES)
def test_fused_step_equals_the_generic_step(kind):
    """4,096 rays (traced in place), 6 steps: the same errors, parameters and covariances at the
    tolerances of tests/test_gpu_centroid.py's test of the same name; the step is one graph
    replay."""
    runs = {mode: _make(4096, mode, kind) for mode in ("generic", "graph")}
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
    assert erf.groups_used == other.groups_used >= 25
    assert int(erf.last_acc[:, 0].sum()) > 2000
    assert erf.centroids().shape == (36, 2)
    assert erf.covariances().shape == erf.residuals().shape == (36, 3)
    np.testing.assert_allclose(erf.residuals().cpu().numpy(), other.residuals().cpu().numpy(),
                               rtol=0, atol=1e-8)
    # the last replayed step's tables are the reference's on that trace's finished rays
    ref, _ = _finished_reference(runs["graph"][1], erf)
    assert ref["inside"].sum() > 2000
    _assert_last_evaluation(erf, ref)


@pytest.mark.parametrize("what", ["covariance", "labels"])
def test_replays_see_in_place_changes(what):
    """Overwriting ``covariance`` (the labels) in place between replays: the next replay reads
    the new values -- the same graph object, one more replay, the reference's tables for the new
    values."""
    opt, eng, lens, _, erf = _make(4096, "graph", "covariance")
    _steps(opt, lens, 5)
    fs = opt._fused_step
    for _ in range(4):
        if fs.graph_replays >= 1:
            break
        _steps(opt, lens, 1)
    assert fs is not None and fs.in_place and fs.graph_replays >= 1 and fs.capture_error is None
    graph, replays, key = fs._graphs[1], fs.graph_replays, erf.graph_key()
    before = erf.last_cov.cpu().numpy().copy()
    if what == "covariance":
        erf.covariance.mul_(0.5)
        erf.covariance[9] = float("nan")
    else:
        erf.labels.copy_((erf.labels + 1) % G_CELLS)
    assert erf.graph_key() == key
    _steps(opt, lens, 1)
    assert fs._graphs[1] is graph and fs.graph_replays == replays + 1
    ref, _ = _finished_reference(eng, erf)
    _assert_last_evaluation(erf, ref)
    after = erf.last_cov.cpu().numpy()
    assert np.nanmax(np.abs(after - before)) > 1e-3
    if what == "covariance":
        assert not after[9, 3:].any()


def _torch_objective(v, label, domain, oob, covariance=None, shape=None, n_groups=G_CELLS):
    """The full objective in torch float64 with DIFFERENTIABLE centroids (and size s): ``v``
    (2, n) the fields, ``label`` (n,) the group of every column.  Per group of at least two
    columns inside the mean, the covariance about it and ``n * |D|_F^2``; plus the penalties."""
    label = torch.as_tensor(label).long()
    lo = torch.tensor([d[0] for d in domain], dtype=torch.float64)[:, None]
    hi = torch.tensor([d[1] for d in domain], dtype=torch.float64)[:, None]
    out = ((v < lo) | (v > hi)).any(dim=0)
    inside, outside = (label >= 0) & ~out, (label >= 0) & out
    ex = torch.relu(lo - v) + torch.relu(v - hi)
    total = oob * (ex * ex).sum(dim=0)[outside].sum()
    for g in range(n_groups):
        at = inside & (label == g)
        m = int(at.sum())
        if m < 2:
            continue
        d = v[:, at] - v[:, at].mean(dim=1, keepdim=True)
        C = [(d[0] * d[0]).mean(), (d[0] * d[1]).mean(), (d[1] * d[1]).mean()]
        if shape is not None:
            s = (C[0] + C[2]) / 2.0
            D = [C[0] - s, C[1], C[2] - s]
        else:
            D = [torch.zeros((), dtype=torch.float64) if bool(torch.isnan(covariance[g, c]))
                 else C[c] - covariance[g, c] for c in range(3)]
        total = total + m * (D[0] * D[0] + 2.0 * (D[1] * D[1]) + D[2] * D[2])
    return total


@pytest.mark.parametrize("kind,ray_dtype", [
    ("covariance", torch.float64), ("round", torch.float64), ("covariance", torch.float32),
    ("round", torch.float32)], ids=["covariance-f64", "round-f64", "covariance-f32", "round-f32"])
def test_parameter_gradient_equals_the_oracle(kind, ray_dtype):
    """4,096 rays, one step: d error / d parameters on the generic path and on the fused step's
    fixed-shape path against the oracle's float64 trace composed with a plain torch restatement
    whose centroids and size ARE differentiated, under autograd.  float64 state: the project's
    1e-9.  float32 state: E32 is what rounding the oracle's finished rows to float32 does to this
    gradient (measured here, on the oracle alone: the rounded rows enter the objective, their
    derivative is the unrounded rows'), and the kernels are bound at max(1e-5, 8 * E32).

    Measured on the MI355X (largest over the two parameter tensors): E32 = 4.5e-8 (covariance) and
    2.6e-8 (round), so the bound is 1e-5; the kernels with float32 state 5.2e-7 and 4.1e-7, the
    generic and the fused path alike; with float64 state 3.8e-12 and 5.9e-12."""
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    opt, eng, lens, (system, target, source), erf = _make(4096, "eager", kind, ray_dtype)
    grads, err_sum, n_terms = opt.raw_gradient()
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    if ray_dtype == torch.float32:
        for k in ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end"):
            src[k] = src[k].float().double()
    src["cell_label"] = erf.labels.cpu().double()
    ref = tracer.ray_trace(osys, src, max_iterations=3,
                           inherit=("wavelength", "object_coords", "cell_label"))
    fin = ref["finished"]
    v = torch.stack([fin["y_end"], fin["z_end"]])
    label = fin["cell_label"].long()
    assert n_terms == 2 * v.shape[1] and v.shape[1] > 2000
    for row, (lo, hi) in zip(v.detach().numpy(), erf.domain):
        assert min(np.abs(row - lo).min(), np.abs(row - hi).min()) > 1e-6
    kw = dict(shape="round") if kind == "round" else dict(covariance=erf.covariance.cpu())
    e = _torch_objective(v, label, erf.domain, erf.oob_weight, **kw)
    rg = torch.autograd.grad(e, q, retain_graph=True)
    tol = 1e-9
    if ray_dtype == torch.float32:
        v32 = v + (v.float().double() - v).detach()
        r32 = torch.autograd.grad(_torch_objective(v32, label, erf.domain, erf.oob_weight, **kw),
                                  q)
        e32 = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(r32, rg))
        tol = max(1e-5, 8.0 * e32)
        print(f"E32 {e32:.2e}: bound {tol:.2e}")
    e = e.detach()
    print(f"error {float(err_sum)!r} oracle {float(e)!r}")
    assert float(e) > 0.0 and abs(float(err_sum) - float(e)) <= 10 * tol * float(e)
    if kind == "covariance":
        # D is no difference of nearly equal numbers: the targets are half the covariance
        D, C = erf.residuals().cpu().numpy(), erf.covariances().cpu().numpy()
        used = np.isfinite(C[:, 0])
        assert (np.abs(D[used, 0]) > 0.4 * C[used, 0]).all()

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
    assert float(err3[1]) == 2 * v.shape[1]


def test_a_sum_with_a_spot_error_runs_fused_and_equals_the_generic_step():
    runs = {mode: _make(4096, mode, "round", with_spot=True) for mode in ("generic", "graph")}
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
    assert runs["graph"][4].groups_used == runs["generic"][4].groups_used >= 25


def test_a_weight_of_zero_switches_the_term_off():
    """SumError([spot, moment], weights=[1, 0]) steps as the SpotError of the same sum alone (its
    own mean): the same parameters at the fused test's tolerance; the term is still evaluated."""
    off = _make(4096, "graph", "round", with_spot=True, weights=[1.0, 0.0])
    alone = _make(4096, "graph", "round", with_spot=True, spot_alone=True)
    a, b = _steps(off[0], off[2], 6), _steps(alone[0], alone[2], 6)
    assert off[0]._fused_step is not None and off[0]._fused_step.graph_replays > 0
    np.testing.assert_allclose(a[0], b[0], rtol=1e-10, atol=0)
    for u, v in zip(a[1], b[1]):
        assert float((u - v).abs().max()) <= 1e-11
    triples = off[0].error_function.last_errors.cpu().numpy()
    assert triples[1, 0] > 0.0 and off[4].groups_used >= 25
    assert float(off[0].error_function.last_coefficients[1]) == 0.0


@pytest.mark.parametrize("what", ["few_rays", "deterministic"])
def test_fallbacks_take_the_generic_path_and_equal_the_reference(what):
    n, kw = (2000, {}) if what == "few_rays" else (4096, dict(deterministic=True))
    runs = {mode: _make(n, mode, "covariance", **kw) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 4) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert fs is None or fs.steps == 0
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11
    opt, eng, _, _, erf = runs["graph"]
    ref, _ = _finished_reference(eng, erf)
    assert ref["inside"].sum() > n // 2 and ref["groups_used"] >= 25
    _assert_last_evaluation(erf, ref)
    # (n terms and 2 G group terms in another order: Higham, eq. 4.4, as the sibling tests)
    assert abs(out["graph"][0][-1] * ref["terms"] - ref["error"]) <= \
        2.0 * (2 * ref["n"] + 2 * G_CELLS) * mr.EPS * ref["abs_sum"] + 1e-12 * ref["error"]


@pytest.mark.parametrize("fields", [("y_end",), ("x_dir", "y_dir")], ids=["y_end", "dirs"])
def test_2d_engine_runs_on_the_generic_path_and_equals_the_reference(fields):
    import tfrt.optimizer as optimizer
    from test_gpu_fused_2d import _segment_lens
    eng, params, _ = _segment_lens(torch.float64)
    eng.optical_system.update()
    eng.ray_trace(4)
    n_source = eng.optical_system.sources["x_start"].shape[0]
    groups = np.arange(n_source) * 9 // n_source                           # neighbours together
    if len(fields) == 1:
        y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
        domain = ((float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))),)   # some rays outside
        kw = dict(covariance=1e-4)
    else:
        domain = ((0.0, 1.0), (-0.2, 0.2))
        kw = dict(shape="round")
    erf = optimizer.MomentError(fields, groups, domain, oob_weight=0.01, **kw)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    ref, _ = _finished_reference(eng, erf)
    assert ref["inside"].sum() > 100 and n_terms == len(fields) * ref["n"]
    assert ref["groups_used"] >= 3 and ref["error"] > 0.0
    if len(fields) == 1:
        assert ref["outside"].sum() > 0
    _assert_last_evaluation(erf, ref)
    assert abs(float(err_sum) - ref["error"]) <= \
        2.0 * (2 * ref["n"] + 18) * mr.EPS * ref["abs_sum"]
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_imaging_example_round_spots_lowers_the_moment_terms_error():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "imaging.py"),
                          "--round-spots", "--rays", "20000", "--steps", "20"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines()
            if ln.startswith("mean squared covariance residual: first")][-1]
    first, last = float(line.split()[5]), float(line.split()[7])
    assert last < first
    assert any(ln.startswith("largest anisotropy over") for ln in out.stdout.splitlines())
