"""
CentroidError on the GPU: tfrt_centroid_error (clear, SpotError's accumulate, with parents their
records, table, seed) against the numpy reference of tests/centroid_error_reference.py, and the
error on the optimiser's paths -- the fused, replayed 3-D step against the generic one, in-place
changes of targets and parents under replay, the parameter gradient against the oracle, a SumError
with a SpotError, the fallbacks, 2-D, the example.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import centroid_error_reference as cr
import direction_fields_reference as dfr
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}
COUNTS = (0, 1, 63, 64, 65, 1000, 4097)
LDS = 1024                                  # ops.SPOT_LDS_GROUPS (asserted below)
SEED_BLOCK = 256                            # the lanes of a workgroup of the seed launch


def _mode(mode, G, two, P):
    if mode == "targets":
        return (("targets", cr.targets_for(G, two)),)
    return (("parents", cr.parents_for(G, P)), ("n_parents", P))


@functools.lru_cache(maxsize=None)
def _case(n, G, np_dtype, two, mode, P, masked, permuted):
    """The inputs and the reference of one case, computed once and shared (never written to)."""
    x, y, mask, group, perm = cr.rays(n, G, np_dtype)
    kw = dict(_mode(mode, G, two, P))
    ref = cr.centroid_error(x.astype(np.float64), y.astype(np.float64) if two else None, group, G,
                            cr.DOMAIN if two else cr.DOMAIN[:1], oob_weight=cr.OOB,
                            mask=mask if masked else None, perm=perm if permuted else None, **kw)
    return x, y, mask, group, perm, kw, ref


def _on_device(kw):
    return {k: torch.tensor(v, device=DEV) if isinstance(v, np.ndarray) else v
            for k, v in kw.items()}


def _kernel(n, G, dtype, dim, two, mode, P, masked, permuted, variant=0, pad=3):
    """tfrt_centroid_error on a case: x and y are the end rows of a ``dim``-D block with ``pad``
    spare columns; the gradient block starts out as NaN to show what is written."""
    from tensorflowraytrace_amd import ops
    x, y, mask, group, perm, kw, _ = _case(n, G, NP_DTYPE[dtype], two, mode, P, masked, permuted)
    rows = torch.full((2 * dim, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[dim, :n] = torch.tensor(x, device=DEV)
    rows[dim + 1, :n] = torch.tensor(y, device=DEV)
    g = torch.tensor(group, device=DEV)
    qbits = ops.spot_qbits(g.numel())
    grid = ops.spot_grid(cr.DOMAIN if two else cr.DOMAIN[:1], qbits)
    grad = torch.full((2 * dim, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    err, _, acc, residual, used, pacc = ops.centroid_error(
        rows[:, :n], dim, dim + 1 if two else -1, g, G, grid, oob_weight=cr.OOB,
        mask=torch.tensor(mask, device=DEV) if masked else None,
        perm=torch.tensor(perm, device=DEV) if permuted else None, grad=grad[:, :n],
        variant=variant, dimension=dim, **_on_device(kw))
    pc = None if pacc is None else ops.centroid_parent_centroids(pacc, grid, 2 if two else 1)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy()
                 for t in (err, grad, acc, residual, used, pacc, pc))


def _bits_equal(a, b):
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _check(got, ref, n, want_grad):
    """``want_grad``: {row: reference gradient row}; every other row must be untouched.  Records
    equal as integers; residual table, parent centroids, gradient and the error triple bit for
    bit (the reference restates the order of the sums over the groups and over the penalties)."""
    err, grad, acc, residual, used, pacc, pc = got
    assert np.array_equal(acc, ref["acc"])
    same = _bits_equal(residual, ref["residual"])
    assert same.all(), f"residuals not bit-equal: groups {np.nonzero(~same.all(axis=1))[0][:5]}"
    assert used.tolist() == [ref["groups_used"], ref["parents_used"]]
    if ref["parent_acc"] is None:
        assert pacc is None
    else:
        assert np.array_equal(pacc, ref["parent_acc"])
        assert _bits_equal(pc, ref["parent_centroids"]).all()
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


def _parent_counts(G):
    return sorted({1, 3, G, 1025})


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("G", [1, 7, LDS, LDS + 1, 2049])
def test_kernel_equals_the_reference(G, dtype, dim):
    """Every count, two fields and one, both modes, with and without mask and perm.  1,025 groups
    take the global atomics, fewer the table in LDS; with 2,049 the table's per-thread loop takes
    a third trip; the parents: 1, 3, G and 1,025 (more parents than groups, a second trip of the
    loop over the parents)."""
    from tensorflowraytrace_amd import ops
    assert ops.SPOT_LDS_GROUPS == LDS and ops.DISTORTION_BLOCK == cr.BLOCK == 1024
    for n in COUNTS:
        for two in (True, False):
            for masked, permuted in ((False, False), (True, True)):
                modes = [("targets", 0)]
                # (every P on the largest count and on n = 65; P = 3 on the others)
                modes += [("parents", P) for P in (_parent_counts(G) if n in (65, 4097) else (3,))]
                for mode, P in modes:
                    ref = _case(n, G, NP_DTYPE[dtype], two, mode, P, masked, permuted)[6]
                    _check(_kernel(n, G, dtype, dim, two, mode, P, masked, permuted), ref, n,
                           _rows_of(ref, dim))
    ref = _case(4097, G, NP_DTYPE[dtype], True, "targets", 0, True, True)[6]
    assert ref["n_inside"] > 1500 and ref["n_penalised"] > 200
    if G == 7:
        assert 0 < ref["groups_used"] < int(ref["rays"].sum()) < G


def test_the_second_trip_of_the_grid_stride_loops():
    """One column more than a full grid of each launch -- the two full grids hold the same number
    of columns --: the first lane of the accumulate launch and of the seed launch goes round
    again."""
    from tensorflowraytrace_amd import _build, ops
    # the constants the kernels are built with: ops states them, the sources are read here
    text = "".join(open(os.path.join(_build.CSRC, f)).read()
                   for f in ("tfrt_common.h", "spot_records.h", "residual_seed.h"))
    for line in (f"constexpr int SPOT_MAX_GRID = {ops.SPOT_MAX_GRID};",
                 "constexpr int SPOT_RAYS_PER_BLOCK = 4 * BLOCK;",
                 f"constexpr int BLOCK = {SEED_BLOCK};",
                 f"constexpr int DISTORTION_SEED_MAX_GRID = {ops.DISTORTION_SEED_MAX_GRID};"):
        assert line in text, line
    assert ops.SPOT_RAYS_PER_BLOCK == 4 * SEED_BLOCK == cr.ACC_COLUMNS
    assert ops.SPOT_MAX_GRID == cr.ACC_MAX_GRID and cr.ACC_BLOCK == SEED_BLOCK
    n = ops.SPOT_MAX_GRID * ops.SPOT_RAYS_PER_BLOCK + 1
    assert n == ops.DISTORTION_SEED_MAX_GRID * SEED_BLOCK + 1
    for mode, P in (("targets", 0), ("parents", 3)):
        ref = _case(n, 7, np.float32, True, mode, P, True, True)[6]
        _check(_kernel(n, 7, torch.float32, 3, True, mode, P, True, True), ref, n, _rows_of(ref, 3))


def test_both_accumulate_variants_and_repeated_calls_give_the_same_bytes():
    for mode, P in (("targets", 0), ("parents", 3)):
        args = (4097, 64, torch.float64, 3, True, mode, P, True, True)
        ref = _case(4097, 64, np.float64, True, mode, P, True, True)[6]
        lds = _kernel(*args, variant=1)
        glb = _kernel(*args, variant=2)
        again = _kernel(*args, variant=0)
        _check(lds, ref, 4097, _rows_of(ref, 3))
        for other in (glb, again):
            for a, b in zip(lds, other):
                assert (a is None and b is None) or a.tobytes() == b.tobytes()
        a = _kernel(4097, 2049, torch.float32, 2, True, mode, P, True, True)
        b = _kernel(4097, 2049, torch.float32, 2, True, mode, P, True, True)
        for u, v in zip(a, b):
            assert (u is None and v is None) or u.tobytes() == v.tobytes()
    with pytest.raises(ValueError):
        _kernel(64, LDS + 1, torch.float64, 3, True, "targets", 0, False, False, variant=1)


def test_a_padded_stride_changes_nothing():
    for mode, P in (("targets", 0), ("parents", 3)):
        a = _kernel(1000, 7, torch.float32, 3, True, mode, P, True, True, pad=0)
        b = _kernel(1000, 7, torch.float32, 3, True, mode, P, True, True, pad=29)
        for u, v in zip(a, b):
            if u is None:
                assert v is None
            elif u.ndim == 2 and u.shape[1] != v.shape[1]:
                assert u[:, :1000].tobytes() == v[:, :1000].tobytes()      # (the gradient block)
            else:
                assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("mode", ["targets", "parents"])
@pytest.mark.parametrize("dim,codes", [(3, (7, 8)), (3, (8,)), (3, (4, 8)), (2, (3, 5)),
                                       (2, (5,))])
def test_direction_and_mixed_fields_are_chained_onto_every_row(dim, codes, mode):
    """Direction and mixed codes of 2-D and 3-D blocks: the centroids are mean direction cosines,
    and the seed writes all 2 d rows of every column through direction_fields.h."""
    from tensorflowraytrace_amd import ops
    n, G = 1000, 7
    block = dfr.rays(n, np.float64, dimension=dim)
    rng = np.random.default_rng(3)
    group = rng.integers(-1, G - 1, n + 3).astype(np.int32)
    mask = np.where(np.arange(n) % 5 == 4, -1, 0).astype(np.int32)
    two = len(codes) == 2
    domain = tuple(dfr.DOMAIN[i] if c >= 2 * dim else (-0.5, 2.5) for i, c in enumerate(codes))
    kw = dict(_mode(mode, G, two, 3))
    if mode == "targets":
        kw["targets"] = kw["targets"] * 0.1
    ref = cr.fields(block, codes, group, G, domain, oob_weight=cr.OOB, mask=mask, **kw)
    assert ref["n_inside"] > 150 and ref["n_penalised"] > 50 and ref["groups_used"] >= 3
    grad = torch.full((2 * dim, n + 3), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.tensor(group, device=DEV)
    qbits = ops.spot_qbits(g.numel())
    grid = ops.spot_grid(domain, qbits)
    out = ops.centroid_error(torch.tensor(block, device=DEV), codes[0], codes[1] if two else -1,
                             g, G, grid, oob_weight=cr.OOB, mask=torch.tensor(mask, device=DEV),
                             grad=grad[:, :n], dimension=dim, **_on_device(kw))
    pc = None if out[5] is None else ops.centroid_parent_centroids(out[5], grid, len(codes))
    torch.cuda.synchronize()
    got = (out[0].cpu().numpy(), grad.cpu().numpy()) + tuple(
        None if t is None else t.cpu().numpy() for t in out[2:] + (pc,))
    _check(got, ref, n, {row: ref["grad"][row] for row in range(2 * dim)})


def test_bad_arguments_are_refused_before_any_launch():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_centroid_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_centroid_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_centroid_error_workspace_bytes(-1, 4) == 0
    assert L.tfrt_centroid_error_workspace_bytes(0, 4) > 0
    t = torch.zeros(1 << 15, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, G=4, dim=3, fx=4, fy=5, x1=1.0, qsx=4.0, oob=0.0, ws=1 << 17, stride=8,
             gstride=8, variant=0, group=p, qbits=40, n_source=8, targets=p, parents=None, P=0,
             pacc=None, used=p, residual=p, acc=p, err=p, dtype=1):
        return L.tfrt_centroid_error(p, stride, n, dtype, dim, None, fx, fy, group, n_source, None,
                                     G, targets, parents, P, pacc, 0.0, x1, qsx, 0.0, 1.0, 4.0,
                                     qbits, oob, p, gstride, err, used, residual, acc, variant, p,
                                     ws, None)
    by_parent = dict(targets=None, parents=p, P=2, pacc=p)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(dim=1), dict(dim=4), dict(fx=9),
                dict(fy=4), dict(dim=2, fx=6), dict(x1=0.0), dict(qsx=0.0), dict(oob=-1.0),
                dict(stride=4), dict(gstride=4), dict(variant=3), dict(group=None),
                dict(n=1 << 31), dict(qbits=53), dict(qbits=0), dict(dtype=7),
                dict(n=1 << 22, stride=1 << 22, gstride=1 << 22), dict(G=LDS + 1, variant=1),
                dict(n_source=-1), dict(targets=None), dict(parents=p, P=2, pacc=p),
                dict(by_parent, P=0), dict(by_parent, P=2 ** 20 + 1), dict(by_parent, pacc=None),
                dict(used=None), dict(residual=None), dict(residual=p + 8), dict(acc=None),
                dict(err=None)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    assert call(ws=8, **by_parent) == -2
    torch.cuda.synchronize()
    assert not t.any()                    # nothing was launched: nothing was written
    assert call(n=0) == 0
    assert call(n=0, **by_parent) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode,P", [("targets", 0), ("parents", 3)])
def test_reused_buffers_allocate_nothing(mode, P):
    from tensorflowraytrace_amd import _lib, ops
    n, G = 4097, 64
    x, y, mask, group, perm, kw, ref = _case(n, G, np.float32, True, mode, P, True, True)
    rows = torch.zeros((6, n), dtype=torch.float32, device=DEV)
    rows[4], rows[5] = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    group, mask, perm = (torch.tensor(v, device=DEV) for v in (group, mask, perm))
    kw = _on_device(kw)
    grad = torch.zeros((6, n), dtype=torch.float64, device=DEV)
    err = torch.zeros(3, dtype=torch.float64, device=DEV)
    acc = torch.zeros((G, 4), dtype=torch.int64, device=DEV)
    used = torch.zeros(2, dtype=torch.float64, device=DEV)
    residual = torch.zeros((G, 2), dtype=torch.float64, device=DEV)
    pacc = torch.zeros((P, 4), dtype=torch.int64, device=DEV) if P else None
    ws = torch.empty(_lib.lib().tfrt_centroid_error_workspace_bytes(n, G), dtype=torch.uint8,
                     device=DEV)
    grid = ops.spot_grid(cr.DOMAIN, ops.spot_qbits(group.numel()))

    def call():
        return ops.centroid_error(rows, 4, 5, group, G, grid, oob_weight=cr.OOB, mask=mask,
                                  perm=perm, grad=grad, err=err, acc=acc, residual=residual,
                                  used_out=used, parent_acc=pacc, workspace=ws, **kw)
    call()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    got = call()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert got[0] is err and got[1] is grad and got[2] is acc and got[3] is residual \
        and got[4] is used and got[5] is pacc
    assert np.array_equal(acc.cpu().numpy(), ref["acc"])
    assert _bits_equal(residual.cpu().numpy(), ref["residual"]).all()


# ------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28
DOMAIN_DIR = ((-0.3, 0.3), (-0.3, 0.3))      # their (y_dir, z_dir)
CELLS = 6                                    # the object: a 6 x 6 grid of cells over +-0.2
KINDS = ("targets", "parents", "direction")


def _cells(object_yz):
    """(labels, points): the cell of every start point on the 6 x 6 grid over +-0.2 and the
    (36, 2) cell centres."""
    c = np.clip(np.floor((object_yz + 0.2) / 0.4 * CELLS), 0, CELLS - 1).astype(np.int64)
    centre = -0.2 + (np.arange(CELLS) + 0.5) * (0.4 / CELLS)
    g = np.arange(CELLS * CELLS)
    return c[:, 0] * CELLS + c[:, 1], np.stack([centre[g // CELLS], centre[g % CELLS]], axis=1)


def _term_kw(kind, points):
    """The fields, the domain and the mode of a kind of term over the 36 cells: the centroid of
    every cell at -4 times its centre (cell 5 not pinned); the cells of a row of the grid
    registered onto each other (cell 7 left out); every cell's mean direction along the axis."""
    G = CELLS * CELLS
    if kind == "targets":
        t = -4.0 * points
        t[5] = np.nan
        return ("y_end", "z_end"), DOMAIN_LENS, dict(targets=t)
    if kind == "parents":
        p = np.arange(G) // CELLS
        p[7] = -1
        return ("y_end", "z_end"), DOMAIN_LENS, dict(parents=p, n_parents=CELLS)
    return ("y_dir", "z_dir"), DOMAIN_DIR, dict(targets=np.zeros((G, 2)))


def _make(n_rays, mode, kind="targets", ray_dtype=torch.float64, with_spot=False, weights=None,
          spot_alone=False, **engine_kw):
    """The lens of tests/test_gpu_distortion.py's ``_make`` with a CentroidError over the 36 cells
    of the object."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype, **engine_kw)
    start = system._amalgamated_sources["object_coords"].detach().cpu().double().numpy()[:, 1:]
    labels, points = _cells(start)
    fields, domain, kw = _term_kw(kind, points)
    erf = cent = optimizer.CentroidError(fields, labels, domain, oob_weight=2.0 / n_rays,
                                         n_groups=CELLS * CELLS, **kw)
    lr = 0.2 / n_rays            # (a sum over the rays, as the SpotError of tests/test_gpu_spot.py)
    if with_spot:
        spot = optimizer.SpotError(("y_end", "z_end"), labels, DOMAIN_LENS,
                                   oob_weight=2.0 / n_rays, n_groups=CELLS * CELLS)
        erf = optimizer.SumError([spot] if spot_alone else [spot, cent], weights=weights,
                                 reduce="mean")
        lr = 0.4
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source), cent


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def _finished_reference(eng, erf):
    """The reference on the engine's finished rays with the term's labels and its CURRENT targets
    or parents."""
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].cpu().numpy()
    dim = eng.dimension
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end") if dim == 3 \
        else ("x_start", "y_start", "x_end", "y_end")
    block = np.stack([fin[f].detach().cpu().double().numpy() for f in names])
    kw = dict(targets=erf.targets.cpu().numpy()) if erf.targets is not None else \
        dict(parents=erf.parents.cpu().numpy(), n_parents=erf.n_parents)
    return cr.fields(block, tuple(erf.rows_for(dim)), erf.labels.cpu().numpy(), erf.n_groups,
                     erf.domain, oob_weight=erf.oob_weight, perm=ids, **kw), ids


def _assert_last_evaluation(erf, ref):
    assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
    assert _bits_equal(erf.last_residual.cpu().numpy(), ref["residual"]).all()
    assert erf.groups_used == ref["groups_used"]
    if erf.parents is not None:
        assert _bits_equal(erf.parent_centroids().cpu().numpy(), ref["parent_centroids"]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_fused_step_equals_the_generic_step(kind):
    """8,192 rays (traced in place), 6 steps: the same errors, parameters and residual tables at
    the tolerances of tests/test_gpu_distortion.py's test of the same name; the step is one graph
    replay."""
    runs = {mode: _make(8192, mode, kind) for mode in ("generic", "graph")}
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
    assert int(erf.last_acc[:, 0].sum()) > 4000
    assert erf.centroids().shape == erf.residuals().shape == (36, 2)
    np.testing.assert_allclose(erf.residuals().cpu().numpy(), other.residuals().cpu().numpy(),
                               rtol=0, atol=1e-8)
    if kind == "parents":
        assert erf.parent_centroids().shape == (CELLS, 2)
    # the last replayed step's tables are the reference's on that trace's finished rays
    ref, _ = _finished_reference(runs["graph"][1], erf)
    assert ref["n_inside"] > 4000
    _assert_last_evaluation(erf, ref)


@pytest.mark.parametrize("kind", ["targets", "parents"])
def test_replays_see_in_place_changes(kind):
    """Overwriting ``targets`` (``parents``) in place between replays: the next replay reads the
    new values -- the same graph object, one more replay, the reference's tables for the new
    values."""
    opt, eng, lens, _, erf = _make(8192, "graph", kind)
    _steps(opt, lens, 5)
    fs = opt._fused_step
    for _ in range(4):
        if fs.graph_replays >= 1:
            break
        _steps(opt, lens, 1)
    assert fs is not None and fs.in_place and fs.graph_replays >= 1 and fs.capture_error is None
    graph, replays, key = fs._graphs[1], fs.graph_replays, erf.graph_key()
    before = erf.last_residual.cpu().numpy().copy()
    if kind == "targets":
        erf.targets.mul_(0.5)
        erf.targets[9] = float("nan")
    else:
        erf.parents.copy_(torch.arange(36, device=DEV, dtype=torch.int32) % CELLS)
        erf.parents[14] = CELLS
    assert erf.graph_key() == key
    _steps(opt, lens, 1)
    assert fs._graphs[1] is graph and fs.graph_replays == replays + 1
    ref, _ = _finished_reference(eng, erf)
    _assert_last_evaluation(erf, ref)
    after = erf.last_residual.cpu().numpy()
    assert np.nanmax(np.abs(after - before)) > 1e-3
    assert not after[9 if kind == "targets" else 14].any()


def _torch_objective(v, label, domain, oob, targets=None, parents=None, n_parents=None):
    """The full objective in torch float64 with DIFFERENTIABLE centroids: ``v`` (k, n) the
    fields, ``label`` (n,) the group of every column in a group or penalised, -1 otherwise.  Per
    group the mean of its columns inside; per parent the mean of the columns inside of its
    groups; the sum over the columns inside of |c_group - t_group|^2, plus the penalties."""
    k = v.shape[0]
    label = torch.as_tensor(label).long()
    lo = torch.tensor([d[0] for d in domain], dtype=torch.float64)[:, None]
    hi = torch.tensor([d[1] for d in domain], dtype=torch.float64)[:, None]
    out = ((v < lo) | (v > hi)).any(dim=0)
    inside, outside = (label >= 0) & ~out, (label >= 0) & out
    ex = torch.relu(lo - v) + torch.relu(v - hi)
    pen = oob * (ex * ex).sum(dim=0)[outside].sum()
    li, vi = label[inside], v[:, inside]
    ones = torch.ones(li.shape[0], dtype=torch.float64)
    if targets is not None:
        t = torch.as_tensor(targets, dtype=torch.float64)
        G = t.shape[0]
        has = torch.isfinite(t).all(dim=1)
        t = torch.where(has[:, None], t, torch.zeros_like(t)).t()
    else:
        p = torch.as_tensor(parents).long()
        G = p.shape[0]
        has = (p >= 0) & (p < n_parents)
        pi = p.clamp(0, n_parents - 1)[li]
        sel = has[li]
        pcnt = torch.zeros(n_parents, dtype=torch.float64).index_add(0, pi[sel], ones[sel])
        pS = torch.zeros((k, n_parents), dtype=torch.float64).index_add(1, pi[sel], vi[:, sel])
        t = (pS / pcnt.clamp(min=1.0))[:, p.clamp(0, n_parents - 1)]
    cnt = torch.zeros(G, dtype=torch.float64).index_add(0, li, ones)
    S = torch.zeros((k, G), dtype=torch.float64).index_add(1, li, vi)
    used = (cnt > 0) & has
    r = S[:, used] / cnt[used] - t[:, used]
    return (cnt[used] * (r * r).sum(dim=0)).sum() + pen


@pytest.mark.parametrize("kind,ray_dtype,tol", [
    ("targets", torch.float64, 1e-9), ("parents", torch.float64, 1e-9),
    ("direction", torch.float64, 1e-9), ("targets", torch.float32, 1e-5),
    ("parents", torch.float32, 1e-5)],
    ids=["targets-f64", "parents-f64", "direction-f64", "targets-f32", "parents-f32"])
def test_parameter_gradient_equals_the_oracle(kind, ray_dtype, tol):
    """4,096 rays, one step: d error / d parameters on the generic path and on the fused step's
    fixed-shape path against the oracle's float64 trace composed with a plain torch restatement
    whose centroids and parents' centroids ARE differentiated, under autograd -- the check of "no
    derivative of a centroid is needed" -- at the project's 1e-9 with float64 state and 1e-5 with
    float32 state (the oracle then traces the source rounded to float32, as
    tests/test_gpu_spot.py's test of the same name does).  Direction fields with float64 state
    only: with float32 state a direction is good to ``eps32 * max|coordinate| / L``."""
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
    if kind == "direction":
        e3 = torch.stack([fin[a + "_end"] - fin[a + "_start"] for a in "xyz"])
        v = (e3 / torch.sqrt((e3 * e3).sum(dim=0)))[1:]
    else:
        v = torch.stack([fin["y_end"], fin["z_end"]])
    label = fin["cell_label"].long()
    assert n_terms == 2 * v.shape[1] and v.shape[1] > 2000
    for row, (lo, hi) in zip(v.detach().numpy(), erf.domain):
        assert min(np.abs(row - lo).min(), np.abs(row - hi).min()) > 1e-6
    kw = dict(targets=erf.targets.cpu()) if erf.targets is not None else \
        dict(parents=erf.parents.cpu(), n_parents=erf.n_parents)
    e = _torch_objective(v, label, erf.domain, erf.oob_weight, **kw)
    rg = torch.autograd.grad(e, q)
    e = e.detach()
    print(f"error {float(err_sum)!r} oracle {float(e)!r}")
    assert float(e) > 0.0 and abs(float(err_sum) - float(e)) <= 10 * tol * float(e)

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


@pytest.mark.parametrize("kind", ["targets", "parents"])
def test_float32_state_fused_equals_generic(kind):
    """float32 state (position fields: with float32 state a direction is good to ``eps32 *
    max|coordinate| / L`` only): the fused step against the generic one, which runs the same
    kernels on the same float32 rows, at the project's 1e-5 for float32 state.  (Both against
    the oracle: ``test_parameter_gradient_equals_the_oracle``.)"""
    tol = 1e-5
    from tensorflowraytrace_amd.fused_step import FusedStep
    opt, eng, lens, _, erf = _make(4096, "eager", kind, torch.float32)
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
    runs = {mode: _make(8192, mode, "direction", with_spot=True) for mode in ("generic", "graph")}
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
    """SumError([spot, centroid], weights=[1, 0]) steps as the SpotError of the same sum alone
    (its own mean): the same parameters at the fused test's tolerance; the term is still
    evaluated."""
    off = _make(8192, "graph", "parents", with_spot=True, weights=[1.0, 0.0])
    alone = _make(8192, "graph", "parents", with_spot=True, spot_alone=True)
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
    n, kw = (2000, {}) if what == "few_rays" else (8192, dict(deterministic=True))
    runs = {mode: _make(n, mode, "parents", **kw) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 4) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert fs is None or fs.steps == 0
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11
    opt, eng, _, _, erf = runs["graph"]
    ref, _ = _finished_reference(eng, erf)
    assert ref["n_inside"] > n // 2 and ref["groups_used"] >= 25
    _assert_last_evaluation(erf, ref)
    assert abs(out["graph"][0][-1] * ref["terms"] - ref["error"]) <= \
        cr.error_bound(ref) + 1e-12 * ref["error"]


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
        kw = dict(parents=np.arange(9) // 3)
    else:
        domain = ((0.0, 1.0), (-0.2, 0.2))
        t = np.tile([1.0, 0.0], (9, 1))
        t[4] = np.nan
        kw = dict(targets=t)
    erf = optimizer.CentroidError(fields, groups, domain, oob_weight=0.01, **kw)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    ref, _ = _finished_reference(eng, erf)
    assert ref["n_inside"] > 100 and n_terms == len(fields) * ref["n"]
    assert ref["groups_used"] >= 3 and ref["error"] > 0.0
    if len(fields) == 1:
        assert ref["n_penalised"] > 0
    _assert_last_evaluation(erf, ref)
    assert abs(float(err_sum) - ref["error"]) <= cr.error_bound(ref)
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_imaging_example_telecentric_lowers_the_centroid_terms_error():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "imaging.py"),
                          "--telecentric", "--rays", "8192", "--steps", "8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines()
            if ln.startswith("mean squared mean direction: first")][-1]
    first, last = float(line.split()[5]), float(line.split()[7])
    assert last < first
    assert any(ln.startswith("largest |mean direction cosine|") for ln in out.stdout.splitlines())
