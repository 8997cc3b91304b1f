"""
CentroidError without a GPU: the CPU path of ops.centroid_error against the numpy reference of
tests/centroid_error_reference.py bit for bit, the invariance under a permutation of the columns,
the residuals that must vanish exactly, the gradient against the analytic gradient of the
unquantised definition, a descent toy, the argument checks of the class, the op and the entry,
the exports, the generic path on CPU tensors, and csrc/centroid_math.h compiled for the host under
the address and undefined-behaviour sanitizers.
"""
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import centroid_error_reference as cr
import direction_fields_reference as dfr
from tensorflowraytrace_amd import ops, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "centroid_host", "centroid_main.cpp")
EPS = cr.EPS


def _mode(mode, G, two, P=None):
    """The keyword arguments of a mode for the reference: ``targets`` or ``parents``."""
    if mode == "targets":
        return dict(targets=cr.targets_for(G, two))
    P = P or max(min(G, 3), 1)
    return dict(parents=cr.parents_for(G, P), n_parents=P)


def _torch_mode(kw):
    out = {k: torch.tensor(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    return out


def _case(n, G, two, mode, masked=False, permuted=False, dtype=np.float64, P=None):
    x, y, mask, group, perm = cr.rays(n, G, dtype)
    domain = cr.DOMAIN if two else cr.DOMAIN[:1]
    kw = _mode(mode, G, two, P)
    ref = cr.centroid_error(x.astype(np.float64), y.astype(np.float64) if two else None, group, G,
                            domain, oob_weight=cr.OOB, mask=mask if masked else None,
                            perm=perm if permuted else None, **kw)
    return (x, y, mask, group, perm, domain, kw), ref


def _cpu(case, two, masked, permuted, dim=3, qbits=None):
    x, y, mask, group, perm, domain, kw = case
    n = x.shape[0]
    rows = torch.full((2 * dim, n), 7.0, dtype=torch.tensor(x).dtype)
    rows[dim], rows[dim + 1] = torch.tensor(x), torch.tensor(y)
    g = torch.tensor(group)
    grad = torch.full((2 * dim, n), float("nan"), dtype=torch.float64)
    qb = ops.spot_qbits(g.numel()) if qbits is None else qbits
    out = ops.centroid_error(
        rows, dim, dim + 1 if two else -1, g,
        kw["targets" if "targets" in kw else "parents"].shape[0], ops.spot_grid(domain, qb),
        oob_weight=cr.OOB,
        mask=torch.tensor(mask) if masked else None, perm=torch.tensor(perm) if permuted else None,
        grad=grad, dimension=dim, qbits=qb, **_torch_mode(kw))
    return [None if t is None else t.numpy() for t in out]


def _bits_equal(a, b):
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _assert_equal(got, ref, dim, two):
    err, grad, acc, residual, used_out, parent_acc = got
    assert np.array_equal(acc, ref["acc"])
    assert _bits_equal(residual, ref["residual"]).all()
    if ref["parent_acc"] is None:
        assert parent_acc is None
    else:
        assert np.array_equal(parent_acc, ref["parent_acc"])
    assert used_out.tolist() == [ref["groups_used"], ref["parents_used"]]
    assert grad[dim].tobytes() == ref["grad_x"].tobytes()
    if two:
        assert grad[dim + 1].tobytes() == ref["grad_y"].tobytes()
    assert np.isnan(np.delete(grad, [dim, dim + 1][:2 if two else 1], axis=0)).all()
    assert err[1] == ref["terms"]
    assert abs(err[0] - ref["error"]) <= cr.error_bound(ref)
    if ref["terms"]:
        assert err[2] == err[0] / err[1]
    else:
        assert np.isnan(err[2])


@pytest.mark.parametrize("mode", ["targets", "parents"])
@pytest.mark.parametrize("G", [1, 7, 1025, 2049])
def test_cpu_path_equals_the_reference(G, mode):
    """Both modes, one and two fields, 2-D and 3-D blocks, f32 and f64 rows, masked and permuted
    columns, labels -1 and G, parents -1 and P, NaN target rows, empty groups; n = 0 and 1."""
    for n in (0, 1, 65, 1000):
        for two in (True, False):
            for flags in ((False, False), (True, True)):
                for dtype, dim in ((np.float64, 3), (np.float32, 2)):
                    case, ref = _case(n, G, two, mode, *flags, dtype=dtype)
                    _assert_equal(_cpu(case, two, *flags, dim=dim), ref, dim, two)
                    if n == 1000 and G == 7:
                        assert 0 < ref["groups_used"] < int(ref["rays"].sum()) < G
                        assert ref["n_penalised"] > 50 and ref["n_inside"] > 400


@pytest.mark.parametrize("mode", ["targets", "parents"])
@pytest.mark.parametrize("dim,codes", [(3, (7, 8)), (3, (8,)), (3, (4, 8)), (2, (3, 5)),
                                       (2, (2, 3)), (2, (5,))])
def test_cpu_path_with_direction_fields_equals_the_reference(dim, codes, mode):
    """Direction and mixed codes: the centroids are mean direction cosines, and all 2 d rows of
    every column are written through the chain rule."""
    n, G = 1000, 7
    block = dfr.rays(n, np.float64, dimension=dim)
    rng = np.random.default_rng(3)
    group = rng.integers(-1, G - 1, n + 3).astype(np.int32)
    mask = np.where(np.arange(n) % 5 == 4, -1, 0).astype(np.int32)
    two = len(codes) == 2
    # (a position field of these blocks spans [-1, 4]; a direction cosine dfr.DOMAIN)
    domain = tuple(dfr.DOMAIN[i] if c >= 2 * dim else (-0.5, 2.5) for i, c in enumerate(codes))
    kw = _mode(mode, G, two)
    if mode == "targets":
        kw["targets"] = kw["targets"] * 0.1
    ref = cr.fields(block, codes, group, G, domain, oob_weight=cr.OOB, mask=mask, **kw)
    assert ref["n_inside"] > 150 and ref["n_penalised"] > 50 and ref["groups_used"] >= 3
    grad = torch.full((2 * dim, n), float("nan"), dtype=torch.float64)
    g = torch.tensor(group)
    out = ops.centroid_error(torch.tensor(block), codes[0], codes[1] if two else -1, g, G,
                             ops.spot_grid(domain, ops.spot_qbits(g.numel())), oob_weight=cr.OOB,
                             mask=torch.tensor(mask), grad=grad, dimension=dim, **_torch_mode(kw))
    assert np.array_equal(out[2].numpy(), ref["acc"])
    assert np.array_equal(out[3].numpy(), ref["residual"], equal_nan=True)
    has_dir = any(c >= 2 * dim for c in codes)
    for row in range(2 * dim):
        if has_dir or row in codes:
            assert grad[row].numpy().tobytes() == ref["grad"][row].tobytes(), row
        else:
            assert np.isnan(grad[row].numpy()).all()
    assert abs(float(out[0][0]) - ref["error"]) <= cr.error_bound(ref)


@pytest.mark.parametrize("mode", ["targets", "parents"])
def test_permuting_the_columns_changes_no_bit(mode):
    """The records are integer sums and the sums over the groups have a fixed order: the records,
    the residual table, the counts and (without penalties, whose sum is the columns') the error
    are the same bits in any order of the columns."""
    n, G = 1000, 7
    (x, y, mask, group, perm, domain, kw), _ = _case(n, G, True, mode)
    rng = np.random.default_rng(1)
    order = rng.permutation(n)
    src = np.arange(n, dtype=np.int32)
    outs = []
    for o in (np.arange(n), order):
        case = (x[o], y[o], mask, group, src[o].copy(), domain, kw)
        rows = torch.zeros((6, n), dtype=torch.float64)
        rows[3], rows[4] = torch.tensor(case[0]), torch.tensor(case[1])
        g = torch.tensor(group)
        grid = ops.spot_grid(domain, ops.spot_qbits(n + 3))
        outs.append(ops.centroid_error(rows, 3, 4, g, G, grid, oob_weight=0.0,
                                       perm=torch.tensor(case[4]),
                                       **_torch_mode(kw)))
    a, b = outs
    assert a[2].numpy().tobytes() == b[2].numpy().tobytes()
    assert a[3].numpy().tobytes() == b[3].numpy().tobytes()
    assert a[4].tolist() == b[4].tolist()
    assert a[0].numpy().tobytes() == b[0].numpy().tobytes()
    if mode == "parents":
        assert a[5].numpy().tobytes() == b[5].numpy().tobytes()
    assert np.array_equal(a[1].numpy()[:, order], b[1].numpy())


@pytest.mark.parametrize("mode", ["targets", "parents"])
@pytest.mark.parametrize("G", [7, 1024, 1025, 2049])
def test_without_penalties_the_cpu_error_is_the_reference_s_bit_for_bit(G, mode):
    """``oob_weight = 0``: every penalty is 0.0, so the error is the groups' sums alone, whose
    shape and order the CPU path restates (``ops.distortion_group_sum``) as the reference does
    (``fixed_sum``): two fields, up to three trips of the loop over the groups, the same bits."""
    n = 4097
    x, y, mask, group, perm = cr.rays(n, G)
    kw = _mode(mode, G, True)
    ref = cr.centroid_error(x, y, group, G, cr.DOMAIN, oob_weight=0.0, mask=mask, perm=perm, **kw)
    assert ref["groups_used"] >= 3 and ref["error"] > 0.0 and ref["n_penalised"] > 200
    rows = torch.zeros((6, n), dtype=torch.float64)
    rows[3], rows[4] = torch.tensor(x), torch.tensor(y)
    g = torch.tensor(group)
    err = ops.centroid_error(rows, 3, 4, g, G, ops.spot_grid(cr.DOMAIN, ops.spot_qbits(g.numel())),
                             oob_weight=0.0, mask=torch.tensor(mask), perm=torch.tensor(perm),
                             **_torch_mode(kw))[0].numpy()
    want = np.array([ref["error"], ref["terms"], ref["mean"]])
    assert _bits_equal(err, want).all(), (err, want)


def test_the_penalty_sum_has_the_shape_of_the_launches():
    """``penalty_sum`` against an independent, lane-by-lane restatement of the two launches with
    Python floats, at counts on both sides of one workgroup, of the grid's limit and of a second
    trip (small strides stand in for 512 workgroups: the constants are arguments of neither, so
    the big case runs once)."""
    rng = np.random.default_rng(2)
    for n in (1, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097, 512 * 1024 + 1):
        pen = rng.uniform(0.0, 1.0, n)
        out = rng.random(n) < 0.3
        B = min(512, (n + 1023) // 1024)
        partial = []
        for b in range(B):
            lanes = [0.0] * 256
            for t in range(256):
                for i in range(256 * b + t, n, 256 * B):
                    if out[i]:
                        lanes[t] += float(pen[i])
            waves = []
            for w in range(4):
                v = lanes[64 * w:64 * w + 64]
                for d in (32, 16, 8, 4, 2, 1):
                    v = [v[k] + v[k ^ d] for k in range(64)]
                waves.append(v[0])
            s = 0.0
            for w in waves:
                s += w
            partial.append(s)
        lanes = partial + [0.0] * (1024 - B)
        total = 0.0
        for w in range(16):
            v = lanes[64 * w:64 * w + 64]
            for d in (32, 16, 8, 4, 2, 1):
                v = [v[k] + v[k ^ d] for k in range(64)]
            total += v[0]
        assert float(cr.penalty_sum(np.where(out, pen, 0.0), out)) == total, n


@pytest.mark.parametrize("G", [1, 7, 1025])
def test_every_group_its_own_parent_has_residuals_exactly_zero(G):
    """``parents = arange(G)``: a parent's record IS its group's, so C_p and c_g are the same
    expression of the same integers and r = 0.0 exactly; one parent with one group likewise."""
    n = 1000
    x, y, mask, group, perm = cr.rays(n, G)
    for two in (True, False):
        domain = cr.DOMAIN if two else cr.DOMAIN[:1]
        ref = cr.centroid_error(x, y if two else None, group, G, domain,
                                parents=np.arange(G, dtype=np.int32), n_parents=G,
                                oob_weight=cr.OOB)
        case = (x, y, mask, group, perm, domain,
                dict(parents=np.arange(G, dtype=np.int32), n_parents=G))
        got = _cpu(case, two, False, False)
        _assert_equal(got, ref, 3, two)
        res = got[3]
        assert ref["groups_used"] == int(ref["rays"].sum()) >= 1
        assert (res[ref["rays"]] == 0.0).all() and np.isnan(res[~ref["rays"]]).all()
        inside = ref["inside"]
        assert not got[1][3][inside].any()
        assert got[0][0] == pytest.approx(ref["error"], abs=cr.error_bound(ref))


def _exact_gradient(x, y, ref, kw, two):
    """The analytic gradient of the UNQUANTISED definition on the reference's classification:
    exact float64 centroids (``math.fsum``, one division), 2 (c_g - t_g) for a ray inside."""
    G = ref["n_groups"]
    li = ref["label"][ref["inside"]]
    out = []
    for v in ((x, y) if two else (x,)):
        vi = v[ref["inside"]]
        c = np.array([math.fsum(vi[li == g]) / max(int((li == g).sum()), 1) for g in range(G)])
        cnt = np.array([int((li == g).sum()) for g in range(G)])
        axis = len(out)
        if "targets" in kw:
            t = kw["targets"][:, axis]
            has = np.isfinite(kw["targets"]).all(axis=1)
        else:
            p, P = kw["parents"].astype(np.int64), kw["n_parents"]
            has = (p >= 0) & (p < P)
            t = np.zeros(G)
            for q in range(P):
                m = has & (p == q) & (cnt > 0)
                rays = np.isin(li, np.nonzero(m)[0])
                if rays.any():
                    t[m] = math.fsum(vi[rays]) / int(rays.sum())
        r = np.where(has & (cnt > 0), c - np.where(has, t, 0.0), 0.0)
        g = np.zeros(v.shape[0])
        g[ref["inside"]] = 2.0 * r[li]
        out.append(g)
    return out


@pytest.mark.parametrize("qbits", [None, 20])
@pytest.mark.parametrize("mode", ["targets", "parents"])
@pytest.mark.parametrize("two", [True, False], ids=["k2", "k1"])
def test_gradient_against_the_exact_definition(two, mode, qbits):
    """The kernel's gradient 2 r on quantised records against the analytic gradient of the
    unquantised definition, per axis at most ``2 / qs + (12 D + 4 M) eps`` with D the width of
    the axis' domain and M the largest absolute value in it.

    ``2 / qs``: every ray's coordinate is rounded to a multiple of 1 / qs, at most half a step
    off, so a mean of them -- a centroid, a parent's centroid -- is at most half a step off; r
    holds one of each (with ``targets`` only the former), the gradient is 2 r:
    2 * (1/2 + 1/2) / qs.

    The rounding term, with u = eps / 2 and every error in x units.  A ray's ``(x - x0) * qs``
    is two operations on a value of at most D: 2 u D, and so at most for a mean of them.  The
    quantised centroid adds ``(double) Sx``, ``/ count`` and ``/ qs`` (u D each) and ``x0 +``
    (u M): 5 u D + u M in all.  The exact centroid is one division of an exact sum: u M.  A
    centroid therefore differs by at most 5 u D + 2 u M beyond its half step, and so does a
    parent's.  ``c - t`` rounds once in each of the two evaluations, |c - t| <= D: 2 u D.  For r:
    2 * (5 u D + 2 u M) + 2 u D = 12 u D + 4 u M; the gradient doubles it (exactly):
    24 u D + 8 u M = (12 D + 4 M) eps.  Derived from the expressions, not measured."""
    n, G = 1000, 7
    (x, y, mask, group, perm, domain, kw), _ = _case(n, G, two, mode)
    x, y = x.astype(np.float64), y.astype(np.float64)
    ref = cr.centroid_error(x, y if two else None, group, G, domain, oob_weight=cr.OOB,
                            qbits=qbits, **kw)
    got = _cpu((x, y, mask, group, perm, domain, kw), two, False, False, qbits=qbits)
    assert got[1][3].tobytes() == ref["grad_x"].tobytes()
    exact = _exact_gradient(x, y, ref, kw, two)
    for axis, (want, qs) in enumerate(zip(exact, (ref["qsx"], ref["qsy"]))):
        lo, hi = domain[axis]
        bound = 2.0 / qs + (12.0 * (hi - lo) + 4.0 * max(abs(lo), abs(hi))) * EPS
        inside = ref["inside"]           # (a ray outside carries the penalty's derivative)
        diff = float(np.abs(got[1][3 + axis] - want)[inside].max())
        print(f"axis {axis}: largest gradient {np.abs(want).max():.3e} difference {diff:.3e} "
              f"bound {bound:.3e}")
        assert np.abs(want[ref["inside"]]).max() > 1e-2
        assert diff <= bound


def test_descent_brings_every_centroid_onto_its_target_and_keeps_the_spread():
    """Plain gradient steps on free points under a ``targets`` term: a ray's gradient is 2 r_g,
    so a step of 1/4 halves every residual; the rays of a group move together, so the spread of a
    group stays what it was."""
    rng = np.random.default_rng(11)
    G, per = 5, 40
    lab = np.repeat(np.arange(G), per)
    centre = rng.uniform(-0.5, 0.5, (G, 2))
    pts = centre[lab] + 0.05 * rng.standard_normal((G * per, 2))
    targets = rng.uniform(-0.5, 0.5, (G, 2))
    erf = optimizer.CentroidError(("y_end", "z_end"), lab, ((-1.0, 1.0), (-1.0, 1.0)),
                                  targets=targets)
    erf.labels = erf.labels.cpu()
    rows = torch.tensor(pts.T.copy())
    spread0 = rows - erf_centroids(rows, lab, G)
    errs = []
    for _ in range(60):
        err, grad = erf.evaluate(rows, 0, 1, erf.labels)[:2]
        errs.append(float(err[0]))
        rows = rows - 0.25 * grad
    assert erf.groups_used == G
    c = erf.centroids().numpy()
    assert np.abs(c - targets).max() <= 1e-12
    assert np.abs(erf.residuals().numpy()).max() <= 1e-12
    assert errs[-1] <= 1e-20 < 1e-3 < errs[0] and errs[1] < 0.3 * errs[0]
    spread = rows - erf_centroids(rows, lab, G)
    assert float((spread - spread0).abs().max()) <= 1e-13       # (60 steps of a few eps each)
    assert float(spread0.abs().max()) > 0.05


def erf_centroids(rows, lab, G):
    lab = torch.tensor(lab)
    c = torch.stack([torch.stack([rows[a, lab == g].mean() for g in range(G)]) for a in (0, 1)])
    return c[:, lab]


def test_ops_argument_errors():
    rows = torch.zeros((6, 5), dtype=torch.float64)
    g = torch.zeros(5, dtype=torch.int32)
    t = torch.zeros((3, 2), dtype=torch.float64)
    p = torch.zeros(3, dtype=torch.int32)
    grid = ops.spot_grid(cr.DOMAIN, ops.spot_qbits(5))
    ok = dict(rows=rows, row_x=4, row_y=5, group=g, n_groups=3, grid=grid, targets=t)
    for bad, match in ((dict(group=g.long()), "group"), (dict(n_groups=0), "n_groups"),
                       (dict(parents=p, n_parents=1), "exactly one"),
                       (dict(targets=None), "exactly one"), (dict(row_y=4), "distinct"),
                       (dict(targets=t[:, :1].contiguous()), "targets"),
                       (dict(targets=t.float()), "targets"),
                       (dict(targets=None, parents=p), "n_parents"),
                       (dict(targets=None, parents=p, n_parents=0), "n_parents"),
                       (dict(targets=None, parents=p, n_parents=2 ** 20 + 1), "n_parents"),
                       (dict(targets=None, parents=p.double(), n_parents=1), "parents"),
                       (dict(targets=None, parents=p[:2], n_parents=1), "parents"),
                       (dict(variant=3), "variant"),
                       (dict(n_groups=1025, targets=torch.zeros((1025, 2), dtype=torch.float64),
                             variant=1), "variant"),
                       (dict(mask=torch.zeros(5)), "mask"),
                       (dict(grad=torch.zeros((4, 5), dtype=torch.float64)), "grad"),
                       (dict(acc=torch.zeros((3, 8), dtype=torch.int64)), "acc"),
                       (dict(used_out=torch.zeros(3, dtype=torch.float64)), "used_out"),
                       (dict(residual=torch.zeros((3, 3), dtype=torch.float64)), "residual"),
                       (dict(targets=None, parents=p, n_parents=2,
                             parent_acc=torch.zeros((3, 4), dtype=torch.int64)), "parent_acc")):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.centroid_error(**kw)


def test_the_class_checks_its_arguments_and_is_exported():
    import tfrt.optimizer
    from tensorflowraytrace_amd import errors, fused_step
    C = optimizer.CentroidError
    assert tfrt.optimizer.CentroidError is C and fused_step.CentroidError is C \
        and errors.CentroidError is C and C in errors._COUPLED
    lab = np.arange(12) % 4
    tg = np.array([[0.0, 0.1], [np.nan, 0.0], [0.2, 0.3], [0.0, 0.0]])
    erf = C(("y_end", "z_end"), lab, cr.DOMAIN, targets=tg)
    assert erf.n_groups == 4 and erf.labels.dtype == torch.int32 and erf.parents is None
    assert erf.targets.dtype == torch.float64 and tuple(erf.targets.shape) == (4, 2)
    assert erf.rows == [4, 5] and erf.seed_rows == 0x30 and erf.on_columns
    with pytest.raises(ValueError, match="2-D engine"):
        erf.rows_for(2)
    far = C(("y_dir", "z_dir"), lab, cr.DOMAIN, parents=[0, 0, 1, -1])
    assert far.has_direction and far.seed_rows == 0x3f and far.rows_for(3) == [7, 8]
    assert far.parents.dtype == torch.int32 and far.n_parents == 2 and far.targets is None
    one = C("y_end", torch.tensor(lab), cr.DOMAIN[:1], targets=tg[:, 0], n_groups=4)
    assert tuple(one.targets.shape) == (4, 1) and one.rows_for(2) == [3]
    every = C("y_end", lab, cr.DOMAIN[:1])                       # neither: one parent for all
    assert every.parents.tolist() == [0, 0, 0, 0] and every.n_parents == 1
    assert C("y_end", lab, cr.DOMAIN[:1], parents=[-1, -1, -1, -1]).n_parents == 1
    assert C("y_end", lab, cr.DOMAIN[:1], parents=[0, 0, 1, 1], n_parents=5).n_parents == 5
    inf = tg.copy()
    inf[2, 1] = np.inf
    for bad in (dict(targets=tg, parents=[0, 0, 1, 1]), dict(fields=("y_end", "y_end")),
                dict(domain=cr.DOMAIN[:1]), dict(domain=((0.0, 0.0), (0.0, 1.0))),
                dict(oob_weight=-1.0), dict(targets=inf), dict(targets=-inf),
                dict(targets=tg[:3]), dict(targets=tg[:, :1]), dict(targets="here"),
                dict(targets=tg, n_parents=2), dict(parents=[0.0, 0.0, 1.0, 1.0]),
                dict(parents=np.zeros(4)), dict(parents=[0, 0, 1]), dict(parents=[[0, 0, 1, 1]]),
                dict(parents=[0, 0, 1, 1], n_parents=0),
                dict(parents=[0, 0, 1, 1], n_parents=2 ** 20 + 1),
                dict(parents=[0, 0, 1, 1], n_parents="many"), dict(groups=np.zeros(3)),
                dict(groups=lambda src: lab), dict(n_groups=0), dict(n_groups=2 ** 20 + 1)):
        kw = dict(fields=("y_end", "z_end"), groups=lab, domain=cr.DOMAIN)
        kw.update(bad)
        with pytest.raises(ValueError, match="CentroidError"):
            C(**kw)
    with pytest.raises(TypeError):
        C(("y_end", "z_end"), lab, cr.DOMAIN, targets=tg, weights=np.ones(12))   # (no weights)
    assert C(("y_end", "z_end"), lambda src: lab, cr.DOMAIN, targets=tg, n_groups=4).labels is None
    for read in (erf.centroids, erf.residuals, far.parent_centroids, lambda: erf.groups_used):
        with pytest.raises(RuntimeError, match="no evaluation"):
            read()
    with pytest.raises(RuntimeError, match="needs parents"):
        erf.parent_centroids()
    # graph_key: the label buffer and the targets / parents buffer; in-place writes keep it
    k0, f0 = erf.graph_key(), far.graph_key()
    erf.labels.add_(0)
    erf.targets.add_(0.0)
    far.parents.add_(0)
    assert erf.graph_key() == k0 and far.graph_key() == f0 and k0 != f0
    erf.targets = erf.targets.clone()
    far.parents = far.parents.clone()
    assert erf.graph_key() != k0 and far.graph_key() != f0
    # a legal term of a SumError, named in its message
    spot = optimizer.SpotError(("y_end", "z_end"), lab, cr.DOMAIN)
    both = optimizer.SumError([spot, erf], reduce="mean")
    assert both.terms == (spot, erf) and both.rows == [4, 5, 4, 5]
    with pytest.raises(ValueError, match="FlatFieldError or CentroidError instances"):
        optimizer.SumError([erf, object()])


class _Engine:
    def __init__(self, block, ids, n_source, dim):
        names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end") if dim == 3 \
            else ("x_start", "y_start", "x_end", "y_end")
        self.dimension = dim
        self.leaves = [torch.tensor(r, requires_grad=True) for r in block]
        self.finished_rays = dict(zip(names, self.leaves))
        self.last_trace = {"finished_id": torch.tensor(ids)}
        self._trace_src = {"x_start": torch.zeros(n_source)}


@pytest.mark.parametrize("mode", ["targets", "parents"])
def test_the_generic_path_returns_the_terms_and_the_gradient_rows(mode):
    """CentroidError.__call__ on CPU tensors: (n, k) terms whose sum is the reference's error and,
    through backward, the reference's gradient on the fields' rows; the read-outs report the
    reference's tables."""
    n, G = 300, 7
    (x, y, mask, group, perm, domain, kw), ref = _case(n, G, True, mode, permuted=True)
    erf = optimizer.CentroidError(("y_end", "z_end"), group, domain, oob_weight=cr.OOB,
                                  n_groups=G, **kw)
    erf.labels = erf.labels.cpu()
    block = np.zeros((6, n))
    block[4], block[5] = x, y
    eng = _Engine(block, perm, n + 3, 3)
    e = erf(eng)
    assert e.shape == (n, 2) and e.dtype == torch.float64
    (3.0 * e.sum()).backward()
    assert abs(float(e.detach().sum()) - ref["error"]) <= cr.error_bound(ref)
    assert np.array_equal(erf.last_acc.numpy(), ref["acc"])
    assert np.array_equal(eng.leaves[4].grad.numpy(), 3.0 * ref["grad_x"])
    assert np.array_equal(eng.leaves[5].grad.numpy(), 3.0 * ref["grad_y"])
    assert eng.leaves[0].grad is None                  # (a row that is no field: untouched)
    assert erf.groups_used == ref["groups_used"] > 2
    assert np.array_equal(erf.residuals().numpy(), ref["residual"], equal_nan=True)
    assert np.array_equal(erf.centroids().numpy(), ref["centroids"], equal_nan=True)
    if mode == "parents":
        assert np.array_equal(erf.parent_centroids().numpy(), ref["parent_centroids"],
                              equal_nan=True)
    eng.finished_rays = {}
    assert erf(eng).shape == (0, 2)
    with pytest.raises(ValueError, match="label"):
        erf(_Engine(block, perm, n, 3))


def test_the_optimiser_takes_the_generic_path_on_the_cpu_backend(cpu_backend):
    """SGD_Optimizer with a CentroidError on the oracle-backed CPU stand-ins: the step's error is
    the reference's on the traced rays."""
    from test_host_logic import _lens_api
    eng, system, lens, target = _lens_api(200)
    groups = np.arange(200) % 5
    domain = ((-5.0, 5.0), (-5.0, 5.0))
    erf = optimizer.CentroidError(("y_end", "z_end"), groups, domain, parents=[0, 0, 1, 1, -1])
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=2e-3, grad_clip=1e9)
    grads, err_sum, n_terms = opt.raw_gradient()
    assert opt._fused_step is None
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].numpy()
    ref = cr.centroid_error(fin["y_end"].detach().numpy(), fin["z_end"].detach().numpy(), groups,
                            5, domain, parents=np.array([0, 0, 1, 1, -1]), n_parents=2, perm=ids)
    assert ref["terms"] == n_terms > 300 and ref["groups_used"] == 4 and ref["error"] > 0.0
    assert abs(float(err_sum) - ref["error"]) <= cr.error_bound(ref)
    assert any(float(g.abs().max()) > 0 for g in grads)


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    L = _lib.lib()
    assert L.tfrt_centroid_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_centroid_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_centroid_error_workspace_bytes(-1, 4) == 0
    small = L.tfrt_centroid_error_workspace_bytes(0, 4)
    assert 0 < small <= L.tfrt_centroid_error_workspace_bytes(1_000_000, 2 ** 20)
    dummy = ctypes.create_string_buffer(1 << 17)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 8)

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
                dict(n=1 << 22, stride=1 << 22, gstride=1 << 22), dict(G=1025, variant=1),
                dict(n_source=-1), dict(targets=None), dict(parents=p, P=2, pacc=p),
                dict(by_parent, P=0), dict(by_parent, P=2 ** 20 + 1), dict(by_parent, pacc=None),
                dict(used=None), dict(residual=None), dict(residual=odd), dict(acc=None),
                dict(err=None)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    assert call(ws=8, **by_parent) == -2


def test_centroid_math_on_the_host_under_the_sanitizers(tmp_path):
    """Every group's weight and centroid, the parents' records and centroids, the residual table
    and the groups' error terms of centroid_math.h equal the reference's bit for bit, in both
    modes and with one and two fields; the program's vectors are exact-size allocations and it
    runs under the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "centroid_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
    for n, G, two, mode, P in ((1000, 7, True, "targets", 0), (1000, 7, True, "parents", 3),
                               (300, 2049, True, "parents", 1025), (1000, 30, False, "targets", 0),
                               (1000, 30, False, "parents", 30), (65, 3, False, "parents", 1),
                               (1, 3, True, "targets", 0), (0, 1, True, "parents", 1)):
        (x, y, mask, group, perm, domain, kw), ref = _case(n, G, two, mode, True, True, P=P or None)
        k = 2 if two else 1
        qbits = cr.qbits_of(group.shape[0])
        one = np.ldexp(1.0, qbits)
        qs = [one / (d[1] - d[0]) for d in domain] + [0.0]
        lo = [d[0] for d in domain] + [0.0]
        tail = f8(kw["targets"]) if mode == "targets" else kw["parents"].astype(np.int32).tobytes()
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(struct.pack("<3q", G, k, P) + f8([lo[0], qs[0], lo[1], qs[1]])
                        + ref["acc"].tobytes() + tail)
        run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert run.returncode == 0, f"{n} {G} {two} {mode}: {run.stdout}{run.stderr}"
        raw = dst.read_bytes()
        assert len(raw) == 8 * ((3 + 2 + 2 + 1) * G + (4 + 3) * P)
        f = np.frombuffer(raw[:64 * G], dtype=np.float64)
        grp = f[:3 * G].reshape(G, 3)
        residual = f[3 * G:5 * G].reshape(G, 2)
        err_t = f[5 * G:7 * G].reshape(G, 2)
        used = f[7 * G:8 * G]
        rays = ref["rays"]
        w = ref["acc"][:, 0].astype(np.float64)
        c = np.zeros((G, 2))
        c[:, :k] = np.where(rays[:, None], ref["centroids"], 0.0)
        assert np.array_equal(grp, np.column_stack([w, c]))
        assert np.array_equal(residual, ref["residual"], equal_nan=True)
        assert np.array_equal(used != 0.0, ref["used"])
        r = np.where(ref["used"][:, None], ref["residual"], 0.0)
        assert np.array_equal(err_t, w[:, None] * (r * r))
        if P:
            pacc = np.frombuffer(raw[64 * G:64 * G + 32 * P], dtype=np.int64).reshape(P, 4)
            par = np.frombuffer(raw[64 * G + 32 * P:], dtype=np.float64).reshape(P, 3)
            assert np.array_equal(pacc, ref["parent_acc"])
            C = np.zeros((P, 2))
            C[:, :k] = np.where(np.isnan(ref["parent_centroids"]), 0.0, ref["parent_centroids"])
            assert np.array_equal(par, np.column_stack([pacc[:, 0].astype(np.float64), C]))
