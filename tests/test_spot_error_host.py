"""
SpotError without a GPU: the numpy reference (tests/spot_error_reference.py) against
torch.autograd on the plain float64 objective, its quantised centroids against exact means, the
CPU path of ops.spot_error -- the same int64 fixed point as the kernels -- against the reference,
the class's argument checks and the entry's refusals.
"""
import math

import numpy as np
import pytest
import torch

import spot_error_reference as sr

EPS = sr.EPS


def _torch_objective(x, y, label, n_groups, domain, oob):
    """sum over groups of sum |x - mean|^2 + penalty as ordinary differentiable torch code
    (float64, the mean differentiated through); ``label``: int64 per ray, outside [0, G): no spot."""
    (x0, x1), (y0, y1) = domain
    ok = torch.isfinite(x) & torch.isfinite(y) & (label >= 0) & (label < n_groups)
    out = (x < x0) | (x > x1) | (y < y0) | (y > y1)
    inside, outside = ok & ~out, ok & out
    xo, yo = x[outside], y[outside]
    ex = torch.clamp(x0 - xo, min=0) + torch.clamp(xo - x1, min=0)
    ey = torch.clamp(y0 - yo, min=0) + torch.clamp(yo - y1, min=0)
    e = (oob * (ex ** 2 + ey ** 2)).sum()
    li = label[inside]
    cnt = torch.zeros(n_groups, dtype=torch.float64).index_add(0, li, torch.ones_like(x[inside]))
    cnt = torch.clamp(cnt, min=1.0)
    for v in (x[inside], y[inside]):
        mean = torch.zeros(n_groups, dtype=torch.float64).index_add(0, li, v) / cnt
        e = e + ((v - mean[li]) ** 2).sum()
    return e


def test_reference_gradient_equals_autograd():
    """The gradient 2 (x - c) is the derivative of the objective WITH the centroid differentiated
    through: the residuals of a group sum to zero."""
    x, y, _, group, _ = sr.points(200, n_groups=5)
    keep = np.isfinite(x) & np.isfinite(y)         # (autograd through a NaN coordinate is NaN)
    x, y, lab = x[keep], y[keep], group[:200][keep]
    ref = sr.spot_error(x, y, lab, 5, sr.DOMAIN, oob_weight=0.3, quantise=False)
    assert ref["n_penalised"] > 5
    sizes = np.bincount(lab[ref["inside"]], minlength=5)
    assert (sizes >= 2).sum() >= 3
    tx = torch.tensor(x, requires_grad=True)
    ty = torch.tensor(y, requires_grad=True)
    e = _torch_objective(tx, ty, torch.tensor(lab).long(), 5, sr.DOMAIN, 0.3)
    gx, gy = torch.autograd.grad(e, [tx, ty])
    assert abs(float(e.detach()) - ref["error"]) <= 1e-12 * max(1.0, ref["error"])
    top = max(float(gx.abs().max()), float(gy.abs().max()))
    assert top > 0
    assert np.abs(gx.numpy() - ref["grad_x"]).max() <= 1e-12 * top
    assert np.abs(gy.numpy() - ref["grad_y"]).max() <= 1e-12 * top


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,G,domain", [(4097, 37, (-1.1, 1.1)), (100000, 5, (-1.1, 1.1)),
                                        (4097, 1025, (9.0, 9.5)), (65, 64, (-100.0, 300.0))])
def test_quantised_centroids_are_within_half_a_step_of_the_exact_means(n, G, domain, dtype):
    """|c - mean| <= 0.5 / qs + 8 eps max(|x0|, |x1|): half a quantisation step -- every q is
    within 0.5 of (x - x0) qs, so is their mean --, and 8 eps of the domain's size for the
    roundings of x - x0, the product, the two divisions and the add.  Derived, not measured.  The
    gradient 2 (x - c) deviates by at most twice that."""
    rng = np.random.default_rng(n + G)
    x0, x1 = domain
    x = rng.uniform(x0, x1, n).astype(dtype)
    x = np.clip(x, dtype(x0), dtype(x1))
    x = x[(x.astype(np.float64) >= x0) & (x.astype(np.float64) <= x1)]
    lab = rng.integers(0, G, x.shape[0]).astype(np.int32)
    ref = sr.spot_error(x, None, lab, G, (domain,))
    assert ref["n_inside"] == x.shape[0] and ref["acc"].dtype == np.int64
    bound = 0.5 / ref["qsx"] + 8 * EPS * max(abs(x0), abs(x1))
    xs = x.astype(np.float64)
    order = np.argsort(lab, kind="stable")
    cuts = np.searchsorted(lab[order], np.arange(G + 1))
    worst = 0.0
    for g in range(G):
        members = xs[order[cuts[g]:cuts[g + 1]]]
        if members.size == 0:
            assert np.isnan(ref["centroids"][g, 0])
            continue
        mean = math.fsum(members.tolist()) / members.size
        worst = max(worst, abs(ref["centroids"][g, 0] - mean))
        exact = 2.0 * (members - mean)
        got = ref["grad_x"][order[cuts[g]:cuts[g + 1]]]
        assert np.abs(got - exact).max() <= 2 * bound
    print(f"largest centroid deviation {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


def _cpu(x, y, group, G, domain, oob=0.0, mask=None, perm=None, dtype=torch.float64, pad=2):
    """ops.spot_error on CPU tensors: the rows sit in a 6-row block (x in row 4, y in row 5) with
    ``pad`` spare columns; the gradient block starts out as NaN to show what is written."""
    from tensorflowraytrace_amd import ops
    two = y is not None
    n = len(x)
    rows = torch.full((6, n + pad), 7.0, dtype=dtype)
    rows[4, :n] = torch.tensor(x).to(dtype)
    if two:
        rows[5, :n] = torch.tensor(y).to(dtype)
    g = torch.tensor(np.asarray(group), dtype=torch.int32)
    qbits = ops.spot_qbits(g.numel())
    grid = ops.spot_grid(domain if two else domain[:1], qbits)
    grad = torch.full((6, n + pad), float("nan"), dtype=torch.float64)
    err, grad_v, acc = ops.spot_error(
        rows[:, :n], 4, 5 if two else -1, g, G, grid, oob,
        mask=None if mask is None else torch.tensor(mask),
        perm=None if perm is None else torch.tensor(perm), grad=grad[:, :n])
    return err.numpy(), grad.numpy(), acc.numpy()


def _compare(got, ref, n, two=True, mask=None):
    err, grad, acc = got
    assert np.array_equal(acc, ref["acc"])
    assert grad[4, :n].tobytes() == ref["grad_x"].tobytes()
    if two:
        assert grad[5, :n].tobytes() == ref["grad_y"].tobytes()
    else:
        assert np.isnan(grad[5]).all()
    assert np.isnan(grad[:4]).all() and np.isnan(grad[:, n:]).all()
    assert abs(err[0] - ref["error"]) <= sr.error_bound(ref), (err[0], ref["error"])
    counting = n if mask is None else int((mask >= 0).sum())
    assert err[1] == (2 if two else 1) * counting == ref["terms"]
    if counting:
        assert abs(err[2] - ref["mean"]) <= sr.error_bound(ref) / err[1] + EPS * abs(ref["mean"])
    else:
        assert np.isnan(err[2])


@pytest.mark.parametrize("G", sr.GROUPS[:5])
@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_cpu_path_equals_the_reference(G, n):
    x, y, mask, group, perm = sr.points(n, n_groups=G)
    for m in (None, mask):
        for p in (None, perm):
            ref = sr.spot_error(x, y, group, G, sr.DOMAIN, oob_weight=0.3, mask=m, perm=p)
            _compare(_cpu(x, y, group, G, sr.DOMAIN, 0.3, m, p), ref, n, mask=m)
            if n == 1000:
                assert ref["n_penalised"] > 20 and ref["n_inside"] > 500
                sizes = ref["acc"][:, 0]
                if G > 1:
                    assert sizes[-1] == 0
                if G > 2:
                    assert sizes[-2] == 1


def test_cpu_path_one_field_and_float32_columns():
    x, y, mask, group, perm = sr.points(1000, np.float32, n_groups=64)
    ref = sr.spot_error(x, None, group, 64, sr.DOMAIN[:1], oob_weight=0.2, mask=mask, perm=perm)
    _compare(_cpu(x, None, group, 64, sr.DOMAIN, 0.2, mask, perm, torch.float32), ref, 1000,
             two=False, mask=mask)
    assert not ref["acc"][:, 2].any()
    ref = sr.spot_error(x, y, group, 64, sr.DOMAIN, oob_weight=0.2)
    _compare(_cpu(x, y, group, 64, sr.DOMAIN, 0.2, None, None, torch.float32), ref, 1000)


def test_edge_cases():
    (x0, x1), (y0, y1) = sr.DOMAIN
    ym = 0.5 * (y0 + y1)
    # exactly on x0 and on x1: inside (closed domain), q = 0 and q = 2^qbits
    x, y, group = np.array([x0, x1]), np.array([ym, ym]), np.array([0, 1], dtype=np.int32)
    ref = sr.spot_error(x, y, group, 2, sr.DOMAIN, oob_weight=1.0)
    q = sr.qbits_of(2)
    assert q == 52 and ref["acc"][0, 1] == 0 and ref["acc"][1, 1] == 2 ** q
    assert ref["n_penalised"] == 0 and ref["error"] == 0.0
    _compare(_cpu(x, y, group, 2, sr.DOMAIN, 1.0), ref, 2)
    # labels -1 and G, a NaN and an infinity: counted as terms, nothing else
    x, y = np.array([0.0, 0.1, np.nan, 0.2, 0.3]), np.array([1.0, 1.0, 1.0, np.inf, 1.5])
    group = np.array([-1, 2, 0, 0, 1], dtype=np.int32)
    ref = sr.spot_error(x, y, group, 2, sr.DOMAIN, oob_weight=1.0)
    got = _cpu(x, y, group, 2, sr.DOMAIN, 1.0)
    _compare(got, ref, 5)
    # (the one ray left is its own group: it sits within the quantisation of its centroid)
    assert ref["acc"][:, 0].tolist() == [0, 1] and got[0][1] == 10.0
    assert got[0][0] <= 2 * (0.5 / min(ref["qsx"], ref["qsy"]) + 8 * EPS * 2.0) ** 2
    assert not got[1][4:, :4].any()
    # every point outside: the penalties and their gradient
    x, y = np.array([x0 - 0.5, x1 + 0.25, 0.0]), np.array([ym, y1 + 1.0, y0 - 2.0])
    group = np.zeros(3, dtype=np.int32)
    ref = sr.spot_error(x, y, group, 1, sr.DOMAIN, oob_weight=0.5)
    want = 0.5 * (0.25 + (0.0625 + 1.0) + 4.0)
    assert abs(ref["error"] - want) <= 4 * EPS * want and not ref["acc"].any()
    assert np.array_equal(ref["grad_x"], [-0.5, 0.25, 0.0])
    assert np.array_equal(ref["grad_y"], [0.0, 1.0, -2.0])
    _compare(_cpu(x, y, group, 1, sr.DOMAIN, 0.5), ref, 3)
    # a ray without a spot takes no penalty either, wherever it is
    ref = sr.spot_error(x, y, np.full(3, -1, dtype=np.int32), 1, sr.DOMAIN, oob_weight=0.5)
    assert ref["error"] == 0.0 and not ref["grad_x"].any()
    _compare(_cpu(x, y, np.full(3, -1, dtype=np.int32), 1, sr.DOMAIN, 0.5), ref, 3)


def test_the_class_checks_its_arguments_and_reports_centroids():
    import tfrt.optimizer as optimizer
    from tensorflowraytrace_amd import fused_step
    assert optimizer.SpotError is fused_step.SpotError
    lab = np.arange(12) % 4
    erf = optimizer.SpotError(("y_end", "z_end"), lab, sr.DOMAIN, oob_weight=0.1)
    assert erf.n_groups == 4 and erf.labels.dtype == torch.int32 and erf.rows == [4, 5]
    assert optimizer.SpotError("y_end", lab, sr.DOMAIN[:1], n_groups=9).n_groups == 9
    one = optimizer.SpotError("y_end", torch.tensor(lab), sr.DOMAIN[:1])
    assert one.rows == [4] and one.rows_for(2) == [3]
    with pytest.raises(ValueError):
        erf.rows_for(2)
    for bad in (dict(fields=("y_end", "w")), dict(fields=("y_end", "y_end")), dict(fields=()),
                dict(domain=sr.DOMAIN[:1]), dict(domain=((1.0, 1.0), (0.0, 1.0))),
                dict(domain=((0.0, float("inf")), (0.0, 1.0))), dict(oob_weight=-1.0),
                dict(oob_weight=float("nan")), dict(groups=np.zeros((3, 2), dtype=np.int64)),
                dict(groups=np.zeros(3)), dict(groups=lambda src: lab), dict(n_groups=0),
                dict(n_groups=2 ** 20 + 1)):
        kw = dict(fields=("y_end", "z_end"), groups=lab, domain=sr.DOMAIN)
        kw.update(bad)
        with pytest.raises(ValueError):
            optimizer.SpotError(**kw)
    assert optimizer.SpotError("y_end", lambda src: lab, sr.DOMAIN[:1], n_groups=4).labels is None
    # graph_key: the label buffer, G, the constants
    k0 = erf.graph_key()
    erf.labels.add_(0)
    assert erf.graph_key() == k0
    erf.labels = erf.labels.clone()
    assert erf.graph_key() != k0
    # neither the fused 2-D step nor ray shards
    from tensorflowraytrace_amd.fused_step import FusedStep

    class _Eng:
        dimension, ray_shard = 2, None

        @staticmethod
        def _custom_ops():
            return False

    class _Opt:
        engine, error_function = _Eng(), one
    assert FusedStep.eligible2d(_Opt()) is False


def test_the_generic_path_returns_the_terms_and_the_gradient_rows():
    """SpotError.__call__ on CPU tensors: (n, k) terms whose sum is the reference's error and,
    through backward, the reference's gradient on the finished rays' fields; the labels come
    through the finished rays' source-ray indices."""
    import tfrt.optimizer as optimizer
    n, G = 300, 7
    x, y, _, group, perm = sr.points(n, n_groups=G)
    ids = np.where((perm < 0) | (perm >= n), 0, perm).astype(np.int32)
    erf = optimizer.SpotError(("y_end", "z_end"), group, sr.DOMAIN, oob_weight=0.3, n_groups=G)
    erf.labels = erf.labels.cpu()

    class _Engine:
        dimension = 3
    eng = _Engine()
    fy = torch.tensor(x, requires_grad=True)
    fz = torch.tensor(y, requires_grad=True)
    eng.finished_rays = {"y_end": fy, "z_end": fz}
    eng.last_trace = {"finished_id": torch.tensor(ids)}
    eng._trace_src = {"x_start": torch.zeros(n + 3)}
    e = erf(eng)
    assert e.shape == (n, 2)
    ref = sr.spot_error(x, y, group, G, sr.DOMAIN, oob_weight=0.3, perm=ids)
    (3.0 * e.sum()).backward()
    assert abs(float(e.detach().sum()) - ref["error"]) <= sr.error_bound(ref)
    assert np.array_equal(erf.last_acc.numpy(), ref["acc"])
    assert np.array_equal(fy.grad.numpy(), 3.0 * ref["grad_x"])
    assert np.array_equal(fz.grad.numpy(), 3.0 * ref["grad_y"])
    c = erf.centroids().numpy()
    assert c.shape == (G, 2) and np.isnan(c[-1]).all()
    assert np.array_equal(c, ref["centroids"], equal_nan=True)
    # the terms of a ray that takes no part are zero
    e = e.detach().numpy()
    assert not e[~(ref["inside"] | ref["outside"])].any() and (e[ref["outside"]].sum(1) > 0).all()
    eng.finished_rays = {}
    assert erf(eng).shape == (0, 2)
    with pytest.raises(ValueError):
        eng.finished_rays = {"y_end": fy, "z_end": fz}
        eng._trace_src = {"x_start": torch.zeros(n)}
        erf(eng)


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    L = _lib.lib()
    assert L.tfrt_spot_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_spot_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_spot_error_workspace_bytes(-1, 4) == 0
    small = L.tfrt_spot_error_workspace_bytes(0, 4)
    assert 0 < small <= L.tfrt_spot_error_workspace_bytes(1_000_000, 2 ** 20)
    dummy = ctypes.create_string_buffer(1 << 17)
    p = ctypes.cast(dummy, ctypes.c_void_p)

    def call(n=8, G=4, row_x=0, row_y=1, x1=1.0, qsx=4.0, oob=0.0, ws=1 << 17, stride=8,
             variant=0, group=p, dtype=1, qbits=40, n_source=8, acc=p, gstride=8):
        return L.tfrt_spot_error(p, stride, n, dtype, None, row_x, row_y, group, n_source, None, G,
                                 0.0, x1, qsx, 0.0, 1.0, 4.0, qbits, oob, p, gstride, p, acc,
                                 variant, p, ws, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(row_x=6), dict(row_y=0),
                dict(x1=0.0), dict(qsx=0.0), dict(oob=-1.0), dict(stride=4), dict(gstride=4),
                dict(variant=3), dict(group=None), dict(n=1 << 31), dict(dtype=7),
                dict(G=1025, variant=1), dict(qsx=float("nan")), dict(oob=float("inf")),
                dict(qbits=53), dict(qbits=0), dict(n=1 << 22, qbits=40, stride=1 << 22,
                                                    gstride=1 << 22),
                dict(n_source=-1), dict(acc=None)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
