"""
DistortionError without a GPU: the numpy reference of tests/distortion_error_reference.py against
torch autograd of the full objective (centroids and fit differentiated through), a planted fit,
the invalid fits, the CPU path of ops.distortion_error against the reference bit for bit, the
class's argument checks, the generic path on CPU tensors and on the oracle-backed CPU stand-ins,
the entry's argument checks, and csrc/distortion_math.h compiled for the host under the address
and undefined-behaviour sanitizers.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import distortion_error_reference as dr
from tensorflowraytrace_amd import ops, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "distortion_host", "distortion_main.cpp")


def _torch_objective(v, label, points, domain, oob, fit):
    """The full objective in torch float64, everything differentiated through: ``v`` (k, n) the
    fields, ``label`` (n,) the group of every column in a group or penalised, -1 otherwise.  Per
    group the mean of its columns inside, the weighted least-squares fit c ~ A p + t over the
    groups with columns (``torch.linalg`` for the affine one), the sum over the columns inside of
    |c_group - (A p_group + t)|^2, plus the penalties."""
    k = v.shape[0]
    label = torch.as_tensor(label).long()
    points = torch.as_tensor(points, dtype=torch.float64)
    lo = torch.tensor([d[0] for d in domain], dtype=torch.float64)[:, None]
    hi = torch.tensor([d[1] for d in domain], dtype=torch.float64)[:, None]
    out = ((v < lo) | (v > hi)).any(dim=0)
    inside, outside = (label >= 0) & ~out, (label >= 0) & out
    ex = torch.relu(lo - v) + torch.relu(v - hi)
    pen = oob * (ex * ex).sum(dim=0)[outside].sum()
    G = points.shape[0]
    li = label[inside]
    cnt = torch.zeros(G, dtype=torch.float64).index_add(0, li, torch.ones(li.shape[0],
                                                                          dtype=torch.float64))
    S = torch.zeros((k, G), dtype=torch.float64).index_add(1, li, v[:, inside])
    used = cnt > 0
    w, c, p = cnt[used], S[:, used] / cnt[used], points[used].t()
    W = w.sum()
    pm, cm = (w * p).sum(dim=1) / W, (w * c).sum(dim=1) / W
    dp, dc = p - pm[:, None], c - cm[:, None]
    Spp, Scp = (w * dp) @ dp.t(), (w * dc) @ dp.t()
    if fit == "scale" or k == 1:
        A = torch.trace(Scp) / torch.trace(Spp) * torch.eye(k, dtype=torch.float64)
    else:
        A = Scp @ torch.linalg.inv(Spp)
    r = dc - A @ dp
    return (w * (r * r).sum(dim=0)).sum() + pen


def _case(n, G, two, fit, masked=False, permuted=False, dtype=np.float64):
    x, y, mask, group, perm, points = dr.rays(n, G, dtype, permuted)
    points = points if two else np.ascontiguousarray(points[:, :1])
    domain = dr.DOMAIN if two else dr.DOMAIN[:1]
    ref = dr.distortion_error(x.astype(np.float64), y.astype(np.float64) if two else None, group,
                              G, points, domain, fit=fit, oob_weight=dr.OOB,
                              mask=mask if masked else None, perm=perm if permuted else None)
    return (x, y, mask, group, perm, points, domain), ref


@pytest.mark.parametrize("n", [1000, 20000])
def test_the_generator_keeps_its_conditions(n):
    for G in (3, 7, 1024, 1025, 2049):
        for two in (True, False):
            for fit in ("scale", "affine"):
                for flags in ((False, False), (True, True)):
                    for dtype in (np.float64, np.float32):
                        dr.assert_generator(_case(n, G, two, fit, *flags, dtype=dtype)[1])


@pytest.mark.parametrize("two", [True, False], ids=["k2", "k1"])
@pytest.mark.parametrize("fit", ["scale", "affine"])
def test_reference_gradient_equals_autograd_of_the_full_objective(fit, two):
    """The reference's gradient 2 r needs no derivative of the fit (the envelope argument) and
    works on quantised records; torch differentiates through the means and the fit.  The sources
    of a difference: the quantisation, half a step 1.75 * 2**-52 per coordinate, and the rounding
    of sums over up to 1,000 columns of coordinates below 2 in both evaluations,
    1000 * eps * 2 = 4.4e-13 in the worst case.  Asserted: 1e-12 absolute on gradient entries of
    order 0.01 to 0.1, and the same relative bound on the error."""
    (x, y, mask, group, perm, points, domain), ref = _case(1000, 7, two, fit)
    counts = ref["inside"] | ref["outside"]
    label = np.where(counts, ref["label"], -1)
    v = np.stack([x, y])[:2 if two else 1]
    v = np.where(np.isfinite(v), v, 0.0)
    t = torch.tensor(v, requires_grad=True)
    e = _torch_objective(t, label, points, domain, dr.OOB, fit)
    g, = torch.autograd.grad(e, t)
    e = e.detach()
    got = np.stack([ref["grad_x"], ref["grad_y"]])[:2 if two else 1] if two \
        else ref["grad_x"][None, :]
    diff = float(np.abs(got - g.numpy()).max())
    print(f"largest gradient entry {np.abs(got).max():.3e}, largest difference {diff:.3e}, "
          f"errors {ref['error']!r} {float(e)!r}")
    assert ref["valid"] and np.abs(got[:, ref["inside"]]).max() > 1e-3
    assert diff <= 1e-12
    assert abs(ref["error"] - float(e)) <= 1e-12 * float(e)


@pytest.mark.parametrize("fit", ["scale", "affine"])
def test_the_fit_recovers_a_planted_map(fit):
    """Columns exactly at A p + t, no noise, no distortion: the fit is the planted one and every
    residual vanishes, up to the rounding of the centroids and the sums (a few eps of
    coordinates of order 1: 1e-13 asserted)."""
    G, per = 12, 40
    points = dr.object_points(G)
    A = dr.PLANTED_A if fit == "affine" else -0.8 * np.eye(2)
    image = points @ A.T + dr.PLANTED_T
    group = np.repeat(np.arange(G), per).astype(np.int32)
    x, y = image[group, 0], image[group, 1]
    ref = dr.distortion_error(x, y, group, G, points, dr.DOMAIN, fit=fit)
    assert ref["valid"] and ref["groups_used"] == G and ref["n_inside"] == G * per
    assert np.abs(ref["matrix"] - A).max() <= 1e-13
    assert np.abs(ref["offset"] - dr.PLANTED_T).max() <= 1e-13
    assert np.abs(ref["residual"]).max() <= 1e-13 and ref["error"] <= 1e-24
    one = dr.distortion_error(x, None, group, G, points[:, :1], dr.DOMAIN[:1], fit=fit)
    assert one["valid"] and one["fit_out"][1] == 0.0 and one["fit_out"][0] == one["fit_out"][3]
    assert not one["residual"][:, 1].any()


def test_invalid_fits_give_zero_inside_terms():
    (x, y, mask, group, perm, points, domain), _ = _case(1000, 7, True, "scale")
    line = np.stack([points[:, 0], 2.0 * points[:, 0]], axis=1)
    same = np.tile(points[:1], (7, 1))
    for fit, grp, pts in (("scale", np.zeros_like(group), points), ("affine", np.zeros_like(group),
                                                                    points),
                          ("scale", group, same), ("affine", group, same),
                          ("affine", group, line)):
        ref = dr.distortion_error(x, y, grp, 7, pts, domain, fit=fit, oob_weight=dr.OOB)
        assert not ref["valid"] and ref["fit_out"][6] == 0.0 and np.isnan(ref["fit_out"][:6]).all()
        assert ref["n_inside"] > 500 and ref["n_penalised"] > 20
        assert not ref["grad_x"][ref["inside"]].any() and not ref["grad_y"][ref["inside"]].any()
        assert ref["grad_x"][ref["outside"]].any()
        assert not ref["residual"][ref["used"]].any() and np.isnan(ref["residual"][~ref["used"]]).all()
        assert ref["error"] == ref["abs_sum"] > 0.0           # the penalties alone
    # collinear object points do have a scale fit
    assert dr.distortion_error(x, y, group, 7, line, domain, fit="scale")["valid"]


def _cpu(case, two, fit, masked, permuted, dim=3):
    x, y, mask, group, perm, points, domain = case
    n = x.shape[0]
    rows = torch.full((2 * dim, n), 7.0, dtype=torch.tensor(x).dtype)
    rows[dim], rows[dim + 1] = torch.tensor(x), torch.tensor(y)
    g = torch.tensor(group)
    grad = torch.full((2 * dim, n), float("nan"), dtype=torch.float64)
    out = ops.distortion_error(
        rows, dim, dim + 1 if two else -1, g, points.shape[0], torch.tensor(points),
        ops.spot_grid(domain, ops.spot_qbits(g.numel())), fit=fit, oob_weight=dr.OOB,
        mask=torch.tensor(mask) if masked else None, perm=torch.tensor(perm) if permuted else None,
        grad=grad, dimension=dim)
    return [t.numpy() for t in out]


@pytest.mark.parametrize("fit", ["scale", "affine"])
@pytest.mark.parametrize("G", [3, 1025, 2049])
def test_cpu_path_equals_the_reference(G, fit):
    for n in (0, 1, 65, 1000):
        for two in (True, False):
            for flags in ((False, False), (True, True)):
                for dtype, dim in ((np.float64, 3), (np.float32, 2)):
                    case, ref = _case(n, G, two, fit, *flags, dtype=dtype)
                    err, grad, acc, fit_out, residual = _cpu(case, two, fit, *flags, dim=dim)
                    assert np.array_equal(acc, ref["acc"])
                    assert np.array_equal(fit_out, ref["fit_out"], equal_nan=True)
                    assert np.array_equal(residual, ref["residual"], equal_nan=True)
                    assert np.array_equal(grad[dim], ref["grad_x"])
                    if two:
                        assert np.array_equal(grad[dim + 1], ref["grad_y"])
                    assert np.isnan(np.delete(grad, [dim, dim + 1][:2 if two else 1], axis=0)).all()
                    assert err[1] == ref["terms"]
                    assert abs(err[0] - ref["error"]) <= dr.error_bound(ref)


def test_ops_argument_errors():
    rows = torch.zeros((6, 5), dtype=torch.float64)
    g = torch.zeros(5, dtype=torch.int32)
    pts = torch.zeros((3, 2), dtype=torch.float64)
    grid = ops.spot_grid(dr.DOMAIN, ops.spot_qbits(5))
    ok = dict(rows=rows, row_x=4, row_y=5, group=g, n_groups=3, points=pts, grid=grid)
    for bad, match in ((dict(group=g.long()), "group"), (dict(n_groups=0), "n_groups"),
                       (dict(fit="rigid"), "fit"), (dict(min_cond=-1.0), "min_cond"),
                       (dict(min_cond=float("nan")), "min_cond"), (dict(row_y=4), "distinct"),
                       (dict(points=pts[:, :1].contiguous()), "points"),
                       (dict(points=pts.float()), "points"), (dict(variant=3), "variant"),
                       (dict(n_groups=1025, points=torch.zeros((1025, 2), dtype=torch.float64),
                             variant=1), "variant"),
                       (dict(mask=torch.zeros(5)), "mask"),
                       (dict(grad=torch.zeros((4, 5), dtype=torch.float64)), "grad"),
                       (dict(acc=torch.zeros((3, 8), dtype=torch.int64)), "acc"),
                       (dict(fit_out=torch.zeros(6, dtype=torch.float64)), "fit_out"),
                       (dict(residual=torch.zeros((3, 3), dtype=torch.float64)), "residual")):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.distortion_error(**kw)


def test_the_class_checks_its_arguments_and_reports_the_fit():
    import tfrt.optimizer
    from tensorflowraytrace_amd import errors, fused_step
    D = optimizer.DistortionError
    assert tfrt.optimizer.DistortionError is D and fused_step.DistortionError is D \
        and D in errors._COUPLED
    lab = np.arange(12) % 4
    pts = dr.object_points(4)
    erf = D(("y_end", "z_end"), lab, pts, dr.DOMAIN)
    assert erf.n_groups == 4 and erf.labels.dtype == torch.int32 and erf.fit == "scale"
    assert erf.min_cond == 1e-9 and erf.points.dtype == torch.float64
    assert erf.rows == [4, 5] and erf.seed_rows == 0x30 and erf.on_columns
    with pytest.raises(ValueError, match="2-D engine"):
        erf.rows_for(2)
    far = D(("y_dir", "z_dir"), lab, pts, dr.DOMAIN, fit="affine")
    assert far.has_direction and far.seed_rows == 0x3f and far.rows_for(3) == [7, 8]
    one = D("y_end", torch.tensor(lab), pts[:, 0], dr.DOMAIN[:1], n_groups=4, min_cond=0.0)
    assert tuple(one.points.shape) == (4, 1) and one.rows_for(2) == [3]
    bad_pts = pts.copy()
    bad_pts[2, 1] = np.nan
    for bad in (dict(fields=("y_end", "y_end")), dict(domain=dr.DOMAIN[:1]), dict(fit="rigid"),
                dict(oob_weight=-1.0), dict(min_cond=-1.0), dict(min_cond=float("inf")),
                dict(min_cond="small"), dict(points=bad_pts), dict(points=pts[:3]),
                dict(points=pts[:, :1]), dict(points="here"), dict(groups=np.zeros(3)),
                dict(groups=lambda src: lab), dict(n_groups=0), dict(n_groups=2 ** 20 + 1)):
        kw = dict(fields=("y_end", "z_end"), groups=lab, points=pts, domain=dr.DOMAIN)
        kw.update(bad)
        with pytest.raises(ValueError, match="DistortionError"):
            D(**kw)
    with pytest.raises(TypeError):
        D(("y_end", "z_end"), lab, pts, dr.DOMAIN, weights=np.ones(12))      # (no weights)
    assert D(("y_end", "z_end"), lambda src: lab, pts, dr.DOMAIN, n_groups=4).labels is None
    for read in (erf.centroids, erf.residuals, erf.fit_parameters):
        with pytest.raises(RuntimeError, match="no evaluation"):
            read()
    # graph_key: the label buffer, the points buffer, fit and min_cond
    k0 = erf.graph_key()
    erf.labels.add_(0)
    erf.points.add_(0.0)
    assert erf.graph_key() == k0
    erf.points = erf.points.clone()
    assert erf.graph_key() != k0
    assert far.graph_key()[-2:] == ("affine", 1e-9) and one.graph_key()[-1] == 0.0
    # a legal term of a SumError
    spot = optimizer.SpotError(("y_end", "z_end"), lab, dr.DOMAIN)
    both = optimizer.SumError([spot, erf], reduce="mean")
    assert both.terms == (spot, erf) and both.rows == [4, 5, 4, 5]
    with pytest.raises(ValueError, match="DistortionError"):
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


@pytest.mark.parametrize("fit", ["scale", "affine"])
def test_the_generic_path_returns_the_terms_and_the_gradient_rows(fit):
    """DistortionError.__call__ on CPU tensors: (n, k) terms whose sum is the reference's error
    and, through backward, the reference's gradient on the fields' rows; the labels come through
    the finished rays' source-ray indices; the accessors report the reference's fit."""
    n, G = 300, 7
    (x, y, mask, group, perm, points, domain), ref = _case(n, G, True, fit, permuted=True)
    erf = optimizer.DistortionError(("y_end", "z_end"), group, points, domain, fit=fit,
                                    oob_weight=dr.OOB, n_groups=G)
    erf.labels, erf.points = erf.labels.cpu(), erf.points.cpu()
    block = np.zeros((6, n))
    block[4], block[5] = x, y
    eng = _Engine(block, perm, n + 3, 3)
    e = erf(eng)
    assert e.shape == (n, 2) and e.dtype == torch.float64
    (3.0 * e.sum()).backward()
    assert abs(float(e.detach().sum()) - ref["error"]) <= dr.error_bound(ref)
    assert np.array_equal(erf.last_acc.numpy(), ref["acc"])
    assert np.array_equal(eng.leaves[4].grad.numpy(), 3.0 * ref["grad_x"])
    assert np.array_equal(eng.leaves[5].grad.numpy(), 3.0 * ref["grad_y"])
    assert eng.leaves[0].grad is None                  # (a row that is no field: untouched)
    fp = erf.fit_parameters()
    assert fp["valid"] == ref["valid"] and fp["groups_used"] == ref["groups_used"]
    assert np.array_equal(fp["matrix"].numpy(), ref["matrix"])
    assert np.array_equal(fp["offset"].numpy(), ref["offset"])
    assert ("magnification" in fp) == (fit == "scale")
    if fit == "scale":
        assert fp["magnification"] == ref["fit_out"][0]
    assert np.array_equal(erf.residuals().numpy(), ref["residual"], equal_nan=True)
    assert np.array_equal(erf.centroids().numpy(), ref["centroids"], equal_nan=True)
    eng.finished_rays = {}
    assert erf(eng).shape == (0, 2)
    with pytest.raises(ValueError, match="label"):
        erf(_Engine(block, perm, n, 3))


def _lens(n_rays):
    from test_host_logic import _lens_api
    eng, system, lens, target = _lens_api(n_rays)
    groups = np.arange(n_rays) % 5
    points = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.5], [0.5, -1.0]])
    return eng, lens, groups, points, ((-5.0, 5.0), (-5.0, 5.0))


@pytest.mark.parametrize("fit", ["scale", "affine"])
def test_the_optimiser_takes_the_generic_path_on_the_cpu_backend(cpu_backend, fit):
    """SGD_Optimizer with a DistortionError on the oracle-backed CPU stand-ins: the step's error
    is the reference's on the traced rays and the parameter gradient is that of the torch
    objective under autograd through the same trace."""
    eng, lens, groups, points, domain = _lens(200)
    erf = optimizer.DistortionError(("y_end", "z_end"), groups, points, domain, fit=fit)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=2e-3, grad_clip=1e9)
    grads, err_sum, n_terms = opt.raw_gradient()
    assert opt._fused_step is None
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].numpy()
    ref = dr.distortion_error(fin["y_end"].detach().numpy(), fin["z_end"].detach().numpy(),
                              groups, 5, points, domain, fit=fit, perm=ids)
    assert ref["terms"] == n_terms > 300 and ref["valid"] and ref["n_penalised"] == 0
    assert abs(float(err_sum) - ref["error"]) <= dr.error_bound(ref)
    eng.clear_ray_history()
    eng.optical_system.update()
    eng.ray_trace(3)
    fin = eng.finished_rays
    assert np.array_equal(eng.last_trace["finished_id"].numpy(), ids)
    e = _torch_objective(torch.stack([fin["y_end"], fin["z_end"]]).double(), ref["label"], points,
                         domain, 0.0, fit)
    want = torch.autograd.grad(e, lens.parameters)
    for g, w in zip(grads, want):
        assert float((g - w).abs().max()) <= 1e-9 * float(w.abs().max())


def test_a_sum_with_a_goal_runs_on_the_cpu_backend(cpu_backend):
    eng, lens, groups, points, domain = _lens(200)
    dist = optimizer.DistortionError(("y_end", "z_end"), groups, points, domain, fit="affine")
    goal = optimizer.GoalError(("y_end", "z_end"), lambda src: -src["object_coords"][:, 1:])
    both = optimizer.SumError([dist, goal], weights=[1.0, 0.25], reduce="mean")
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, both, 3, learning_rate=1e-3, grad_clip=1e9)
    e = float(opt.single_step(None))
    triples = both.last_errors.numpy()
    assert triples.shape == (2, 3) and triples[0, 1] > 300 and triples[1, 1] == triples[0, 1]
    assert abs(e - (triples[0, 2] + 0.25 * triples[1, 2])) <= 1e-12 * abs(e)
    assert dist.fit_parameters()["valid"] and dist.residuals().shape == (5, 2)


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    L = _lib.lib()
    assert L.tfrt_distortion_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_distortion_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_distortion_error_workspace_bytes(-1, 4) == 0
    small = L.tfrt_distortion_error_workspace_bytes(0, 4)
    assert 0 < small <= L.tfrt_distortion_error_workspace_bytes(1_000_000, 2 ** 20)
    dummy = ctypes.create_string_buffer(1 << 17)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 8)

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
                dict(n=1 << 22, stride=1 << 22, gstride=1 << 22), dict(G=1025, variant=1),
                dict(n_source=-1), dict(points=None), dict(fit=2), dict(fit=-1),
                dict(min_cond=-1.0), dict(min_cond=float("nan")), dict(fit_out=None),
                dict(residual=None), dict(residual=odd), dict(acc=None), dict(err=None)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2


def test_distortion_math_on_the_host_under_the_sanitizers(tmp_path):
    """Every group's weight, point and centroid, its terms of the two fit passes, the fit and the
    residual table of distortion_math.h equal the reference's bit for bit, for both fits and one
    and two fields; the program's vectors are exact-size allocations and it runs under the
    address and undefined-behaviour sanitizers."""
    exe = tmp_path / "distortion_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
    for n, G, two, fit in ((1000, 7, True, "scale"), (1000, 7, True, "affine"),
                           (300, 2049, True, "affine"), (1000, 30, False, "affine"),
                           (65, 3, False, "scale"), (1, 3, True, "scale"), (0, 1, True, "affine")):
        (x, y, mask, group, perm, points, domain), ref = _case(n, G, two, fit, True, True)
        k = 2 if two else 1
        qbits = dr.qbits_of(group.shape[0])
        one = np.ldexp(1.0, qbits)
        qs = [one / (d[1] - d[0]) for d in domain] + [0.0]
        lo = [d[0] for d in domain] + [0.0]
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(struct.pack("<4q", G, k, 1 if fit == "affine" else 0, ref["groups_used"])
                        + f8([lo[0], qs[0], lo[1], qs[1], dr.MIN_COND]) + f8(ref["means"])
                        + f8(ref["moments"]) + ref["acc"].tobytes() + f8(points))
        run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert run.returncode == 0, f"{n} {G} {two} {fit}: {run.stdout}{run.stderr}"
        raw = np.frombuffer(dst.read_bytes(), dtype=np.float64)
        assert raw.shape[0] == (5 + 5 + 7 + 2 + 2) * G + 8
        grp, mean_t, mom_t = (raw[a * G:b * G].reshape(G, b - a) for a, b in
                              ((0, 5), (5, 10), (10, 17)))
        fit_out = raw[17 * G:17 * G + 8]
        residual, err_t = (raw[17 * G + 8 + a * G:17 * G + 8 + b * G].reshape(G, 2)
                           for a, b in ((0, 2), (2, 4)))
        used = ref["used"]
        w = ref["acc"][:, 0].astype(np.float64)
        c = np.zeros((G, 2))
        c[:, :k] = np.where(used[:, None], ref["centroids"], 0.0)
        p = np.zeros((G, 2))
        p[:, :k] = np.where(used[:, None], points, 0.0)
        assert np.array_equal(grp, np.column_stack([w, p, c]))
        assert np.array_equal(mean_t, np.column_stack([w, w * p[:, 0], w * p[:, 1], w * c[:, 0],
                                                       w * c[:, 1]]))
        with np.errstate(invalid="ignore"):
            dp, dc = p - ref["means"][:2], c - ref["means"][2:]
            want = np.column_stack([w * (dp[:, 0] * dp[:, 0]), w * (dp[:, 0] * dp[:, 1]),
                                    w * (dp[:, 1] * dp[:, 1]), w * (dc[:, 0] * dp[:, 0]),
                                    w * (dc[:, 0] * dp[:, 1]), w * (dc[:, 1] * dp[:, 0]),
                                    w * (dc[:, 1] * dp[:, 1])])
        assert np.array_equal(mom_t[used], want[used]) and not mom_t[~used].any()
        assert np.array_equal(fit_out, ref["fit_out"], equal_nan=True)
        assert np.array_equal(residual, ref["residual"], equal_nan=True)
        r = np.where(used[:, None], ref["residual"], 0.0)
        assert np.array_equal(err_t, w[:, None] * (r * r))
