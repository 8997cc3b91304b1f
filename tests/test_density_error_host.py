"""
DensityError without a GPU: the numpy reference (tests/density_error_reference.py) against
torch.autograd on a plain float64 formulation, its quantised histogram against the unquantised
one, its anchor to analyze.DistributionDifferential, and the CPU path of ops.density_error -- the
same int64 fixed point as the kernels -- against the reference.
"""
import numpy as np
import pytest
import torch

import density_error_reference as dr

EPS = dr.EPS


def _torch_objective(x, y, g, domain, oob):
    """The unquantised objective as ordinary differentiable torch code (float64)."""
    (x0, x1), (y0, y1) = domain
    ny, nx = g.shape
    sx, sy = nx / (x1 - x0), ny / (y1 - y0)
    ok = torch.isfinite(x) & torch.isfinite(y)
    out = (x < x0) | (x > x1) | (y < y0) | (y > y1)
    inside, outside = ok & ~out, ok & out
    xo, yo = x[outside], y[outside]
    ex = torch.clamp(x0 - xo, min=0) + torch.clamp(xo - x1, min=0)
    ey = torch.clamp(y0 - yo, min=0) + torch.clamp(yo - y1, min=0)
    penalty = (oob * (ex ** 2 + ey ** 2)).sum()
    xi, yi = x[inside], y[inside]

    def axis(v, lo, scale, nb):
        u = (v - lo) * scale - 0.5
        f = torch.floor(u.detach())
        i0 = f.long()
        return i0.clamp(0, nb - 1), (i0 + 1).clamp(0, nb - 1), u - f
    ia, ib, tx = axis(xi, x0, sx, nx)
    ja, jb, ty = axis(yi, y0, sy, ny)
    H = torch.zeros(nx * ny, dtype=torch.float64)
    for k, w in ((ja * nx + ia, (1 - ty) * (1 - tx)), (ja * nx + ib, (1 - ty) * tx),
                 (jb * nx + ia, ty * (1 - tx)), (jb * nx + ib, ty * tx)):
        H = H.index_add(0, k, w)
    s = torch.linalg.norm(H)
    gf = g.reshape(-1)
    if float(s.detach()) == 0.0:
        return (gf * gf).sum() + penalty
    return ((H / s - gf) ** 2).sum() + penalty


@pytest.mark.parametrize("nx,ny", [(7, 3), (1, 1)])
def test_reference_gradient_equals_autograd(nx, ny):
    x, y, _ = dr.points(200)
    keep = np.isfinite(x) & np.isfinite(y)         # (autograd through a NaN coordinate is NaN)
    x, y = x[keep], y[keep]
    goal = dr.goal_of(nx, ny)
    ref = dr.density_error(x, y, goal, dr.DOMAIN, oob_weight=0.3, quantise=False)
    assert ref["n_penalised"] > 5 and ref["contributions"].sum() > 4 * 100
    tx = torch.tensor(x, requires_grad=True)
    ty = torch.tensor(y, requires_grad=True)
    e = _torch_objective(tx, ty, torch.tensor(dr.normalise(goal)), dr.DOMAIN, 0.3)
    gx, gy = torch.autograd.grad(e, [tx, ty])
    assert abs(float(e.detach()) - ref["error"]) <= 1e-12 * max(1.0, ref["error"])
    top = max(float(gx.abs().max()), float(gy.abs().max()))
    assert top > 0
    assert np.abs(gx.numpy() - ref["grad_x"]).max() <= 1e-12 * top
    assert np.abs(gy.numpy() - ref["grad_y"]).max() <= 1e-12 * top


@pytest.mark.parametrize("nx,ny", [(7, 3), (1, 1), (64, 64)])
def test_quantised_histogram_is_within_half_a_unit_per_contribution(nx, ny):
    """Every weight is rounded to the nearest multiple of 2^-32: it moves by at most 2^-33, so a
    bin that received c_b weights moves by at most c_b 2^-33.  Derived, not measured."""
    x, y, _ = dr.points(1000)
    goal = dr.goal_of(nx, ny)
    q = dr.density_error(x, y, goal, dr.DOMAIN)
    u = dr.density_error(x, y, goal, dr.DOMAIN, quantise=False)
    assert q["Hq"].dtype == np.int64
    assert (np.abs(q["H"] - u["H"]) <= q["contributions"] * 2.0 ** -33).all()
    # total weight 1 per ray inside, to within the same bound
    n_inside = q["contributions"].sum() // 4
    assert abs(int(q["Hq"].sum()) - n_inside * 2 ** 32) <= 2 * n_inside


@pytest.mark.parametrize("n_bins", [4, 10])
def test_points_on_bin_centres_give_distribution_differential(n_bins):
    """With every point on a bin centre (all inside) the soft histogram is the hard one: the error
    is analyze.DistributionDifferential's on the same points, within 16 B eps."""
    import tfrt.analyze as analyze
    domain = ((-1.0, 1.0), (0.0, 4.0))           # (bin widths and centres exact in binary)
    rng = np.random.default_rng(3)
    i, j = rng.integers(0, n_bins, 500), rng.integers(0, n_bins, 500)
    x = domain[0][0] + (i + 0.5) * (2.0 / n_bins)
    y = domain[1][0] + (j + 0.5) * (4.0 / n_bins)
    if n_bins == 10:                             # (0.2-wide bins are not exact: say where they sit)
        x, y = np.round(x, 12), np.round(y, 12)
    goal = dr.goal_of(n_bins, n_bins)
    want = float(analyze.DistributionDifferential(torch.tensor(goal), domain)(
        torch.tensor(x), torch.tensor(y)))
    ref = dr.density_error(x, y, goal, domain)
    hard = np.zeros((n_bins, n_bins), dtype=np.int64)
    np.add.at(hard, (j, i), 1)
    if n_bins == 4:
        assert np.array_equal(ref["Hq"], hard * 2 ** 32)
    assert abs(ref["error"] - want) <= 16 * n_bins * n_bins * EPS


def _cpu(x, y, goal, domain, oob=0.0, mask=None, dtype=torch.float64):
    from tensorflowraytrace_amd import ops
    two = y is not None
    rows = torch.stack([torch.tensor(x), torch.tensor(y)]) if two else torch.tensor(x).reshape(1, -1)
    g = torch.tensor(dr.normalise(goal)).contiguous()
    nx = g.shape[-1]
    grid = ops.density_grid(domain, nx, g.shape[0] if two else None)
    err, grad, hq = ops.density_error(rows.to(dtype), 0, 1 if two else -1, g, grid, oob,
                                      mask=None if mask is None else torch.tensor(mask))
    return err.numpy(), grad.numpy(), hq.numpy()


def _compare(got, ref, two=True):
    err, grad, hq = got
    assert np.array_equal(hq, ref["Hq"])
    assert err[1] == 1.0 and err[0] == err[2]
    assert abs(err[0] - ref["error"]) <= dr.error_bound(ref), (err[0], ref["error"])
    tol = dr.gradient_bound(ref)
    assert np.abs(grad[0] - ref["grad_x"]).max(initial=0.0) <= tol
    if two:
        assert np.abs(grad[1] - ref["grad_y"]).max(initial=0.0) <= tol


@pytest.mark.parametrize("nx,ny", dr.BINS[:4])
@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_cpu_path_equals_the_reference(nx, ny, n):
    x, y, mask = dr.points(n)
    goal = dr.goal_of(nx, ny)
    for m in (None, mask):
        ref = dr.density_error(x, y, goal, dr.DOMAIN, oob_weight=0.3, mask=m)
        # first: the reference's two summation orders agree within the bounds (else the
        # derivation of the bounds is wrong)
        plain = dr.density_error(x, y, goal, dr.DOMAIN, oob_weight=0.3, mask=m, pairwise=False)
        assert np.array_equal(plain["Hq"], ref["Hq"])
        assert abs(plain["error"] - ref["error"]) <= dr.error_bound(ref)
        tol = dr.gradient_bound(ref)
        assert np.abs(plain["grad_x"] - ref["grad_x"]).max(initial=0.0) <= tol
        assert np.abs(plain["grad_y"] - ref["grad_y"]).max(initial=0.0) <= tol
        got = _cpu(x, y, goal, dr.DOMAIN, 0.3, m)
        _compare(got, ref)
        off = ~(np.isfinite(x) & np.isfinite(y)) | (False if m is None else m < 0)
        assert (got[1][:, off] == 0.0).all()


def test_cpu_path_one_field_and_float32_columns():
    x, y, mask = dr.points(1000, np.float32)
    goal = dr.goal_of(7, 1, two=False)
    ref = dr.density_error(x, None, goal, dr.DOMAIN[:1], oob_weight=0.2, mask=mask)
    _compare(_cpu(x, None, goal, dr.DOMAIN[:1], 0.2, mask, torch.float32), ref, two=False)
    goal = dr.goal_of(7, 3)
    ref = dr.density_error(x, y, goal, dr.DOMAIN, oob_weight=0.2)
    _compare(_cpu(x, y, goal, dr.DOMAIN, 0.2, None, torch.float32), ref)


def test_edge_cases():
    (x0, x1), (y0, y1) = dr.DOMAIN
    goal = dr.goal_of(4, 4)
    ym = 0.5 * (y0 + y1)
    # exactly on x0 / on x1: inside (closed domain), all weight in the edge column, gradient 0 in x
    for xe, col in ((x0, 0), (x1, 3)):
        ref = dr.density_error(np.array([xe]), np.array([ym]), goal, dr.DOMAIN, oob_weight=1.0)
        assert ref["penalty"] == 0.0 and ref["Hq"].sum() == 2 ** 32
        assert ref["Hq"][:, col].sum() == 2 ** 32 and ref["grad_x"][0] == 0.0
        _compare(_cpu(np.array([xe]), np.array([ym]), goal, dr.DOMAIN, 1.0), ref)
    # on a bin centre: one bin gets everything
    xc, yc = x0 + 2.5 * (x1 - x0) / 4, y0 + 1.5 * (y1 - y0) / 4
    ref = dr.density_error(np.array([xc]), np.array([yc]), goal, dr.DOMAIN)
    assert ref["Hq"][1, 2] == 2 ** 32 and ref["Hq"].sum() == 2 ** 32
    _compare(_cpu(np.array([xc]), np.array([yc]), goal, dr.DOMAIN), ref)
    # a NaN coordinate: nothing, zero gradient
    x, y = np.array([np.nan, 0.0, 0.1]), np.array([1.0, np.nan, 1.0])
    ref = dr.density_error(x, y, goal, dr.DOMAIN, oob_weight=1.0)
    got = _cpu(x, y, goal, dr.DOMAIN, 1.0)
    _compare(got, ref)
    assert ref["Hq"].sum() == 2 ** 32 and (got[1][:, :2] == 0.0).all() and np.isfinite(got[0]).all()
    # no point at all: sum g^2 = 1
    ref = dr.density_error(np.zeros(0), np.zeros(0), goal, dr.DOMAIN)
    got = _cpu(np.zeros(0), np.zeros(0), goal, dr.DOMAIN)
    assert abs(ref["error"] - 1.0) <= 16 * 16 * EPS and abs(got[0][0] - 1.0) <= 16 * 16 * EPS
    assert not got[2].any()
    # every point outside: sum g^2 + the penalties, gradient = the penalty's
    x, y = np.array([x0 - 0.5, x1 + 0.25, 0.0]), np.array([ym, y1 + 1.0, y0 - 2.0])
    ref = dr.density_error(x, y, goal, dr.DOMAIN, oob_weight=0.5)
    want = 0.5 * (0.25 + (0.0625 + 1.0) + 4.0)
    assert abs(ref["penalty"] - want) <= 4 * EPS * want and not ref["Hq"].any()
    assert np.array_equal(ref["grad_x"], [-0.5, 0.25, 0.0])
    assert np.array_equal(ref["grad_y"], [0.0, 1.0, -2.0])
    got = _cpu(x, y, goal, dr.DOMAIN, 0.5)
    _compare(got, ref)
    assert np.array_equal(got[1][0], ref["grad_x"]) and np.array_equal(got[1][1], ref["grad_y"])


def test_the_class_states_its_goal_like_distribution_differential():
    import tfrt.analyze as analyze
    import tfrt.optimizer as optimizer
    domain = ((-1.0, 1.0), (0.0, 3.0))

    def bump(gx, gy):
        return torch.exp(-(gx ** 2 + (gy - 1.0) ** 2))
    erf = optimizer.DensityError(("y_end", "z_end"), bump, domain, bins=(6, 4))
    dd = analyze.DistributionDifferential(bump, domain, x_bins=6, y_bins=4)
    assert erf.goal.shape == (4, 6) and erf.goal.dtype == torch.float64
    assert torch.equal(erf.goal.cpu(), dd._goal.cpu()) and erf.g is erf.goal
    assert erf.grid == (-1.0, 1.0, 3.0, 0.0, 3.0, 4.0 / 3.0)
    with pytest.raises(ValueError):
        optimizer.DensityError(("y_end", "z_end"), np.zeros((3, 3)), domain)
    with pytest.raises(ValueError):
        optimizer.DensityError(("y_end",), np.ones((3, 3)), domain[:1])
    with pytest.raises(ValueError):
        optimizer.DensityError(("y_end", "z_end"), np.ones((300, 300)), domain)
    with pytest.raises(ValueError):
        optimizer.DensityError(("y_end", "w"), np.ones((3, 3)), domain)
    with pytest.raises(ValueError):
        optimizer.DensityError(("y_end", "z_end"), np.ones((3, 3)), ((1.0, 1.0), (0.0, 1.0)))
    one = optimizer.DensityError("y_end", np.ones(5), ((0.0, 1.0),))
    assert one.rows == [4] and one.rows_for(2) == [3]
    with pytest.raises(ValueError):
        erf.rows_for(2)
    # neither fused 2-D step nor anything but the three error classes
    from tensorflowraytrace_amd.fused_step import FusedStep

    class _Eng:
        dimension, ray_shard = 2, None

        @staticmethod
        def _custom_ops():
            return False

    class _Opt:
        engine, error_function = _Eng(), one
    assert FusedStep.eligible2d(_Opt()) is False


def test_the_generic_path_returns_one_term_and_the_gradient_rows():
    """DensityError.__call__ on CPU tensors: a (1,) error and, through backward, the reference's
    gradient on the finished rays' fields."""
    import tfrt.optimizer as optimizer
    x, y, _ = dr.points(300)
    goal = dr.goal_of(7, 3)
    erf = optimizer.DensityError(("y_end", "z_end"), goal, dr.DOMAIN, oob_weight=0.3)
    erf.goal = erf.goal.cpu()

    class _Engine:
        dimension = 3
    eng = _Engine()
    fy = torch.tensor(x, requires_grad=True)
    fz = torch.tensor(y, requires_grad=True)
    eng.finished_rays = {"y_end": fy, "z_end": fz}
    e = erf(eng)
    assert e.shape == (1,)
    ref = dr.density_error(x, y, goal, dr.DOMAIN, oob_weight=0.3)
    (3.0 * e.sum()).backward()
    assert abs(float(e) - ref["error"]) <= dr.error_bound(ref)
    assert np.array_equal(erf.last_hq.numpy(), ref["Hq"])
    tol = 3.0 * dr.gradient_bound(ref)
    assert np.abs(fy.grad.numpy() - 3.0 * ref["grad_x"]).max() <= tol
    assert np.abs(fz.grad.numpy() - 3.0 * ref["grad_y"]).max() <= tol
    eng.finished_rays = {}
    assert abs(float(erf(eng)) - 1.0) <= 16 * 21 * EPS


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    L = _lib.lib()
    assert L.tfrt_density_error_workspace_bytes(10, 0, 4) == 0
    assert L.tfrt_density_error_workspace_bytes(10, 512, 512) == 0
    assert L.tfrt_density_error_workspace_bytes(-1, 4, 4) == 0
    small = L.tfrt_density_error_workspace_bytes(0, 4, 4)
    assert 0 < small <= L.tfrt_density_error_workspace_bytes(1_000_000, 256, 256)
    dummy = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(dummy, ctypes.c_void_p)

    def call(n=8, nx=4, ny=4, row_x=0, row_y=1, x1=1.0, sx=4.0, oob=0.0, ws=1 << 16, stride=8,
             variant=0, goal=p, dtype=1):
        return L.tfrt_density_error(p, stride, n, dtype, None, row_x, row_y, goal, nx, ny, 0.0, x1,
                                    sx, 0.0, 1.0, 4.0, oob, p, 8, p, p, variant, p, ws, None)
    for bad in (dict(n=-1), dict(nx=0), dict(nx=512, ny=512), dict(row_x=6), dict(row_y=0),
                dict(x1=0.0), dict(sx=0.0), dict(oob=-1.0), dict(stride=4), dict(variant=3),
                dict(goal=None), dict(row_y=-1), dict(n=1 << 31), dict(dtype=7),
                dict(nx=128, ny=128, variant=1), dict(sx=float("nan")), dict(oob=float("inf"))):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
