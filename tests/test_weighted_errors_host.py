"""
Weighted DensityError and SpotError without a GPU: the CPU paths of ops.density_error and
ops.spot_error -- the same fixed point as the kernels -- against the numpy / Python-integer
reference of tests/weighted_errors_reference.py, the limbs against the exact sums, the
normalisation, the gradient against a finite difference, ``spot_wbits`` and the constructors'
refusals.
"""
import numpy as np
import pytest
import torch

import density_error_reference as dr
import spot_error_reference as sr
import weighted_errors_reference as wr

COUNTS = (0, 1, 63, 64, 65, 1000, 4097)
OOB = 0.3


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------ the inputs' guard
@pytest.mark.parametrize("n", COUNTS)
def test_the_inputs_hold_what_they_promise(n):
    x, y, mask, group, perm, weight, wbits = wr.spot_inputs(n, n_groups=3)
    for m, p in ((None, None), (mask, perm)):
        ref = wr.spot_error(x, y, group, 3, sr.DOMAIN, weight, OOB, mask=m, perm=p)
        wr.guard(n, ref["inside"], weight, p, wr.special_weights(wbits))
    if n >= 64:
        # half a quantum and a quarter round to 0, one and a half to 2 (ties to even)
        at = dict(zip(wr.special_weights(wbits)[:5], wr.SPECIAL_AT))
        ref = wr.spot_error(x, y, group, 3, sr.DOMAIN, weight, OOB)
        q = np.ldexp(1.0, -wbits)
        assert ref["wq"][at[0.5 * q]] == 0 and ref["wq"][at[0.25 * q]] == 0
        assert ref["wq"][at[1.5 * q]] == 2 and ref["wq"][at[1.0]] == 2 ** wbits
    x, y, mask, perm, weight = wr.density_inputs(n)
    for m, p in ((None, None), (mask, perm)):
        ref = wr.density_error(x, y, dr.goal_of(7, 5), dr.DOMAIN, weight, OOB, mask=m, perm=p)
        wr.guard(n, ref["inside"] & (ref["w"] > 0), weight, p, wr.special_weights(20))


# ------------------------------------------------------------------------------ the CPU paths
def _spot_cpu(n, G, two, masked, permuted, dtype=np.float64):
    from tensorflowraytrace_amd import ops
    x, y, mask, group, perm, weight, wbits = wr.spot_inputs(n, dtype, n_groups=G)
    rows = torch.full((6, n), 7.0, dtype=torch.float32 if dtype == np.float32 else torch.float64)
    rows[4], rows[5] = torch.tensor(x), torch.tensor(y)
    grad = torch.full((6, n), float("nan"), dtype=torch.float64)
    qbits = ops.spot_qbits(group.shape[0])
    grid = ops.spot_grid(sr.DOMAIN if two else sr.DOMAIN[:1], qbits)
    err, grad, acc = ops.spot_error(
        rows, 4, 5 if two else -1, torch.tensor(group), G, grid, OOB,
        mask=torch.tensor(mask) if masked else None, perm=torch.tensor(perm) if permuted else None,
        grad=grad, weights=torch.tensor(weight))
    ref = wr.spot_error(x, y if two else None, group, G, sr.DOMAIN if two else sr.DOMAIN[:1],
                        weight, OOB, mask=mask if masked else None,
                        perm=perm if permuted else None)
    return err.numpy(), grad.numpy(), acc.numpy(), ref


@pytest.mark.parametrize("G", (1, 3, 512, 513))
def test_spot_cpu_path_equals_the_reference(G):
    """Records as integers, gradients bit for bit (non-counting columns 0, untouched rows NaN),
    error within ``error_bound``; and the limbs against the exact, unsplit sums."""
    for n in COUNTS:
        for two in (True, False):
            for masked, permuted in ((False, False), (True, True)):
                err, grad, acc, ref = _spot_cpu(n, G, two, masked, permuted)
                assert acc.shape == (G, 8) and np.array_equal(acc, ref["acc"])
                for g in range(G):
                    for k in range(2):
                        hi, lo = int(acc[g, 1 + 2 * k]), int(acc[g, 2 + 2 * k])
                        assert (hi << ref["h"]) + lo == ref["exact"][g, k]
                assert np.array_equal(_bits(grad[4]), _bits(ref["grad_x"]))
                if two:
                    assert np.array_equal(_bits(grad[5]), _bits(ref["grad_y"]))
                else:
                    assert np.isnan(grad[5]).all()
                assert np.isnan(grad[:4]).all()
                print(f"n {n} error {err[0]!r} reference {ref['error']!r} "
                      f"bound {sr.error_bound(ref):.3e}")
                assert abs(err[0] - ref["error"]) <= sr.error_bound(ref)
                assert err[1] == ref["terms"]


@pytest.mark.parametrize("nx,ny", ((1, 1), (7, 5), (64, 64)))
def test_density_cpu_path_equals_the_reference(nx, ny):
    """Histogram as integers; the gradient bit for bit from the path's own pulls (which it leaves
    in the workspace) and within ``gradient_bound`` of the reference's pulls -- their sums over
    the bins are torch's here and numpy's there --; error within ``error_bound``."""
    from tensorflowraytrace_amd import ops
    for n in COUNTS:
        for two in (True, False):
            for masked, permuted in ((False, False), (True, True)):
                x, y, mask, perm, weight = wr.density_inputs(n)
                dom = dr.DOMAIN if two else dr.DOMAIN[:1]
                goal = dr.goal_of(nx, ny, two) if two else dr.goal_of(nx * ny, 1, False)
                rows = torch.full((6, n), 7.0, dtype=torch.float64)
                rows[4], rows[5] = torch.tensor(x), torch.tensor(y)
                grad = torch.full((6, n), float("nan"), dtype=torch.float64)
                g = torch.tensor(dr.normalise(goal)).contiguous()
                grid = ops.density_grid(dom, g.shape[-1], g.shape[0] if two else None)
                ws = torch.zeros(8 * g.numel(), dtype=torch.uint8)
                err, grad, hq = ops.density_error(
                    rows, 4, 5 if two else -1, g, grid, OOB,
                    mask=torch.tensor(mask) if masked else None,
                    perm=torch.tensor(perm) if permuted else None, grad=grad, workspace=ws,
                    weights=torch.tensor(weight))
                kw = dict(mask=mask if masked else None, perm=perm if permuted else None)
                ref = wr.density_error(x, y if two else None, goal, dom, weight, OOB, **kw)
                own = wr.density_error(x, y if two else None, goal, dom, weight, OOB,
                                       pulls=ws.view(torch.float64).numpy(), **kw)
                assert np.array_equal(hq.numpy(), ref["Hq"])
                grad = grad.numpy()
                assert np.array_equal(_bits(grad[4]), _bits(own["grad_x"]))
                assert np.abs(grad[4] - ref["grad_x"]).max(initial=0.0) <= dr.gradient_bound(ref)
                if two:
                    assert np.array_equal(_bits(grad[5]), _bits(own["grad_y"]))
                    assert np.abs(grad[5] - ref["grad_y"]).max(initial=0.0) <= dr.gradient_bound(ref)
                assert np.isnan(grad[:4]).all()
                assert abs(float(err[0]) - ref["error"]) <= dr.error_bound(ref)


def test_all_ones_weights_give_the_unweighted_sums():
    """W == 2**wbits * count, and the recombined limbs equal 2**wbits * Sx of the unweighted
    reference, as integers."""
    from tensorflowraytrace_amd import ops
    n, G = 4097, 37
    x, y, mask, group, perm = sr.points(n, n_groups=G)
    wbits = ops.spot_wbits(group.shape[0])
    rows = torch.stack([torch.tensor(x), torch.tensor(y)])
    grid = ops.spot_grid(sr.DOMAIN, ops.spot_qbits(group.shape[0]))
    _, _, acc = ops.spot_error(rows, 0, 1, torch.tensor(group), G, grid, OOB,
                               mask=torch.tensor(mask), perm=torch.tensor(perm),
                               weights=torch.ones(group.shape[0], dtype=torch.float64))
    plain = sr.spot_error(x, y, group, G, sr.DOMAIN, OOB, mask=mask, perm=perm)["acc"]
    h = ops.spot_qbits(group.shape[0]) // 2
    assert plain[:, 0].sum() > n // 2
    for g in range(G):
        rec = [int(v) for v in acc[g]]
        assert rec[0] == (int(plain[g, 0]) << wbits) and rec[5] == int(plain[g, 0])
        assert (rec[1] << h) + rec[2] == int(plain[g, 1]) << wbits
        assert (rec[3] << h) + rec[4] == int(plain[g, 2]) << wbits
        assert rec[6] == 0 and rec[7] == 0


def test_doubling_all_weights_changes_nothing():
    """Only ratios matter: the classes divide by the maximum once."""
    from tensorflowraytrace_amd import optimizer
    rng = np.random.default_rng(2)
    w = 0.05 + rng.random(500)
    lab = np.arange(500) % 4
    a = optimizer.SpotError(("y_end", "z_end"), lab, sr.DOMAIN, weights=w)
    b = optimizer.SpotError(("y_end", "z_end"), lab, sr.DOMAIN, weights=2.0 * w)
    assert a.weights.dtype == torch.float64 and float(a.weights.max()) == 1.0
    assert torch.equal(a.weights, b.weights)
    goal = dr.goal_of(7, 5)
    c = optimizer.DensityError(("y_end", "z_end"), goal, dr.DOMAIN, weights=torch.tensor(w))
    d = optimizer.DensityError(("y_end", "z_end"), goal, dr.DOMAIN, weights=torch.tensor(2.0 * w))
    assert torch.equal(c.weights, d.weights) and float(c.weights.min()) >= 0.0
    assert optimizer.DensityError(("y_end", "z_end"), goal, dr.DOMAIN).weights_of({}) is None


def test_plain_form_gradient_is_the_finite_difference():
    """``(2 * wr) * dx`` is the gradient of ``sum wr |x - c_w|**2`` with the weighted centroid
    differentiated through (the weighted residuals of a group sum to zero): central differences of
    the unquantised form.  Step 1e-6 on coordinates of order 1: truncation is zero for a quadratic,
    rounding about eps * E / step = 1e-16 * 1e3 / 1e-6 = 1e-7 at worst; bound 1e-6."""
    x, y, _, group, _, weight, wbits = wr.spot_inputs(200, n_groups=5)
    keep = np.isfinite(x) & np.isfinite(y)
    x, y, lab, w = x[keep], y[keep], group[:200][keep], weight[:200][keep]
    w = np.where(np.isfinite(w) & (w >= 0) & (w <= 1), w, 0.5)

    def f(xv, yv):
        return wr.spot_error(xv, yv, lab, 5, sr.DOMAIN, w, OOB, quantise=False)

    ref = f(x, y)
    assert ref["n_inside"] > 100 and ref["n_penalised"] > 5
    step = 1e-6
    # (not the points on the domain's edge: the objective jumps there)
    (x0, x1), (y0, y1) = sr.DOMAIN
    off_edge = (np.minimum(np.abs(x - x0), np.abs(x - x1)) > 1e-3) \
        & (np.minimum(np.abs(y - y0), np.abs(y - y1)) > 1e-3)
    for i in list(np.nonzero(ref["inside"] & off_edge)[0][:12]) \
            + list(np.nonzero(ref["outside"] & off_edge)[0][:4]):
        for arr, key in ((x, "grad_x"), (y, "grad_y")):
            up, dn = arr.copy(), arr.copy()
            up[i] += step
            dn[i] -= step
            args = (lambda a: (a, y)) if arr is x else (lambda a: (x, a))
            fd = (f(*args(up))["error"] - f(*args(dn))["error"]) / (2 * step)
            assert abs(fd - ref[key][i]) <= 1e-6, (i, key, fd, ref[key][i])


@pytest.mark.parametrize("N", (1, 4096, 10 ** 6, 2 ** 31 - 1))
def test_spot_wbits_and_the_overflow_bound(N):
    from tensorflowraytrace_amd import ops
    qbits, wbits = ops.spot_qbits(N), ops.spot_wbits(N)
    assert wbits == wr.wbits_of(N) == min(20, 62 - N.bit_length() - -(-qbits // 2))
    assert 1 <= wbits <= 20
    # every sum of N rays stays below 2^62: W, the high limb (qx >> h <= 2^ceil(qbits / 2)) and
    # the low limb (< 2^h)
    h = qbits // 2
    assert N * 2 ** wbits * ((2 ** qbits) >> h) < 2 ** 62
    assert N * 2 ** wbits * (2 ** h) < 2 ** 62
    assert N < 2 ** (62 - wbits - (qbits + 1) // 2)


def test_constructor_errors():
    from tensorflowraytrace_amd import optimizer
    lab = np.arange(8) % 2
    goal = dr.goal_of(4, 4)

    def spot(w):
        return optimizer.SpotError(("y_end", "z_end"), lab, sr.DOMAIN, weights=w)

    def density(w):
        return optimizer.DensityError(("y_end", "z_end"), goal, dr.DOMAIN, weights=w)

    ok = np.linspace(0.1, 1.0, 8)
    assert spot(ok).weights.numel() == 8 and density(ok).weights.numel() == 8
    bad = [np.where(np.arange(8) == 3, -0.5, ok), np.where(np.arange(8) == 3, np.nan, ok),
           np.where(np.arange(8) == 3, np.inf, ok), np.zeros(8), np.ones((2, 4)), np.arange(8)]
    for make in (spot, density):
        for w in bad:
            with pytest.raises(ValueError):
                make(w)
    with pytest.raises(ValueError):
        spot(np.ones(7))                      # one weight per label
    src = {"x_start": torch.zeros(9, dtype=torch.float64)}
    with pytest.raises(ValueError):
        density(ok).weights_of(src)           # one weight per source ray
    # a callable is evaluated on the source's fields, normalised and cached
    calls = []

    def cos(fields):
        calls.append(1)
        return 2.0 + fields["x_start"]

    erf = density(cos)
    assert erf.weights is None
    w1 = erf.weights_of(src)
    assert erf.weights_of(src) is w1 and len(calls) == 1 and float(w1.max()) == 1.0
    with pytest.raises(ValueError):
        density(lambda fields: -torch.ones(9, dtype=torch.float64)).weights_of(src)
    key = erf.graph_key()
    erf.weights.mul_(0.5)
    assert erf.graph_key() == key
    erf.weights = erf.weights.clone()
    assert erf.graph_key() != key
    s = spot(ok)
    assert s.graph_key()[-1] == 20
