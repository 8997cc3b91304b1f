"""
TransportError without a GPU: the CPU path of ``ops.transport_error`` against the numpy
restatement of the definition (tests/transport_error_reference.py) -- ranks equal as integers,
gradient rows bit for bit, the error within ``error_bound`` --, the properties of the quantile
tables, order independence, the descent that motivates the objective (a blob that starts outside
the domain, where a DensityError's histogram has no gradient, is transported onto the goal), the
constructor's errors, and csrc/transport_math.h on the host: tests/transport_host/transport_main.cpp
(its own main) compiled with g++ and the address and undefined-behaviour sanitizers.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import transport_error_reference as ref
from tensorflowraytrace_amd import ops, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "transport_host", "transport_main.cpp")

CASES = [(family, n, K, Q)
         for family in ref.FAMILIES
         for n, K, Q in ((1, 1, 2), (65, 3, 2), (1025, 8, 1024), (1023, 1, 1024))]


def _setup(K, Q, two):
    goal = ref.goal_of(16, 12, two)
    domain = ref.DOMAIN if two else ref.DOMAIN[:1]
    cs = ops.transport_directions(K, 2 if two else 1)
    tables = ops.transport_tables(goal, domain, cs, Q)
    return goal, domain, cs, tables


def _evaluate(x, y, mask, domain, cs, tables, dtype=torch.float64, pad=0):
    """ops.transport_error on the CPU over rows (y, x) -- row_x = 1, row_y = 0 -- of a block with
    ``pad`` extra columns."""
    n = x.shape[0]
    two = y is not None
    block = torch.zeros((2, n + pad), dtype=dtype)
    block[1, :n] = torch.as_tensor(x).to(dtype)
    if two:
        block[0, :n] = torch.as_tensor(y).to(dtype)
    rows = block[:, :n]
    return ops.transport_error(rows, 1, 0 if two else -1, torch.as_tensor(tables),
                               ops.transport_grid(domain), torch.as_tensor(cs),
                               mask=None if mask is None else torch.as_tensor(mask))


def _check(out, want, two):
    err, grad, rank2 = out
    assert np.array_equal(rank2.numpy().astype(np.int64), want["rank2"])
    assert np.array_equal(grad[1].numpy(), want["grad_x"])
    if two:
        assert np.array_equal(grad[0].numpy(), want["grad_y"])
    total, terms, mean = want["error"]
    assert float(err[1]) == terms
    assert abs(float(err[0]) - total) <= ref.error_bound(want)
    if terms == 0:
        assert float(err[0]) == 0.0 and np.isnan(float(err[2]))
        assert not grad.any()
    else:
        assert abs(float(err[2]) - mean) <= ref.error_bound(want) / terms


@pytest.mark.parametrize("family,n,K,Q", CASES)
def test_cpu_path_equals_the_reference(family, n, K, Q):
    two = K > 1 or n == 1025
    goal, domain, cs, tables = _setup(K, Q, two)
    x, y, mask = ref.points(family, n, seed=n)
    if not two:
        y = None
    want = ref.transport_error(x, y, tables, cs, domain, mask)
    _check(_evaluate(x, y, mask, domain, cs, tables), want, two)
    if family in ("all_invalid",):
        assert want["n_valid"] == 0
    if family == "one_valid":
        assert want["n_valid"] == 1 and (want["rank2"].max(axis=1) == 1).all()
    if family == "ties":
        assert (want["rank2"] == n).all()         # first = 0, count = n


def test_float32_state_is_upcast():
    """float32 rows give the reference of the upcast values; a padded stride changes nothing."""
    goal, domain, cs, tables = _setup(3, 64, True)
    x, y, mask = ref.points("masked", 333, seed=5)
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    want = ref.transport_error(x32.astype(np.float64), y32.astype(np.float64), tables, cs, domain,
                               mask)
    _check(_evaluate(x32, y32, mask, domain, cs, tables, torch.float32, pad=7), want, True)


def test_tables_equal_the_reference_and_do_not_decrease():
    for two, K, Q in ((True, 8, 1024), (True, 3, 2), (False, 1, 1024), (False, 1, 7)):
        goal, domain, cs, tables = _setup(K, Q, two)
        assert tables.shape == (K, Q + 1) and tables.dtype == np.float64
        assert np.array_equal(tables, ref.tables(goal, cs, Q))
        assert (np.diff(tables, axis=1) >= 0).all()
    # explicit angles are taken as given
    theta = np.array([0.1, 1.3, 2.9])
    assert np.array_equal(ops.transport_directions(theta),
                          np.stack([np.cos(theta), np.sin(theta)], axis=1))


@pytest.mark.parametrize("nx,Q", [(1, 16), (4, 64), (16, 1024)])
def test_uniform_goal_gives_the_identity_up_to_half_a_subcell(nx, Q):
    """cm of a uniform goal is the sub-cell centres themselves; np.interp clamps outside the first
    and the last of them: |T[m] - m / Q| <= 1 / (2 * 4 * nx), reached at both ends.  (Bin counts
    that are powers of two: the centres, the knots and the differences are then exact in float64
    and the bound is tested as it stands.)"""
    T = ops.transport_tables(np.ones(nx), ((2.0, 5.0),), ops.transport_directions(1, 1), Q)[0]
    dev = np.abs(T - np.arange(Q + 1) / Q)
    half = 1.0 / (2 * 4 * nx)
    assert dev.max() <= half and dev[0] == half and dev[-1] == half
    # two fields, along the axes: the same
    T2 = ops.transport_tables(np.ones((2, nx)), ((0.0, 1.0), (0.0, 2.0)),
                              ops.transport_directions(np.array([0.0])), Q)
    assert np.abs(T2[0] - np.arange(Q + 1) / Q).max() <= half
    T3 = ops.transport_tables(np.ones((nx, 2)), ((0.0, 1.0), (0.0, 2.0)),   # ny = nx bins along eta
                              np.array([[0.0, 1.0]]), Q)
    assert np.abs(T3[0] - np.arange(Q + 1) / Q).max() <= half


def test_set_goal_writes_into_the_same_buffer():
    goal = ref.goal_of(16, 12)
    erf = optimizer.TransportError(("y_end", "z_end"), goal, ref.DOMAIN, directions=3, knots=64)
    assert tuple(erf.tables.shape) == (3, 65) and erf.tables.dtype == torch.float64
    assert np.array_equal(erf.tables.cpu().numpy(), ref.tables(goal, ref.directions(3), 64))
    ptr, key = erf.tables.data_ptr(), erf.graph_key()
    other = goal[::-1].copy()
    erf.set_goal(other)
    assert erf.tables.data_ptr() == ptr and erf.graph_key() == key
    assert np.array_equal(erf.tables.cpu().numpy(), ref.tables(other, ref.directions(3), 64))
    with pytest.raises(ValueError, match="shape"):
        erf.set_goal(np.ones((12, 15)))
    with pytest.raises(ValueError, match="zero everywhere"):
        erf.set_goal(np.zeros((12, 16)))
    # default: 8 directions, 1,024 knots; one field: one direction
    assert tuple(optimizer.TransportError(("y_end", "z_end"), goal, ref.DOMAIN).tables.shape) \
        == (8, 1025)
    one = optimizer.TransportError("y_end", ref.goal_of(16, 1, False), ref.DOMAIN[:1], knots=8)
    assert tuple(one.tables.shape) == (1, 9)
    # a callable goal with bins=, as DensityError takes it
    fn = optimizer.TransportError(("y_end", "z_end"), lambda X, Y: torch.exp(-(X * X + Y * Y)),
                                  ref.DOMAIN, bins=(16, 12), directions=2, knots=16)
    assert fn.goal_shape == (12, 16)


@pytest.mark.parametrize("family", ["uniform", "ties", "masked", "nonfinite"])
def test_permuting_the_columns_permutes_ranks_and_gradients(family):
    goal, domain, cs, tables = _setup(4, 256, True)
    x, y, mask = ref.points(family, 777, seed=3)
    perm = np.random.default_rng(11).permutation(777)
    err, grad, rank2 = _evaluate(x, y, mask, domain, cs, tables)
    errp, gradp, rank2p = _evaluate(x[perm], y[perm], None if mask is None else mask[perm], domain,
                                    cs, tables)
    assert torch.equal(rank2[:, perm], rank2p)
    assert np.array_equal(grad.numpy()[:, perm], gradp.numpy())
    assert float(err[1]) == float(errp[1])
    want = ref.transport_error(x, y, tables, cs, domain, mask)
    assert abs(float(err[0]) - float(errp[0])) <= ref.error_bound(want)


def test_descent_transports_a_blob_from_outside_onto_the_goal():
    """4,096 points start as a blob of sigma 0.05 at (1.5, -0.5) in domain units -- outside the
    domain, where a DensityError's histogram term has no gradient at all -- and 40 steps of
    ``x -= (0.5 / K) * grad`` bring the mean term below 1e-3 of its start (a numpy prototype of the
    definition reached about 1e-5; the factor of 100 is margin for another generator)."""
    K, n = 8, 4096
    xs = (np.arange(16) + 0.5) / 16
    X, Y = np.meshgrid(xs, xs, indexing="xy")
    goal = np.exp(-((X - 0.3) ** 2 + (Y - 0.3) ** 2) / 0.02) \
        + np.exp(-((X - 0.7) ** 2 + (Y - 0.65) ** 2) / 0.02)
    domain = ((0.0, 1.0), (0.0, 1.0))
    cs = torch.as_tensor(ops.transport_directions(K))
    tables = torch.as_tensor(ops.transport_tables(goal, domain, cs.numpy(), 1024))
    grid = ops.transport_grid(domain)
    rng = np.random.default_rng(20240607)
    pts = torch.as_tensor(np.stack([1.5 + 0.05 * rng.standard_normal(n),
                                    -0.5 + 0.05 * rng.standard_normal(n)]))

    g = torch.as_tensor(goal / np.linalg.norm(goal))
    _, dgrad, hq = ops.density_error(pts, 0, 1, g, ops.density_grid(domain, 16, 16), 0.0)
    assert not dgrad.any() and not hq.any()

    means = []
    for _ in range(40):
        err, grad, _ = ops.transport_error(pts, 0, 1, tables, grid, cs)
        means.append(float(err[2]))
        pts = pts - (0.5 / K) * grad
    err, _, _ = ops.transport_error(pts, 0, 1, tables, grid, cs)
    means.append(float(err[2]))
    print(f"mean term: start {means[0]:.3e}, after 40 steps {means[-1]:.3e}")
    assert means[-1] < 1e-3 * means[0]
    assert bool(((pts >= 0) & (pts <= 1)).all(dim=0).double().mean() > 0.99)


def test_constructor_errors():
    T = optimizer.TransportError
    goal = ref.goal_of(16, 12)
    ok = dict(goal=goal, domain=ref.DOMAIN)
    with pytest.raises(ValueError, match="direction fields"):
        T(("y_dir", "z_dir"), **ok)
    with pytest.raises(ValueError, match="direction fields"):
        T(("y_end", "z_dir"), **ok)
    with pytest.raises(ValueError, match="weights"):
        T(("y_end", "z_end"), weights=np.ones(8), **ok)
    with pytest.raises(ValueError, match="zero everywhere"):
        T(("y_end", "z_end"), np.zeros((12, 16)), ref.DOMAIN)
    with pytest.raises(ValueError, match="non-negative"):
        T(("y_end", "z_end"), -goal, ref.DOMAIN)
    with pytest.raises(ValueError, match="distinct fields"):
        T(("y_end", "y_end"), **ok)
    with pytest.raises(ValueError, match="domain"):
        T(("y_end", "z_end"), goal, ((0.0, 1.0),))
    with pytest.raises(ValueError, match="domain"):
        T(("y_end", "z_end"), goal, ((0.0, 1.0), (1.0, 1.0)))
    with pytest.raises(ValueError, match="dimension"):
        T(("y_end", "z_end"), goal[0], ref.DOMAIN)
    with pytest.raises(ValueError, match="bins"):
        T(("y_end", "z_end"), lambda X, Y: X, ref.DOMAIN)
    for bad in (0, 65, -1, 2.5, [], [0.0, np.nan], np.zeros((2, 2)), "many"):
        with pytest.raises(ValueError, match="directions"):
            T(("y_end", "z_end"), directions=bad, **ok)
    for bad in (1, 0, 65537, 10.5, None, "many"):
        with pytest.raises(ValueError, match="knots"):
            T(("y_end", "z_end"), knots=bad, **ok)
    # exported where DensityError is, and through the tfrt shim
    import tfrt.optimizer
    assert tfrt.optimizer.TransportError is T
    assert ops.TRANSPORT_KEY_BITS == ref.KEY_BITS == 26


def test_ops_argument_errors():
    goal, domain, cs, tables = _setup(3, 16, True)
    rows = torch.zeros((2, 5), dtype=torch.float64)
    grid, T, A = ops.transport_grid(domain), torch.as_tensor(tables), torch.as_tensor(cs)
    with pytest.raises(ValueError, match="rows"):
        ops.transport_error(rows, 0, 0, T, grid, A)
    with pytest.raises(ValueError, match="rows"):
        ops.transport_error(rows, 0, 2, T, grid, A)
    with pytest.raises(ValueError, match="directions"):
        ops.transport_error(rows, 0, -1, T, grid, A)            # one field, three directions
    with pytest.raises(ValueError, match="tables"):
        ops.transport_error(rows, 0, 1, T.float(), grid, A)
    with pytest.raises(ValueError, match="tables"):
        ops.transport_error(rows, 0, 1, T, grid, A[:2])
    with pytest.raises(ValueError, match="rank2"):
        ops.transport_error(rows, 0, 1, T, grid, A, rank2=torch.zeros((3, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="dimension"):
        ops.transport_error(rows, 0, 1, T, grid, A, dimension=3)


def _pack(n, K, Q, two, grid, cs, tables, x, y, valid, rank2, nv):
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).tobytes()       # noqa: E731
    return (struct.pack("<4q", n, K, Q, int(two)) + f8(grid) + f8(cs) + f8(tables) + f8(x) + f8(y)
            + i4(valid) + i4(rank2) + i4([nv]))


def test_transport_math_on_the_host_under_the_sanitizers(tmp_path):
    """Keys, projections and interpolated targets of transport_math.h equal the reference's, for
    every family; the program's tables are exact-size allocations, so a read past T[Q] -- the
    mid-rank of the last ray lands on z = Q exactly with one valid ray and Q = 2 -- would be
    found."""
    exe = tmp_path / "transport_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    for family in ref.FAMILIES:
        for n, K, Q, two in ((257, 5, 2, True), (64, 1, 1024, False), (1, 2, 3, True)):
            goal, domain, cs, tables = _setup(K, Q, two)
            x, y, mask = ref.points(family, n, seed=7)
            want = ref.transport_error(x, y if two else None, tables, cs, domain, mask)
            valid = want["rank2"][0] >= 0
            src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
            src.write_bytes(_pack(n, K, Q, two, ops.transport_grid(domain), cs, tables, x, y, valid,
                                  want["rank2"], max(want["n_valid"], 1)))
            run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
            assert run.returncode == 0, f"{family} {n} {K} {Q}: {run.stdout}{run.stderr}"
            raw = dst.read_bytes()
            keys = np.frombuffer(raw[:4 * K * n], dtype=np.uint32).reshape(K, n)
            p, t = np.frombuffer(raw[4 * K * n:], dtype=np.float64).reshape(2, K, n)
            assert np.array_equal(keys.astype(np.int64), want["keys"]), family
            assert np.array_equal(p, want["p"]) and np.array_equal(t, want["t"]), family
