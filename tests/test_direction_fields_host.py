"""
The direction fields (x_dir, y_dir, z_dir) of DensityError and SpotError without a GPU: the numpy
reference (tests/direction_fields_reference.py) against torch.autograd on e / |e|, the CPU path of
ops.density_error / ops.spot_error with ``dimension`` against the reference, the classes' field
codes, argument checks and generic path, and position fields through both entries.
"""
import numpy as np
import pytest
import torch

import density_error_reference as dr
import direction_fields_reference as df
import spot_error_reference as sr

EPS = df.EPS
OOB = 0.3
BINS = (7, 3)                                     # (nx, ny)
MIXED_DOMAIN = ((-1.5, 1.0), df.DOMAIN[0])        # (y_end, y_dir): a phase-space pair

# (name, dimension, codes, domain)
CASES = [
    ("one", 3, (7,), df.DOMAIN[:1]),
    ("two", 3, (7, 8), df.DOMAIN),
    ("mixed", 3, (4, 7), MIXED_DOMAIN),
    ("mixed_start", 3, (8, 1), (df.DOMAIN[1], (-0.6, 0.8))),
    ("2d_one", 2, (5,), df.DOMAIN[:1]),
    ("2d_mixed", 2, (5, 3), (df.DOMAIN[0], (-1.5, 1.0))),
    # x_dir on a 2-D block is code 4 (1 / sqrt(1 + a^2), a ~ N(0, .35): 0.8 .. 1), x_end code 2
    ("2d_x_dir", 2, (4,), ((0.9, 0.995),)),
    ("2d_both", 2, (4, 5), ((0.9, 0.995), df.DOMAIN[0])),
    ("2d_x_end_y_dir", 2, (2, 5), ((0.0, 2.5), df.DOMAIN[0])),
    ("2d_x_dir_x_start", 2, (4, 0), ((0.9, 0.995), (-0.6, 0.8))),
]
IDS = [c[0] for c in CASES]


def test_the_generator_gives_the_recorded_census():
    want = {64: (59, 27, 32), 65: (60, 25, 35), 1000: (901, 467, 434), 20000: (18006, 9183, 8823)}
    for dtype in (np.float64, np.float32):
        for n, (counting, inside, penalised) in want.items():
            c = df.assert_generator(n, df.rays(n, dtype), (7, 8), df.DOMAIN, compare_f32=True)
            assert (c["counting"], c["inside"], c["penalised"]) == (counting, inside, penalised)
            assert c["min_L"] > 0.5


@pytest.mark.parametrize("codes", [(6, 7, 8), (7, 8), (8, 6), (7,)])
def test_reference_chain_equals_autograd(codes):
    """sum_k gv_k * d_(a_k) with d = e / |e| under float64 autograd: the chain's rows within
    4 eps max|G| (a handful of roundings per entry, each relative to a quantity below max|G| L / L)."""
    n = 500
    block = df.rays(n, np.float64)
    d, L, ok = df.directions(block)
    block, d, L = block[:, ok], d[:, ok], L[ok]
    rng = np.random.default_rng(3)
    gv = [rng.normal(0, 1, block.shape[1]) for _ in codes]
    got = df.chain(gv, codes, d, L, np.ones_like(L, dtype=bool))
    t = torch.tensor(block, requires_grad=True)
    e = t[3:] - t[:3]
    dd = e / torch.sqrt((e * e).sum(dim=0))
    obj = sum((torch.tensor(g) * dd[c - 6]).sum() for g, c in zip(gv, codes))
    want, = torch.autograd.grad(obj, t)
    top = float(np.abs(got).max())
    worst = float(np.abs(got - want.numpy()).max())
    print(f"max|G| {top:.3g}, max abs difference {worst:.3g}")
    assert top > 0.5 and worst <= 4 * EPS * top


def _density_grad_check(grad, ref, codes, dim):
    """Inside rays within the bound per entry, every other column bit for bit."""
    inside = ref["inside"]
    rest = ~inside
    assert grad[:, rest].tobytes() == ref["grad"][:, rest].tobytes()
    top = max(float(np.abs(g).max()) for g in ref["gv"])
    gb = dr.gradient_bound(ref)
    L = ref["L"][inside]
    # the chain adds at most three gv errors (gb each) and a handful of roundings, all divided by L
    bound = (3 * gb + 8 * EPS * top) / L
    diff = np.abs(grad[:, inside] - ref["grad"][:, inside])
    print(f"gradient: max difference {diff.max():.3g}, least bound {bound.min():.3g}")
    assert (diff <= bound[None, :]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_density_cpu_path_equals_the_reference(case, dtype):
    from tensorflowraytrace_amd import ops
    _, dim, codes, domain = case
    two = len(codes) == 2
    nx, ny = BINS if two else (BINS[0], 1)
    goal = dr.goal_of(nx, ny, two)
    for n in (65, 1000):
        block = df.rays(n, dtype, dimension=dim)
        if codes in ((7, 8), (7,), (5,)):
            df.assert_generator(n, block, codes, domain)
        mask = np.where(np.arange(n) % 5 == 4, -1, 0).astype(np.int32)
        for m in (None, mask):
            ref = df.density(block, codes, goal, domain, OOB, mask=m)
            assert ref["inside"].sum() > n / 8 and ref["n_penalised"] > 0
            grid = ops.density_grid(domain, nx, ny if two else None)
            err, grad, hq = ops.density_error(
                torch.tensor(block), codes[0], codes[1] if two else -1,
                torch.tensor(dr.normalise(goal)), grid, OOB,
                mask=None if m is None else torch.tensor(m), dimension=dim)
            assert np.array_equal(hq.numpy(), ref["Hq"])
            assert abs(float(err[0]) - ref["error"]) <= dr.error_bound(ref)
            assert float(err[1]) == 1.0 and float(err[2]) == float(err[0])
            _density_grad_check(grad.numpy(), ref, codes, dim)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_spot_cpu_path_equals_the_reference(case, dtype):
    from tensorflowraytrace_amd import ops
    _, dim, codes, domain = case
    two = len(codes) == 2
    for n, G in ((65, 3), (1000, 37)):
        block = df.rays(n, dtype, dimension=dim)
        rng = np.random.default_rng(n)
        group = rng.integers(-1, G, n + 3).astype(np.int32)
        perm = rng.permutation(n).astype(np.int32)
        perm[5] = -1
        mask = np.where(np.arange(n) % 5 == 4, -1, 0).astype(np.int32)
        for m, p in ((None, None), (mask, perm)):
            ref = df.spot(block, codes, group, G, domain, OOB, mask=m, perm=p)
            assert ref["n_inside"] > n / 8 and ref["n_penalised"] > 0
            qbits = ops.spot_qbits(group.shape[0])
            err, grad, acc = ops.spot_error(
                torch.tensor(block), codes[0], codes[1] if two else -1, torch.tensor(group), G,
                ops.spot_grid(domain, qbits), OOB, mask=None if m is None else torch.tensor(m),
                perm=None if p is None else torch.tensor(p), dimension=dim)
            assert np.array_equal(acc.numpy(), ref["acc"])
            assert abs(float(err[0]) - ref["error"]) <= sr.error_bound(ref)
            assert float(err[1]) == ref["terms"]
            assert grad.numpy().tobytes() == ref["grad"].tobytes()
            assert np.abs(ref["grad"]).max() > 0


def test_position_fields_give_the_same_bits_through_both_entries():
    """("y_end", "z_end"): ``dimension=None`` (the old entries) and ``dimension=3`` with the codes
    4, 5 -- error, gradient block and histogram / records bit for bit."""
    import tfrt.optimizer as optimizer
    n = 1000
    block = torch.tensor(df.rays(n, np.float32))
    domain = ((-1.5, 1.0), (-1.0, 1.5))
    dens = optimizer.DensityError(("y_end", "z_end"), dr.goal_of(7, 3), domain, oob_weight=OOB)
    dens.goal = dens.goal.cpu()
    group = np.arange(n) % 9
    spot = optimizer.SpotError(("y_end", "z_end"), group, domain, oob_weight=OOB)
    spot.labels = spot.labels.cpu()
    assert dens.rows == [4, 5] and spot.rows == [4, 5]
    for old, new in ((dens.evaluate(block, 4, 5), dens.evaluate(block, 4, 5, dimension=3)),
                     (spot.evaluate(block, 4, 5, spot.labels),
                      spot.evaluate(block, 4, 5, spot.labels, dimension=3))):
        for a, b in zip(old, new):
            assert a.numpy().tobytes() == b.numpy().tobytes()
        assert float(old[1].abs().max()) > 0 and not bool(old[1][:4].any())


def test_field_codes_and_argument_checks():
    import tfrt.optimizer as optimizer
    goal = dr.goal_of(7, 3)
    make = {
        "density": lambda fields, domain=df.DOMAIN: optimizer.DensityError(
            fields, goal if len(domain) == 2 else dr.goal_of(7, 1, False), domain),
        "spot": lambda fields, domain=df.DOMAIN: optimizer.SpotError(fields, np.arange(8) % 3,
                                                                     domain),
    }
    for name, new in make.items():
        erf = new(("y_dir", "z_dir"))
        assert erf.rows == [7, 8] and erf.rows_for(3) == [7, 8] and erf.has_direction
        assert new(("x_dir",), df.DOMAIN[:1]).rows == [6]
        assert new(("y_end", "y_dir")).rows == [4, 7]
        two_d = new(("x_dir", "y_dir"))
        assert two_d.rows == [6, 7] and two_d.rows_for(2) == [4, 5]
        assert new(("y_end", "y_dir")).rows_for(2) == [3, 5]
        # position fields as before
        old = new(("y_end", "z_end"))
        assert old.rows == [4, 5] and not old.has_direction
        assert new(("y_end",), df.DOMAIN[:1]).rows_for(2) == [3]
        with pytest.raises(ValueError):
            erf.rows_for(2)                              # z_dir on a 2-D engine
        with pytest.raises(ValueError):
            new(("z_end", "y_dir")).rows_for(2)
        with pytest.raises(ValueError):
            new(("y_dir", "y_dir"))
        with pytest.raises(ValueError):
            new(("w_dir", "y_dir"))
        with pytest.raises(ValueError):
            new(("dir",), df.DOMAIN[:1])
    # the field codes are part of what a captured step has baked in, through ``rows``
    assert make["spot"](("y_dir", "z_dir")).rows != make["spot"](("y_end", "z_end")).rows


def test_ops_refuse_bad_field_codes():
    from tensorflowraytrace_amd import ops
    block = torch.tensor(df.rays(10, np.float64))
    goal = torch.tensor(dr.normalise(dr.goal_of(7, 3)))
    grid = ops.density_grid(df.DOMAIN, 7, 3)
    for kw in (dict(dimension=1), dict(dimension=4), dict(dimension=2), dict(x=9), dict(y=9),
               dict(x=7, y=7), dict(x=-1)):
        d = kw.get("dimension", 3)
        with pytest.raises(ValueError):
            ops.density_error(block, kw.get("x", 7), kw.get("y", 8), goal, grid, dimension=d)
        with pytest.raises(ValueError):
            ops.spot_error(block, kw.get("x", 7), kw.get("y", 8),
                           torch.zeros(10, dtype=torch.int32), 1,
                           ops.spot_grid(df.DOMAIN, 40), dimension=d)


class _Engine:
    def __init__(self, block, dim, ids=None):
        names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end") if dim == 3 else \
            ("x_start", "y_start", "x_end", "y_end")
        self.dimension = dim
        self.leaves = [torch.tensor(r, requires_grad=True) for r in block]
        self.finished_rays = dict(zip(names, self.leaves))
        n = block.shape[1]
        self.last_trace = {"finished_id": torch.tensor(np.arange(n, dtype=np.int32) if ids is None
                                                       else ids)}
        self._trace_src = {"x_start": torch.zeros(n)}

    def grad(self):
        return np.stack([t.grad.numpy() for t in self.leaves])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_generic_path_hands_autograd_every_gradient_row(case):
    """``__call__`` on CPU tensors with a stub engine: the reference's error and, through
    backward, its 2d gradient rows on the engine's geometry fields."""
    import tfrt.optimizer as optimizer
    _, dim, codes, domain = case
    names = (("x_start", "y_start", "z_start", "x_end", "y_end", "z_end", "x_dir", "y_dir", "z_dir")
             if dim == 3 else ("x_start", "y_start", "x_end", "y_end", "x_dir", "y_dir"))
    fields = tuple(names[c] for c in codes)
    two = len(codes) == 2
    n, G = 300, 7
    block = df.rays(n, np.float64, dimension=dim)

    nx, ny = BINS if two else (BINS[0], 1)
    goal = dr.goal_of(nx, ny, two)
    erf = optimizer.DensityError(fields, goal, domain, oob_weight=OOB)
    erf.goal = erf.goal.cpu()
    eng = _Engine(block, dim)
    e = erf(eng)
    assert e.shape == (1,)
    e.sum().backward()
    ref = df.density(block, codes, goal, domain, OOB)
    assert np.array_equal(erf.last_hq.numpy(), ref["Hq"])
    assert abs(float(e.detach()) - ref["error"]) <= dr.error_bound(ref)
    _density_grad_check(eng.grad(), ref, codes, dim)

    rng = np.random.default_rng(1)
    group = rng.integers(-1, G - 1, n).astype(np.int32)          # (the last group stays empty)
    ids = rng.permutation(n).astype(np.int32)
    erf = optimizer.SpotError(fields, group, domain, oob_weight=OOB, n_groups=G)
    erf.labels = erf.labels.cpu()
    eng = _Engine(block, dim, ids)
    e = erf(eng)
    assert e.shape == (n, len(codes))
    (3.0 * e.sum()).backward()
    ref = df.spot(block, codes, group, G, domain, OOB, perm=ids)
    assert np.array_equal(erf.last_acc.numpy(), ref["acc"])
    assert abs(float(e.detach().sum()) - ref["error"]) <= sr.error_bound(ref)
    assert eng.grad().tobytes() == (3.0 * ref["grad"]).tobytes()
    c = erf.centroids().numpy()
    assert c.shape == (G, len(codes)) and np.isnan(c[-1]).all()
    assert np.array_equal(c, ref["centroids"], equal_nan=True)
    e = e.detach().numpy()
    assert not e[~ref["counts"]].any() and (e[ref["outside"]].sum(1) > 0).all()
    if dim == 2 and "z_dir" not in fields:
        with pytest.raises(ValueError):
            optimizer.SpotError(("z_dir",), group, domain[:1])(eng)
    if len(codes) == 2:
        # the chain rule has summed both fields into the rows: unlike weights are refused
        with pytest.raises(ValueError):
            (erf(eng) * torch.tensor([1.0, 2.0])).sum().backward()


def test_entries_refuse_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    L = _lib.lib()
    dummy = ctypes.create_string_buffer(1 << 17)
    p = ctypes.cast(dummy, ctypes.c_void_p)

    def density(dim=3, fx=7, fy=8, ny=4, n=8, stride=8):
        return L.tfrt_density_error_fields(p, stride, n, 1, dim, None, fx, fy, p, 4, ny, 0.0, 1.0,
                                           4.0, 0.0, 1.0, 4.0, 0.0, p, 8, p, p, 0, p, 1 << 17, None)

    def spot(dim=3, fx=7, fy=8, n=8, stride=8, G=4):
        return L.tfrt_spot_error_fields(p, stride, n, 1, dim, None, fx, fy, p, 8, None, G, 0.0, 1.0,
                                        4.0, 0.0, 1.0, 4.0, 40, 0.0, p, 8, p, p, 0, p, 1 << 17,
                                        None)
    for call in (density, spot):
        for bad in (dict(dim=1), dict(dim=4), dict(fx=9), dict(fy=9), dict(dim=2, fx=6),
                    dict(dim=2, fy=6), dict(fx=7, fy=7), dict(fx=-1), dict(fy=-2), dict(n=-1),
                    dict(stride=4)):
            assert call(**bad) == -1, (call.__name__, bad)
    assert density(fy=-1, ny=4) == -1             # one field wants ny == 1, as today
    assert spot(G=0) == -1
