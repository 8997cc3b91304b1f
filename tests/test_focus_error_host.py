"""
FocusError without a GPU: the numpy restatement of the definition
(tests/focus_error_reference.py) against torch autograd of the full objective (the foci
differentiated through), the backward error of its solve, the CPU path of ``ops.focus_error``
against it -- records equal as integers, foci and gradients bit for bit, the error within
``error_bound`` --, the class (constructor, ``foci()``, the generic path on the CPU backend, a
term of a ``SumError``), the C entry's refusals, and csrc/focus_math.h on the host:
tests/focus_host/focus_main.cpp (its own main) compiled with g++ and the address and
undefined-behaviour sanitizers.
"""
import os
import struct
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import focus_error_reference as fr
from tensorflowraytrace_amd import ops, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "focus_host", "focus_main.cpp")

# census(n, 7) of the generator, float64, 3-D, no mask, no perm (2-D: the same counts): what
# every test that uses ``rays`` relies on, recorded so that a change of the generator shows.
CENSUS = {
    64: dict(counting=55, with_term=49, degenerate=3, non_finite=2, outside=2, parallel=5,
             single=1, empty=0, foci=4),
    65: dict(counting=56, with_term=50, degenerate=3, non_finite=2, outside=2, parallel=5,
             single=1, empty=0, foci=4),
    1000: dict(counting=871, with_term=776, degenerate=56, non_finite=43, outside=28, parallel=94,
               single=1, empty=0, foci=4),
    20000: dict(counting=17423, with_term=15488, degenerate=1125, non_finite=869, outside=581,
                parallel=1934, single=1, empty=0, foci=4),
}


@pytest.mark.parametrize("n", sorted(CENSUS))
def test_the_generator_keeps_its_guard(n):
    for dim in (2, 3):
        for dtype in (np.float64, np.float32):
            for masked, permuted in ((False, False), (True, True)):
                c = fr.assert_generator(n, 7, fr.census(n, 7, dtype, dim, permuted, masked))
                if dtype == np.float64 and not masked:
                    print(n, dim, c)
                    assert {k: c[k] for k in CENSUS[n]} == CENSUS[n]
    # the group counts at which the kernels change their path keep the first two conditions
    for G in (3, ops.FOCUS_LDS_GROUPS, ops.FOCUS_LDS_GROUPS + 1):
        fr.assert_generator(n, G, fr.census(n, G, masked=True, permuted=True))


def _torch_objective(block, label, n_groups, has_focus):
    """The full objective in torch float64: per group A = sum P, b = sum P e in the scene's own
    coordinates, X = solve(A, b) -- differentiated through --, the sum over the group's rays of
    |P (e - X)|^2.  ``label``: the group of every column that counts, -1 otherwise."""
    d = block.shape[0] // 2
    v = block[d:] - block[:d]
    u = v / torch.sqrt((v * v).sum(dim=0))
    eye = torch.eye(d, dtype=torch.float64)
    total = torch.zeros((), dtype=torch.float64)
    for k in range(n_groups):
        if not has_focus[k]:
            continue
        at = torch.nonzero(torch.as_tensor(label == k))[:, 0]
        uk, ek = u[:, at], block[d:, at]
        P = eye[:, :, None] - uk[:, None, :] * uk[None, :, :]            # (d, d, n_k)
        A = P.sum(dim=2)
        b = torch.einsum("abi,bi->a", P, ek)
        X = torch.linalg.solve(A, b)
        r = torch.einsum("abi,bi->ai", P, ek - X[:, None])
        total = total + (r * r).sum()
    return total


def _autograd_difference(n, G, dim):
    """(largest |reference gradient - autograd gradient| / largest |autograd gradient|, relative
    difference of the errors) on the generator's columns."""
    block, _, group, _ = fr.rays(n, G, np.float64, dim)
    ref = fr.focus_error(block, group, G, fr.DOMAIN)
    label = np.where(ref["counts"], ref["label"], -1)
    # (a column that does not count may hold a NaN: it is no part of the torch objective)
    clean = np.where(ref["counts"][None, :], block, 0.0)
    clean[dim:, ~ref["counts"]] = 1.0
    t = torch.tensor(clean, requires_grad=True)
    e = _torch_objective(t, label, G, ref["has_focus"])
    g, = torch.autograd.grad(e, t)
    g = g.numpy()
    assert ref["has"].sum() > n / 2 and not ref["grad"][:, ~ref["has"]].any()
    assert not g[:, ~ref["has"]].any()
    return (float(np.abs(ref["grad"] - g).max() / np.abs(g).max()),
            abs(ref["error"] - float(e.detach())) / float(e.detach()))


@pytest.mark.parametrize("dim", [2, 3])
def test_reference_gradient_equals_autograd_of_the_full_objective(dim):
    """The reference's gradient needs no derivative of the focus (the envelope argument) and works
    on quantised records; torch differentiates through ``torch.linalg.solve``.  The only sources
    of a difference are the quantisation and the envelope argument: a focus is off by about
    2**-pbits of the box (pbits = 40 at 1,003 source rays, R = 1.75: 1.6e-12 scene units), and a
    gradient entry by twice that, while the largest entry is of the size of the lines' noise
    (a few 0.01).  Measured on the CPU at n = 1000, G = 7: the largest difference of a gradient
    entry, relative to the largest entry, was 1.08e-11 in 2-D and 1.01e-11 in 3-D (the errors
    agreed to 6e-16); asserted is 10 x the larger, 1.1e-10."""
    rel, rel_e = _autograd_difference(1000, 7, dim)
    print(f"{dim}-D: gradient rel diff {rel:.3e}, error rel diff {rel_e:.3e}")
    assert rel <= 1.1e-10 and rel_e <= 1.1e-10


def _solve_backward_error(n, G, dtype, dim):
    """max over the groups with a focus of max_a |A x - b|_a / (|A| |x| + |b|)_a, in eps, of the
    reference's solve on the generator's records (A and b as the solve takes them)."""
    block, _, group, _ = fr.rays(n, G, dtype, dim)
    ref = fr.focus_error(block, group, G, fr.DOMAIN)
    inv = np.ldexp(1.0, -ref["pbits"])
    worst = 0.0
    for k in np.nonzero(ref["has_focus"])[0]:
        rec = ref["acc"][k]
        a = (rec[1:].astype(np.float64) * inv) / float(rec[0])
        A = np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])[:dim, :dim]
        b, x = a[6:6 + dim], ref["table"][k, :dim]
        # (the residual in exact rational arithmetic: in float64 it would carry a rounding of its
        # own, of the size of what is measured)
        res = [abs(sum(F(A[i, j]) * F(x[j]) for j in range(dim)) - F(b[i])) for i in range(dim)]
        den = [sum(abs(F(A[i, j]) * F(x[j])) for j in range(dim)) + abs(F(b[i]))
               for i in range(dim)]
        worst = max(worst, max(float(r / q) for r, q in zip(res, den)) / fr.EPS)
    return worst


def test_the_solve_is_backward_stable_on_the_generators_groups():
    """The cofactor solve on well-conditioned groups (det > 1e-3): the componentwise backward
    error, residuals in exact rational arithmetic, stays within 4 x the largest value measured
    (focus_error_reference.SOLVE_BACKWARD_EPS, where the figure is recorded)."""
    worst = 0.0
    for n in (64, 65, 1000, 20000):
        for dim in (2, 3):
            for dtype in (np.float64, np.float32):
                b = _solve_backward_error(n, 7, dtype, dim)
                print(f"n {n} {dim}-D {np.dtype(dtype).name}: {b:.3f} eps")
                worst = max(worst, b)
    assert 0.0 < worst <= 4 * fr.SOLVE_BACKWARD_EPS


def _evaluate(block, mask, group, perm, G, dim, pad=0, **kw):
    """ops.focus_error on the CPU over the block with ``pad`` spare columns."""
    n = block.shape[1]
    wide = torch.full((2 * dim, n + pad), 7.0, dtype=torch.as_tensor(block).dtype)
    wide[:, :n] = torch.as_tensor(block)
    return ops.focus_error(wide[:, :n], torch.as_tensor(group), G,
                           ops.focus_grid(fr.DOMAIN[:dim]), fr.MIN_DET,
                           mask=None if mask is None else torch.as_tensor(mask),
                           perm=None if perm is None else torch.as_tensor(perm), dimension=dim,
                           **kw)


def _check(out, ref):
    err, grad, acc, foci = out
    assert acc.dtype == torch.int64 and np.array_equal(acc.numpy(), ref["acc"])
    assert np.array_equal(foci.numpy(), ref["table"], equal_nan=True)
    assert np.array_equal(np.isnan(foci.numpy()), np.isnan(ref["table"]))
    assert grad.numpy().tobytes() == ref["grad"].tobytes() \
        or np.array_equal(grad.numpy(), ref["grad"])
    assert float(err[1]) == ref["terms"]
    assert abs(float(err[0]) - ref["error"]) <= fr.error_bound(ref)
    if ref["terms"] == 0:
        assert float(err[0]) == 0.0 and np.isnan(float(err[2])) and not grad.any()
    else:
        assert abs(float(err[2]) - ref["mean"]) <= fr.error_bound(ref) / ref["terms"]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("masked,permuted", [(False, False), (True, True), (True, False),
                                             (False, True)])
@pytest.mark.parametrize("n,G", [(0, 3), (1, 3), (63, 3), (64, 7), (65, 7), (1000, 7),
                                 (1000, 257), (20000, 256)])
def test_cpu_path_equals_the_reference(n, G, masked, permuted, dim):
    for dtype in (np.float64, np.float32):
        for in_range in (False, True):
            block, mask, group, perm = fr.rays(n, G, dtype, dim, permuted)
            if in_range:                # without the labels -1 and G
                group = np.clip(group, 0, G - 1)
            mask, perm = (mask if masked else None), (perm if permuted else None)
            ref = fr.focus_error(block, group, G, fr.DOMAIN, mask=mask, perm=perm)
            _check(_evaluate(block, mask, group, perm, G, dim, pad=3), ref)
            if n >= 64 and G == 7:
                par, single, empty = fr.specials(G)
                assert not ref["has_focus"][[par, single, empty]].any()
                assert ref["has_focus"][:par].all()
                assert np.isnan(ref["foci"][par:]).all()


def test_the_foci_are_the_points_the_lines_were_made_for():
    """20,000 lines through 4 points with noise 0.01: the solved foci lie within 0.01 of the
    points the lines of a group pass through in the mean, and the quantisation moves the foci and
    the gradient by a relative 2**-pbits only (the plain float64 form against the records)."""
    n, G = 20000, 7
    block, _, group, _ = fr.rays(n, G)
    ref = fr.focus_error(block, group, G, fr.DOMAIN)
    plain = fr.focus_error(block, group, G, fr.DOMAIN, quantise=False)
    assert np.array_equal(ref["has_focus"], plain["has_focus"])
    scale = 2.0 ** -ref["pbits"]
    assert np.nanmax(np.abs(ref["table"][:, :3] - plain["table"][:, :3])) <= 64 * scale
    assert np.abs(ref["grad"] - plain["grad"]).max() <= 64 * scale * np.abs(plain["grad"]).max()
    # the mean term is the noise's: two (3-D) perpendicular components of variance 1e-4 each
    assert 0.5 * 2e-4 < ref["mean"] < 2 * 2e-4
    # reused buffers, another stride: the same bits
    out = _evaluate(block, None, group, None, G, 3)
    again = _evaluate(block, None, group, None, G, 3, pad=5, grad=torch.full((6, n), np.nan,
                      dtype=torch.float64), acc=out[2].clone().fill_(5), foci=out[3].clone())
    for a, b in zip(out, again):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_ops_argument_errors():
    rows = torch.zeros((6, 5), dtype=torch.float64)
    g = torch.zeros(5, dtype=torch.int32)
    grid = ops.focus_grid(fr.DOMAIN)
    assert len(grid) == 11 and grid[6:9] == (5.75, 0.5 * (-1.2 + 1.3), 0.25) \
        and grid[9:] == (1.75, 1.0 / 1.75)
    assert ops.focus_grid(fr.DOMAIN[:2])[4:6] == (0.0, 0.0)
    assert ops.focus_pbits(1000) == 40 and ops.focus_pbits(1 << 20) == 39 \
        and ops.focus_pbits((1 << 31) - 1) == 29
    assert ops.FOCUS_LDS_GROUPS == 256
    for bad in (fr.DOMAIN[:1], ((0.0, 1.0), (1.0, 1.0)), ((0.0, 1.0), (0.0, float("inf"))), 3.0):
        with pytest.raises(ValueError, match="domain"):
            ops.focus_grid(bad)
    ok = dict(rows=rows, groups=g, n_groups=3, grid=grid, min_det=1e-6)
    for bad, match in ((dict(groups=g.long()), "groups"), (dict(n_groups=0), "n_groups"),
                       (dict(n_groups=2 ** 20 + 1), "n_groups"), (dict(rows=rows[:4]), "rows"),
                       (dict(dimension=4), "rows"), (dict(grid=grid[:6]), "grid"),
                       (dict(min_det=0.0), "min_det"), (dict(min_det=float("nan")), "min_det"),
                       (dict(variant=3), "variant"), (dict(n_groups=257, variant=1), "variant"),
                       (dict(mask=torch.zeros(5)), "mask"),
                       (dict(perm=torch.zeros(4, dtype=torch.int32)), "perm"),
                       (dict(grad=torch.zeros((4, 5), dtype=torch.float64)), "grad"),
                       (dict(acc=torch.zeros((3, 4), dtype=torch.int64)), "acc"),
                       (dict(foci=torch.zeros((3, 3), dtype=torch.float64)), "foci")):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.focus_error(**kw)


def test_the_class_checks_its_arguments_and_reports_foci():
    import tfrt.optimizer
    from tensorflowraytrace_amd import errors, fused_step
    F = optimizer.FocusError                 # noqa: F811
    assert tfrt.optimizer.FocusError is F and fused_step.FocusError is F and F in errors._COUPLED
    lab = np.arange(12) % 4
    erf = F(lab, fr.DOMAIN)
    assert erf.n_groups == 4 and erf.labels.dtype == torch.int32 and erf.min_det == 1e-12
    assert erf.rows == [0, 1, 2, 3, 4, 5] and erf.seed_rows == 0x3f and erf.on_columns
    assert erf.rows_for(3) == erf.rows
    flat = F(torch.tensor(lab), fr.DOMAIN[:2], n_groups=9, min_det=1e-6)
    assert flat.n_groups == 9 and flat.rows_for(2) == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="2-D engine"):
        erf.rows_for(2)
    with pytest.raises(ValueError, match="3-D engine"):
        flat.rows_for(3)
    for bad in (dict(domain=fr.DOMAIN[:1]), dict(domain=((1.0, 1.0),) * 3),
                dict(domain=((0.0, float("inf")),) * 3), dict(domain=None), dict(min_det=0.0),
                dict(min_det=-1.0), dict(min_det=float("nan")), dict(min_det="small"),
                dict(groups=np.zeros((3, 2), dtype=np.int64)), dict(groups=np.zeros(3)),
                dict(groups=lambda src: lab), dict(groups=np.zeros(0, dtype=np.int64)),
                dict(n_groups=0), dict(n_groups=2 ** 20 + 1), dict(n_groups="many")):
        kw = dict(groups=lab, domain=fr.DOMAIN)
        kw.update(bad)
        with pytest.raises(ValueError, match="FocusError"):
            F(**kw)
    with pytest.raises(TypeError):
        F(lab, fr.DOMAIN, weights=np.ones(12))           # (no weights: not this class's keyword)
    with pytest.raises(TypeError):
        F(("y_end", "z_end"), lab, fr.DOMAIN, fields=("y_end",))
    assert F(lambda src: lab, fr.DOMAIN, n_groups=4).labels is None
    with pytest.raises(RuntimeError, match="no evaluation"):
        erf.foci()
    # graph_key: the label buffer, G, the constants
    k0 = erf.graph_key()
    erf.labels.add_(0)
    assert erf.graph_key() == k0
    erf.labels = erf.labels.clone()
    assert erf.graph_key() != k0 and F(lab, fr.DOMAIN, min_det=1e-6).graph_key()[3] == 1e-6
    # a legal term of a SumError, not of the fused 2-D step
    goal = optimizer.GoalError(("y_end", "z_end"), torch.zeros((12, 2)))
    both = optimizer.SumError([erf, goal], reduce="mean")
    assert both.terms == (erf, goal) and both.rows == [0, 1, 2, 3, 4, 5, 4, 5]
    with pytest.raises(ValueError, match="FocusError"):
        optimizer.SumError([erf, object()])

    class _Eng:
        dimension, ray_shard = 2, None

        @staticmethod
        def _custom_ops():
            return False

    class _Opt:
        engine, error_function = _Eng(), flat
    assert fused_step.FusedStep.eligible2d(_Opt()) is False


class _Engine:
    def __init__(self, block, ids, n_source, dim):
        names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end") if dim == 3 \
            else ("x_start", "y_start", "x_end", "y_end")
        self.dimension = dim
        self.leaves = [torch.tensor(r, requires_grad=True) for r in block]
        self.finished_rays = dict(zip(names, self.leaves))
        self.last_trace = {"finished_id": torch.tensor(ids)}
        self._trace_src = {"x_start": torch.zeros(n_source)}


@pytest.mark.parametrize("dim", [2, 3])
def test_the_generic_path_returns_the_terms_and_the_gradient_rows(dim):
    """FocusError.__call__ on CPU tensors: (n, 1) terms whose sum is the reference's error and,
    through backward, the reference's gradient on all 2 d geometry fields; the labels come through
    the finished rays' source-ray indices; ``foci()`` are the reference's."""
    n, G = 300, 7
    block, _, group, perm = fr.rays(n, G, np.float64, dim, permuted=True)
    erf = optimizer.FocusError(group, fr.DOMAIN[:dim], n_groups=G, min_det=fr.MIN_DET)
    erf.labels = erf.labels.cpu()
    eng = _Engine(block, perm, n + 3, dim)
    e = erf(eng)
    assert e.shape == (n, 1) and e.dtype == torch.float64
    ref = fr.focus_error(block, group, G, fr.DOMAIN, perm=perm)
    (3.0 * e.sum()).backward()
    assert abs(float(e.detach().sum()) - ref["error"]) <= fr.error_bound(ref)
    assert np.array_equal(e.detach().numpy()[:, 0], ref["term"])
    assert tuple(erf.last_acc.shape) == (G, 10) and erf.last_acc.dtype == torch.int64
    assert np.array_equal(erf.last_acc.numpy(), ref["acc"])
    for leaf, want in zip(eng.leaves, ref["grad"]):
        assert np.array_equal(leaf.grad.numpy(), 3.0 * want)
    f = erf.foci().numpy()
    assert f.shape == (G, dim) and np.array_equal(f, ref["foci"], equal_nan=True)
    assert np.isnan(f[fr.specials(G)[0]:]).all() and np.isfinite(f[:fr.specials(G)[0]]).all()
    eng.finished_rays = {}
    assert erf(eng).shape == (0, 1)
    with pytest.raises(ValueError, match="labels"):
        eng2 = _Engine(block, perm, n, dim)
        erf(eng2)
    with pytest.raises(ValueError, match="engine"):
        eng3 = _Engine(block, perm, n + 3, dim)
        eng3.dimension = 5 - dim
        erf(eng3)


def _lens(n_rays):
    from test_host_logic import _lens_api
    eng, system, lens, target = _lens_api(n_rays)
    groups = np.arange(n_rays) % 5
    box = ((9.0, 11.0), (-5.0, 5.0), (-5.0, 5.0))           # the target plane is x = 10
    return eng, lens, groups, box


def test_the_optimiser_takes_the_generic_path_on_the_cpu_backend(cpu_backend):
    """SGD_Optimizer with a FocusError on the oracle-backed CPU stand-ins: the step's error is
    the reference's on the traced rays, the parameter gradient is that of the torch objective
    under autograd through the same trace, and a few steps lower the error."""
    eng, lens, groups, box = _lens(200)
    erf = optimizer.FocusError(groups, box, min_det=fr.MIN_DET)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=2e-3, grad_clip=1e9)
    grads, err_sum, n_terms = opt.raw_gradient()
    assert opt._fused_step is None
    fin = eng.finished_rays
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
    block = np.stack([fin[k].detach().numpy() for k in names])
    ids = eng.last_trace["finished_id"].numpy()
    ref = fr.focus_error(block, groups, 5, box, perm=ids)
    assert ref["terms"] == n_terms > 150 and ref["has_focus"].all()
    assert abs(float(err_sum) - ref["error"]) <= fr.error_bound(ref)
    assert np.array_equal(erf.foci().numpy(), ref["foci"])
    # the same trace again, under autograd with the torch objective (the foci differentiated
    # through)
    eng.clear_ray_history()
    eng.optical_system.update()
    eng.ray_trace(3)
    fin = eng.finished_rays
    assert np.array_equal(eng.last_trace["finished_id"].numpy(), ids)
    t = torch.stack([fin[k] for k in names]).double()
    e = _torch_objective(t, np.where(ref["counts"], ref["label"], -1), 5, ref["has_focus"])
    want = torch.autograd.grad(e, lens.parameters)
    for g, w in zip(grads, want):
        assert float((g - w).abs().max()) <= 1e-9 * float(w.abs().max())
    errs = [float(opt.single_step(None)) for _ in range(6)]
    print("errors:", errs)
    assert errs[-1] < errs[0]


def test_a_sum_with_a_goal_runs_on_the_cpu_backend(cpu_backend):
    eng, lens, groups, box = _lens(200)
    focus = optimizer.FocusError(groups, box, min_det=fr.MIN_DET)
    goal = optimizer.GoalError(("y_end", "z_end"), lambda src: -src["object_coords"][:, 1:])
    both = optimizer.SumError([focus, goal], weights=[1.0, 0.25], reduce="mean")
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, both, 3, learning_rate=1e-3, grad_clip=1e9)
    e = float(opt.single_step(None))
    triples = both.last_errors.numpy()
    assert triples.shape == (2, 3) and triples[0, 1] > 150 and triples[1, 1] == 2 * triples[0, 1]
    assert abs(e - (triples[0, 2] + 0.25 * triples[1, 2])) <= 1e-12 * abs(e)
    assert focus.foci().shape == (5, 3)


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    L = _lib.lib()
    assert L.tfrt_focus_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_focus_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_focus_error_workspace_bytes(-1, 4) == 0
    small = L.tfrt_focus_error_workspace_bytes(0, 4)
    assert 0 < small <= L.tfrt_focus_error_workspace_bytes(1_000_000, 2 ** 20)
    dummy = ctypes.create_string_buffer(1 << 17)
    p = ctypes.cast(dummy, ctypes.c_void_p)

    def call(n=8, G=4, dim=3, x1=1.0, y1=1.0, z1=1.0, ws=1 << 17, stride=8, gstride=8, variant=0,
             group=p, dtype=1, pbits=40, n_source=8, acc=p, foci=p, err=p, min_det=1e-6):
        return L.tfrt_focus_error(p, stride, n, dtype, dim, None, group, n_source, None, G,
                                  0.0, x1, 0.0, y1, 0.0, z1, pbits, min_det, p, gstride, err, acc,
                                  foci, variant, p, ws, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(dim=1), dict(dim=4),
                dict(x1=0.0), dict(y1=float("nan")), dict(z1=float("inf")), dict(z1=-1.0),
                dict(stride=4), dict(gstride=4), dict(variant=3), dict(group=None),
                dict(n=1 << 31), dict(dtype=7), dict(G=257, variant=1), dict(pbits=41),
                dict(pbits=0), dict(n=1 << 21, pbits=40, stride=1 << 21, gstride=1 << 21),
                dict(n_source=-1), dict(acc=None), dict(foci=None), dict(err=None),
                dict(min_det=0.0), dict(min_det=float("nan"))):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    # (z1 is not looked at in 2-D)
    assert call(dim=2, z1=-1.0, ws=8) == -2


def _pack(n, dim, G, pbits, box, min_det, e, u, L, counts, label):
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).tobytes()       # noqa: E731
    lo, hi, c, R, iR = box
    pad = lambda v: list(v) + [0.0] * (3 - len(v))                         # noqa: E731
    return (struct.pack("<4q", n, dim, G, pbits) + f8(pad(lo) + pad(hi) + pad(c) + [R, iR, min_det])
            + f8(e) + f8(u) + f8(L) + i4(counts) + i4(label))


def test_focus_math_on_the_host_under_the_sanitizers(tmp_path):
    """The box test, the normalised end points, every ray's ten integer slots, the groups'
    records, the solved table, the determinants and every ray's term and gradient of
    focus_math.h equal the reference's bit for bit, in both dimensions, from float32 and float64
    rows; the program's vectors are exact-size allocations and it runs under the address and
    undefined-behaviour sanitizers."""
    exe = tmp_path / "focus_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    for n, G, dim, dtype in ((257, 7, 3, np.float64), (1000, 7, 2, np.float32),
                             (64, 3, 3, np.float32), (300, 257, 2, np.float64),
                             (1, 3, 3, np.float64), (0, 3, 2, np.float64)):
        block, mask, group, perm = fr.rays(n, G, dtype, dim, permuted=True)
        ref = fr.focus_error(block, group, G, fr.DOMAIN, mask=mask, perm=perm)
        e = block[dim:].astype(np.float64)
        lo, hi, *_ = box = fr.box_of(fr.DOMAIN[:dim])
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(_pack(n, dim, G, ref["pbits"], box, fr.MIN_DET, e, ref["u"], ref["L"],
                              ref["counts"], np.clip(ref["label"], 0, G - 1)))
        run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert run.returncode == 0, f"{n} {G} {dim}: {run.stdout}{run.stderr}"
        raw = dst.read_bytes()
        at = 0

        def take(count, dt):
            nonlocal at
            out = np.frombuffer(raw[at:at + count * np.dtype(dt).itemsize], dtype=dt)
            at += count * np.dtype(dt).itemsize
            return out
        inside = take(n, np.int32)
        m = take(dim * n, np.float64).reshape(dim, n)
        q = take(10 * n, np.int64).reshape(n, 10)
        acc = take(10 * G, np.int64).reshape(G, 10)
        table = take(4 * G, np.float64).reshape(G, 4)
        det = take(G, np.float64)
        term = take(n, np.float64)
        gs = take(dim * n, np.float64).reshape(dim, n)
        ge = take(dim * n, np.float64).reshape(dim, n)
        assert at == len(raw)
        with np.errstate(invalid="ignore"):
            want = ((e >= lo[:, None]) & (e <= hi[:, None])).all(axis=0)
        assert np.array_equal(inside != 0, want)
        c = ref["counts"]
        assert np.array_equal(m[:, c], ref["m"][:, c]) and not m[:, ~c].any()
        assert np.array_equal(q.sum(axis=0), ref["acc"].sum(axis=0)) and not q[~c].any()
        assert np.array_equal(acc, ref["acc"])
        assert np.array_equal(table, ref["table"], equal_nan=True)
        assert np.array_equal(det, ref["det"], equal_nan=True)
        assert np.array_equal(term, ref["term"])
        assert np.array_equal(np.concatenate([gs, ge]), ref["grad"])
