"""
SumError on the GPU: tfrt_goal_error_columns and tfrt_error_combine against the numpy reference of
tests/error_combine_reference.py -- bit for bit, except the goal sum, which is checked at the bound
of a float64 sum of non-negative terms --, and the sum of terms on the optimiser's paths: the
fused, replayed 3-D step against the generic one, one term with weight 1 against the term alone,
``set_weights`` between replays, the parameter gradient against the oracle, the fallbacks, 2-D,
the two examples.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import density_error_reference as dr
import error_combine_reference as ref
from test_density_error_host import _torch_objective
from test_error_combine_host import combine_case, goal_case
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 2, 63, 64, 65, 127, 1023, 1025, 4097)
# (stride beyond n, first element of the block in a float64 buffer): an even stride at a 16-byte
# aligned address takes two columns per lane; an odd stride, or a block that starts 8 bytes off,
# takes the scalar path
LAYOUTS = {"even": (2, 0), "odd": (1, 0), "offset8": (2, 1)}
MASKS8 = (0x3f, 0x30, 0x03, 0x11, 0x20, 0x3f, 0x0c, 0x30)


def _block(values, pad, first, fill=7.0):
    """``values`` (rows, n) on the device as the leading columns of a (rows, stride) block that
    starts ``first`` elements into its buffer; stride = n + pad rounded so that its parity is
    pad's.  Returns (the (rows, n) view, the buffer)."""
    rows, n = values.shape
    stride = n + pad + ((n + pad) % 2 != pad % 2)
    t = torch.as_tensor(values)
    buf = torch.full((rows * stride + first + 2,), fill, dtype=t.dtype, device=DEV)
    view = buf[first:first + rows * stride].view(rows, stride)[:, :n]
    view.copy_(t.to(DEV))
    return view, buf


@functools.lru_cache(maxsize=None)
def _goal_reference(n, n_rows, fields, mask_kind, perm_kind, np_dtype, by_ray):
    rows, goal, mask, perm = goal_case(n, n_rows, fields, mask_kind, perm_kind, n + 1, np_dtype)
    table = np.ascontiguousarray(goal.T) if by_ray else goal
    return rows, table, mask, perm, ref.goal_error_columns(rows, fields, table, mask, perm, by_ray)


def _goal_kernel(n, n_rows, fields, mask_kind, perm_kind, np_dtype, by_ray, layout):
    from tensorflowraytrace_amd import ops
    rows, table, mask, perm, want = _goal_reference(n, n_rows, fields, mask_kind, perm_kind,
                                                    np_dtype, by_ray)
    pad, first = LAYOUTS[layout]
    block, _ = _block(rows, pad, first)
    grad, gbuf = _block(np.full((n_rows, n), np.nan), pad, first, fill=np.nan)
    err, g = ops.goal_error_columns(
        block, fields, torch.as_tensor(table).to(DEV),
        mask=None if mask is None else torch.as_tensor(mask).to(DEV),
        perm=None if perm is None else torch.as_tensor(perm).to(DEV), by_ray=by_ray, grad=grad)
    torch.cuda.synchronize()
    return err.cpu().numpy(), g.cpu().numpy(), gbuf.cpu().numpy(), want


def _check_goal(got, fields, n_rows):
    err, grad, gbuf, want = got
    for r in range(n_rows):
        if r in fields:
            assert np.array_equal(ref.bits(grad[r]), ref.bits(want["grad"][r]))
        else:
            assert np.isnan(grad[r]).all()           # rows it does not own are never written
    n = grad.shape[1]
    assert np.isnan(gbuf).sum() == gbuf.size - len(fields) * n      # nothing beyond the columns
    total, terms, mean = want["error"]
    bound = ref.sum_bound(want["terms_each"])
    print(f"n {n}: sum {err[0]!r} reference {total!r} bound {bound:.3e}")
    assert err[1] == terms
    assert abs(err[0] - total) <= bound
    if terms == 0:
        assert err[0] == 0.0 and np.isnan(err[2])
    else:
        assert abs(err[2] - mean) <= bound / terms + abs(mean) * ref.EPS


@pytest.mark.parametrize("np_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_rows,fields", [(4, (3,)), (6, (4, 5)), (6, (5, 0, 3))])
def test_goal_columns_kernel_equals_the_reference(n_rows, fields, np_dtype):
    cases = [("none", "none", False, "even"), ("partial", "permutation", True, "odd"),
             ("partial", "out_of_range", False, "offset8"), ("all_negative", "none", True, "even")]
    for n in COUNTS:
        for mask_kind, perm_kind, by_ray, layout in cases:
            _check_goal(_goal_kernel(n, n_rows, fields, mask_kind, perm_kind, np_dtype, by_ray,
                                     layout), fields, n_rows)


def test_goal_columns_kernel_float16_state():
    _check_goal(_goal_kernel(1025, 6, (4, 5), "partial", "out_of_range", np.float16, False, "odd"),
                (4, 5), 6)


def _combine_kernel(K, n, n_rows, reduce, layout, with_grad=True):
    from tensorflowraytrace_amd import ops
    masks = tuple(m & ((1 << n_rows) - 1) for m in MASKS8[:K])
    terms, weights = combine_case(K, n, n_rows, masks, seed=K * 100 + n,
                                  zero_terms=(K - 1,) if K > 1 else ())
    if K > 2:
        weights[1] = 0.0
    want = ref.error_combine([(g if with_grad else None, m, e) for g, m, e in terms], weights,
                             reduce, n, n_rows)
    pad, first = LAYOUTS[layout]
    tt = [(_block(g, pad, first)[0] if with_grad else None, m, torch.as_tensor(e).to(DEV))
          for g, m, e in terms]
    out, obuf = _block(np.full((n_rows, n), np.nan), pad, first, fill=np.nan)
    err, grad, coeff = ops.error_combine(tt, torch.as_tensor(weights).to(DEV), reduce, n=n,
                                         n_rows=n_rows, out=out if with_grad and n else None)
    torch.cuda.synchronize()
    return (err.cpu().numpy(), None if grad is None else grad.cpu().numpy(), coeff.cpu().numpy(),
            obuf.cpu().numpy(), want)


def _check_combine(got, n, n_rows):
    err, grad, coeff, obuf, want = got
    assert np.array_equal(ref.bits(coeff), ref.bits(want["coeff"]))
    assert np.array_equal(ref.bits(err), ref.bits(np.array(want["error"])))
    if want["grad"] is None:
        assert grad is None and np.isnan(obuf).all()
    else:
        assert np.array_equal(ref.bits(grad), ref.bits(want["grad"]))
        assert np.isnan(obuf).sum() == obuf.size - n_rows * n       # nothing beyond the columns


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("n_rows", [4, 6])
def test_combine_kernel_equals_the_reference(n_rows, K, layout):
    """Every count on the 16-byte path (even strides, aligned blocks) and on the scalar one (odd
    strides; blocks that start 8 bytes off), sum and mean, a term without terms and a weight of
    0: bit for bit."""
    for n in COUNTS:
        for reduce in ("sum", "mean"):
            _check_combine(_combine_kernel(K, n, n_rows, reduce, layout), n, n_rows)
    _check_combine(_combine_kernel(K, 1025, n_rows, "mean", layout, with_grad=False), 1025, n_rows)


def test_combine_of_one_term_with_weight_one_returns_its_own_bits():
    from tensorflowraytrace_amd import ops
    n = 4097
    for layout in LAYOUTS:
        g = np.random.default_rng(4).standard_normal((6, n))
        g[2, :5] = [-0.0, 0.0, np.inf, -np.inf, 5e-324]
        block, _ = _block(g, *LAYOUTS[layout])
        e = torch.tensor([3.25, 17.0, 3.25 / 17.0], dtype=torch.float64, device=DEV)
        err, out, coeff = ops.error_combine(
            [(block, 0b110100, e)], torch.ones(1, dtype=torch.float64, device=DEV), n_rows=6)
        out = out.cpu().numpy()
        for r in range(6):
            want = g[r] if r in (2, 4, 5) else np.zeros(n)
            assert np.array_equal(ref.bits(out[r]), ref.bits(want)), (layout, r)
        assert err.tolist() == [3.25, 1.0, 3.25] and coeff.tolist() == [1.0]


def test_two_calls_give_the_same_bits_and_reused_buffers_allocate_nothing():
    from tensorflowraytrace_amd import _lib, ops
    a = _goal_kernel(4097, 6, (4, 5), "partial", "permutation", np.float32, False, "even")
    b = _goal_kernel(4097, 6, (4, 5), "partial", "permutation", np.float32, False, "even")
    c = _combine_kernel(8, 4097, 6, "mean", "even")
    d = _combine_kernel(8, 4097, 6, "mean", "even")
    for p, q in ((a, b), (c, d)):
        for u, v in zip(p[:3], q[:3]):
            assert u.tobytes() == v.tobytes()

    n = 5000
    rows, goal, mask, perm = goal_case(n, 6, (4, 5), "partial", "permutation", 3)
    rows, goal = torch.as_tensor(rows).to(DEV), torch.as_tensor(goal).to(DEV)
    mask, perm = torch.as_tensor(mask).to(DEV), torch.as_tensor(perm).to(DEV)
    grads = [torch.zeros((6, n), dtype=torch.float64, device=DEV) for _ in range(2)]
    errs = torch.zeros((2, 3), dtype=torch.float64, device=DEV)
    out = torch.zeros((6, n), dtype=torch.float64, device=DEV)
    err = torch.zeros(3, dtype=torch.float64, device=DEV)
    coeff = torch.zeros(2, dtype=torch.float64, device=DEV)
    weights = torch.tensor([0.5, 2.0], dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.lib().tfrt_goal_error_columns_workspace_bytes(n), dtype=torch.uint8,
                     device=DEV)

    def both():
        for k in range(2):
            got = ops.goal_error_columns(rows, (4, 5), goal, mask=mask, perm=perm, grad=grads[k],
                                         err=errs[k], workspace=ws)
            assert got[1] is grads[k]
        return ops.error_combine([(grads[k], 0b110000, errs[k]) for k in range(2)], weights,
                                 "mean", out=out, err=err, coeff=coeff)
    both()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    got = both()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert got[0] is err and got[1] is out and got[2] is coeff
    assert float(err[1]) == 1.0 and float(coeff[0]) == 0.5 / float(errs[0, 1])


def test_bad_arguments():
    import ctypes
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_goal_error_columns_workspace_bytes(-1) == 0
    assert L.tfrt_goal_error_columns_workspace_bytes(1 << 31) == 0
    wsb = L.tfrt_goal_error_columns_workspace_bytes(0)
    assert 0 < wsb == L.tfrt_goal_error_columns_workspace_bytes(1_000_000)
    t = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    other = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    p, q = t.data_ptr(), other.data_ptr()

    def goal(n=8, stride=8, dtype=1, n_rows=6, fields=(4, 5), n_source=8, gstride=8, table=p,
             grad_stride=8, ws=wsb, err=p):
        codes = (ctypes.c_int32 * max(len(fields), 1))(*fields)
        return L.tfrt_goal_error_columns(p, stride, n, dtype, n_rows, None, None, n_source, codes,
                                         len(fields), table, 8, 1, q, grad_stride, err, p, ws, None)
    for bad in (dict(n=-1), dict(n=1 << 31), dict(n_rows=5), dict(stride=4), dict(grad_stride=4),
                dict(fields=(4, 6)), dict(fields=(4, -1)), dict(fields=(4, 4)), dict(fields=()),
                dict(n_rows=4, fields=(4,)), dict(n_source=-1), dict(table=None), dict(err=None),
                dict(dtype=7)):
        assert goal(**bad) == -1, bad
    assert goal(ws=8) == -2
    assert goal(n=0) == 0
    torch.cuda.synchronize()
    assert float(t[0]) == 0.0 and float(t[1]) == 0.0 and np.isnan(float(t[2]))   # err of no column

    def combine(K=2, n=8, n_rows=6, weights=p, err=p, coeff=p + 64, out=q, out_stride=8, stride=8,
                grad=p + 1024, mask=0b110000, reduce=0, grads=None, triple=p + 128):
        desc = (_lib.CombineTerm * max(K, 1))()
        for k in range(min(K, len(desc))):
            desc[k].grad = grad if grads is None else grads[k]
            desc[k].stride, desc[k].row_mask, desc[k].error = stride, mask, triple
        return L.tfrt_error_combine(desc, K, weights, reduce, n, n_rows, out, out_stride, err,
                                    coeff, None)
    for bad in (dict(K=0), dict(K=9), dict(n_rows=5), dict(weights=None), dict(err=None),
                dict(coeff=None), dict(stride=4), dict(out_stride=4), dict(out=p + 1024),
                dict(out=p + 1024 + 8 * 40), dict(out=None), dict(mask=1 << 6), dict(reduce=2),
                dict(n=-1), dict(triple=None), dict(grads=(p + 1024, None)),
                dict(stride=1 << 31)):
        assert combine(**bad) == -1, bad
    assert combine() == 0
    assert combine(n=0, out=None) == 0 and combine(grads=(None, None), out=None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28
DIRECTIONS = 4


def _gauss16(gx, gy):
    return torch.exp(-(gx ** 2 + gy ** 2) / (2 * 0.5 ** 2))


def _goal(src):
    return -src["object_coords"][:, 1:]


def _term(kind, n_rays):
    import tfrt.optimizer as optimizer
    if kind == "density":
        return optimizer.DensityError(("y_end", "z_end"), _gauss16, DOMAIN_LENS,
                                      oob_weight=2.0 / n_rays, bins=16)
    if kind == "transport":
        return optimizer.TransportError(("y_end", "z_end"), _gauss16, DOMAIN_LENS, bins=16,
                                        directions=DIRECTIONS, knots=256)
    if kind == "spot":
        return optimizer.SpotError(("y_end", "z_end"), torch.arange(n_rays) % 37, DOMAIN_LENS,
                                   oob_weight=2.0 / n_rays)
    return optimizer.GoalError(("y_end", "z_end"), _goal)


# kinds, weights, reduce, learning rate: each term steps as it does alone in its own tests
# (density 0.05; transport 2 / (n K), spot 0.2 / n per summed term)
def _transport_density(n_rays):
    return ("transport", "density"), (40.0 / (n_rays * DIRECTIONS), 1.0), "sum", 0.05


def _spot_goal(n_rays):
    return ("spot", "goal"), (1.0, 1.0), "mean", 0.4


def _make(n_rays, mode, combination, ray_dtype=torch.float64, weights=None, **engine_kw):
    """The lens of tests/test_gpu_density.py's ``_make`` with a SumError."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype, **engine_kw)
    kinds, w, reduce, lr = combination(n_rays)
    erf = optimizer.SumError([_term(kind, n_rays) for kind in kinds],
                             w if weights is None else weights, reduce)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=lr, grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source)


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


@pytest.mark.parametrize("combination", [_transport_density, _spot_goal],
                         ids=["transport+density", "spot+goal-mean"])
def test_fused_step_equals_the_generic_step(combination):
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    the single errors' tests of the same name; the step is one graph replay."""
    runs = {mode: _make(8192, mode, combination) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 6) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert runs["generic"][0]._fused_step is None
    assert fs is not None and fs.in_place and fs.capture_error is None, fs and fs.capture_error
    assert fs.graph_replays > 0
    print("errors, generic:", out["generic"][0], "graph:", out["graph"][0])
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11
    assert abs(out["generic"][0][-1] - out["generic"][0][0]) > 1e-6 * out["generic"][0][0]
    # the terms' own triples and the coefficients of the last step, on both paths
    fused, generic = (runs[m][0].error_function for m in ("graph", "generic"))
    np.testing.assert_allclose(fused.last_errors.cpu().numpy(), generic.last_errors.cpu().numpy(),
                               rtol=1e-10, atol=0)
    np.testing.assert_allclose(fused.last_coefficients.cpu().numpy(),
                               generic.last_coefficients.cpu().numpy(), rtol=1e-15, atol=0)
    e = fused.last_errors.cpu().numpy()
    c = fused.last_coefficients.cpu().numpy()
    assert abs((c * e[:, 0]).sum() - out["graph"][0][-1]) <= 1e-12 * abs(out["graph"][0][-1])
    # every term keeps what it keeps when it runs alone
    for term in fused.terms:
        for name in ("last_hq", "last_rank2", "last_acc"):
            if hasattr(term, name):
                assert getattr(term, name) is not None
    # the ray-face tests are counted once per step, not once per term
    before = int(fs.tests_total)
    float(runs["graph"][0].single_step(None))
    st = fs._state
    assert int(fs.tests_total) - before == int(st.row_passes[:st.N].sum()) * st.M > 0


@pytest.mark.parametrize("kind", ["density", "spot", "transport"])
def test_one_term_with_weight_one_is_the_term_alone(kind):
    """SumError([t], [1.0]) against t alone, on two fresh optimisers, one _enqueue_gradient each:
    the seed blocks and the error are equal bit for bit; the parameter gradients to 1e-11 (the
    in-place sweep's atomics are not ordered)."""
    import tfrt.optimizer as optimizer
    from tensorflowraytrace_amd.fused_step import FusedStep
    got = {}
    for what in ("alone", "sum"):
        eng, system, lens, target, source = _build_lens(8192, k=3)
        term = _term(kind, 8192)
        erf = term if what == "alone" else optimizer.SumError([term], [1.0])
        opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=0.05,
                                      grad_clip=1e9, graph=False, speculative=False)
        opt.suppress_warnings = True
        opt.raw_gradient()           # (a generic trace shows that this source is traced in place)
        assert FusedStep.eligible(opt, (), {})
        fs = FusedStep(opt, graph=False)
        grads, err3 = fs._enqueue_gradient()
        torch.cuda.synchronize()
        assert fs.in_place
        got[what] = (fs._state.g_fin.cpu().numpy(), err3.cpu().numpy(),
                     [g.cpu() for g in grads])
    assert bool(got["alone"][0].any())
    assert np.array_equal(ref.bits(got["sum"][0]), ref.bits(got["alone"][0]))
    assert ref.bits(got["sum"][1][:1]) == ref.bits(got["alone"][1][:1])
    assert got["sum"][1][1] == 1.0
    for a, b in zip(got["sum"][2], got["alone"][2]):
        assert float((a - b).abs().max()) <= 1e-11 * float(b.abs().max())


def test_set_weights_is_seen_by_replays_without_a_recapture():
    opt, eng, lens, _ = _make(8192, "graph", _transport_density)
    _steps(opt, lens, 6)
    fs, erf = opt._fused_step, opt.error_function
    assert fs.graph_replays > 0
    before, e_before = fs.graph_replays, float(opt.single_step(None))
    ptr = erf.weights.data_ptr()
    erf.set_weights([0.0, 3.0])
    e_after = float(opt.single_step(None))
    assert erf.weights.data_ptr() == ptr
    assert fs.graph_replays == before + 2 and abs(e_after - e_before) > 1e-3 * e_before
    assert erf.last_coefficients.tolist() == [0.0, 3.0]
    # weights (1, 0): the step's error is the first term's own
    erf.set_weights([1.0, 0.0])
    e_first = float(opt.single_step(None))
    assert fs.graph_replays == before + 3
    own = float(erf.last_errors[0, 0])
    assert abs(e_first - own) <= 1e-12 * abs(own)
    assert erf.terms[1].last_hq is not None and int(erf.terms[1].last_hq.sum()) > 0


def test_parameter_gradient_equals_the_oracle():
    """4,096 rays of float64 state, one step: d error / d parameters of SumError([DensityError,
    GoalError], (0.7, 1e-3)) on the generic path and on the fused step's fixed-shape path against
    the oracle's float64 trace composed with the torch restatements of both terms under autograd,
    at the terms' own tolerance."""
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    tol = 1e-9
    weights = (0.7, 1e-3)
    opt, eng, lens, (system, target, source) = _make(
        4096, "eager", lambda n: (("density", "goal"), weights, "sum", 0.05))
    erf = opt.error_function
    grads, err_sum, n_terms = opt.raw_gradient()
    assert n_terms == 1
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    out = tracer.ray_trace(osys, src, max_iterations=3, inherit=("wavelength", "object_coords"))
    fin = out["finished"]
    y, z = fin["y_end"], fin["z_end"]
    assert y.shape[0] > 3000 and int(((y.abs() > 1.1) | (z.abs() > 1.1)).sum()) > 50
    density = _torch_objective(y, z, erf.terms[0].goal.cpu(), DOMAIN_LENS, erf.terms[0].oob_weight)
    goal = ((torch.stack([y, z], 1) + fin["object_coords"][:, 1:]) ** 2).sum()
    e = weights[0] * density + weights[1] * goal
    rg = torch.autograd.grad(e, q)
    e = e.detach()
    assert min(float(weights[1] * goal.detach()), float(weights[0] * density.detach())) > 1e-3 * float(e)
    assert abs(float(err_sum) - float(e)) <= 10 * tol * float(e)

    def compare(got, what):
        for g, r in zip(got, rg):
            rel = float((g.cpu() - r).abs().max() / r.abs().max())
            print(f"{what}: parameter gradient rel err {rel:.2e}")
            assert rel < tol, what
    compare(grads, "generic")
    # (the generic trace above has shown that this source is traced in place)
    assert FusedStep.eligible(opt, (), {})
    fs = FusedStep(opt, graph=False)
    fused, err3 = fs._enqueue_gradient()
    torch.cuda.synchronize()
    assert fs.in_place
    compare(fused, "fused")
    assert abs(float(err3[0]) - float(e)) <= 10 * tol * float(e) and float(err3[1]) == 1.0
    assert float(erf.last_errors[1, 1]) == 2.0 * y.shape[0]


@pytest.mark.parametrize("what", ["few_rays", "deterministic"])
def test_fallbacks_take_the_generic_path(what):
    n, kw = (2000, {}) if what == "few_rays" else (8192, dict(deterministic=True))
    runs = {mode: _make(n, mode, _transport_density, **kw) for mode in ("generic", "graph")}
    out = {mode: _steps(r[0], r[2], 4) for mode, r in runs.items()}
    fs = runs["graph"][0]._fused_step
    assert fs is None or fs.steps == 0
    np.testing.assert_allclose(out["graph"][0], out["generic"][0], rtol=1e-10, atol=0)
    for a, b in zip(out["graph"][1], out["generic"][1]):
        assert float((a - b).abs().max()) <= 1e-11


def test_2d_engine_runs_on_the_generic_path_and_equals_the_reference():
    import tfrt.optimizer as optimizer
    from test_gpu_fused_2d import _segment_lens
    eng, params, _ = _segment_lens(torch.float64)
    goal = dr.goal_of(9, 1, two=False)
    eng.optical_system.update()
    eng.ray_trace(4)
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    domain = ((float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))),)    # some rays outside
    weights = (0.7, 0.25)
    erf = optimizer.SumError(
        [optimizer.DensityError(("y_end",), goal, domain, oob_weight=0.01),
         optimizer.GoalError(("y_end",), lambda src: 0.5 * src["y_start"].double())], weights)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    assert n_terms == 1
    fin = eng.finished_rays
    y = fin["y_end"].detach().cpu().double().numpy()
    want_d = dr.density_error(y, None, goal, domain, oob_weight=0.01)
    assert np.array_equal(erf.terms[0].last_hq.cpu().numpy(), want_d["Hq"])
    ids = eng.last_trace["finished_id"].cpu().numpy().astype(np.int32)
    table = erf.terms[1].table(eng._trace_src).cpu().numpy()
    want_g = ref.goal_error_columns(y[None, :].repeat(4, 0), (3,), table, perm=ids)
    assert want_g["error"][1] == y.shape[0] > 100 and want_g["error"][0] > 0
    last = erf.last_errors.cpu().numpy()
    bound_d, bound_g = dr.error_bound(want_d), ref.sum_bound(want_g["terms_each"])
    assert abs(last[0, 0] - want_d["error"]) <= bound_d and last[0, 1] == 1.0
    assert abs(last[1, 0] - want_g["error"][0]) <= bound_g and last[1, 1] == y.shape[0]
    want = ref.error_combine([(None, 0, last[0]), (None, 0, last[1])], weights)
    assert float(err_sum) == want["error"][0]
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def _example(name, *flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name), *flags,
                          "--rays", "20000", "--steps", "8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)

    def first_last(prefix):
        line = [ln for ln in out.stdout.splitlines() if ln.startswith(prefix)][-1]
        words = line[len(prefix):].replace("->", " ").split()
        return float(words[1]), float(words[3])
    return out.stdout, first_last


def test_illumination_example_with_both_objectives_lowers_the_error():
    text, first_last = _example("illumination.py", "--combined")
    first, last = first_last("combined error at full weights:")
    assert last < first
    assert "transport error (mean term): first" in text and "density error: first" in text


def test_imaging_example_with_a_magnification_lowers_the_error():
    text, first_last = _example("imaging.py", "--magnification", "1.0")
    first, last = first_last("combined error:")
    assert last < first
    first, last = first_last("mean squared image distance:")
    assert last < first
