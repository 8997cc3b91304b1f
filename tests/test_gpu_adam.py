"""
The Adam rule (``Adam_Optimizer``) on the fused, graph-replayed step: the C ABI
(tfrt_adam_multi[_finish]) bit for bit against a numpy restatement of the Keras rule, the fused
step (eager and replayed) against the generic path in 3-D and 2-D, phases replaying one graph, and
fused and generic steps sharing one state.

The rule (Keras ``Adam``, non-amsgrad), on the processed gradient ``g`` (non-finite -> 0, scale,
clip) with persistent float64 ``m``, ``v`` (zero at first) and ``{t, p1, p2}`` (``{0, 1, 1}``):

    t = t + 1;  p1 = p1 * beta1;  p2 = p2 * beta2          (running products, not pow())
    lr_t = adam_learning_rate * sqrt(1 - p2) / (1 - p1)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * (g * g)
    param -= lr_t * m / (sqrt(v) + epsilon)

every operation rounded on its own.

Fused against generic: the update itself is bit-equal on both paths (the same kernel on the same
state); what differs is the order in which float64 atomics sum the gradient, as in
test_gpu_momentum.py, whose tolerances these tests take: 1e-11 relative on the errors and 1e-12
absolute on the parameters, 1e-10 / 1e-11 in coherent order (another ray order altogether).  Adam
does not widen them: a relative change d of a gradient entry moves its update by at most
adam_learning_rate * d (1e-3 * 1e-13 here), less than SGD's own lr * g * d.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_fused_step import _goal, _params
from test_gpu_engine import _build_lens

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))


def _restate(g, p, m, v, st, scale, clip, lr, beta1, beta2, eps):
    """tfrt_adam_multi for one tensor in numpy float64, one rounding per operation.  ``st`` is
    {t, p1, p2}; returns (processed, p, m, v, st)."""
    g = np.where(np.isfinite(g), g, 0.0) * scale
    g = np.where(g < -clip, -clip, np.where(g > clip, clip, g))
    st = np.array([st[0] + 1.0, st[1] * beta1, st[2] * beta2])
    lr_t = lr * np.sqrt(1.0 - st[2]) / (1.0 - st[1])
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    p = p - lr_t * m / (np.sqrt(v) + eps)
    return g, p, m, v, st


# ------------------------------------------------------------------------------------ C ABI
_BADARG = -1     # TFRT_E_BADARG
# (256 threads per workgroup: 4097 elements are 17 of them; a tensor without elements in the middle)
_SIZES = {1: [4097], 3: [65, 0, 4097], 8: [1, 63, 64, 0, 65, 4097, 64, 63]}


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _on_dev(arrs):
    return [torch.tensor(a, dtype=torch.float64, device=DEV) for a in arrs]


def _gradient(rng, n, clip_scale):
    g = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3)
    special = rng.random(n) < 0.1
    g[special] = rng.choice([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e3 * clip_scale,
                             -1e3 * clip_scale], size=int(special.sum()))
    return g


def _rows(n_tensors):
    rows = [[1.5, 0.5, 1e-3, 0.9, 0.999, 1e-7] for _ in range(n_tensors)]
    rows[n_tensors // 2] = [0.7, 2.0, 0.02, 0.8, 0.95, 1e-5]     # one tensor with values of its own
    return rows


def _state0(n_tensors):
    return np.tile(np.array([0.0, 1.0, 1.0]), (n_tensors, 1))


def _same(t, want):
    """Equal as numbers and as bits (the sign of a zero included)."""
    got = t.cpu().numpy()
    return np.array_equal(got, want) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("n_tensors", [1, 3, 8])
def test_adam_cabi_is_bitwise_the_rule(n_tensors):
    from tensorflowraytrace_amd import _lib, ops
    L = _lib.lib()
    rng = np.random.default_rng(300 + n_tensors)
    sizes = _SIZES[n_tensors]
    rows = _rows(n_tensors)
    p = [rng.standard_normal(n) for n in sizes]
    m = [np.zeros(n) for n in sizes]
    v = [np.zeros(n) for n in sizes]
    st = _state0(n_tensors)
    p_d, m_d, v_d = _on_dev(p), _on_dev(m), _on_dev(v)
    st_d = torch.tensor(st, dtype=torch.float64, device=DEV)
    hyper = torch.tensor(rows, dtype=torch.float64, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = [torch.full((n,), 7.0, dtype=torch.float64, device=DEV) for n in sizes]
    nn = (ctypes.c_int64 * n_tensors)(*sizes)
    s = ops._stream(hyper)
    seen = set()
    for step in range(12):
        if step == 6:       # through the device table: another learning rate and beta2 from here on
            for r in rows:
                r[2], r[4] = r[2] * 0.5, 0.99
            hyper.copy_(torch.tensor(rows, dtype=torch.float64))
        g = [_gradient(rng, n, r[1] / r[0]) for n, r in zip(sizes, rows)]
        for x in g:
            seen |= {"nan"} if np.isnan(x).any() else set()
            seen |= {"inf"} if np.isposinf(x).any() else set()
            seen |= {"-inf"} if np.isneginf(x).any() else set()
            seen |= {"0"} if (x == 0.0).any() else set()
        for x, r in zip(g, rows):
            seen |= {"clip"} if (np.abs(x[np.isfinite(x)] * r[0]) > r[1]).any() else set()
        g_d = _on_dev(g)
        _lib.check(L.tfrt_adam_multi(n_tensors, _ptrs(g_d), _ptrs(out), _ptrs(p_d), _ptrs(m_d),
                                     _ptrs(v_d), nn, ops._p(hyper), ops._p(st_d), ops._p(ticket), s),
                   "tfrt_adam_multi")
        torch.cuda.synchronize()
        for k in range(n_tensors):
            gw, p[k], m[k], v[k], st[k] = _restate(g[k], p[k], m[k], v[k], st[k], *rows[k])
            assert _same(out[k], gw), (step, k)
            assert _same(p_d[k], p[k]), (step, k)
            assert _same(m_d[k], m[k]), (step, k)
            assert _same(v_d[k], v[k]), (step, k)
            assert g_d[k].cpu().numpy().tobytes() == g[k].tobytes()     # only read (NaN included)
        assert _same(st_d, st), step                             # every tensor, the empty one too
        assert int(ticket) == 0, step
    assert seen == {"nan", "inf", "-inf", "0", "clip"}
    assert st[0][0] == 12.0 and all(np.isfinite(x).all() for x in p)

    # argument checks (nothing is launched)
    void = (ctypes.c_void_p * n_tensors)()
    good = [n_tensors, _ptrs(g_d), None, _ptrs(p_d), _ptrs(m_d), _ptrs(v_d), nn, ops._p(hyper),
            ops._p(st_d), ops._p(ticket), s]
    for at, bad in ((0, 9), (3, None), (4, None), (5, None), (7, None), (8, None), (9, None)):
        args = list(good)
        args[at] = bad
        assert L.tfrt_adam_multi(*args) == _BADARG, at
    if 4097 in sizes:
        for at in (3, 4, 5):
            args = list(good)
            args[at] = void
            assert L.tfrt_adam_multi(*args) == _BADARG, at
    assert L.tfrt_adam_multi_finish(*good[:10], None, s) == _BADARG
    torch.cuda.synchronize()
    assert _same(st_d, st) and int(ticket) == 0


def test_adam_cabi_null_and_aliased_processed():
    """``processed == NULL``, one NULL entry, and ``processed`` aliasing ``grad``: the same
    parameters and state as with a buffer of its own."""
    from tensorflowraytrace_amd import _lib, ops
    L = _lib.lib()
    rng = np.random.default_rng(17)
    n_tensors, sizes, rows = 3, _SIZES[3], _rows(3)
    nn = (ctypes.c_int64 * n_tensors)(*sizes)
    hyper = torch.tensor(rows, dtype=torch.float64, device=DEV)
    p0 = [rng.standard_normal(n) for n in sizes]
    grads = [[_gradient(rng, n, r[1] / r[0]) for n, r in zip(sizes, rows)] for _ in range(3)]
    s = ops._stream(hyper)
    results = {}
    for mode in ("own", "null", "null entry", "alias"):
        p_d = _on_dev(p0)
        m_d, v_d = [torch.zeros_like(x) for x in p_d], [torch.zeros_like(x) for x in p_d]
        st_d = torch.tensor(_state0(n_tensors), dtype=torch.float64, device=DEV)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        for g in grads:
            g_d = _on_dev(g)
            own = [torch.full_like(x, 7.0) for x in g_d]
            if mode == "null entry":
                processed = (ctypes.c_void_p * n_tensors)(own[0].data_ptr(), None, None)
            else:
                processed = {"own": _ptrs(own), "null": None, "alias": _ptrs(g_d)}[mode]
            _lib.check(L.tfrt_adam_multi(n_tensors, _ptrs(g_d), processed, _ptrs(p_d), _ptrs(m_d),
                                         _ptrs(v_d), nn, ops._p(hyper), ops._p(st_d),
                                         ops._p(ticket), s), mode)
        torch.cuda.synchronize()
        last = {"own": own, "alias": g_d, "null entry": own[:1]}.get(mode, [])
        results[mode] = (p_d, m_d, v_d, [st_d], last)
    ref = results["own"]
    for mode in ("null", "null entry", "alias"):
        for a, b in zip(results[mode][:4], ref[:4]):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), mode
    assert all(torch.equal(x, y) for x, y in zip(results["alias"][4], ref[4]))
    assert torch.equal(results["null entry"][4][0], ref[4][0])
    assert float(ref[3][0][1, 0]) == 3.0


def test_adam_cabi_finish_equals_update_then_goal_finish():
    """tfrt_adam_multi_finish = tfrt_adam_multi + tfrt_goal_finish, bit for bit, on a pending sum
    of tfrt_goal_error3d_deferred (and the sum equals tfrt_goal_error3d's); the spare workgroup
    takes part in the ticket, so the state advances once there too."""
    from tensorflowraytrace_amd import _lib, ops
    L = _lib.lib()
    gen = torch.Generator(device=DEV).manual_seed(11)
    cap, n, n_src, P = 50_001, 43_210, 60_000, 3
    fin = torch.randn((6, cap), dtype=torch.float64, device=DEV, generator=gen)
    ids = torch.randint(0, n_src, (cap,), dtype=torch.int32, device=DEV, generator=gen)
    goal = torch.randn((2, n_src), dtype=torch.float64, device=DEV, generator=gen)
    counts = torch.zeros(8 * (P + 1), dtype=torch.int32, device=DEV)
    counts[8 * P + 1] = n
    fields = (ctypes.c_int32 * 6)(4, 5, 0, 0, 0, 0)
    wsb = L.tfrt_goal_error3d_workspace_bytes(cap)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    g_fin = torch.zeros((6, cap), dtype=torch.float64, device=DEV)
    err_ref = torch.zeros(3, dtype=torch.float64, device=DEV)
    s = ops._stream(fin)
    common = (ops._p(fin), cap, ops._p(ids), _lib.F64, ops._p(counts), P, fields, 2, ops._p(goal),
              n_src, 1, ops._p(g_fin))
    _lib.check(L.tfrt_goal_error3d(*common, ops._p(err_ref), None, 0, None, ops._p(ws), wsb, s),
               "tfrt_goal_error3d")
    pending = _lib.GoalPending()
    err_a = torch.zeros(3, dtype=torch.float64, device=DEV)
    _lib.check(L.tfrt_goal_error3d_deferred(*common, ops._p(err_a), None, 0, None, ops._p(ws), wsb,
                                            ctypes.byref(pending), s), "tfrt_goal_error3d_deferred")
    err_b = torch.zeros(3, dtype=torch.float64, device=DEV)
    pending_b = _lib.GoalPending.from_buffer_copy(pending)
    pending_b.error_out = err_b.data_ptr()

    sizes = [300, 5000, 1]
    k = len(sizes)
    rng = np.random.default_rng(5)
    rows = torch.tensor(_rows(k), dtype=torch.float64, device=DEV)
    # grad, param, m, v (v >= 0: it is a running mean of squares)
    base = [[torch.tensor(rng.standard_normal(n), dtype=torch.float64, device=DEV) for n in sizes]
            for _ in range(4)]
    base[3] = [t.abs() for t in base[3]]
    nn = (ctypes.c_int64 * k)(*sizes)
    a = [[t.clone() for t in ts] for ts in base]
    b = [[t.clone() for t in ts] for ts in base]
    st_a = torch.tensor(_state0(k), dtype=torch.float64, device=DEV)
    st_b = st_a.clone()
    ticket = torch.zeros(2, dtype=torch.int32, device=DEV)
    for _ in range(2):        # (twice: the second launch finds the ticket the first one left)
        _lib.check(L.tfrt_adam_multi(k, _ptrs(a[0]), None, _ptrs(a[1]), _ptrs(a[2]), _ptrs(a[3]), nn,
                                     ops._p(rows), ops._p(st_a), ops._p(ticket), s),
                   "tfrt_adam_multi")
        _lib.check(L.tfrt_goal_finish(ctypes.byref(pending), s), "tfrt_goal_finish")
        _lib.check(L.tfrt_adam_multi_finish(k, _ptrs(b[0]), None, _ptrs(b[1]), _ptrs(b[2]),
                                            _ptrs(b[3]), nn, ops._p(rows), ops._p(st_b),
                                            ctypes.c_void_p(ticket.data_ptr() + 4),
                                            ctypes.byref(pending_b), s), "tfrt_adam_multi_finish")
    torch.cuda.synchronize()
    assert torch.equal(err_a, err_b) and torch.equal(err_a, err_ref)
    assert float(err_a[1]) == 2 * n
    for ta, tb in zip(a, b):
        for x, y in zip(ta, tb):
            assert torch.equal(x, y)
    assert torch.equal(st_a, st_b) and float(st_a[0, 0]) == 2.0
    assert ticket.tolist() == [0, 0]
    assert not torch.equal(a[1][0], base[1][0])

    # tensors without elements and a pending sum: the spare workgroup alone counts the step
    none = (ctypes.c_int64 * k)(0, 0, 0)
    _lib.check(L.tfrt_adam_multi_finish(k, _ptrs(b[0]), None, _ptrs(b[1]), _ptrs(b[2]), _ptrs(b[3]),
                                        none, ops._p(rows), ops._p(st_b), ops._p(ticket),
                                        ctypes.byref(pending_b), s), "empty, finish")
    _lib.check(L.tfrt_adam_multi(k, _ptrs(a[0]), None, _ptrs(a[1]), _ptrs(a[2]), _ptrs(a[3]), none,
                                 ops._p(rows), ops._p(st_a), ops._p(ticket), s), "empty")
    torch.cuda.synchronize()
    assert torch.equal(st_a, st_b) and float(st_a[0, 0]) == 3.0 and ticket.tolist() == [0, 0]
    assert torch.equal(err_a, err_b)


# ------------------------------------------------------------------- fused against generic
def _make(n_rays, mode, k=3, accumulators=False, **kw):
    """test_gpu_fused_step._make with an Adam_Optimizer.  mode: 'generic' (fused=False), 'eager'
    (fused, no graph), 'graph'."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=k, ray_dtype=torch.float64)
    erf = optimizer.GoalError(("y_end", "z_end"), _goal)
    opt = optimizer.Adam_Optimizer(
        eng, lens.parameters, erf, 3, learning_rate=3e-4, grad_clip=1e9,
        fused=False if mode == "generic" else "auto", graph="auto" if mode == "graph" else False,
        speculative=False, **kw)
    opt.suppress_warnings = True
    acc = None
    if accumulators:
        import tfrt.mesh_tools as mt
        _, a = mt.mesh_parametrization_tools(lens.surfaces[0].zero_points, 0)
        acc = [torch.as_tensor(np.asarray(a)), None]
    return opt, eng, lens, acc


def _run(opt, acc, steps, lrs=None):
    errs = []
    for i in range(steps):
        errs.append(float(opt.single_step(acc, lr_scale=1.0 if lrs is None else lrs[i])))
    return errs


def _compare(runs, ref, err_rtol, p_tol):
    ref_err, ref_p = runs[ref][0], runs[ref][1]
    for mode, (err, p, *_rest) in runs.items():
        if mode == ref:
            continue
        np.testing.assert_allclose(err, ref_err, rtol=err_rtol, atol=0, err_msg=mode)
        for a, b in zip(p, ref_p):
            assert float((a - b).abs().max()) <= p_tol, mode


def _state(opt):
    return [t.detach().cpu().clone() for t in opt._adam_m + opt._adam_v + [opt._adam_state]]


@pytest.mark.parametrize("accumulators", [False, True])
def test_adam_fused_and_graph_steps_equal_the_generic_path(accumulators):
    steps = 10
    lrs = list(np.linspace(1.0, 0.3, steps))
    runs = {}
    for mode in ("generic", "eager", "graph"):
        opt, eng, lens, acc = _make(1500, mode, accumulators=accumulators)
        runs[mode] = (_run(opt, acc, steps, lrs), _params(lens) + _state(opt), opt)
    assert runs["generic"][2]._fused_step is None
    assert all(np.isfinite(runs["generic"][0]))
    assert all(float(m.abs().max()) > 0 for m in runs["generic"][2]._adam_m)
    for mode in ("eager", "graph"):
        assert runs[mode][2]._fused_step is not None, mode
        assert runs[mode][2]._adam_state[:, 0].tolist() == [steps, steps], mode
    assert runs["eager"][2]._fused_step.graph_replays == 0
    g = runs["graph"][2]._fused_step
    assert g.capture_error is None, g.capture_error
    assert g.graph_replays >= 6
    _compare(runs, "generic", 1e-11, 1e-12)


def test_adam_fused_step_in_coherent_order_equals_the_generic_path():
    steps = 10
    runs = {}
    for mode in ("generic", "graph"):
        opt, eng, lens, acc = _make(6000, mode, k=6)
        eng.coherent = mode == "graph"
        runs[mode] = (_run(opt, None, steps), _params(lens) + _state(opt), opt, eng)
    g = runs["graph"][2]._fused_step
    assert g.capture_error is None and g.graph_replays >= 6
    assert g.folded_backward           # (from 4096 rays on: ordered rays, one-launch reverse sweep)
    assert getattr(runs["graph"][3], "_order_cache", None) is not None
    _compare(runs, "generic", 1e-10, 1e-11)


def _arc(mode, rowwise, **kw):
    import optimize_arc
    from tfrt.optimizer import Adam_Optimizer, GoalError, RowwiseError
    s = optimize_arc.build(200, ray_dtype=torch.float64)
    if rowwise:
        erf = RowwiseError(lambda r: r["y_end"] ** 2)
    else:
        n = s["system"].sources["x_start"].shape[0]
        erf = GoalError(("y_end",), torch.zeros(n, dtype=torch.float64, device=DEV))
    opt = Adam_Optimizer(s["engine"], [s["parameter"]], erf, 2, learning_rate=1.0, grad_clip=0.1,
                         adam_learning_rate=0.02, fused=mode != "generic", graph=mode == "graph",
                         **kw)
    return opt, s["parameter"]


@pytest.mark.parametrize("rowwise", [False, True])
def test_adam_fused_2d_step_equals_the_generic_step(rowwise):
    """The single arc of examples/optimize_arc.py, with a GoalError and with the same error as a
    RowwiseError."""
    steps = 10
    runs = {}
    for mode in ("generic", "eager", "graph"):
        opt, parameter = _arc(mode, rowwise)
        errs = _run(opt, None, steps, [1.0, 0.7, 0.5, 1.2, 0.9, 0.6, 1.0, 0.8, 1.0, 0.7])
        runs[mode] = (errs, [parameter.detach().cpu().clone()] + _state(opt), opt)
    assert runs["generic"][2]._fused_step is None
    assert runs["eager"][2]._fused_step.graph_replays == 0
    fs = runs["graph"][2]._fused_step
    assert fs is not None and fs.capture_error is None and fs.graph_replays >= 6
    assert runs["generic"][0][-1] < runs["generic"][0][0]
    _compare(runs, "generic", 1e-11, 1e-12)


def test_adam_phases_replay_one_graph(monkeypatch):
    """training_routine whose phases change the learning rate, adam_learning_rate and beta1: they
    are values in the device table, so the graph captured in the first phase replays through all
    three."""
    import tensorflowraytrace_amd.fused_step as fs
    captures = []
    orig = fs.FusedStep._capture

    def counting(self, *a, **k):
        captures.append(self.steps)
        return orig(self, *a, **k)

    monkeypatch.setattr(fs.FusedStep, "_capture", counting)
    routine = [{"steps": 5, "learning_rate": 1.0, "beta1": 0.9},
               {"steps": 4, "learning_rate": (1.0, 0.5), "beta1": 0.5, "adam_learning_rate": 5e-4},
               {"steps": 5, "learning_rate": 0.5, "beta1": 0.8, "beta2": 0.99}]
    runs = {}
    for mode in ("generic", "graph"):
        opt, eng, lens, acc = _make(1500, mode)
        opt.training_routine(routine, report_frequency=0, show_time=False)
        assert opt.iterations == 14
        assert (opt.beta1, opt.beta2, opt.adam_learning_rate) == (0.8, 0.99, 5e-4)
        runs[mode] = ([], _params(lens) + _state(opt), opt)
    g = runs["graph"][2]._fused_step
    assert g.capture_error is None, g.capture_error
    assert len(captures) == 1, captures
    assert g.graph_replays >= 14 - 4
    p1 = 0.9 ** 0     # (the running product of the betas in force, step by step)
    for b in [0.9] * 5 + [0.5] * 4 + [0.8] * 5:
        p1 = p1 * b
    assert runs["graph"][2]._adam_state[:, :2].tolist() == [[14.0, p1]] * 2
    _compare(runs, "generic", 1e-11, 1e-12)


def test_adam_state_survives_a_change_of_path_and_resets_in_place():
    """Fused, generic, then fused steps continue one trajectory equal to an all-generic run;
    after reset_state() the next step is step 1 of a fresh optimiser on the same parameters, on
    the graph that was captured before."""
    runs = {}
    opt, eng, lens, acc = _make(1500, "graph")
    errs = _run(opt, None, 5)
    fs = opt._fused_step
    assert fs is not None and fs.capture_error is None and fs.graph_replays >= 1
    replays = fs.graph_replays
    buffers = opt._adam_m + opt._adam_v + [opt._adam_state]
    opt.fused = False
    errs += _run(opt, None, 3)
    assert fs.graph_replays == replays
    opt.fused = "auto"
    errs += _run(opt, None, 3)
    assert opt._fused_step is fs and fs.capture_error is None and fs.graph_replays > replays
    assert all(a is b for a, b in zip(opt._adam_m + opt._adam_v + [opt._adam_state], buffers))
    assert opt._adam_state[:, 0].tolist() == [11.0, 11.0]
    runs["mixed"] = (errs, _params(lens) + _state(opt))
    ref, _eng, ref_lens, _acc = _make(1500, "generic")
    runs["generic"] = (_run(ref, None, 11), _params(ref_lens) + _state(ref))
    _compare(runs, "generic", 1e-11, 1e-12)

    # reset, one replayed step | a fresh optimiser on the same parameters, one generic step
    opt.reset_state()
    assert opt._adam_state.tolist() == [[0.0, 1.0, 1.0]] * 2
    fresh, _eng, fresh_lens, _acc = _make(1500, "generic")
    with torch.no_grad():
        for q, p in zip(fresh_lens.parameters, lens.parameters):
            q.copy_(p)
    graphs, replays = fs._graphs, fs.graph_replays
    e_reset = _run(opt, None, 1)
    assert fs._graphs is graphs and fs.graph_replays == replays + 1       # replayed, not re-captured
    e_fresh = _run(fresh, None, 1)
    assert opt._adam_state[:, 0].tolist() == [1.0, 1.0]
    _compare({"reset": (e_reset, _params(lens) + _state(opt)),
              "fresh": (e_fresh, _params(fresh_lens) + _state(fresh))}, "fresh", 1e-11, 1e-12)


def test_adam_lowers_the_error_of_the_single_arc():
    """40 Adam steps on the arc of examples/optimize_arc.py (``--adam``: the example's values) end
    below the error they started from: the sign of the step and the handling of the state, not a
    measurement.  The rule moves the parameter by about adam_learning_rate per step towards the
    focus.  The restatement of the rule, driven on the host by the oracle's 2-D tracer and its
    autograd gradient over the same scene and the same clip, meets it with the example's values
    (adam_learning_rate 0.05): mean error 0.1009 -> 0.0022, the parameter 5.0 -> 3.29 (0.0375 at
    0.02 and 0.0976 at the default 0.001: smaller steps, the same sign)."""
    import optimize_arc
    errors, s = optimize_arc.run(ray_count=10, steps=40, adam=True, verbose=False)
    assert s["optimizer"].update_rule == "adam"
    assert s["optimizer"]._adam_state[0, 0] == 40.0
    assert np.isfinite(errors).all() and errors[-1] < errors[0]
