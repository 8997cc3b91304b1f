"""
SpotError on the GPU: tfrt_spot_error (accumulate, seed, finish) against the numpy reference of
tests/spot_error_reference.py, and the error on the optimiser's paths -- the fused, replayed 3-D
step against the generic one, labels under replay, a re-drawn source, the parameter gradient
against the oracle, the fallbacks, 2-D, the example.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spot_error_reference as sr
from test_gpu_engine import _build_lens, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}
COUNTS = (0, 1, 63, 64, 65, 1000, 4097)


@functools.lru_cache(maxsize=None)
def _reference(n, G, two, f32, masked, permuted):
    """The reference of one case, computed once and shared (never written to)."""
    x, y, mask, group, perm = sr.points(n, np.float32 if f32 else np.float64, n_groups=G)
    return sr.spot_error(x, y if two else None, group, G, sr.DOMAIN if two else sr.DOMAIN[:1],
                         oob_weight=0.3, mask=mask if masked else None,
                         perm=perm if permuted else None)


def _kernel(n, G, two, dtype, masked, permuted, variant=0, pad=3):
    """tfrt_spot_error on the points of a case: the rows sit in a 6-row block (x in row 4, y in
    row 5) with ``pad`` spare columns; the gradient block starts out as NaN to show what is
    written."""
    from tensorflowraytrace_amd import ops
    x, y, mask, group, perm = sr.points(n, NP_DTYPE[dtype], n_groups=G)
    rows = torch.full((6, n + pad), 7.0, dtype=dtype, device=DEV)
    rows[4, :n] = torch.tensor(x, device=DEV)
    rows[5, :n] = torch.tensor(y, device=DEV)
    g = torch.tensor(group, device=DEV)
    qbits = ops.spot_qbits(g.numel())
    grid = ops.spot_grid(sr.DOMAIN if two else sr.DOMAIN[:1], qbits)
    grad = torch.full((6, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    m = torch.tensor(mask, device=DEV) if masked else None
    p = torch.tensor(perm, device=DEV) if permuted else None
    err, _, acc = ops.spot_error(rows[:, :n], 4, 5 if two else -1, g, G, grid, 0.3, mask=m, perm=p,
                                 grad=grad[:, :n], variant=variant)
    torch.cuda.synchronize()
    return err.cpu().numpy(), grad.cpu().numpy(), acc.cpu().numpy(), mask


def _check(got, ref, n, two, masked):
    err, grad, acc, mask = got
    assert np.array_equal(acc, ref["acc"])
    first = {}
    for name, row, want in (("x", 4, ref["grad_x"]), ("y", 5, ref["grad_y"])):
        if want is None:
            assert np.isnan(grad[row]).all()             # (one field: the entry owns one row)
            continue
        same = grad[row, :n].view(np.int64) == want.view(np.int64)
        if not same.all():
            i = int(np.nonzero(~same)[0][0])
            first[name] = (i, grad[row, i], want[i])
    assert not first, f"gradient entries that are not bit-equal (index, kernel, reference): {first}"
    assert np.isnan(grad[:4]).all() and np.isnan(grad[:, n:]).all()
    print(f"error {err[0]!r} reference {ref['error']!r} bound {sr.error_bound(ref):.3e}")
    assert abs(err[0] - ref["error"]) <= sr.error_bound(ref)
    counting = int((mask >= 0).sum()) if masked else n
    assert err[1] == (2 if two else 1) * counting
    if counting:
        assert err[2] == err[0] / err[1]
    else:
        assert np.isnan(err[2]) and err[0] == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("G", sr.GROUPS)
def test_kernel_equals_the_reference(G, dtype):
    """Every count, two fields and one, with and without the mask, with and without perm.  1,025
    and 5,000 groups take the global atomics, fewer the table in LDS."""
    f32 = dtype == torch.float32
    for n in COUNTS:
        for two in (True, False):
            for masked in (False, True):
                for permuted in (False, True):
                    ref = _reference(n, G, two, f32, masked, permuted)
                    _check(_kernel(n, G, two, dtype, masked, permuted), ref, n, two, masked)


def test_both_accumulate_variants_give_the_same_bits():
    ref = _reference(4097, 64, True, False, True, True)
    lds = _kernel(4097, 64, True, torch.float64, True, True, variant=1)
    glb = _kernel(4097, 64, True, torch.float64, True, True, variant=2)
    _check(lds, ref, 4097, True, True)
    for a, b in zip(lds[:3], glb[:3]):
        assert a.tobytes() == b.tobytes()
    from tensorflowraytrace_amd import _lib
    with pytest.raises(_lib.TfrtError):
        _kernel(10, 1025, True, torch.float64, False, False, variant=1)


def test_two_calls_give_the_same_bits():
    for G in (64, 5000):
        a = _kernel(4097, G, True, torch.float32, True, True)
        b = _kernel(4097, G, True, torch.float32, True, True)
        for u, v in zip(a[:3], b[:3]):
            assert u.tobytes() == v.tobytes()


def test_contention_every_column_at_one_place_in_one_group():
    """100,000 columns at the same place in the same group: the exact integer sums."""
    from tensorflowraytrace_amd import ops
    n = 100_000
    (x0, x1), (y0, y1) = sr.DOMAIN
    px, py = x0 + 0.3 * (x1 - x0), y0 + 0.55 * (y1 - y0)
    rows = torch.empty((2, n), dtype=torch.float64, device=DEV)
    rows[0], rows[1] = px, py
    group = torch.full((n,), 2, dtype=torch.int32, device=DEV)
    one = sr.spot_error(np.array([px]), np.array([py]), np.array([2]), 3, sr.DOMAIN,
                        qbits=sr.qbits_of(n))
    q = one["acc"][2]
    assert q[0] == 1 and q[1] > 0 and q[2] > 0
    grid = ops.spot_grid(sr.DOMAIN, ops.spot_qbits(n))
    for variant in (1, 2):
        err, grad, acc = ops.spot_error(rows, 0, 1, group, 3, grid, variant=variant)
        acc = acc.cpu().numpy()
        assert acc[2].tolist() == [n, n * int(q[1]), n * int(q[2]), 0] and not acc[:2].any()
        assert float(err[1]) == 2 * n


def test_bad_arguments():
    from tensorflowraytrace_amd import _lib
    L = _lib.lib()
    assert L.tfrt_spot_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_spot_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_spot_error_workspace_bytes(-1, 4) == 0
    assert L.tfrt_spot_error_workspace_bytes(0, 4) > 0
    t = torch.zeros(1 << 15, dtype=torch.float64, device=DEV)
    p = t.data_ptr()

    def call(n=8, G=4, row_x=0, row_y=1, x1=1.0, qsx=4.0, oob=0.0, ws=1 << 17, stride=8,
             variant=0, group=p, qbits=40, n_source=8):
        return L.tfrt_spot_error(p, stride, n, 1, None, row_x, row_y, group, n_source, None, G, 0.0,
                                 x1, qsx, 0.0, 1.0, 4.0, qbits, oob, p, 8, p, p, variant, p, ws,
                                 None)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(row_x=6), dict(row_y=0),
                dict(x1=0.0), dict(qsx=0.0), dict(oob=-1.0), dict(stride=4), dict(variant=3),
                dict(group=None), dict(n=1 << 31), dict(qbits=53),
                dict(n=1 << 22, qbits=40, stride=1 << 22), dict(G=1025, variant=1)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    assert call(n=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ the optimiser
DOMAIN_LENS = ((-1.1, 1.1), (-1.1, 1.1))     # the lens' finished rays fill a disk of radius ~1.28


def _make(n_rays, mode, ray_dtype=torch.float64, fields=("y_end", "z_end"), random_rays=False,
          n_groups=37, **engine_kw):
    """The lens of tests/test_gpu_density.py's ``_make`` with a SpotError over 37 groups."""
    import tfrt.optimizer as optimizer
    eng, system, lens, target, source = _build_lens(n_rays, k=3, ray_dtype=ray_dtype,
                                                    random_rays=random_rays, **engine_kw)
    groups = torch.arange(n_rays) % n_groups
    erf = optimizer.SpotError(fields, groups, DOMAIN_LENS, oob_weight=2.0 / n_rays)
    # (the error is a sum over the rays, a DensityError of order 1: the step size of
    # tests/test_gpu_density.py divided by the ray count, times 4 so that six steps still move)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=0.2 / n_rays,
                                  grad_clip=1e9,
                                  fused=False if mode == "generic" else "auto",
                                  graph="auto" if mode == "graph" else False, speculative=False)
    opt.suppress_warnings = True
    return opt, eng, lens, (system, target, source)


def _steps(opt, lens, steps):
    errs = [float(opt.single_step(None)) for _ in range(steps)]
    return errs, [p.detach().cpu().clone() for p in lens.parameters]


def _inside(fin):
    y, z = fin["y_end"].double(), fin["z_end"].double()
    return (y.abs() <= 1.1) & (z.abs() <= 1.1)


def test_fused_step_equals_the_generic_step():
    """8,192 rays (traced in place), 6 steps: the same errors and parameters at the tolerances of
    tests/test_gpu_density.py's fixed-shape-against-generic test; the step is one graph replay."""
    runs = {mode: _make(8192, mode) for mode in ("generic", "graph")}
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
    # the records of the last replayed step can be read afterwards: every finished ray inside
    # the domain is in one of them
    erf = runs["graph"][0].error_function
    inside = int(_inside(runs["graph"][1].finished_rays).sum())
    assert inside > 4000 and int(erf.last_acc[:, 0].sum()) == inside
    assert erf.centroids().shape == (37, 2) and bool(torch.isfinite(erf.centroids()).all())


@pytest.mark.parametrize("n_groups", [28, 64])
def test_records_are_cleared_at_every_replay(n_groups):
    """Record tables of 896 and 2,048 bytes (37 groups above: 1,184): after several replays the
    counts are those of ONE step and the fourth word of every record is still 0."""
    opt, eng, lens, _ = _make(8192, "graph", random_rays=True, n_groups=n_groups)
    _steps(opt, lens, 9)
    fs = opt._fused_step
    erf = opt.error_function
    assert fs is not None and fs.graph_replays >= 3 and fs.capture_error is None
    acc = erf.last_acc.cpu()
    inside = int(_inside(eng.finished_rays).sum())
    assert inside > 4000 and int(acc[:, 0].sum()) == inside and not bool(acc[:, 3].any())


def test_labels_overwritten_in_place_are_seen_by_replays_and_other_labels_recapture():
    opt, eng, lens, _ = _make(8192, "graph")
    _steps(opt, lens, 6)
    fs = opt._fused_step
    erf = opt.error_function
    assert fs.graph_replays > 0
    before, e_before = fs.graph_replays, float(opt.single_step(None))
    erf.labels.copy_(torch.arange(8192, device=erf.labels.device) // 222)     # neighbours together
    e_after = float(opt.single_step(None))
    assert fs.graph_replays == before + 2 and abs(e_after - e_before) > 1e-3 * e_before
    erf.labels = erf.labels.clone()                   # another buffer: not the captured one
    float(opt.single_step(None))
    assert fs.graph_replays == before + 2


def test_a_redrawn_source_keeps_its_labels_under_replay():
    """The source is re-drawn (and re-ordered) inside the graph at every step; the kernel looks
    the labels up through the trace's order itself: the records of the last replay equal the
    reference on that trace's finished rays, their source-ray indices and the labels."""
    opt, eng, lens, _ = _make(8192, "graph", random_rays=True)
    _steps(opt, lens, 5)
    fs = opt._fused_step
    erf = opt.error_function
    # (five steps are one generic step, the eager warm-up and the capture: the first REPLAY is
    # the step after them, and a replay is what this test is about)
    for _ in range(4):
        if fs.graph_replays >= 2:
            break
        _steps(opt, lens, 1)
    assert fs is not None and fs.in_place and fs.graph_replays >= 2 and fs.capture_error is None
    acc = erf.last_acc.cpu().numpy().copy()
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].cpu().numpy()
    ref = sr.spot_error(fin["y_end"].cpu().numpy(), fin["z_end"].cpu().numpy(),
                        erf.labels.cpu().numpy(), 37, DOMAIN_LENS, oob_weight=erf.oob_weight,
                        perm=ids)
    assert ref["n_inside"] > 4000 and len(set(ids.tolist())) == ids.shape[0]
    assert np.array_equal(acc, ref["acc"])


def _torch_objective(y, z, label, n_groups, domain, oob):
    from test_spot_error_host import _torch_objective as objective
    return objective(y, z, label, n_groups, domain, oob)


@pytest.mark.parametrize("ray_dtype,tol", [(torch.float64, 1e-9), (torch.float32, 1e-5)],
                         ids=["f64", "f32"])
def test_parameter_gradient_equals_the_oracle(ray_dtype, tol):
    """4,096 rays, one step: d error / d parameters on the generic path and on the fused step's
    fixed-shape path against the oracle's float64 trace composed with the plain torch objective
    (the means differentiated through) under autograd."""
    from tensorflowraytrace_amd.fused_step import FusedStep
    from oracle import tracer
    opt, eng, lens, (system, target, source) = _make(4096, "eager", ray_dtype)
    erf = opt.error_function
    grads, err_sum, n_terms = opt.raw_gradient()
    q = [p.detach().cpu().clone().requires_grad_(True) for p in lens.parameters]
    osys, src = _oracle_for(system, lens, target, source, q)
    if ray_dtype == torch.float32:
        for k in ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end"):
            src[k] = src[k].float().double()
    src["spot_label"] = erf.labels.cpu().double()
    ref = tracer.ray_trace(osys, src, max_iterations=3,
                           inherit=("wavelength", "object_coords", "spot_label"))
    y, z = ref["finished"]["y_end"], ref["finished"]["z_end"]
    label = ref["finished"]["spot_label"].long()
    assert n_terms == 2 * y.shape[0]
    # no finished ray within 1e-6 of the domain's edge: the in / out decision is the same in
    # float32 and float64
    for v, (lo, hi) in zip((y.detach().numpy(), z.detach().numpy()), DOMAIN_LENS):
        assert min(np.abs(v - lo).min(), np.abs(v - hi).min()) > 1e-6
    assert int(((y.abs() > 1.1) | (z.abs() > 1.1)).sum()) > 50       # the penalty takes part
    e = _torch_objective(y, z, label, 37, DOMAIN_LENS, erf.oob_weight)
    rg = torch.autograd.grad(e, q)
    e = e.detach()
    print(f"error {float(err_sum)!r} oracle {float(e)!r}")
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
    assert abs(float(err3[0]) - float(e)) <= 10 * tol * float(e)
    assert float(err3[1]) == 2 * y.shape[0]


@pytest.mark.parametrize("what", ["few_rays", "deterministic"])
def test_fallbacks_take_the_generic_path(what):
    n, kw = (2000, {}) if what == "few_rays" else (8192, dict(deterministic=True))
    runs = {mode: _make(n, mode, **kw) for mode in ("generic", "graph")}
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
    eng.optical_system.update()
    eng.ray_trace(4)
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    n_source = eng.optical_system.sources["x_start"].shape[0]
    domain = ((float(np.quantile(y, 0.1)), float(np.quantile(y, 0.9))),)    # some rays outside
    groups = np.arange(n_source) % 9
    erf = optimizer.SpotError(("y_end",), groups, domain, oob_weight=0.01)
    opt = optimizer.SGD_Optimizer(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
                                  sgd_learning_rate=1.0)
    e0 = float(opt.single_step(None))
    assert opt._fused_step is None
    grads, err_sum, n_terms = opt.raw_gradient()
    y = eng.finished_rays["y_end"].detach().cpu().double().numpy()
    ids = eng.last_trace["finished_id"].cpu().numpy()
    ref = sr.spot_error(y, None, groups, 9, domain, oob_weight=0.01, perm=ids)
    assert ref["n_penalised"] > 0 and ref["n_inside"] > 100 and n_terms == y.shape[0]
    assert np.array_equal(erf.last_acc.cpu().numpy(), ref["acc"])
    assert abs(float(err_sum) - ref["error"]) <= sr.error_bound(ref)
    assert np.isfinite(e0) and any(float(g.abs().max()) > 0 for g in grads)


def test_imaging_example_shrinks_the_spots():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "imaging.py"),
                          "--rays", "8192", "--steps", "8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("rms spot: first")][-1]
    first, last = float(line.split()[3]), float(line.split()[5])
    assert last < first
