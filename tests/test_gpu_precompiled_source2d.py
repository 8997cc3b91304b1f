"""A 2-D PrecompiledSource made on the device (csrc/tfrt_source.hip: tfrt_source2d_program of kind
TFRT_SRC_POOL, tfrt_source2d_pool_rows; tfrt/sources.py:1099-1358): a stored pool of 2-D rays,
re-sampled with replacement and jittered by a normal perturbation of the end points at every
update.  The reference draws with TensorFlow's unseeded generator; here rows and normals come from
the counter-based generator, so parity is the distribution (tolerances from the sample size), the
assembly of the rays (exact: a ray IS its pool row; the draw against a numpy restatement of the
header's words), and that nothing else about a trace or an optimiser step depends on how the rays
were made."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from source_reference import philox_uv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO2 = ("x_start", "y_start", "x_end", "y_end")
sys.path.insert(0, os.path.join(ROOT, "examples"))


def _dist():
    import tfrt.distributions as d
    return d


def _pool_fields(n, seed=0, wavelengths=None):
    """n distinct rays of a beam along +x (from x = -1 to x = 0, heights in [-1.4, 1.4], a small
    slope), a distinct wavelength each (or drawn from ``wavelengths``), a per-ray ``rank`` and a
    2-column field."""
    rng = np.random.default_rng(seed)
    ramp = np.arange(n, dtype=np.float64) / n
    ys = rng.uniform(-1.4, 1.4, size=n)
    f = {"x_start": -1.0 + 1e-3 * ramp, "y_start": ys, "x_end": 1e-3 * ramp,
         "y_end": ys + rng.uniform(-0.02, 0.02, size=n)}
    f["wavelength"] = (np.linspace(450.0, 650.0, n) if wavelengths is None
                       else np.asarray(wavelengths, dtype=np.float64)[rng.integers(0, len(wavelengths), n)])
    f["rank"] = ys / 1.4
    f["tag"] = np.stack([np.arange(n, dtype=np.float64), -0.5 * np.arange(n, dtype=np.float64)], axis=1)
    return f


def _source(fields, sample_count, **kw):
    import tfrt.sources as sources
    src = sources.PrecompiledSource(2, sample_count=sample_count, **kw)
    src.from_samples([fields])
    assert src.device_mode and isinstance(src._fields, sources.PoolRaySet)
    return src


def _dev(fields):
    return {k: torch.as_tensor(v).to(DEV) for k, v in fields.items()}


# ------------------------------------------------------------------- numpy restatement
def _philox_uv(seed, stream, epoch, n):
    """Both float64 of Philox4x32-10(counter = (sample, epoch), key = (seed, stream)) for samples
    0 .. n-1: 53 bits of output words (0, 1) and of (2, 3), in [0, 1) (tests/source_reference.py)."""
    return philox_uv(seed, stream, epoch, n)


# ------------------------------------------------------------------------------ 1. one draw
def test_every_ray_is_its_pool_row_in_every_form_the_set_hands_out():
    d = _dist()
    d.seed(5)
    n_pool, n = 4099, 100_003                      # a prime pool, a tail wavefront
    fields = _pool_fields(n_pool)
    pool = _dev(fields)
    records = torch.stack([pool[g] for g in GEO2], dim=1)            # (n_pool, 4)
    src = _source(fields, n)
    rs = src._fields
    assert list(rs.keys())[:4] == list(GEO2) and set(rs.keys()) == set(fields.keys())
    assert rs.n_rays == n
    with pytest.raises(NotImplementedError):
        rs.order()
    rows = rs.rows()
    assert rows.dtype == torch.int32 and rows.shape == (n,)
    rl = rows.long()
    assert int(rl.min()) >= 0 and int(rl.max()) < n_pool
    assert len(torch.unique(rl)) == n_pool                           # (24 draws per row: all occur)
    got = torch.stack([src[g] for g in GEO2])                        # (4, n) float64
    assert got.dtype == torch.float64
    assert torch.equal(got, records[rl].t())                         # bit for bit
    for f in ("wavelength", "rank", "tag"):
        assert torch.equal(src[f], pool[f][rl]), f
    for dt in (torch.float32, torch.float64):
        blk = rs.ray_block(dt)
        assert blk.shape == (4, n) and blk.dtype == dt
        assert torch.equal(blk, got.to(dt))                          # float32: the float64 one rounded
        assert rs.ray_block(dt) is blk                               # persistent
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(n, generator=g).int().to(DEV)
    pv = rs.permuted(perm)
    assert torch.equal(pv.rows(), rows[perm.long()])
    assert torch.equal(pv.ray_block(torch.float32), got.float()[:, perm.long()])
    assert torch.equal(pv["y_end"], src["y_end"][perm.long()])
    assert torch.equal(pv["tag"], pool["tag"][rl][perm.long()])
    sh = rs.shard(1000, 8000)
    assert torch.equal(sh.ray_block(torch.float64), got[:, 1000:8000])
    assert torch.equal(sh.rows(), rows[1000:8000]) and torch.equal(sh["tag"], pool["tag"][rl[1000:8000]])
    tail = rs.shard(n - 67, n)                                       # the last, partial wavefront
    assert torch.equal(tail.ray_block(torch.float64), got[:, n - 67:])
    # the same draw until update(), another one after it -- in place
    assert src._fields.rows() is rows and torch.equal(torch.stack([src[g] for g in GEO2]), got)
    key, ident = rs.cache_key, rs.identity
    blk32 = rs.ray_block(torch.float32)
    src.update()
    rs2 = src._fields
    assert rs2.cache_key != key and rs2.identity == ident
    rows2 = rs2.rows()
    assert float((rows2 != rows).double().mean()) > 0.99
    assert rs2.ray_block(torch.float32) is blk32
    assert torch.equal(blk32, records[rows2.long()].t().float())
    # two sources with the same seed agree, draw after draw; another seed draws other rows
    d.seed(5)
    twin = _source(fields, n)
    assert torch.equal(twin._fields.rows(), rows)
    twin.update()
    assert torch.equal(twin._fields.rows(), rows2)
    d.seed(6)
    other = _source(fields, n)
    assert float((other._fields.rows() != rows).double().mean()) > 0.99


# -------------------------------------------------------------- 2. the header's words
def test_rows_and_normals_are_the_stated_function_of_the_generator():
    """The draw as include/tfrt_hip.h states it, restated in numpy: rows exactly; the normals to
    1e-12 absolute (float64 log, sqrt and sincospi are good to a few ulp on values of magnitude
    <= 8.6, i.e. about 1e-14: a hundredfold margin)."""
    d = _dist()
    d.seed(12345)
    n_pool, n = 4099, 100_003
    fields = _pool_fields(n_pool, seed=2)
    pool = _dev(fields)
    s_start, s_end = (0.0, 2e-3), (5e-3, 1e-3)       # x_start has no sigma; y has both
    src = _source(fields, n, start_perturbation=s_start, end_perturbation=s_end)
    sp = src._dev_program[1]
    seed, stream = int(sp.pool_seed), int(sp.pool_stream)
    assert (sp.sigma_start[0], sp.sigma_start[1], sp.sigma_end[0], sp.sigma_end[1]) == s_start + s_end
    for epoch in (1, 2):
        assert int(src._epoch_dev) == epoch
        u0, _ = _philox_uv(seed, stream, epoch, n)
        want_rows = np.minimum(np.floor(u0 * n_pool), n_pool - 1).astype(np.int64)
        rows = src._fields.rows()
        assert np.array_equal(rows.cpu().numpy(), want_rows)
        rl = rows.long()
        assert torch.equal(src["x_start"], pool["x_start"][rl])      # sigma 0: the stored coordinate
        for q, axis in enumerate("xy"):
            u, v = _philox_uv(seed, stream + 1 + q, epoch, n)
            r = np.sqrt(-2.0 * np.log(1.0 - u))
            for suffix, sigma, z in (("_start", s_start[q], r * np.cos(2 * np.pi * v)),
                                     ("_end", s_end[q], r * np.sin(2 * np.pi * v))):
                if sigma == 0.0:
                    continue
                f = axis + suffix
                got = ((src[f] - pool[f][rl]) / sigma).cpu().numpy()
                # (the difference field - pool is itself rounded at the field's magnitude <= 1.5:
                # 2.2e-16 / sigma <= 2.2e-13 for the smallest sigma here)
                err = float(np.abs(got - z).max())
                print(f"epoch {epoch} {f}: max |z_device - z_numpy| = {err:.3e}")
                assert err <= 1e-12, (epoch, f, err)
        src.update()


# ------------------------------------------------------------------------------ 3. statistics
def test_rows_are_uniform_and_the_perturbation_is_normal():
    """Tolerances from the sample size n alone: five standard errors of each statistic."""
    d = _dist()
    d.seed(41)
    n_pool, n, K = 65536, 1 << 20, 256
    fields = _pool_fields(n_pool)
    pool = _dev(fields)
    s_x, s_y = 1e-2, 3e-3
    src = _source(fields, n, end_perturbation=(s_x, s_y))
    rl = src._fields.rows().long()
    counts = torch.bincount(rl // (n_pool // K), minlength=K).double()
    chi2 = float(((counts - n / K) ** 2 / (n / K)).sum())
    assert chi2 < (K - 1) + 5 * math.sqrt(2 * (K - 1)), chi2
    for f in ("x_start", "y_start"):                                 # sigma 0: the stored coordinate
        assert torch.equal(src[f], pool[f][rl]), f
    res = {}
    for f, s in (("x_end", s_x), ("y_end", s_y)):
        r = (src[f] - pool[f][rl]) / s
        assert bool(torch.isfinite(r).all())
        assert float(r.abs().max()) <= 8.6                           # Box-Muller at 53 bits
        mean, var = float(r.mean()), float(r.var(unbiased=False))
        kurt = float(((r - r.mean()) ** 4).mean()) / var ** 2
        assert abs(mean) < 5 / math.sqrt(n), (f, mean)
        assert abs(var - 1) < 5 * math.sqrt(2 / n), (f, var)
        assert abs(kurt - 3) < 5 * math.sqrt(24 / n), (f, kurt)
        res[f] = r
    corr = float((res["x_end"] * res["y_end"]).mean() - res["x_end"].mean() * res["y_end"].mean())
    corr /= float(res["x_end"].std() * res["y_end"].std())
    assert abs(corr) < 5 / math.sqrt(n), corr
    # start and end normals of one axis come from one Box-Muller pair: independent all the same
    src2 = _source(fields, n, start_perturbation=2e-3, end_perturbation=2e-3)
    rl2 = src2._fields.rows().long()
    a = (src2["y_start"] - pool["y_start"][rl2]) / 2e-3
    b = (src2["y_end"] - pool["y_end"][rl2]) / 2e-3
    assert float(a.abs().max()) <= 8.6 and float(b.abs().max()) <= 8.6
    assert abs(float(a.var(unbiased=False)) - 1) < 5 * math.sqrt(2 / n)
    assert abs(float((a * b).mean())) < 5 / math.sqrt(n)
    assert abs(float((a * a * b * b).mean()) - 1) < 5 * math.sqrt(8 / n)    # var(a^2 b^2) = 9 - 1
    old = src2["y_end"].clone()
    src2.update()
    assert float((src2["y_end"] - old).abs().max()) > 1e-3


# ------------------------------------------------------------------------ 4. no down-sampling
def test_without_downsampling_the_device_source_is_the_pool_in_order():
    d = _dist()
    d.seed(2)
    n_pool = 4099
    fields = _pool_fields(n_pool)
    pool = _dev(fields)
    src = _source(fields, 17, do_downsample=False)
    for _ in range(2):
        rs = src._fields
        assert rs.n_rays == n_pool
        assert torch.equal(rs.rows(), torch.arange(n_pool, dtype=torch.int32, device=DEV))
        for f in fields:
            assert torch.equal(src[f], pool[f]), f
        assert torch.equal(rs.ray_block(torch.float64), torch.stack([pool[g] for g in GEO2]))
        src.update()


def test_one_wavelength_is_handed_out_as_an_expanded_scalar():
    d = _dist()
    d.seed(2)
    src = _source(_pool_fields(3001, wavelengths=[575.0]), 10_000)
    w = src["wavelength"]
    assert w.shape == (10_000,) and w.stride(0) == 0 and float(w[0]) == 575.0
    src.update()
    assert src["wavelength"].data_ptr() == w.data_ptr()               # (the engine's table stays)


# ------------------------------------------------------------------------------ 5. trace
def _segments_and_arcs(source, **engine_kw):
    """scene_configs' 2-D scene (64 refracting arcs under a mirror polyline of 255 segments, a target
    wall) as an engine-level system over ``source``."""
    import scene_configs
    import tfrt.boundaries as boundaries
    import tfrt.engine as engine
    import tfrt.materials as materials
    import tfrt.operation as operation
    sets, _, _ = scene_configs._scene_5b(1)
    system = engine.OpticalSystem2D()
    for name, fs in sets.items():
        b = boundaries.ManualArcBoundary() if name.endswith("arcs") else \
            boundaries.ManualSegmentBoundary()
        for f, v in fs.items():
            b[f] = v
        setattr(system, name, [b])
    system.sources = [source]
    system.materials = [{"n": materials.vacuum}, {"n": materials.acrylic},
                        {"n": materials.reflective}]
    eng = engine.OpticalEngine(2, [operation.StandardReaction()], ray_dtype=torch.float64,
                               compile_dead_rays=True, compile_stopped_rays=True,
                               simple_ray_inheritance={"wavelength", "tag"}, **engine_kw)
    eng.optical_system = system
    system.update()
    eng.validate_system()
    return eng, system


def test_trace_of_a_device_made_pool_source_equals_the_trace_of_its_rays_as_plain_tensors():
    import scene_configs
    import tfrt.sources as sources
    d = _dist()
    d.seed(21)
    n = 8192
    _, rays, _ = scene_configs._scene_5b(5003, seed=3)
    fields = {g: rays[k] for k, g in enumerate(GEO2)}
    fields["wavelength"] = np.asarray([450.0, 550.0, 650.0])[np.arange(5003) % 3]
    fields["tag"] = np.stack([np.arange(5003.0), -np.arange(5003.0)], axis=1)
    pre = _source(fields, n, end_perturbation=(1e-3, 1e-3))
    eng, system = _segments_and_arcs(pre)
    classes = ("finished", "active", "dead", "stopped")
    names = GEO2 + ("wavelength", "tag")
    for _ in range(2):
        system.update()
        assert pre.device_mode
        eng.ray_trace(4)
        got = {c: {f: getattr(eng, c + "_rays")[f].clone() for f in names}
               for c in classes if bool(getattr(eng, c + "_rays"))}
        faces = {k: v.clone() for k, v in eng.last_trace.items()
                 if k.endswith(("_face", "_id")) and isinstance(v, torch.Tensor)}
        assert got["dead"]["x_start"].shape[0] > n // 2          # (most rays leave this scene)
        assert "finished" in got
        manual = sources.ManualSource(2)
        for f in pre.keys():
            manual[f] = pre[f].clone()
        eng2, system2 = _segments_and_arcs(manual)
        eng2.ray_trace(4)
        for c in classes:
            assert bool(getattr(eng2, c + "_rays")) == (c in got), c
        for c, fs in got.items():
            for f, v in fs.items():
                assert torch.equal(v, getattr(eng2, c + "_rays")[f]), (c, f)
        assert len(faces) >= 4
        for k, v in faces.items():
            assert torch.equal(v, eng2.last_trace[k]), k


# ------------------------------------------------------------------------------- 6. step
def _step_runs(error, momentum, fields, steps=12, n=8192, seed=33):
    """(errors, final parameter, optimiser, scene, draws) of a fused, graph-replayed run and of a
    generic one over examples/optimize_arc.py's single-arc scene with a 2-D pool source, built after
    the same seed.  The optimiser is that of test_gpu_source2d_programs._step_runs."""
    import optimize_arc
    from tfrt.optimizer import GoalError, RowwiseError, SGD_Optimizer
    d = _dist()
    out = {}
    for mode in ("graph", "generic"):
        d.seed(seed)
        s = optimize_arc.build(10, ray_dtype=torch.float64)
        eng, system = s["engine"], s["system"]
        source = _source(fields, n, end_perturbation=(0.0, 2e-3))
        system.sources = [source]
        eng.add_inheritable_field("rank")
        system.update()
        s["source"] = source
        if error == "goal":
            erf = GoalError(("y_end",), torch.zeros(n, dtype=torch.float64, device=DEV))
        else:
            erf = RowwiseError(lambda r: (1.0 + r["rank"] ** 2) * r["y_end"] ** 2)
        opt = SGD_Optimizer(eng, [s["parameter"]], erf, 2, learning_rate=0.02, grad_clip=0.05,
                            sgd_learning_rate=1.0, fused=mode == "graph", graph=mode == "graph",
                            apply_momentum=momentum, nesterov=True)
        errors, draws = [], []
        for _ in range(steps):
            errors.append(float(opt.single_step(None, momentum=0.6 if momentum else 0.0)))
            draws.append(source["y_end"].clone())            # the rays of the step just run
        torch.cuda.synchronize()
        out[mode] = (errors, s["parameter"].detach().cpu().clone(), opt, s, draws)
    return out


def _check_step_runs(runs, steps):
    """The assertions, and exactly the tolerances, of test_gpu_source2d_programs.
    test_fused_2d_step_over_a_redrawn_source_is_captured_and_equals_the_generic_step."""
    import tfrt.sources as sources
    assert runs["generic"][2]._fused_step is None
    fs = runs["graph"][2]._fused_step
    assert fs is not None and fs.capture_error is None, getattr(fs, "capture_error", None)
    assert fs.graph_replays > 0 and fs.steps == steps
    for mode in runs:
        source = runs[mode][3]["source"]
        assert source.device_mode and isinstance(source._fields, sources.PoolRaySet)
        errors = runs[mode][0]
        assert all(np.isfinite(errors)) and len(set(errors)) == steps, errors   # a new draw every step
    # the rays really are re-drawn under replay: the last steps are replays, their sources differ
    # from step to step, and they are the very draws of the generic run (same seed, same epochs)
    draws, generic_draws = runs["graph"][4], runs["generic"][4]
    assert fs.graph_replays >= 3
    for k in range(steps - 3, steps):
        assert float((draws[k] - draws[k - 1]).abs().max()) > 1e-3, k
        assert torch.equal(draws[k], generic_draws[k]), k
    print("graph  ", runs["graph"][0], "\ngeneric", runs["generic"][0])
    np.testing.assert_allclose(runs["graph"][0], runs["generic"][0], rtol=1e-10, atol=0)
    a, b = runs["graph"][1], runs["generic"][1]
    assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max()), (a, b)
    assert float((b - 5.0).abs().max()) > 0                  # the parameter did move


@pytest.mark.parametrize("momentum", [False, True])
@pytest.mark.parametrize("error", ["goal", "rowwise"])
def test_fused_2d_step_over_a_pool_source_is_captured_and_equals_the_generic_step(error, momentum):
    steps = 12
    runs = _step_runs(error, momentum, _pool_fields(4099, wavelengths=[550.0]), steps)
    _check_step_runs(runs, steps)
    # the ray sets of the last (replayed) step, cut lazily, belong to the last draw
    eng, source = runs["graph"][3]["engine"], runs["graph"][3]["source"]
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].long()
    assert fin["y_end"].shape == ids.shape and ids.shape[0] > 0
    assert torch.equal(fin["rank"], source["rank"][ids])


def test_fused_2d_step_over_a_pool_of_three_wavelengths_follows_every_draw():
    """"index" mode, several wavelengths: the per-ray n(lambda) table is made from the rows of every
    draw (inside the captured step: the wavelength column is a gather through them).  No jitter
    here and a pool of three wavelengths whose rays are otherwise symmetric would still change the
    error from step to step only through n(lambda) and the drawn heights; a table that stayed that
    of the captured draw would separate the replayed run from the generic one."""
    steps = 10
    runs = _step_runs("rowwise", False, _pool_fields(4099, wavelengths=[450.0, 550.0, 650.0]),
                      steps, seed=35)
    _check_step_runs(runs, steps)
    eng, source = runs["graph"][3]["engine"], runs["graph"][3]["source"]
    assert eng._reaction()[0]                                # "index" mode
    assert len(set(source["wavelength"].tolist())) == 3
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].long()
    assert torch.equal(fin["wavelength"], source["wavelength"][ids])
    # the table the replayed step traced with is the one of its own draw
    n_table = eng._table_cache[1]
    want = eng.optical_system.material_table(source["wavelength"])
    assert torch.equal(n_table, want)


# ------------------------------------------------------------------------- 7. invalidation
def test_clear_from_samples_and_sample_count_drop_what_was_made_before():
    d = _dist()
    d.seed(3)
    src = _source(_pool_fields(4099), 8000)
    old = src._fields.ray_block(torch.float32)
    old_rows = src._fields.rows()
    program = src._dev_program[1]
    assert src._dev_buffers and src._dev_views and src._pool_records is not None
    assert tuple(src._pool_records.shape) == (4099, 4)
    src.clear()
    assert not src and not src.device_mode and src._pool_records is None and src._pool_fields == {}
    assert all(name not in src.__dict__ for name in ("_dev_buffers", "_dev_views", "_dev_program"))
    fields = _pool_fields(3001, seed=4)
    src.from_samples([fields])
    assert src.device_mode and src._fields.n_rays == 8000
    blk = src._fields.ray_block(torch.float32)
    assert blk is not old and src._dev_program[1] is not program
    rows = src._fields.rows()
    assert rows is not old_rows and int(rows.max()) < 3001
    rec = torch.stack([torch.as_tensor(fields[g]) for g in GEO2], dim=1).to(DEV)
    assert torch.equal(blk, rec[rows.long()].t().float())
    # another pool straight over the old one
    fields2 = _pool_fields(2003, seed=5)
    src.from_samples([fields2])
    assert "_dev_buffers" not in src.__dict__ or not src._dev_buffers
    rec2 = torch.stack([torch.as_tensor(fields2[g]) for g in GEO2], dim=1).to(DEV)
    rows2 = src._fields.rows()
    assert int(rows2.max()) < 2003
    assert torch.equal(src._fields.ray_block(torch.float64), rec2[rows2.long()].t())
    # another sample_count: a block of the new size, another program
    ident = src._fields.identity
    src.sample_count = 5001
    src.update()
    assert src._fields.n_rays == 5001 and src._fields.identity != ident
    assert src._fields.ray_block(torch.float64).shape == (4, 5001)
    assert src["tag"].shape == (5001, 2) and src._fields.rows().shape == (5001,)
    # other sigmas: another program, the jitter shows
    ident = src._fields.identity
    src.end_perturbation = (0.0, 1e-2)
    src.update()
    assert src._fields.identity != ident
    moved = src["y_end"] - rec2[src._fields.rows().long(), 3]
    assert 5e-3 < float(moved.std()) < 2e-2
    assert torch.equal(src["x_end"], rec2[src._fields.rows().long(), 2])


# ------------------------------------------------------------------------------- 8. example
@pytest.mark.parametrize("host", [False, True])
def test_optimize_arc_pool_source_example_runs_in_both_modes(host):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "optimize_arc.py"), "--pool-source",
           "--rays", "4096", "--steps", "5"] + (["--host"] if host else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["device_mode"] is (not host)
    assert res["rays"] == 4096 and res["steps"] == 5 and res["ms_per_step"] > 0
    assert res["pool_rays"] > 8192                           # the finished rays of stage 1
    assert math.isfinite(res["error_first"]) and math.isfinite(res["error_last"])
    assert res["error_last"] < res["error_first"], res       # the error decreases
    assert res["graph_replayed"] is (not host) and (res["graph_replays"] > 0) is (not host)
