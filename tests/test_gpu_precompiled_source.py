"""PrecompiledSource made on the device (csrc/tfrt_source.hip, TFRT_SRC_POOL; tfrt/sources.py:
1099-1358): a stored pool of rays, re-sampled with replacement and jittered by a normal perturbation
of the end points at every update.  The reference draws with tf.random.uniform(maxval=..., int32) /
tf.random.normal, unseeded; here the rows and normals come from the counter-based generator, so
parity is the distribution (tolerances derived from the sample size), the assembly of the rays
(exact: a ray IS its pool row), and that nothing else about a trace or an optimiser step depends on
how the rays were made."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
E_BADARG = -1


def _dist():
    import tfrt.distributions as d
    return d


def _pool_fields(n, seed=0, wavelengths=None):
    """n distinct rays of a bundle (object disc at x = -10 to an aperture at x = 0), a distinct
    wavelength each (or drawn from ``wavelengths``), the start points as ``object_coords`` and a
    2-column field."""
    rng = np.random.default_rng(seed)

    def disc(r):
        rr, th = r * np.sqrt(rng.uniform(size=n)), rng.uniform(0.0, 2 * math.pi, size=n)
        return rr * np.cos(th), rr * np.sin(th)

    ys, zs = disc(0.2)
    ye, ze = disc(0.8)
    ramp = np.arange(n, dtype=np.float64) / n
    f = {"x_start": -10.0 + 1e-3 * ramp, "y_start": ys, "z_start": zs,
         "x_end": 1e-3 * ramp, "y_end": ye, "z_end": ze}
    f["wavelength"] = (np.linspace(450.0, 650.0, n) if wavelengths is None
                       else np.asarray(wavelengths, dtype=np.float64)[rng.integers(0, len(wavelengths), n)])
    f["object_coords"] = np.stack([f["x_start"], ys, zs], axis=1)
    f["tag"] = np.stack([np.arange(n, dtype=np.float64), -0.5 * np.arange(n, dtype=np.float64)], axis=1)
    return f


def _source(fields, sample_count, **kw):
    import tfrt.sources as sources
    src = sources.PrecompiledSource(3, sample_count=sample_count, **kw)
    src.from_samples([fields])
    assert src.device_mode and isinstance(src._fields, sources.PoolRaySet)
    return src


def _dev(fields):
    return {k: torch.as_tensor(v).to(DEV) for k, v in fields.items()}


# ------------------------------------------------------------------------------ one draw

def test_every_ray_is_its_pool_row_in_every_form_the_set_hands_out():
    d = _dist()
    d.seed(5)
    n_pool, n = 65536, 1 << 20
    fields = _pool_fields(n_pool)
    pool = _dev(fields)
    records = torch.stack([pool[g] for g in GEO], dim=1)             # (n_pool, 6)
    src = _source(fields, n)
    rs = src._fields
    assert set(rs.keys()) == set(fields.keys()) and rs.n_rays == n
    rows = rs.rows()
    assert rows.dtype == torch.int32 and rows.shape == (n,)
    rl = rows.long()
    assert int(rl.min()) >= 0 and int(rl.max()) < n_pool
    got = torch.stack([src[g] for g in GEO])                         # (6, n) float64
    assert got.dtype == torch.float64
    assert torch.equal(got, records[rl].t())                         # bit for bit
    for f in ("wavelength", "object_coords", "tag"):
        assert torch.equal(src[f], pool[f][rl]), f
    for dt in (torch.float32, torch.float64):
        blk = rs.ray_block(dt)
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
    # the same draw until update(), another one after it -- in place
    assert src._fields.rows() is rows and torch.equal(torch.stack([src[g] for g in GEO]), got)
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


def test_without_downsampling_the_device_source_is_the_pool_in_order():
    d = _dist()
    d.seed(2)
    fields = _pool_fields(5000)
    pool = _dev(fields)
    src = _source(fields, 17, do_downsample=False)
    rs = src._fields
    assert rs.n_rays == 5000
    assert torch.equal(rs.rows(), torch.arange(5000, dtype=torch.int32, device=DEV))
    for f in fields:
        assert torch.equal(src[f], pool[f]), f
    src.update()
    assert torch.equal(src["y_end"], pool["y_end"])


def test_one_wavelength_is_handed_out_as_an_expanded_scalar():
    d = _dist()
    d.seed(2)
    fields = _pool_fields(3000, wavelengths=[575.0])
    src = _source(fields, 10000)
    w = src["wavelength"]
    assert w.shape == (10000,) and w.stride(0) == 0 and float(w[0]) == 575.0
    src.update()
    assert src["wavelength"].data_ptr() == w.data_ptr()               # (the engine's table stays)


def test_rows_are_uniform_and_the_perturbation_is_normal():
    """Tolerances from the sample size n alone: five standard errors of each statistic."""
    d = _dist()
    d.seed(41)
    n_pool, n, K = 65536, 1 << 20, 256
    fields = _pool_fields(n_pool)
    pool = _dev(fields)
    s_y, s_z = 1e-2, 3e-3
    src = _source(fields, n, end_perturbation=(0.0, s_y, s_z))
    rl = src._fields.rows().long()
    counts = torch.bincount(rl // (n_pool // K), minlength=K).double()
    chi2 = float(((counts - n / K) ** 2 / (n / K)).sum())
    assert chi2 < (K - 1) + 5 * math.sqrt(2 * (K - 1)), chi2
    for f in ("x_start", "y_start", "z_start", "x_end"):             # sigma 0: the stored coordinate
        assert torch.equal(src[f], pool[f][rl]), f
    res = {}
    for f, s in (("y_end", s_y), ("z_end", s_z)):
        r = (src[f] - pool[f][rl]) / s
        assert bool(torch.isfinite(r).all())
        assert float(r.abs().max()) <= 8.6                           # Box-Muller at 53 bits
        mean, var = float(r.mean()), float(r.var(unbiased=False))
        kurt = float(((r - r.mean()) ** 4).mean()) / var ** 2
        assert abs(mean) < 5 / math.sqrt(n), (f, mean)
        assert abs(var - 1) < 5 * math.sqrt(2 / n), (f, var)
        assert abs(kurt - 3) < 5 * math.sqrt(24 / n), (f, kurt)
        res[f] = r
    corr = float((res["y_end"] * res["z_end"]).mean() - res["y_end"].mean() * res["z_end"].mean())
    corr /= float(res["y_end"].std() * res["z_end"].std())
    assert abs(corr) < 5 / math.sqrt(n), corr
    # start and end normals of one axis come from one Box-Muller pair: independent all the same
    src2 = _source(fields, n, start_perturbation=2e-3, end_perturbation=2e-3)
    rl2 = src2._fields.rows().long()
    a = (src2["y_start"] - pool["y_start"][rl2]) / 2e-3
    b = (src2["y_end"] - pool["y_end"][rl2]) / 2e-3
    assert abs(float(a.var(unbiased=False)) - 1) < 5 * math.sqrt(2 / n)
    assert abs(float((a * b).mean())) < 5 / math.sqrt(n)
    assert abs(float((a * a * b * b).mean()) - 1) < 5 * math.sqrt(8 / n)    # var(a^2 b^2) = 9 - 1
    old = src2["y_end"].clone()
    src2.update()
    assert float((src2["y_end"] - old).abs().max()) > 1e-3


@pytest.mark.parametrize("stable", [True, False])
def test_order_of_a_pool_program_is_a_permutation_made_for_the_rays_it_draws(stable):
    """tfrt_source3d_order(_cells) evaluates the program in float32 for the keys; the row is chosen
    in float64 there too, so the order is as compact over the float64 rays as tfrt_ray_order's of the
    generated block -- keys made for other rows would be as good as a random order."""
    from tensorflowraytrace_amd import ops
    d = _dist()
    d.seed(11)
    n = 300_000
    src = _source(_pool_fields(65536), n, end_perturbation=(0.0, 1e-4, 1e-4))
    rs = src._fields
    perm = rs.order(stable=stable)
    assert perm.dtype == torch.int32 and perm.shape == (n,)
    assert torch.equal(torch.sort(perm.long())[0], torch.arange(n, device=perm.device))
    block = rs.ray_block(torch.float32)
    ref = ops.ray_order(block, None)

    def spread(p):      # mean diagonal of the end-point bounding box of a wavefront's 64 rays
        yz = block[4:6, p.long()][:, :n // 64 * 64].reshape(2, -1, 64)
        ext = yz.max(dim=2)[0] - yz.min(dim=2)[0]
        return float(ext.pow(2).sum(dim=0).sqrt().mean())

    assert spread(perm) <= 1.1 * spread(ref)
    g = torch.Generator().manual_seed(0)
    assert spread(perm) < 0.2 * spread(torch.randperm(n, generator=g).to(perm.device))
    src.update()
    perm2 = src._fields.order(stable=stable)
    assert not torch.equal(perm, perm2)
    assert torch.equal(torch.sort(perm2.long())[0], torch.arange(n, device=perm.device))


@pytest.mark.parametrize("stable", [True, False])
def test_the_float32_keys_of_a_pool_program_are_those_of_the_rows_it_draws(stable):
    """The keys of a down-sampling pool program against the keys of a program that does not sample:
    its pool IS the drawn rows, in order.  Both are made by the same float32 evaluation of the same
    rays in the same frame, so they agree bit for bit -- unless the key evaluation picked its rows
    differently from tfrt_source3d_pool_rows (a float32 product u * pool_count names another row for
    about pool_count * 2^-24 of the rays: some four thousand of these)."""
    from tensorflowraytrace_amd import ops
    d = _dist()
    d.seed(19)
    n_pool, n = 65536, 1 << 20
    fields = _pool_fields(n_pool)
    src = _source(fields, n)
    rs = src._fields
    rl = rs.rows().long().cpu().numpy()
    perm, keys = ops.source3d_order(src._dev_program[1], n, device=DEV, stable=stable, return_keys=True)
    drawn = _source({g: fields[g][rl] for g in GEO}, 1, do_downsample=False)
    assert drawn._fields.n_rays == n
    perm2, keys2 = ops.source3d_order(drawn._dev_program[1], n, device=DEV, stable=stable,
                                      return_keys=True)
    assert len(torch.unique(keys)) > n_pool // 2               # (the keys tell the rows apart)
    assert torch.equal(keys, keys2)
    if stable:
        assert torch.equal(perm, perm2)


def test_clear_and_from_samples_drop_what_was_made_from_the_old_pool():
    d = _dist()
    d.seed(3)
    src = _source(_pool_fields(5000), 8000)
    old = src._fields.ray_block(torch.float32)
    assert src._dev_buffers and src._dev_views and src._pool_records is not None
    src.clear()
    assert not src and not src.device_mode and src._pool_records is None and src._pool_fields == {}
    assert all(name not in src.__dict__ for name in ("_dev_buffers", "_dev_views", "_dev_program"))
    fields = _pool_fields(3000, seed=4)
    src.from_samples([fields])
    assert src.device_mode and src._fields.n_rays == 8000
    blk = src._fields.ray_block(torch.float32)
    assert blk is not old
    rec = torch.stack([torch.as_tensor(fields[g]) for g in GEO], dim=1).to(DEV)
    assert torch.equal(blk, rec[src._fields.rows().long()].t().float())


def test_the_c_abi_refuses_bad_pool_programs_before_any_launch():
    from tensorflowraytrace_amd import _lib, ops
    d = _dist()
    d.seed(1)
    n_pool, n = 4096, 10000
    fields = _pool_fields(n_pool)
    src = _source(fields, n, end_perturbation=(0.0, 1e-3, 0.0))
    good = src._dev_program[1]
    L = _lib.lib()
    rays = torch.zeros((6, n), dtype=torch.float32, device=DEV)
    rows = torch.zeros(n, dtype=torch.int32, device=DEV)
    perm = torch.zeros(n, dtype=torch.int32, device=DEV)
    wsb = L.tfrt_ray_order_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    stream = ops._stream(rays)

    def calls(sp, count=n):
        return (L.tfrt_source3d_generate(sp, None, 0, count, _lib.F32, rays.data_ptr(), n, None, 0, stream),
                L.tfrt_source3d_pool_rows(sp, None, 0, count, rows.data_ptr(), stream),
                L.tfrt_source3d_order(sp, 0, count, None, 0, None, perm.data_ptr(), None, ws.data_ptr(),
                                      wsb, stream),
                L.tfrt_source3d_order_cells(sp, 0, count, None, 0, None, perm.data_ptr(), None,
                                            ws.data_ptr(), wsb, stream))

    def variant(**changes):
        sp = _lib.Source3DProgram.from_buffer_copy(good)
        for k, v in changes.items():
            if isinstance(v, tuple):
                for q, x in enumerate(v):
                    getattr(sp, k)[q] = x
            else:
                setattr(sp, k, v)
        return sp

    assert calls(variant()) == (0, 0, 0, 0)
    bad = [variant(pool=None), variant(pool_count=0), variant(pool_count=-5),
           variant(pool_count=1 << 31), variant(sigma_end=(0.0, -1e-3, 0.0)),
           variant(sigma_start=(float("nan"), 0.0, 0.0)), variant(sigma_end=(0.0, 0.0, float("inf"))),
           variant(pool_epoch=None),                                              # samples and perturbs
           variant(pool_epoch=None, sigma_end=(0.0, 0.0, 0.0)),                   # samples
           variant(pool_epoch=None, pool_downsample=0, n_rays=n_pool),            # perturbs
           variant(pool_downsample=0)]                                            # n_rays != pool_count
    for sp in bad:
        assert calls(sp) == (E_BADARG,) * 4
    torch.cuda.synchronize()
    # the rows of another kind of program do not exist; nothing sampled, nothing perturbed: no counter
    assert L.tfrt_source3d_pool_rows(variant(kind=_lib.SRC_APERTURE), None, 0, n, rows.data_ptr(),
                                     stream) == E_BADARG
    plain = variant(pool_epoch=None, pool_downsample=0, n_rays=n_pool, sigma_end=(0.0, 0.0, 0.0))
    assert calls(plain, n_pool) == (0, 0, 0, 0)
    want = torch.stack([torch.as_tensor(fields[g]) for g in GEO]).float().to(DEV)
    assert torch.equal(rays[:, :n_pool], want)
    assert calls(plain, n_pool + 1)[:2] == (E_BADARG, E_BADARG)                   # past the last ray


# ------------------------------------------------------------------------------ traces and steps

def _lens(n_hint, **kw):
    from test_gpu_engine import _build_lens
    return _build_lens(n_hint, **kw)


def test_trace_of_a_device_made_pool_source_equals_the_trace_of_its_rays_as_plain_tensors():
    import tfrt.sources as sources
    d = _dist()
    d.seed(21)
    fields = _pool_fields(30000)
    del fields["tag"]
    eng, system, lens, target, _ = _lens(64, k=6, ray_dtype=torch.float32, compile_dead_rays=True,
                                         compile_stopped_rays=True)
    pre = _source(fields, 20000, end_perturbation=(0.0, 1e-3, 1e-3))
    system.sources = [pre]
    names = ("x_start", "y_end", "z_end", "object_coords", "wavelength")
    for _ in range(2):
        system.update()
        eng.ray_trace(4)
        assert eng._trace_perm is not None                  # ordered, from the program
        got = {c: {f: getattr(eng, c + "_rays")[f].clone() for f in names}
               for c in ("finished", "active", "dead") if bool(getattr(eng, c + "_rays"))}
        assert got["finished"]["x_start"].shape[0] > 10000
        manual = sources.ManualSource(3)
        for f in pre.keys():
            manual[f] = pre[f].clone()
        eng2, system2, *_ = _lens(64, k=6, ray_dtype=torch.float32, coherent=False,
                                  compile_dead_rays=True, compile_stopped_rays=True)
        system2.sources = [manual]
        system2.update()
        eng2.ray_trace(4)
        assert eng2._trace_perm is None
        for c, fs in got.items():
            for f, v in fs.items():
                assert torch.equal(v, getattr(eng2, c + "_rays")[f]), (c, f)


def _goal(src):
    return -src["object_coords"][:, 1:]


def _rowwise(rays):
    dy = rays["y_end"].double() + rays["object_coords"][:, 1]
    dz = rays["z_end"].double() + rays["object_coords"][:, 2]
    return torch.stack([dy ** 2, dz ** 2], dim=1)


def _optimizers(fields, n_rays, seed, kind, momentum):
    import tfrt.optimizer as optimizer
    d = _dist()
    out = {}
    for mode in ("generic", "graph"):
        d.seed(seed)
        kw = dict(coherent=False) if mode == "generic" else {}
        eng, system, lens, target, _ = _lens(64, k=5, ray_dtype=torch.float64, **kw)
        pre = _source(fields, n_rays, end_perturbation=(0.0, 1e-3, 1e-3))
        system.sources = [pre]
        system.update()
        if kind == "rowwise":
            erf = optimizer.RowwiseError(_rowwise)
        else:
            erf = optimizer.GoalError(("y_end", "z_end"), _goal,
                                      rowwise=(kind == "goal_rowwise" and mode == "graph"))
        opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=2e-5, grad_clip=1e9,
                                      fused=False if mode == "generic" else "auto",
                                      graph="auto" if mode == "graph" else False, speculative=False,
                                      apply_momentum=momentum, nesterov=True)
        opt.suppress_warnings = True
        out[mode] = (opt, eng, lens, pre)
    return out


def _compare_steps(runs, steps, momentum):
    errs, terms, params = {}, {}, {}
    for mode, (opt, eng, lens, pre) in runs.items():
        errs[mode], terms[mode] = [], []
        for _ in range(steps):
            errs[mode].append(float(opt.single_step(None, momentum=0.6 if momentum else 0.0)))
            terms[mode].append(int(float(opt.last_error_terms)))
        params[mode] = [p.detach().cpu().clone() for p in lens.parameters]
    fs = runs["graph"][0]._fused_step
    assert runs["generic"][0]._fused_step is None
    assert fs is not None and fs.capture_error is None, fs and fs.capture_error
    assert fs.graph_replays > 0 and fs.in_place
    assert runs["graph"][1]._trace_perm is not None
    assert runs["graph"][3].device_mode and runs["generic"][3].device_mode
    assert len(set(errs["generic"])) == steps               # a new draw every step
    assert terms["graph"] == terms["generic"] and min(terms["generic"]) > 0
    np.testing.assert_allclose(errs["graph"], errs["generic"], rtol=1e-10, atol=0)
    sums = {m: np.asarray(errs[m]) * np.asarray(terms[m]) for m in errs}
    np.testing.assert_allclose(sums["graph"], sums["generic"], rtol=1e-10, atol=0)
    for a, b in zip(params["graph"], params["generic"]):
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())


@pytest.mark.parametrize("momentum", [False, True])
@pytest.mark.parametrize("kind", ["goal", "goal_rowwise", "rowwise"])
def test_fused_step_over_a_pool_source_equals_the_generic_natural_order_step(kind, momentum):
    """dev/precompile_sample.py's loop: the pool is re-sampled at every step.  The fused step draws
    it in place, orders it on the device and replays one launch graph; the generic step traces the
    same draws (same seed, same streams) in natural order through torch autograd."""
    fields = _pool_fields(20000, wavelengths=[575.0])
    runs = _optimizers(fields, 12000, 33, kind, momentum)
    _compare_steps(runs, 12, momentum)
    # the ray sets of the last (replayed) step, cut lazily, belong to the last draw
    opt, eng, lens, pre = runs["graph"]
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].long()
    assert torch.equal(fin["object_coords"], pre["object_coords"][ids])


def test_fused_step_over_a_pool_of_three_wavelengths_follows_every_draw():
    """"index" mode, several wavelengths: the per-ray n(lambda) table is made from the rows of
    every draw (inside the captured step: the wavelength column is a gather through them)."""
    fields = _pool_fields(20000, wavelengths=[450.0, 550.0, 650.0])
    runs = _optimizers(fields, 12000, 35, "goal_rowwise", False)
    _compare_steps(runs, 10, False)
    opt, eng, lens, pre = runs["graph"]
    assert len(set(pre["wavelength"].tolist())) == 3
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].long()
    assert torch.equal(fin["wavelength"], pre["wavelength"][ids])


def test_two_stage_run_from_finished_rays_to_an_optimised_back_part():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import staged_trace
    d = _dist()
    d.seed(7)
    result, errors, state = staged_trace.run(ray_count=6000, steps=20, warmup=4, lens_res_scale=0.2,
                                             pool_rays=20000)
    pool = state["pool"]
    assert result["device_mode"] and pool.device_mode
    assert 15000 < pool.sampling_domain_size <= 20000          # the finished rays of stage 1
    assert set(pool.keys()) == set(staged_trace.FIELDS)
    assert len(errors) == 24 and all(np.isfinite(errors))
    first, last = np.mean(errors[:3]), np.mean(errors[-3:])
    assert last < first, (first, last)                         # its error falls
    assert float(state["lens"].parameters[0].detach().abs().max()) > 1e-5


@pytest.mark.parametrize("host", [False, True])
def test_staged_trace_example_runs_in_both_modes(host):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "staged_trace.py"), "--rays", "20000",
           "--steps", "20"] + (["--host"] if host else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["device_mode"] is (not host)
    assert res["rays"] == 20000 and res["steps"] == 20 and res["ms_per_step"] > 0
    assert math.isfinite(res["error_first"]) and math.isfinite(res["error_last"])
    if not host:
        assert res["graph_replays"] > 0
