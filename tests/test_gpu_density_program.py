"""The density points program (TFRT_PTS_DENSITY: csrc/density_map.h inside eval_points, reached
through tfrt_points_generate, tfrt_source3d_generate, tfrt_source3d_order and the fused optimiser
step) value by value against tests/density_reference.py: Philox4x32-10 restated in numpy, pushed
through scipy's interp1d restated as a search (tests/test_density_reference_host.py holds that
restatement to ``ArbitraryDistribution.__call__`` bit for bit, and shows that no sample of these
inputs sits on a cell edge or a knot).  Every sample is compared: float64 outputs at rtol = 0,
atol = 1e-13, the bound of tests/test_gpu_source_programs_exact.py -- coordinates stay within about
10 -- and state-dtype blocks bit for bit.  Every comparison prints its largest difference."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import sources as osources
import density_reference as dr
import source_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 1e-13
GEO = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
WAVELENGTH = np.array([575.0])
BADARG = -1                         # TFRT_E_BADARG


def _dist():
    import tfrt.distributions as d
    return d


def _np(t):
    return t.detach().cpu().numpy()


def _close(got, want, what):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"{what}: max |device - reference| = {err:.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, err_msg=str(what))


def _attach(d, dist, t):
    return d.BasePointTransformation(dist, rotation=t.get("quat"), translation=t.get("shift"),
                                     scale=t.get("scale"))


def _make(d, name, n, ranked, **kw):
    base, rank = dr.distributions(name)
    kw.setdefault("conserve_etendue", False)
    return d.ArbitraryBasePoints(base, n, rank_distribution=rank if ranked else None, **kw)


# ---------------------------------------------------------- 1. the distribution's properties
def _compare_properties(dist, name, ranked, transformed, epoch, n, **ref_kw):
    pts, a0, a1 = (a[:n] for a in dr.case_reference(name, ranked, transformed, epoch, **ref_kw))
    got = dist.points
    assert got.is_cuda
    _close(got, pts if transformed else np.ascontiguousarray(pts[:, 1:]), (name, transformed, epoch, n, "points"))
    if ranked:
        _close(dist.ranks, np.stack([a0, a1], axis=1), (name, transformed, epoch, n, "ranks"))
    else:
        assert dist.ranks is None


@pytest.mark.parametrize("n", dr.COUNTS)
@pytest.mark.parametrize("transformed", [False, True])
@pytest.mark.parametrize("ranked", [False, True])
@pytest.mark.parametrize("name", dr.GPU_CASES)
def test_points_and_ranks_are_philox_pushed_through_the_reference_search(name, ranked, transformed, n):
    d = _dist()
    d.seed(sr.SEED)
    filler = d.RandomUniformCircle(3, 1.0)                  # (takes stream 1: ours is stream 2)
    dist = _make(d, name, n, ranked)
    assert dist.__dict__.get("_device_active") and dist._stream_id == sr.STREAM
    _compare_properties(dist, name, ranked, False, 1, n)
    assert int(dist._epoch_dev) == 1
    if transformed:
        _attach(d, dist, sr.TRANSFORMATION)
        _compare_properties(dist, name, ranked, False, 1, n)     # in effect with the next update
    dist.update()
    _compare_properties(dist, name, ranked, transformed, 2, n)
    assert int(dist._epoch_dev) == 2
    del filler


def test_tables_are_uploaded_once_and_the_program_is_cached():
    d = _dist()
    d.seed(sr.SEED)
    dist = _make(d, "array12", 64, True)
    pg = dist.program()
    tables = dist._program_cache[3]
    assert np.array_equal(_np(tables[0]), dr.pack(dr.case_tables("array12")[0]))
    assert np.array_equal(_np(tables[1]), dr.pack(dr.case_tables("array12")[1]))
    assert int(pg.kind) == dr.DENSITY and (int(pg.x_count), int(pg.y_count)) == (12, 12)
    dist.update()
    assert dist.program() is pg and dist._program_cache[3] is tables
    dist.rank_scale_factor = 2.0                             # part of the key: a new program,
    pg2 = dist.program()
    assert pg2 is not pg and float(pg2.rank_scale) == 2.0
    assert dist._program_cache[3][0] is tables[0]            # the same uploaded tables


def test_enforce_etendue_reads_back_once_and_scales_the_ranks():
    d = _dist()
    d.seed(sr.SEED)
    filler = d.RandomUniformCircle(3, 1.0)
    n = 1000
    dist = _make(d, "gauss64", n, True, conserve_etendue=True)
    assert dist.__dict__.get("_device_active")
    pts, a0, a1 = dr.case_reference("gauss64", True, False, 1)
    want = float(np.linalg.norm(pts[:, 1:], axis=1).mean() / np.linalg.norm(np.stack([a0, a1], 1), axis=1).mean())
    assert abs(dist.rank_scale_factor - want) <= 1e-12 * want
    _close(dist.ranks, want * np.stack([a0, a1], axis=1), "ranks after enforce_etendue")
    dist.update()
    pts, a0, a1 = dr.case_reference("gauss64", True, False, 2)
    _close(dist.ranks, want * np.stack([a0, a1], axis=1), "ranks of the next draw")
    del filler


def test_without_auto_reroll_only_the_first_update_and_reroll_step_the_epoch():
    d = _dist()
    d.seed(sr.SEED)
    filler = d.RandomUniformCircle(3, 1.0)
    dist = _make(d, "callable53", 65, True, auto_reroll=False)
    _compare_properties(dist, "callable53", True, False, 1, 65)
    for _ in range(2):
        dist.update()
        _compare_properties(dist, "callable53", True, False, 1, 65)
        assert int(dist._epoch_dev) == 1
    dist.reroll()
    dist.update()
    _compare_properties(dist, "callable53", True, False, 2, 65)
    assert int(dist._epoch_dev) == 2
    del filler


def test_other_rank_limits_and_set_device_random_keep_the_host_path():
    d = _dist()
    base, rank = dr.distributions("array12")
    other = d.ArbitraryDistribution(np.ones((12, 12)), ((-0.5, 1.5), (2.0, 3.0 + 1e-9)))
    assert not d.ArbitraryBasePoints(base, 10, rank_distribution=other, conserve_etendue=False) \
        .__dict__.get("_device_active")
    d.set_device_random(False)
    try:
        d.seed(4)
        dist = d.ArbitraryBasePoints(base, 100, rank_distribution=rank, conserve_etendue=False)
        assert not dist.__dict__.get("_device_active")
        d.seed(4)
        t, _ = dr.case_tables("array12")
        bx = d._uniform(100, t.x_min, t.x_max).cpu().numpy()
        by = d._uniform(100, t.y_min, t.y_max).cpu().numpy()
        assert np.array_equal(_np(dist.points), np.stack(base(bx, by), 1))
        assert np.array_equal(_np(dist.ranks), np.stack(rank(bx, by), 1))
    finally:
        d.set_device_random(True)


# -------------------------------------------------------------------- 2. the C ABI
def _program(name, ranked, transformed, count, seed, stream, epoch_tensor, rank_scale=0.75):
    """A tfrt_points_program by hand, from the reference's numbers; (program, what it points at)."""
    from tensorflowraytrace_amd import _lib
    t, rt = dr.case_tables(name)
    tables = [torch.from_numpy(dr.pack(t)).to(DEV), torch.from_numpy(dr.pack(rt)).to(DEV)]
    pg = _lib.PointsProgram()
    pg.kind, pg.stream, pg.count, pg.table = dr.DENSITY, stream, count, None
    for k, v in enumerate((t.x_min, t.x_max, t.y_min, t.y_max)):
        pg.p[k] = v
    tr = sr.transformation(transformed)
    pg.has_scale = pg.has_quat = pg.has_shift = 1 if transformed else 0
    for k in range(3):
        pg.scale[k] = tr["scale"][k] if transformed else 0.0
        pg.shift[k] = tr["shift"][k] if transformed else 0.0
    for k in range(4):
        pg.quat[k] = tr["quat"][k] if transformed else 0.0
    pg.seed = seed
    pg.epoch = epoch_tensor.data_ptr()
    pg.x_count, pg.y_count = t.x_count, t.y_count
    pg.density = tables[0].data_ptr()
    pg.rank_density = tables[1].data_ptr() if ranked else None
    pg.rank_scale = rank_scale
    return pg, tables


@pytest.mark.parametrize("name", dr.GPU_CASES)
def test_key_and_counter_edges_through_the_c_abi(name):
    """The seed's high word is set and the stream XORs into it; the epoch's high word is set (written
    into the device counter directly); samples are read through `first` and an index, with
    point_columns 3 and 2, and with each output NULL in turn."""
    from tensorflowraytrace_amd import _lib, ops
    transformed = name != "array12"
    epoch = torch.tensor([sr.ABI_EPOCH], dtype=torch.int64, device=DEV)
    assert sr.ABI_SEED >> 32 and sr.ABI_EPOCH >> 32
    pg, keep = _program(name, True, transformed, sr.ABI_COUNT, sr.ABI_SEED, sr.ABI_STREAM, epoch)
    first, n = sr.ABI_FIRST, sr.ABI_N
    ref = dr.case_reference(name, True, transformed, sr.ABI_EPOCH, seed=sr.ABI_SEED,
                            stream=sr.ABI_STREAM, count=n, first=first, rank_scale=0.75)
    assert np.abs(ref[1]).max() > 0.1
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).int()
    index = perm.to(DEV)
    assert int(perm.max()) + first < sr.ABI_COUNT
    pick = perm.long().numpy()
    for idx, rows in ((index, pick), (None, np.arange(n))):
        for cols in (3, 2):
            pts, a0, a1 = ops.points_generate(pg, n, first=first, index=idx, columns=cols,
                                              want_aux=True, device=DEV)
            want = ref[0][rows] if cols == 3 else np.ascontiguousarray(ref[0][rows][:, 1:])
            _close(pts, want, (name, "points", cols, idx is not None))
            _close(a0, ref[1][rows], (name, "aux0", cols))
            _close(a1, ref[2][rows], (name, "aux1", cols))
    L = _lib.lib()
    want = (ref[0][pick], ref[1][pick], ref[2][pick])
    for absent in range(3):
        bufs = [torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
                for shape in ((n, 3), (n,), (n,))]
        ptrs = [None if k == absent else ctypes.c_void_p(b.data_ptr()) for k, b in enumerate(bufs)]
        rc = L.tfrt_points_generate(ctypes.byref(pg), ctypes.c_void_p(index.data_ptr()), first, n,
                                    ptrs[0], 3, ptrs[1], ptrs[2], ops._stream(index))
        assert rc == 0
        torch.cuda.synchronize()
        for k, b in enumerate(bufs):
            if k == absent:
                assert bool(torch.isnan(b).all())
            else:
                _close(b, want[k], (name, "absent", absent, "output", k))
    # without rank tables the two numbers are 0
    plain, keep2 = _program(name, False, transformed, sr.ABI_COUNT, sr.ABI_SEED, sr.ABI_STREAM, epoch)
    pts, a0, a1 = ops.points_generate(plain, n, first=first, columns=3, want_aux=True, device=DEV)
    _close(pts, ref[0], (name, "points without ranks"))
    assert not bool(a0.any()) and not bool(a1.any())
    assert int(epoch) == sr.ABI_EPOCH                       # (read, never written)
    del keep, keep2


def test_invalid_density_programs_are_refused_before_any_launch():
    from tensorflowraytrace_amd import _lib, ops
    L = _lib.lib()
    epoch = torch.ones(1, dtype=torch.int64, device=DEV)
    out = torch.full((8, 3), float("nan"), dtype=torch.float64, device=DEV)

    def rc_of(change):
        pg, keep = _program("array12", True, False, 8, 1, 1, epoch)
        change(pg)
        rc = L.tfrt_points_generate(ctypes.byref(pg), None, 0, 8, ctypes.c_void_p(out.data_ptr()), 3,
                                    None, None, ops._stream(out))
        sp = _lib.Source3DProgram()
        sp.kind, sp.n_rays, sp.a, sp.b = _lib.SRC_APERTURE, 8, pg, pg
        rays = L.tfrt_source3d_generate(ctypes.byref(sp), None, 0, 8, _lib.F64, None, 0,
                                        ctypes.c_void_p(out.data_ptr()), 8, ops._stream(out))
        torch.cuda.synchronize()
        del keep
        return rc, rays

    def setp(k, v):
        def change(pg):
            pg.p[k] = v
        return change

    changes = {"no tables": lambda pg: setattr(pg, "density", None),
               "no epoch": lambda pg: setattr(pg, "epoch", None),
               "x_count 0": lambda pg: setattr(pg, "x_count", 0),
               "y_count -1": lambda pg: setattr(pg, "y_count", -1),
               "x_max == x_min": setp(1, -0.5), "x_max < x_min": setp(1, -1.0),
               "y_max == y_min": setp(3, 2.0), "NaN limit": setp(0, float("nan")),
               "infinite limit": setp(3, float("inf")),
               "a kind past the last": lambda pg: setattr(pg, "kind", 6)}
    for what, change in changes.items():
        assert rc_of(change) == (BADARG, BADARG), what
    assert bool(torch.isnan(out).all())                     # nothing was launched
    assert rc_of(lambda pg: None)[0] == 0


# ------------------------------------------------------------------------ 3. rays
N = dr.N


def _aperture(d, name, transformed=True):
    """Density start points (stream 1) and RandomUniformCircle end points (stream 2)."""
    import tfrt.sources as sources
    a = _make(d, name, N, True)
    if transformed:
        _attach(d, a, sr.TRANSFORMATION)
    case = sr.POINT_CASES["circle"]
    b = case["make"](d.RandomUniformCircle, N)
    _attach(d, b, sr.TRANSFORMATION_B)
    src = sources.AperatureSource(3, a, b, list(WAVELENGTH), dense=False,
                                  extra_fields={"goal": ("start_point", a, "ranks")})

    def want(epoch):
        start, a0, a1 = dr.case_reference(name, True, transformed, epoch, seed=sr.SOURCE_SEED, stream=1)
        u0, u1 = sr.philox_uv(sr.SOURCE_SEED, 2, epoch, N)
        end = sr.points(case["kind"], case["params"], u0, u1, **sr.TRANSFORMATION_B)[0]
        return osources.aperature_source(start, end, WAVELENGTH, False), np.stack([a0, a1], axis=1)
    return src, (a, b), want


@pytest.mark.parametrize("name", dr.GPU_CASES)
def test_rays_are_the_oracles_assembly_of_the_reference_points(name):
    """The source's constructor updates its distributions (epoch 2: the transformations are in
    effect); update() makes epoch 3.  The float32 state block is the reference rounded once."""
    from tensorflowraytrace_amd import _lib, ops
    d = _dist()
    d.seed(sr.SOURCE_SEED)
    src, inputs, want = _aperture(d, name)
    assert src._device_program() is not None
    assert [x._stream_id for x in inputs] == [1, 2]
    sp = src._dev_program[1]
    assert int(sp.a.kind) == _lib.PTS_DENSITY and int(sp.b.kind) == _lib.PTS_CIRCLE
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1)).int().to(DEV)
    for epoch in sr.SOURCE_EPOCHS:
        fields, goal = want(epoch)
        assert all(int(x._epoch_dev) == epoch for x in inputs)
        block = np.stack([np.ascontiguousarray(fields[f]) for f in GEO])
        for dt in (torch.float32, torch.float64):
            rays, fl = ops.source3d_generate(sp, N, dtype=dt, fields=True, device=DEV)
            _close(fl, block, (name, epoch, "fields"))
            assert torch.equal(rays, fl.to(dt))              # rounded once
            if dt == torch.float32:
                assert np.array_equal(_np(rays), block.astype(np.float32)), "state block, bit for bit"
        for f in GEO:
            _close(src[f], np.ascontiguousarray(fields[f]), (name, epoch, f))
        # the goal rows: the whole set, and made in a permuted view's own order
        _close(src["goal"], goal, (name, epoch, "goal"))
        pv = src._fields.permuted(perm)
        _close(pv["goal"], goal[perm.long().cpu().numpy()], (name, epoch, "goal, permuted"))
        assert torch.equal(pv.ray_block(torch.float64)[1], src["y_start"][perm.long()])
        src.update()


# ----------------------------------------------------------------------- 4. the order
@pytest.mark.parametrize("name", dr.GPU_CASES)
def test_order_keys_belong_to_the_rays_that_are_generated(name):
    """tfrt_source3d_order over the program returns a permutation: the stable argsort of its keys.
    The keys come from a float32 evaluation of the program; the search and the cell of this kind run
    in float64 inside it, so they are the keys of the very points tfrt_points_generate writes: the
    same entry point over a second program, whose start points are those generated points as a
    TFRT_PTS_TABLE (rounded to float32 where the first program rounds its own), hands out the same
    keys, bit for bit.  A cell chosen in float32 takes another y curve for some samples and the keys
    part.  (The keys are not those tfrt_ray_order makes for the generated block, for no kind: that
    entry point spans its key grid over the extents of all rays, the program's over 256 sampled rays
    widened by 1/16 -- tfrt_order.hip, tests/test_gpu_source_programs.py.)"""
    from tensorflowraytrace_amd import _lib, ops
    d = _dist()
    d.seed(sr.SOURCE_SEED)
    src, inputs, want = _aperture(d, name, transformed=False)
    assert src._device_program() is not None
    sp = src._dev_program[1]
    assert int(sp.a.kind) == _lib.PTS_DENSITY and not int(sp.a.has_shift)
    perm, keys = ops.source3d_order(sp, N, device=DEV, stable=True, return_keys=True)
    assert perm.dtype == torch.int32 and perm.shape == (N,)
    ku = _np(keys).view(np.uint32)
    assert np.array_equal(np.sort(_np(perm)), np.arange(N))
    assert np.array_equal(_np(perm), np.argsort(ku, kind="stable").astype(np.int32))
    assert len(np.unique(ku)) >= N // 64
    points = ops.points_generate(sp.a, N, columns=3, device=DEV)[0]
    _close(points, dr.case_reference(name, True, False, 2, seed=sr.SOURCE_SEED, stream=1)[0], "table")
    table = _lib.Source3DProgram.from_buffer_copy(sp)
    table.a = _lib.PointsProgram()
    table.a.kind, table.a.count, table.a.table = _lib.PTS_TABLE, N, points.data_ptr()
    perm_t, keys_t = ops.source3d_order(table, N, device=DEV, stable=True, return_keys=True)
    same = int((keys == keys_t).sum())
    print(f"{name}: {same} of {N} keys equal those of the generated points")
    assert torch.equal(keys, keys_t) and torch.equal(perm, perm_t)
    fast, keys_fast = ops.source3d_order(sp, N, device=DEV, stable=False, return_keys=True)
    assert torch.equal(keys_fast, keys)
    pf = _np(fast).astype(np.int64)
    assert np.array_equal(np.sort(pf), np.arange(N))
    assert bool((np.diff(ku[pf].astype(np.int64)) >= 0).all())


# ------------------------------------------------------------------- 5. the fused step
N_STEP = 4096


def _optimizers(seed):
    import importlib.util
    import os
    import tfrt.optimizer as optimizer
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples",
                        "illumination.py")
    spec = importlib.util.spec_from_file_location("examples_illumination", path)
    illumination = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(illumination)
    d = _dist()
    out = {}
    for mode in ("generic", "graph"):
        d.seed(seed)
        kw = dict(coherent=False) if mode == "generic" else {}
        s = illumination.build(N_STEP, illumination.COARSEST_EDGE, rowwise=(mode == "graph"),
                               ray_dtype=torch.float64, **kw)
        opt = optimizer.SGD_Optimizer(s["engine"], s["lens"].parameters, s["error_function"], 3,
                                      learning_rate=1e-4, grad_clip=1e9,
                                      fused=False if mode == "generic" else "auto",
                                      graph="auto" if mode == "graph" else False, speculative=False)
        opt.suppress_warnings = True
        out[mode] = (opt, s)
    return out


def test_fused_step_over_density_rays_is_captured_and_equals_the_generic_step():
    """examples/illumination.py at its coarsest mesh: the goal rides along as the ranks.  The fused
    step draws the source in place, orders it and replays one launch graph; the generic step traces
    the same draws (same seed, same streams, the same device programs) in natural order through
    torch autograd.  Tolerances: those of tests/test_gpu_source_programs.py for device-made sources."""
    runs = _optimizers(seed=33)
    steps = 9
    errs, params = {}, {}
    for mode, (opt, s) in runs.items():
        assert s["start_points"].__dict__.get("_device_active")
        assert s["source"]._device_program() is not None
        errs[mode] = [float(opt.single_step(None)) for _ in range(steps)]
        params[mode] = [p.detach().cpu().clone() for p in s["lens"].parameters]
    fs = runs["graph"][0]._fused_step
    assert fs is not None and fs.capture_error is None, fs.capture_error
    assert fs.graph_replays > 0 and fs.graph_replays >= steps - 5
    assert len(set(errs["generic"])) == steps               # a new draw every step
    print("errors, generic:", errs["generic"], "graph:", errs["graph"])
    np.testing.assert_allclose(errs["graph"], errs["generic"], rtol=1e-10, atol=0)
    for a, b in zip(params["graph"], params["generic"]):
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())
    assert float(max(p.abs().max() for p in params["graph"])) > 0.0
    # the ray sets of the last (replayed) step, cut lazily, carry the goal of the last draw
    opt, s = runs["graph"]
    eng = s["engine"]
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].long()
    assert ids.numel() > N_STEP // 2
    assert torch.equal(fin["goal"], s["source"]["goal"][ids])
