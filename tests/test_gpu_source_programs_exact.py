"""The 3-D source programs (csrc/source_programs.h: eval_points, eval_pool, eval_ray, reached through
tfrt_points_generate, tfrt_source3d_generate, tfrt_source3d_pool_rows and tfrt_source3d_order) value
by value against tests/source_reference.py: Philox4x32-10 restated in numpy, pushed through the
reference project's formulas in float64, the rays assembled by oracle/sources.py.  Every sample is
compared (tests/test_source_reference_host.py shows on the reference alone that no sample of these
inputs sits where rounding could matter): float64 outputs at rtol = 0, atol = 1e-13 -- coordinates
stay within about 10, so that is some 50 ulp, and a wrong formula misses by many orders (largest
difference seen on an MI355X over all comparisons of this file: 2.4e-14) -- and state-dtype blocks
bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import sources as osources
import source_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PI = math.pi
ATOL = 1e-13
GEO = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
PROPERTIES = ("points", "ranks", "polar_ranks", "angles")


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


# ---------------------------------------------------------- 1. distributions, by class
def _compare_properties(dist, name, transformed, epoch, n):
    case = sr.POINT_CASES[name]
    pts, a0, a1 = (a[:n] for a in sr.case_reference(name, transformed, epoch))
    want = sr.class_properties(case["kind"], case["params"], pts, a0, a1, transformed)
    for prop in PROPERTIES:
        assert hasattr(dist, prop) == (prop in want), prop
        if prop in want:
            got = getattr(dist, prop)
            assert got.is_cuda
            _close(got, want[prop], (name, transformed, epoch, n, prop))


@pytest.mark.parametrize("n", sr.COUNTS)
@pytest.mark.parametrize("transformed", [False, True])
@pytest.mark.parametrize("name", sorted(sr.POINT_CASES))
def test_distributions_are_philox_pushed_through_the_reference_formulas(name, transformed, n):
    d = _dist()
    case = sr.POINT_CASES[name]
    d.seed(sr.SEED)
    filler = d.RandomUniformCircle(3, 1.0)                  # (takes stream 1: ours is stream 2)
    dist = case["make"](getattr(d, case["cls"]), n)
    assert dist.__dict__.get("_device_active") and dist._stream_id == sr.STREAM
    _compare_properties(dist, name, False, 1, n)
    assert int(dist._epoch_dev) == 1
    if transformed:
        _attach(d, dist, sr.TRANSFORMATION)
        _compare_properties(dist, name, False, 1, n)        # in effect with the next update
    dist.update()
    _compare_properties(dist, name, transformed, 2, n)
    assert int(dist._epoch_dev) == 2
    del filler


# -------------------------------------------------------------------- 2. the C ABI
def _points_program(name, transformed, count, seed, stream, epoch_tensor):
    """A tfrt_points_program by hand, from the reference's numbers."""
    from tensorflowraytrace_amd import _lib
    case = sr.POINT_CASES[name]
    pg = _lib.PointsProgram()
    pg.kind, pg.stream, pg.count, pg.table = case["kind"], stream, count, None
    for k, v in enumerate(case["params"]):
        pg.p[k] = v
    t = sr.transformation(transformed)
    pg.has_scale = pg.has_quat = pg.has_shift = 1 if transformed else 0
    for k in range(3):
        pg.scale[k] = t["scale"][k] if transformed else 0.0
        pg.shift[k] = t["shift"][k] if transformed else 0.0
    for k in range(4):
        pg.quat[k] = t["quat"][k] if transformed else 0.0
    pg.seed = seed
    pg.epoch = epoch_tensor.data_ptr()
    return pg


@pytest.mark.parametrize("name", sr.ABI_CASES)
def test_key_and_counter_edges_through_the_c_abi(name):
    """The seed's high word is set and the stream XORs into it; the epoch's high word is set (written
    into the device counter directly); samples are read through `first` and an index."""
    from tensorflowraytrace_amd import _lib, ops
    case = sr.POINT_CASES[name]
    transformed = name in ("circle_wedge", "hemisphere")
    epoch = torch.tensor([sr.ABI_EPOCH], dtype=torch.int64, device=DEV)
    assert sr.ABI_SEED >> 32 and sr.ABI_EPOCH >> 32
    pg = _points_program(name, transformed, sr.ABI_COUNT, sr.ABI_SEED, sr.ABI_STREAM, epoch)
    first, n = sr.ABI_FIRST, sr.ABI_N
    u0, u1 = sr.philox_uv(sr.ABI_SEED, sr.ABI_STREAM, sr.ABI_EPOCH, n, first=first)
    ref = sr.points(case["kind"], case["params"], u0, u1, **sr.transformation(transformed))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).int()
    index = perm.to(DEV)
    assert int(perm.max()) + first < sr.ABI_COUNT
    pick = perm.long().numpy()
    for idx, rows in ((index, pick), (None, np.arange(n))):
        for cols in (3, 2):
            pts, a0, a1 = ops.points_generate(pg, n, first=first, index=idx, columns=cols,
                                              want_aux=True, device=DEV)
            want = ref[0][rows] if cols == 3 else ref[0][rows][:, 1:]
            _close(pts, want, (name, "points", cols, idx is not None))
            _close(a0, ref[1][rows], (name, "aux0", cols))
            _close(a1, ref[2][rows], (name, "aux1", cols))
    # each output pointer NULL in turn: the other two are written as before
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
    assert int(epoch) == sr.ABI_EPOCH                       # (read, never written)


def test_epoch_advance_steps_eight_counters_and_the_draw_follows():
    from tensorflowraytrace_amd import ops
    base = torch.zeros(8, dtype=torch.int64, device=DEV)
    counters = [base[k:k + 1] for k in range(8)]
    assert len({c.data_ptr() for c in counters}) == 8
    for _ in range(3):
        ops.epoch_advance(counters)
    assert base.tolist() == [3] * 8
    for name in ("sphere_lambert", "circle_wedge"):
        case = sr.POINT_CASES[name]
        pg = _points_program(name, True, sr.N, sr.SEED, sr.STREAM, counters[5])
        pts, a0, a1 = ops.points_generate(pg, sr.N, columns=3, want_aux=True, device=DEV)
        ref = sr.case_reference(name, True, 3)
        _close(pts, ref[0], (name, "points at epoch 3"))
        _close(a0, ref[1], (name, "aux0 at epoch 3"))
        _close(a1, ref[2], (name, "aux1 at epoch 3"))
    assert base.tolist() == [3] * 8


# ------------------------------------------------------------------------ 3. sources
N = sr.N
WAVELENGTH = np.array([575.0])
CENTER = np.array([1.0, -2.0, 0.5])
POINT_AIM = np.array([1.0, 1.0, 0.2])
ANGULAR_CENTER = np.array([0.0, 1.0, 0.0])
ANGULAR_AIM = np.array([0.0, 0.0, 1.0])


def _input(d, name, t=None, n=N):
    case = sr.POINT_CASES[name]
    dist = case["make"](getattr(d, case["cls"]), n)
    if t is not None:
        _attach(d, dist, t)
    return dist


def _input_reference(name, stream, epoch, t=None, n=N, plane=False):
    """The points of a source's input as its class publishes them ((n, 2) for an untransformed
    planar distribution: ``plane``)."""
    case = sr.POINT_CASES[name]
    u0, u1 = sr.philox_uv(sr.SOURCE_SEED, stream, epoch, n)
    pts = sr.points(case["kind"], case["params"], u0, u1, **(t or {}))[0]
    return pts[:, 1:] if plane else pts


def _aperture(d, flag):
    import tfrt.sources as sources
    a = _input(d, "circle", sr.TRANSFORMATION)              # stream 1
    b = _input(d, "square", sr.TRANSFORMATION_B)            # stream 2
    src = sources.AperatureSource(3, a, b, list(WAVELENGTH), dense=False)

    def want(epoch):
        return osources.aperature_source(_input_reference("circle", 1, epoch, sr.TRANSFORMATION),
                                         _input_reference("square", 2, epoch, sr.TRANSFORMATION_B),
                                         WAVELENGTH, False)
    return src, (a, b), want


def _point(d, flag):
    import tfrt.sources as sources
    ang = _input(d, "sphere_lambert")                       # stream 1
    src = sources.PointSource(3, tuple(CENTER), tuple(POINT_AIM), ang, list(WAVELENGTH), dense=False,
                              start_on_center=flag, ray_length=2.5)

    def want(epoch):
        return osources.point_source_3d(CENTER, POINT_AIM, _input_reference("sphere_lambert", 1, epoch),
                                        WAVELENGTH, False, start_on_center=flag, ray_length=2.5)
    return src, (ang,), want


def _angular(d, flag):
    import tfrt.sources as sources
    base = _input(d, "square")                              # stream 1
    ang = _input(d, "sphere_uniform")                       # stream 2
    src = sources.AngularSource(3, tuple(ANGULAR_CENTER), tuple(ANGULAR_AIM), ang, base,
                                list(WAVELENGTH), dense=False, start_on_base=flag, ray_length=0.5)

    def want(epoch):
        return osources.angular_source_3d(ANGULAR_CENTER, ANGULAR_AIM,
                                          _input_reference("sphere_uniform", 2, epoch),
                                          _input_reference("square", 1, epoch, plane=True),
                                          WAVELENGTH, False, start_on_base=flag, ray_length=0.5)
    return src, (base, ang), want


SOURCES = {"aperture": (_aperture, (True,)), "point": (_point, (True, False)),
           "angular": (_angular, (True, False))}
SOURCE_CASES = [(kind, flag) for kind in sorted(SOURCES) for flag in SOURCES[kind][1]]


def _check_set(src, want, n, what):
    """Fields against the oracle's, the blocks against the fields, a shard and a permuted view
    against the whole set."""
    import tfrt.sources as sources
    rs = src._fields
    assert isinstance(rs, sources.DeviceRaySet) and rs.n_rays == n
    assert set(rs.keys()) == set(GEO) | {"wavelength"}
    for f in GEO:
        _close(src[f], np.ascontiguousarray(want[f]), (what, f))
    np.testing.assert_array_equal(_np(src["wavelength"]), want["wavelength"])
    fields = torch.stack([src[f] for f in GEO])
    for dt in (torch.float32, torch.float64):
        blk = rs.ray_block(dt)
        assert blk.shape == (6, n) and blk.dtype == dt
        assert torch.equal(blk, fields.to(dt))               # rounded once, bit for bit
    first = n // 5
    sh = rs.shard(first, first + n // 3)
    assert sh.n_rays == n // 3
    for dt in (torch.float32, torch.float64):
        assert torch.equal(sh.ray_block(dt), fields[:, first:first + n // 3].to(dt))
    assert torch.equal(sh["z_end"], fields[5, first:first + n // 3])
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).int().to(DEV)
    pv = rs.permuted(perm)
    assert torch.equal(pv.ray_block(torch.float32), fields.float()[:, perm.long()])
    assert torch.equal(pv.ray_block(torch.float64), fields[:, perm.long()])
    assert torch.equal(pv["x_end"], fields[3, perm.long()])
    return fields


@pytest.mark.parametrize("kind,flag", SOURCE_CASES)
def test_sources_are_the_oracles_assembly_of_the_reference_points(kind, flag):
    """``flag``: start_on_center / start_on_base.  The source's constructor updates its
    distributions (epoch 2: the transformations are in effect); update() makes epoch 3."""
    d = _dist()
    d.seed(sr.SOURCE_SEED)
    src, inputs, want = SOURCES[kind][0](d, flag)
    assert src._device_program() is not None
    assert [x._stream_id for x in inputs] == list(range(1, len(inputs) + 1))
    assert int(src._dev_program[1].swap) == (0 if flag else 1)
    old = None
    for epoch in sr.SOURCE_EPOCHS:
        fields = _check_set(src, want(epoch), N, (kind, flag, epoch))
        assert all(int(x._epoch_dev) == epoch for x in inputs)
        assert old is None or float((fields - old).abs().max()) > 1e-3      # a new draw
        old = fields.clone()
        src.update()


@pytest.mark.parametrize("partner", ["random", "static"])
def test_an_input_with_one_sample_is_broadcast(partner):
    """count == 1: a device-random distribution of one sample (every ray takes its sample 0), or a
    StaticUniformCircle of one point (a TABLE program)."""
    import tfrt.sources as sources
    from tensorflowraytrace_amd import _lib
    d = _dist()
    d.seed(sr.SOURCE_SEED)
    a = _input(d, "circle", sr.TRANSFORMATION)              # stream 1
    if partner == "random":
        b = _input(d, "circle", sr.TRANSFORMATION_B, n=1)   # stream 2
    else:
        b = d.StaticUniformCircle(1, 0.9)
        _attach(d, b, sr.TRANSFORMATION_B)
        b.update()
    src = sources.AperatureSource(3, a, b, list(WAVELENGTH), dense=False)
    assert src._device_program() is not None
    sp = src._dev_program[1]
    assert int(sp.b.count) == 1 and int(sp.a.count) == N and int(sp.n_rays) == N
    assert int(sp.b.kind) == (_lib.PTS_CIRCLE if partner == "random" else _lib.PTS_TABLE)
    if partner == "random":
        one = _input_reference("circle", 2, 2, sr.TRANSFORMATION_B, n=1)
    else:       # StaticUniformCircle (distributions.py:1570-1582) of one point: index 1/2
        r, theta = math.sqrt(0.5), PI * (1 + 5 ** 0.5) * 0.5
        one = np.array([[0.0, 0.9 * r * math.cos(theta), 0.9 * r * math.sin(theta)]])
        one = osources.rotate_vector_by_quaternion(sr.TRANSFORMATION_B["quat"], one) \
            + np.array(sr.TRANSFORMATION_B["shift"])
    want = osources.aperature_source(_input_reference("circle", 1, 2, sr.TRANSFORMATION),
                                     np.broadcast_to(one, (N, 3)), WAVELENGTH, False)
    fields = _check_set(src, want, N, ("broadcast", partner))
    assert bool((fields[3:] == fields[3:, :1]).all())       # one end point for every ray


# --------------------------------------------------------------------------- 4. the pool
def _pool_fields(n, seed=0):
    """n distinct rays of a bundle (object disc at x = -10 to an aperture at x = 0)."""
    rng = np.random.default_rng(seed)

    def disc(r):
        rr, th = r * np.sqrt(rng.uniform(size=n)), rng.uniform(0.0, 2 * PI, size=n)
        return rr * np.cos(th), rr * np.sin(th)

    ys, zs = disc(0.2)
    ye, ze = disc(0.8)
    ramp = np.arange(n, dtype=np.float64) / n
    return {"x_start": -10.0 + 1e-3 * ramp, "y_start": ys, "z_start": zs,
            "x_end": 1e-3 * ramp, "y_end": ye, "z_end": ze,
            "wavelength": np.linspace(450.0, 650.0, n)}


def _pool_source(fields, sample_count, **kw):
    import tfrt.sources as sources
    src = sources.PrecompiledSource(3, sample_count=sample_count, **kw)
    src.from_samples([fields])
    assert src.device_mode and isinstance(src._fields, sources.PoolRaySet)
    return src


def test_pool_rows_and_normals_are_the_stated_function_of_the_generator():
    """The draw as include/tfrt_hip.h states it: rows without exception; a coordinate whose sigma
    is 0 is the stored value bit for bit, the others the stored value plus sigma times the
    Box-Muller normal to 1e-13 (sigma <= 2e-3 and |z| <= 8.6: the normal itself to some 1e-11)."""
    d = _dist()
    seed, n_pool, n = 12345, 1000, N
    d.seed(seed)
    fields = _pool_fields(n_pool, seed=2)
    records = np.stack([fields[g] for g in GEO], axis=1)
    s_start, s_end = (0.0, 1e-3, 2e-3), (1e-3, 0.0, 5e-4)
    src = _pool_source(fields, n, start_perturbation=s_start, end_perturbation=s_end)
    sp = src._dev_program[1]
    assert int(sp.pool_seed) == seed and int(sp.pool_stream) == 1 and int(sp.pool_count) == n_pool
    assert tuple(sp.sigma_start) == s_start and tuple(sp.sigma_end) == s_end
    old = None
    for epoch in (1, 2):
        assert int(src._epoch_dev) == epoch
        numbers = [sr.philox_uv(seed, 1 + k, epoch, n) for k in range(4)]
        rows, start, end = sr.pool_rays(records, numbers, s_start, s_end, True)
        got_rows = _np(src._fields.rows())
        assert got_rows.dtype == np.int32 and np.array_equal(got_rows, rows)
        want = np.concatenate([start, end], axis=1)
        sigmas = s_start + s_end
        got = np.stack([_np(src[g]) for g in GEO], axis=1)
        for k, g in enumerate(GEO):
            if sigmas[k] == 0.0:
                assert np.array_equal(got[:, k], records[rows, k]), g       # bit for bit
            else:
                assert float(np.abs(got[:, k] - records[rows, k]).max()) > sigmas[k]
            _close(got[:, k], want[:, k], ("pool", epoch, g))
        fields64 = torch.from_numpy(got.T.copy()).to(DEV)
        for dt in (torch.float32, torch.float64):
            assert torch.equal(src._fields.ray_block(dt), fields64.to(dt))
        assert np.array_equal(_np(src["wavelength"]), fields["wavelength"][rows])
        assert old is None or not np.array_equal(old, rows)
        old = rows
        src.update()


def test_pool_without_sampling_and_sigmas_is_the_pool_in_order_and_needs_no_counter():
    from tensorflowraytrace_amd import _lib, ops
    d = _dist()
    d.seed(7)
    n_pool = 1000
    fields = _pool_fields(n_pool, seed=3)
    records = torch.from_numpy(np.stack([fields[g] for g in GEO], axis=1)).to(DEV)
    src = _pool_source(fields, 17, do_downsample=False)
    assert src._fields.n_rays == n_pool
    plain = _lib.Source3DProgram.from_buffer_copy(src._dev_program[1])
    plain.pool_epoch = None                                  # nothing sampled, nothing jittered
    assert not plain.pool_downsample and int(plain.n_rays) == n_pool
    assert not any(plain.sigma_start) and not any(plain.sigma_end)
    for dt in (torch.float32, torch.float64):
        rays, fl = ops.source3d_generate(plain, n_pool, dtype=dt, fields=True, device=DEV)
        assert torch.equal(fl, records.t()) and torch.equal(rays, records.t().to(dt))
    rows = ops.source3d_pool_rows(plain, n_pool, device=DEV)
    assert torch.equal(rows, torch.arange(n_pool, dtype=torch.int32, device=DEV))
    assert torch.equal(torch.stack([src[g] for g in GEO]), records.t())


# -------------------------------------------------------------------------- 5. the order
@pytest.mark.parametrize("kind", sorted(SOURCES))
def test_order_of_a_procedural_program_sorts_its_own_keys(kind):
    """stable: the stable argsort of the keys the launch hands out; the faster order: a permutation
    along which the keys do not fall; the keys a deterministic function of the program.  (What the
    float32 keys are made of is the compactness tests' matter, tests/test_gpu_source_programs.py.)"""
    from tensorflowraytrace_amd import ops
    d = _dist()
    d.seed(sr.SOURCE_SEED)
    src, inputs, want = SOURCES[kind][0](d, True)
    assert src._device_program() is not None
    sp = src._dev_program[1]
    perm, keys = ops.source3d_order(sp, N, device=DEV, stable=True, return_keys=True)
    assert perm.dtype == torch.int32 and perm.shape == (N,) and keys.shape == (N,)
    ku = _np(keys).view(np.uint32)
    assert len(np.unique(ku)) >= N // 64                     # (at least a key per wavefront of rays)
    assert np.array_equal(_np(perm), np.argsort(ku, kind="stable").astype(np.int32))
    fast, keys_fast = ops.source3d_order(sp, N, device=DEV, stable=False, return_keys=True)
    assert torch.equal(keys_fast, keys)
    pf = _np(fast).astype(np.int64)
    assert np.array_equal(np.sort(pf), np.arange(N))
    assert bool((np.diff(ku[pf].astype(np.int64)) >= 0).all())
    again, keys_again = ops.source3d_order(sp, N, device=DEV, stable=True, return_keys=True)
    assert torch.equal(keys_again, keys) and torch.equal(again, perm)
