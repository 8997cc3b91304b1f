"""2-D sources made on the device (csrc/tfrt_source.hip: tfrt_samples_generate,
tfrt_source2d_generate) behind the reference's classes: the four 1-D random distributions
(RandomUniformAngularDistribution, RandomLambertianAngularDistribution, RandomUniformBeam,
RandomUniformAperaturePoints), the 2-D branches of the Point / Angular / Aperature sources
(tfrt/sources.py:464-1095) and the fused, graph-replayed 2-D optimiser step over a source that is
re-drawn at every step (dev/light_guide.py:45-49 builds such a source).  The reference's generator
is TensorFlow's and unseeded: parity is the distribution, the exact assembly of the rays, and that
nothing else about a trace depends on how the rays were made."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import sources as osources
from source_reference import philox_uv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PI = math.pi
GEO2 = ("x_start", "y_start", "x_end", "y_end")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))


def _dist():
    import tfrt.distributions as d
    return d


# ------------------------------------------------------------------- numpy restatement
def _philox_u(seed, stream, epoch, n):
    """First float64 of Philox4x32-10(counter = (sample, epoch), key = (seed, stream)) for samples
    0 .. n-1: 53 bits of the first two output words, in [0, 1) (tests/source_reference.py)."""
    return philox_uv(seed, stream, epoch, n)[0]


def _beam_numbers(beam_start, beam_end, central_angle):
    """BeamPointBase._update's host numbers: (start rank, end rank, the point of rank 1)."""
    rank_scale = max(abs(beam_start), abs(beam_end))
    r0, r1 = beam_start / rank_scale, beam_end / rank_scale
    scale = beam_start / abs(r0)
    return r0, r1, np.array([scale * math.cos(central_angle - PI / 2),
                             scale * math.sin(central_angle - PI / 2)])


# one entry per distribution: constructor, and u -> {attribute: values} (the host formulas)
def _uniform_angle(u, lo=-0.4, hi=0.9):
    angle = lo + (hi - lo) * u
    return {"angles": angle, "ranks": angle / max(abs(lo), abs(hi), 1e-300)}


def _lambert_angle(u, lo=-0.5, hi=1.25):
    rank = math.sin(lo) + (math.sin(hi) - math.sin(lo)) * u
    return {"angles": np.arcsin(rank), "ranks": rank}


def _beam(u, start=-1.5, end=0.5, central=0.3):
    r0, r1, endpoint = _beam_numbers(start, end, central)
    rank = r0 + (r1 - r0) * u
    return {"ranks": rank, "points": endpoint[None, :] * rank[:, None]}


def _aperture(u, start=(0.25, -1.0), end=(2.0, 3.0)):
    start, end = np.array(start), np.array(end)
    return {"ranks": u[:, None], "points": start[None, :] + u[:, None] * (end - start)[None, :]}


CASES = {
    "uniform_angle": (lambda d, n: d.RandomUniformAngularDistribution(-0.4, 0.9, n),
                      _uniform_angle),
    "lambert_angle": (lambda d, n: d.RandomLambertianAngularDistribution(-0.5, 1.25, n),
                      _lambert_angle),
    "beam": (lambda d, n: d.RandomUniformBeam(-1.5, 0.5, n, central_angle=0.3), _beam),
    "aperture": (lambda d, n: d.RandomUniformAperaturePoints((0.25, -1.0), (2.0, 3.0), n),
                 _aperture),
}


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("case", sorted(CASES))
def test_values_are_philox_pushed_through_the_host_formulas(case):
    d = _dist()
    make, formula = CASES[case]
    seed, n = 77, 5000
    d.seed(seed)
    filler = d.RandomUniformBeam(-1.0, 1.0, 3)            # (takes stream 1: ours is stream 2)
    dist = make(d, n)
    assert dist.__dict__.get("_device_active") and dist._stream_id == 2
    first = {}
    for name, want in formula(_philox_u(seed, 2, 1, n)).items():
        got = getattr(dist, name)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == want.shape
        assert getattr(dist, name) is got                   # the same draw until the next update
        np.testing.assert_allclose(_np(got), want, rtol=0, atol=1e-13)
        first[name] = _np(got).copy()
    dist.update()
    for name, want in formula(_philox_u(seed, 2, 2, n)).items():
        got = _np(getattr(dist, name))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
        assert float(np.abs(got - first[name]).max()) > 1e-3         # a new draw
    # the same seed and fresh objects: the same numbers again
    d.seed(seed)
    filler = d.RandomUniformBeam(-1.0, 1.0, 3)
    again = make(d, n)
    for name, values in first.items():
        assert np.array_equal(_np(getattr(again, name)), values)
    del filler


# ----------------------------------------------------------------------- 2. distribution
def test_underlying_numbers_are_uniform_at_a_million_samples():
    """Tolerances from the sample size alone, five standard errors of each statistic: the mean of
    n uniform numbers has variance 1/(12 n), their sample variance (mu4 - sigma^4)/n = 1/(180 n),
    a chi-square over K equally likely bins has mean K - 1 and variance 2 (K - 1)."""
    d = _dist()
    d.seed(5)
    n = 1 << 20
    lo, hi = -0.5, 1.25
    r0, r1, _ = _beam_numbers(-1.5, 0.5, 0.3)
    lam = CASES["lambert_angle"][0](d, n)
    us = {
        "uniform_angle": (CASES["uniform_angle"][0](d, n).angles + 0.4) / 1.3,
        "lambert_angle": (lam.ranks - math.sin(lo)) / (math.sin(hi) - math.sin(lo)),
        "beam": (CASES["beam"][0](d, n).ranks - r0) / (r1 - r0),
        "aperture": CASES["aperture"][0](d, n).ranks.reshape(-1),
    }
    for name, u in us.items():
        assert tuple(u.shape) == (n,)
        assert float(u.min()) >= -1e-15 and float(u.max()) <= 1 + 1e-15, name
        mean, var = float(u.mean()), float(u.var(unbiased=False))
        print(f"{name}: mean - 1/2 = {mean - 0.5:.3e} (5 se {5 * math.sqrt(1 / 12 / n):.3e}), "
              f"var - 1/12 = {var - 1 / 12:.3e} (5 se {5 * math.sqrt(1 / 180 / n):.3e})")
        assert abs(mean - 0.5) < 5 * math.sqrt(1 / 12 / n), (name, mean)
        assert abs(var - 1 / 12) < 5 * math.sqrt(1 / 180 / n), (name, var)
    # Lambertian: the ranks (sines of the angles) are uniform on [sin lo, sin hi]
    K = 64
    ranks = lam.ranks
    assert float(ranks.min()) >= math.sin(lo) - 1e-15 and float(ranks.max()) <= math.sin(hi) + 1e-15
    assert torch.allclose(torch.sin(lam.angles), ranks, rtol=0, atol=1e-13)
    counts = torch.histc(ranks, bins=K, min=math.sin(lo), max=math.sin(hi)).double()
    assert int(counts.sum()) == n
    chi2 = float(((counts - n / K) ** 2 / (n / K)).sum())
    print(f"chi2 {chi2:.2f}, K - 1 = {K - 1}, 5 se {5 * math.sqrt(2 * (K - 1)):.2f}")
    assert abs(chi2 - (K - 1)) < 5 * math.sqrt(2 * (K - 1)), chi2


# --------------------------------------------------------------------------- 3. assembly
def _check_set(src, want, n):
    """Fields against the oracle's, the float32 block against the fields, shards and a permuted
    view against the whole set."""
    import tfrt.sources as sources
    rs = src._fields
    assert isinstance(rs, sources.DeviceRaySet2D) and rs.n_rays == n
    assert set(rs.keys()) == set(GEO2) | {"wavelength"}
    for f in GEO2:
        assert src[f].shape == (n,) and src[f].dtype == torch.float64
        np.testing.assert_allclose(_np(src[f]), want[f], rtol=0, atol=1e-13, err_msg=f)
    np.testing.assert_array_equal(_np(src["wavelength"]), want["wavelength"])
    fields = torch.stack([src[f] for f in GEO2])
    for dt in (torch.float32, torch.float64):
        blk = rs.ray_block(dt)
        assert blk.shape == (4, n) and blk.dtype == dt
        assert torch.equal(blk, fields.to(dt))               # rounded once, bit for bit
        assert rs.ray_block(dt) is blk                       # persistent
    cut = n // 3
    for lo, hi in ((0, cut), (cut, n)):
        sh = rs.shard(lo, hi)
        assert torch.equal(sh.ray_block(torch.float64), fields[:, lo:hi])
        assert torch.equal(sh["y_end"], fields[3, lo:hi])
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(n, generator=g).int().to(DEV)
    pv = rs.permuted(perm)
    assert torch.equal(pv.ray_block(torch.float32), fields.float()[:, perm.long()])
    assert torch.equal(pv["x_end"], fields[2, perm.long()])
    assert rs.identity == src._fields.identity and rs.cache_key != pv.cache_key
    return fields


@pytest.mark.parametrize("start_on", [True, False])
def test_sources_assemble_like_the_oracle(start_on):
    import tfrt.sources as sources
    d = _dist()
    d.seed(9)
    n = 6000
    center, central, wl = (1.25, -0.75), 0.35, [550.0]
    # a point source over a Lambertian fan
    ang = d.RandomLambertianAngularDistribution(-0.5, 1.25, n)
    ps = sources.PointSource(2, center, central, ang, wl, dense=False, start_on_center=start_on,
                             ray_length=2.5)
    assert ps._device_program() is not None
    want = osources.point_source_2d(np.array(center), central, _np(ang.angles), np.array(wl),
                                    False, start_on_center=start_on, ray_length=2.5)
    _check_set(ps, want, n)
    # an angular source: a random beam and a random fan; then the beam with ONE static angle
    beam = d.RandomUniformBeam(-1.5, 0.5, n, central_angle=0.3)
    fan = d.RandomUniformAngularDistribution(-0.4, 0.9, n)
    for angles in (fan, d.StaticUniformAngularDistribution(0.1, 0.1, 1)):
        an = sources.AngularSource(2, center, central, angles, beam, wl, dense=False,
                                   start_on_base=start_on, ray_length=0.5)
        want = osources.angular_source_2d(np.array(center), central, _np(angles.angles),
                                          _np(beam.points), np.array(wl), False,
                                          start_on_base=start_on, ray_length=0.5)
        fields = _check_set(an, want, n)
        old = fields.clone()
        blk = an._fields.ray_block(torch.float32)
        an.update()                                          # re-drawn in place
        assert an._fields.ray_block(torch.float32) is blk
        new = torch.stack([an[f] for f in GEO2])
        assert torch.equal(blk, new.float())
        assert float((new - old).abs().max()) > 1e-3
    # an aperture source: two random point sets; then random start points and static end points
    a = d.RandomUniformAperaturePoints((0.25, -1.0), (0.5, 1.0), n)
    for b in (d.RandomUniformAperaturePoints((4.0, -2.0), (4.5, 2.0), n),
              d.StaticUniformAperaturePoints((4.0, -2.0), (4.5, 2.0), n)):
        ap = sources.AperatureSource(2, a, b, wl, dense=False)
        want = osources.aperature_source(_np(a.points), _np(b.points), np.array(wl), False)
        _check_set(ap, want, n)


def test_extra_fields_of_a_live_distribution_come_in_the_asked_order():
    import tfrt.sources as sources
    d = _dist()
    d.seed(4)
    n = 3000
    beam = d.RandomUniformBeam(-1.5, 0.5, n)
    fan = d.RandomLambertianAngularDistribution(-0.3, 0.3, n)
    src = sources.AngularSource(2, (0.0, 0.0), 0.0, fan, beam, [500.0], dense=False,
                                extra_fields={"ranks": ("base_point", beam, "ranks"),
                                              "base": ("base_point", beam, "points"),
                                              "fan": ("angle", fan, "angles"),
                                              "tag": ("whole", np.arange(n, dtype=np.float64))})
    rs = src._fields
    assert set(rs.keys()) == set(GEO2) | {"wavelength", "ranks", "base", "fan", "tag"}
    assert torch.equal(src["ranks"], beam.ranks) and torch.equal(src["base"], beam.points)
    assert torch.equal(src["fan"], fan.angles)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2)).int().to(DEV)
    pv, sh = rs.permuted(perm), rs.shard(100, 900)
    for name, whole in (("ranks", beam.ranks), ("base", beam.points), ("fan", fan.angles),
                        ("tag", src["tag"])):
        assert torch.equal(pv[name], whole[perm.long()]), name
        assert torch.equal(sh[name], whole[100:900]), name


# ------------------------------------------------------------------------------ 4. trace
def test_trace_of_a_device_made_source_equals_the_trace_of_its_rays_as_plain_tensors():
    import optimize_arc
    import tfrt.sources as sources
    d = _dist()
    d.seed(21)
    n = 20000
    s = optimize_arc.build(n, ray_dtype=torch.float64, random_source=True)
    eng, system, source = s["engine"], s["system"], s["source"]
    s2 = optimize_arc.build(10, ray_dtype=torch.float64)
    eng2, system2 = s2["engine"], s2["system"]
    for e in (eng, eng2):
        e.compile_dead_rays = e.compile_stopped_rays = True
    classes = ("finished", "active", "dead", "stopped")
    for _ in range(2):
        system.update()
        assert isinstance(source._fields, sources.DeviceRaySet2D)
        eng.ray_trace(2)
        got = {c: {f: getattr(eng, c + "_rays")[f].clone() for f in GEO2 + ("wavelength",)}
               for c in classes if bool(getattr(eng, c + "_rays"))}
        assert got["finished"]["x_start"].shape[0] > n // 2
        manual = sources.ManualSource(2)
        for f in source.keys():
            manual[f] = source[f].clone()
        system2.sources = [manual]
        system2.update()
        eng2.ray_trace(2)
        for c in classes:
            assert bool(getattr(eng2, c + "_rays")) == (c in got), c
        for c, fields in got.items():
            for f, v in fields.items():
                assert torch.equal(v, getattr(eng2, c + "_rays")[f]), (c, f)


# ------------------------------------------------------------------------------- 5. step
def _step_runs(error, steps=12, n=8192, seed=33):
    """(errors, final parameter, optimiser) of a fused, graph-replayed run and of a generic one
    over the single-arc scene with a RandomUniformBeam source, built after the same seed."""
    import optimize_arc
    from tfrt.optimizer import GoalError, RowwiseError, SGD_Optimizer
    d = _dist()
    out = {}
    for mode in ("graph", "generic"):
        d.seed(seed)
        s = optimize_arc.build(n, ray_dtype=torch.float64, random_source=True)
        eng, source = s["engine"], s["source"]
        if error == "goal":
            erf = GoalError(("y_end",), torch.zeros(n, dtype=torch.float64, device=DEV))
        else:
            source.extra_fields = {"ranks": ("base_point", source.base_point_distribution, "ranks")}
            eng.add_inheritable_field("ranks")
            s["system"].update()
            erf = RowwiseError(lambda r: (1.0 + r["ranks"] ** 2) * r["y_end"] ** 2)
        opt = SGD_Optimizer(eng, [s["parameter"]], erf, 2, learning_rate=0.02, grad_clip=0.05,
                            sgd_learning_rate=1.0, fused=mode == "graph", graph=mode == "graph")
        errors, draws = [], []
        for _ in range(steps):
            errors.append(float(opt.single_step(None)))
            draws.append(source["y_start"].clone())          # the rays of the step just run
        torch.cuda.synchronize()
        out[mode] = (errors, s["parameter"].detach().cpu().clone(), opt, s, draws)
    return out


@pytest.mark.parametrize("error", ["goal", "rowwise"])
def test_fused_2d_step_over_a_redrawn_source_is_captured_and_equals_the_generic_step(error):
    import tfrt.sources as sources
    steps = 12
    runs = _step_runs(error, steps)
    assert runs["generic"][2]._fused_step is None
    fs = runs["graph"][2]._fused_step
    assert fs is not None and fs.capture_error is None, getattr(fs, "capture_error", None)
    assert fs.graph_replays > 0 and fs.steps == steps
    for mode in runs:
        assert isinstance(runs[mode][3]["source"]._fields, sources.DeviceRaySet2D)
        errors = runs[mode][0]
        assert all(np.isfinite(errors)) and len(set(errors)) > 1, errors
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
    # the ray sets of the last (replayed) step, cut lazily, belong to the last draw
    eng, source = runs["graph"][3]["engine"], runs["graph"][3]["source"]
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].long()
    assert fin["y_end"].shape == ids.shape and ids.shape[0] > 0
    if error == "rowwise":
        assert torch.equal(fin["ranks"], source["ranks"][ids])


def test_a_static_partner_is_keyed_by_its_parameters():
    """A static distribution publishes a new tensor with the same values at every update: the
    source's program (and with it the captured step's signature) must hold still across updates,
    and follow the distribution when one of its parameters changes."""
    import tfrt.sources as sources
    d = _dist()
    d.seed(8)
    n = 2000
    beam = d.RandomUniformBeam(-1.5, 0.5, n)
    angles = d.StaticUniformAngularDistribution(0.1, 0.1, 1)
    src = sources.AngularSource(2, (0.5, -0.25), 0.2, angles, beam, [500.0], dense=False)
    first = angles.angles
    identity = src._fields.identity
    src.update()
    assert angles.angles is not first                        # made again, as on the host path
    assert src._fields.identity == identity
    angles.min_angle = angles.max_angle = 0.3
    src.update()
    assert src._fields.identity != identity
    want = osources.angular_source_2d(np.array((0.5, -0.25)), 0.2, np.array([0.3]),
                                      _np(beam.points), np.array([500.0]), False)
    for f in GEO2:
        np.testing.assert_allclose(_np(src[f]), want[f], rtol=0, atol=1e-13, err_msg=f)
    # a static beam under a transformation is not a function of its parameters: the torch path
    sbeam = d.StaticUniformBeam(-1.0, 1.0, n)
    d.BasePointTransformation(sbeam, translation=(1.0, 0.0, 0.0))
    sbeam.update()
    assert sbeam._static_key() is None


# -------------------------------------------------------------------------- 6. fall-backs
def test_differentiable_dense_and_switched_off_sources_keep_the_torch_path():
    import tfrt.sources as sources
    d = _dist()
    d.seed(5)
    n = 4000
    fan = d.RandomUniformAngularDistribution(-0.4, 0.9, n)
    beam = d.RandomUniformBeam(-1.5, 0.5, n)
    center = torch.tensor([1.0, -2.0], dtype=torch.float64, device=DEV, requires_grad=True)
    ps = sources.PointSource(2, center, 0.2, fan, [500.0], dense=False)
    assert ps._device_program() is None
    assert not isinstance(ps._fields, sources.DeviceRaySet)
    err = (ps["x_end"] ** 2 + 3.0 * ps["y_start"]).sum()
    g, = torch.autograd.grad(err, [center])
    assert abs(float(g[1]) - 3.0 * n) < 1e-6 * n and abs(float(g[0])) > 0.0
    # the same source without a gradient request is made on the device
    ps2 = sources.PointSource(2, center.detach(), 0.2, fan, [500.0], dense=False)
    assert ps2._device_program() is not None
    assert isinstance(ps2._fields, sources.DeviceRaySet2D)
    # dense: every base point with every wavelength
    dense = sources.AngularSource(2, (0.0, 0.0), 0.0, d.StaticUniformAngularDistribution(0, 0, 1),
                                  beam, [450.0, 550.0, 650.0], dense=True)
    assert dense._device_program() is None
    assert dense["x_start"].shape == (3 * n,)
    # no live random input: nothing to re-draw
    static = sources.AngularSource(2, (0.0, 0.0), 0.0, d.StaticUniformAngularDistribution(0, 0, 1),
                                   d.StaticUniformBeam(-1.5, 0.5, n), [500.0], dense=False)
    assert static._device_program() is None
    d.set_device_random(False)
    try:
        off = sources.AngularSource(2, (0.0, 0.0), 0.0, fan, beam, [500.0], dense=False)
        assert off._device_program() is None
        assert not fan.__dict__.get("_device_active") and not beam.__dict__.get("_device_active")
        assert isinstance(off["x_start"], torch.Tensor) and off["x_start"].shape == (n,)
        first = off["y_start"].clone()
        off.update()
        assert not torch.equal(first, off["y_start"])        # torch's generator, new tensors
    finally:
        d.set_device_random(True)
    fan.update()
    assert fan.__dict__.get("_device_active")
