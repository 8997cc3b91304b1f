"""Host side of the 2-D source programs (tfrt_samples_generate, tfrt_source2d_generate): malformed
programs are refused before any launch, and on the CPU device the four 1-D random distributions
still draw with the torch generator, number for number as before they had a device form."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    return _lib.lib()


def test_malformed_2d_programs_are_refused_before_any_launch(lib):
    from tensorflowraytrace_amd import _lib
    dummy = ctypes.create_string_buffer(1 << 12)
    ptr = ctypes.cast(dummy, ctypes.c_void_p)

    def samples(kind=_lib.SMP_UNIFORM_ANGLE, count=10, epoch=ptr, lo=-0.5, hi=0.5, table=None,
                columns=0):
        pg = _lib.SamplesProgram()
        pg.kind, pg.count, pg.epoch, pg.lo, pg.hi = kind, count, epoch, lo, hi
        pg.table, pg.columns, pg.rank_scale = table, columns, 0.5
        return pg

    def generate_samples(pg, n=10, cols=1):
        return lib.tfrt_samples_generate(ctypes.byref(pg), None, 0, n, ptr, cols, None, None)

    for bad in (samples(kind=5), samples(kind=-1), samples(epoch=None), samples(lo=0.5, hi=-0.5),
                samples(lo=float("nan")), samples(count=-1),
                samples(kind=_lib.SMP_TABLE, columns=1),               # a table without storage
                samples(kind=_lib.SMP_TABLE, table=ptr, columns=3)):
        assert generate_samples(bad) == -1
    assert generate_samples(samples(), n=11) == -1                   # more than the program has
    assert generate_samples(samples(), cols=2) == -1                 # angles are one column
    assert generate_samples(samples(kind=_lib.SMP_BEAM), cols=1) == -1
    assert lib.tfrt_samples_generate(None, None, 0, 10, ptr, 1, None, None) == -1
    assert generate_samples(samples(), n=0) == 0                     # nothing to do: no launch

    def source(kind=_lib.SRC_ANGULAR, a=None, b=None, n_rays=10):
        sp = _lib.Source2DProgram()
        sp.kind, sp.n_rays, sp.ray_length = kind, n_rays, 1.0
        sp.a = a if a is not None else samples(kind=_lib.SMP_BEAM)
        sp.b = b if b is not None else samples()
        return sp

    def generate(sp, n=10, dtype=_lib.F64, stride=10):
        return lib.tfrt_source2d_generate(ctypes.byref(sp), None, 0, n, dtype, ptr, stride, None, 0,
                                          None)

    for bad in (source(kind=3), source(kind=-1),                      # (a pool has no 2-D form)
                source(b=samples(kind=9)), source(a=samples(kind=9)),
                source(b=samples(epoch=None)), source(a=samples(kind=_lib.SMP_BEAM, epoch=None)),
                source(b=samples(lo=1.0, hi=0.0)),
                source(a=samples(kind=_lib.SMP_BEAM, count=3)), source(b=samples(count=3)),
                source(a=samples()),                                  # base points must be points
                source(b=samples(kind=_lib.SMP_BEAM)),                # angles must be angles
                source(kind=_lib.SRC_APERTURE),                       # end points must be points
                source(kind=_lib.SRC_POINT, b=samples(kind=_lib.SMP_APERTURE_POINTS)),
                source(n_rays=-1)):
        assert generate(bad) == -1
    ok = source()
    assert generate(ok, n=11) == -1 and generate(ok, stride=5) == -1 and generate(ok, dtype=7) == -1
    assert lib.tfrt_source2d_generate(None, None, 0, 10, _lib.F64, ptr, 10, None, 0, None) == -1
    assert generate(ok, n=0) == 0
    one = source(a=samples(kind=_lib.SMP_BEAM, count=1), b=samples(count=1), n_rays=0)
    assert generate(one, n=0) == 0


def test_on_the_cpu_the_four_distributions_draw_as_before():
    """The values are those of the change's parent (torch generator, seed 2024, this order of
    construction), recorded once."""
    import tfrt.distributions as d
    import tensorflowraytrace_amd.config as config
    assert config.get_device().type == "cpu"
    d.seed(2024)
    a = d.RandomUniformAngularDistribution(-0.4, 0.9, 4)
    lam = d.RandomLambertianAngularDistribution(-0.5, 0.25, 4)
    b = d.RandomUniformBeam(-1.5, 0.5, 4, central_angle=0.3)
    p = d.RandomUniformAperaturePoints((0.0, -1.0), (2.0, 3.0), 4)
    for dist in (a, lam, b, p):
        assert not dist.__dict__.get("_device_active")
    want = {
        (a, "angles"): [-0.07015448365239735, 0.6071156312806366, 0.03578370745162779,
                        0.5359215550239506],
        (a, "ranks"): [-0.07794942628044149, 0.6745729236451518, 0.0397596749462531,
                       0.5954683944710562],
        (lam, "angles"): [0.1599970328624211, -0.3277070982732982, -0.19886640010489495,
                          -0.18076326831140258],
        (lam, "ranks"): [0.15931527737437323, -0.32187299636130295, -0.19755820001330215,
                         -0.1797804579176004],
        (b, "points"): [[0.18559135068472254, -0.5999663825980156],
                        [0.37835088880462464, -1.2231055664575248],
                        [0.3658336619531441, -1.1826407749328425],
                        [0.25332830167231574, -0.8189415304284945]],
        (b, "ranks"): [-0.41867718123565645, -0.8535251403597076, -0.8252874168034636,
                       -0.571485572361385],
        (p, "points"): [[1.6292411256696047, 2.2584822513392093],
                        [1.4409294120923226, 1.8818588241846452],
                        [1.2539934183305463, 1.5079868366610927],
                        [0.7549345421387241, 0.5098690842774483]],
        (p, "ranks"): [[0.8146205628348023], [0.7204647060461613], [0.6269967091652732],
                       [0.37746727106936206]],
    }
    for (dist, name), values in want.items():
        got = getattr(dist, name)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64
        assert got.tolist() == values, (type(dist).__name__, name)
    a.update()
    assert a.angles.tolist() == [0.7204747790583118, 0.2829128326341023, 0.2720509723737682,
                                 0.7049877120767091]
    # a 2-D source over them keeps the torch path on the CPU
    import tfrt.sources as sources
    src = sources.AngularSource(2, (-1.0, 0.5), 0.2, a, b, [550.0], dense=False)
    assert src._device_program() is None
    np.testing.assert_allclose(src["x_start"].numpy(),
                               -1.0 + np.cos(0.2) * b.points[:, 0].numpy()
                               - np.sin(0.2) * b.points[:, 1].numpy(), rtol=0, atol=1e-15)


def test_static_1d_distributions_update_as_before():
    """What a static distribution publishes is made again at every update(), as before the 2-D
    device programs: a BasePointTransformation sees untransformed points each time, a source over
    static distributions follows a centre that is stepped in place, and a differentiable end point
    can be differentiated after every update."""
    import tfrt.distributions as d
    import tfrt.sources as sources
    beam = d.StaticUniformBeam(-1.0, 1.0, 3)
    d.BasePointTransformation(beam, translation=(1.0, 0.0, 0.0))
    ap = d.StaticUniformAperaturePoints((0.0, -1.0), (0.0, 1.0), 3)
    d.BasePointTransformation(ap, translation=(1.0, 0.0, 0.0))
    for _ in range(3):
        beam.update()
        ap.update()
        assert beam.points.shape == (3, 3) and beam.points[:, 0].tolist() == [1.0, 1.0, 1.0]
        assert ap.points.shape == (3, 3) and ap.points[:, 0].tolist() == [1.0, 1.0, 1.0]
        np.testing.assert_allclose(beam.points[:, 2].numpy(), [-1.0, 0.0, 1.0], atol=1e-15)
        assert ap.points[:, 2].tolist() == [-1.0, 0.0, 1.0]
    # a centre stepped in place between updates (what the optimiser's apply step does)
    c = torch.zeros(2, dtype=torch.float64, requires_grad=True)
    src = sources.AngularSource(2, c, 0.0, d.StaticUniformAngularDistribution(0, 0, 1),
                                d.StaticUniformBeam(-1.0, 1.0, 3), [500.0], dense=False)
    for k in range(3):
        src.update()
        # (the beam lies along y: its x is cos(-pi/2) times the rank, 6e-17 at most)
        np.testing.assert_allclose(src["x_start"].detach().numpy(), [float(k)] * 3, rtol=0, atol=1e-15)
        with torch.no_grad():
            c.add_(1.0)
    # a differentiable end point: one backward per update, no in-place step in between
    end = torch.tensor([0.0, 1.0], dtype=torch.float64, requires_grad=True)
    pts = d.StaticUniformAperaturePoints((0.0, -1.0), end, 3)
    for _ in range(2):
        pts.update()
        g, = torch.autograd.grad(pts.points.sum(), [end])
        assert g.tolist() == [1.5, 1.5]
