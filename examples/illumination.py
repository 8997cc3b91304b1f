#!/usr/bin/env python3
"""
Illumination design, the workflow of the reference's dev/PCF_lens.py: "these rays start distributed
like A and must land distributed like B".  The start points of an AperatureSource follow a two-bump
density (ArbitraryBasePoints over an ArbitraryDistribution); their ranks -- a flat density
evaluated at the same uniform seeds -- ride along as the extra field ``goal``
(dev/PCF_lens.py:141-143), and a two-surface parametric acrylic lens (the one of
examples/hexalens.py) is shaped so that every ray lands at -m times its goal: the bumps are spread
into an even square.

On a HIP device the density map is part of the source's device program: the rays are re-drawn in
place every step, the goal rows are made in the order the rays are traced in, and the whole step is
replayed from one HIP graph.  ``--host`` runs what there was before: scipy's interp1d on the host
and an upload at every step, which the optimiser cannot capture.

    python examples/illumination.py [--rays 20000] [--steps 30] [--edge 0.12] [--host]

``--density-error`` optimises the same scene against the target density directly, without ranks: a
``DensityError`` over (y_end, z_end) whose goal is the even square itself, on a grid of ``--bins``
bins per axis -- no transport map is needed, and rays that are lost or stopped simply do not count.
``--generic`` forces the generic path (``fused=False``) for comparison.

``--lambertian-weights`` (with ``--density-error``) treats the start plane as a Lambertian emitter:
the aperture source samples its rays evenly over the lens, and every ray carries ``cos theta`` of
its start direction to the emitter's normal as its radiant power -- the ``weights`` of the
``DensityError``, a callable on the source's fields, evaluated again whenever the rays are re-drawn.

    python examples/illumination.py --density-error [--bins 64] [--generic] [--lambertian-weights]

``--transport-error`` optimises the same scene and the same goal by sliced optimal transport
instead: a ``TransportError`` over (y_end, z_end) with ``--directions`` projection directions pulls
every ray towards the goal's quantile at its own rank, so the step has a signal even where the
landing pattern and the goal do not overlap.  ``--generic`` as above.

    python examples/illumination.py --transport-error [--directions 8] [--bins 64] [--generic]

``--combined`` runs both objectives as the two terms of one step, ``SumError([TransportError,
DensityError])``: transport first -- it still points home where the histogram's gradient vanishes
--, density for the detail.  ``set_weights`` moves the balance from the one to the other as the run
goes; the weights live in a device buffer, so the replayed graph sees them without a re-capture.
One trace, two error evaluations, one combination and one reverse sweep per step; both terms'
own errors are printed.

    python examples/illumination.py --combined [--directions 8] [--bins 64] [--generic]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tfrt.boundaries as boundaries          # noqa: E402
import tfrt.distributions as distributions    # noqa: E402
import tfrt.drawing as drawing                # noqa: E402
import tfrt.engine as engine                  # noqa: E402
import tfrt.materials as materials            # noqa: E402
import tfrt.mesh_tools as mt                  # noqa: E402
import tfrt.operation as operation            # noqa: E402
import tfrt.optimizer as optimizer            # noqa: E402
import tfrt.sources as sources                # noqa: E402

COARSEST_EDGE = 0.4        # the coarsest lens mesh the example is run with (the tests' lens)
DENSITY_CELLS = 64
DENSITY_LEARNING_RATE = 0.05


def two_bumps(size):
    """The source's density on [-size, size]^2: two Gaussian bumps on a faint floor."""
    def density(gx, gy):
        a = np.exp(-((gx + 0.4 * size) ** 2 + (gy - 0.3 * size) ** 2) / (2 * (0.25 * size) ** 2))
        b = np.exp(-((gx - 0.5 * size) ** 2 + (gy + 0.2 * size) ** 2) / (2 * (0.18 * size) ** 2))
        return 0.02 + a + 0.7 * b
    return density


def even_square(size, domain_size, bins):
    """The target of ``--density-error``: 1 on the bins whose centre lies in [-size, size]^2, 0 on
    the margin up to ``domain_size``."""
    centres = (np.arange(bins) + 0.5) * (2 * domain_size / bins) - domain_size
    inside = (np.abs(centres) <= size).astype(np.float64)
    return inside[:, None] * inside[None, :]


def lambertian(src):
    """cos theta of a source ray's start direction to the emitter's normal (1, 0, 0): the weights
    of ``--lambertian-weights``, a callable on the source's field dict."""
    d = [src[a + "_end"].double() - src[a + "_start"].double() for a in "xyz"]
    return d[0].abs() / torch.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def build(ray_count=20000, lens_res_scale=0.12, source_distance=10.0, magnification=1.0,
          object_size=0.2, lens_aperature=1.0, rowwise=True, density_error=False, bins=64,
          lambertian_weights=False, transport_error=False, directions=8, combined=False,
          **engine_kw):
    # (the same scene: no ranks ride along)
    density_error = density_error or transport_error or combined
    limits = ((-object_size, object_size, DENSITY_CELLS), (-object_size, object_size, DENSITY_CELLS))
    start_density = distributions.ArbitraryDistribution(two_bumps(object_size), limits)
    goal_density = distributions.ArbitraryDistribution(lambda gx, gy: np.ones_like(gx), limits)
    # (a DensityError needs no transport map: no ranks ride along)
    start_points = distributions.ArbitraryBasePoints(
        start_density, ray_count, rank_distribution=None if density_error else goal_density)
    distributions.BasePointTransformation(start_points, translation=(-source_distance, 0, 0))
    end_points = distributions.RandomUniformCircle(ray_count, 0.98 * lens_aperature)
    distributions.BasePointTransformation(end_points)
    source = sources.AperatureSource(
        3, start_points, end_points, [drawing.YELLOW], dense=False,
        extra_fields={} if density_error else {"goal": ("start_point", start_points, "ranks")})

    zero_points = mt.circular_mesh(lens_aperature, lens_res_scale)
    zero_points.rotate_y(90)
    zero_points.rotate_x(90)
    top_parent = mt.get_closest_point(zero_points, (0, 0, 0))
    vertex_update_map, accumulator = mt.mesh_parametrization_tools(zero_points, top_parent)

    lens = boundaries.ParametricMultiTriangleBoundary(
        zero_points, boundaries.FromVectorVG((1, 0, 0)),
        [boundaries.ThicknessConstraint(0.0, "min"), boundaries.ThicknessConstraint(0.2, "min")],
        [True, False],
        material_list=[{"mat_in": 1, "mat_out": 0}] * 2,
        vertex_update_map=vertex_update_map)
    target = boundaries.ManualTriangleBoundary(mesh=mt.plane(
        center=(source_distance * magnification, 0, 0), direction=(1, 0, 0), i_size=100, j_size=100))
    target.frozen = True

    system = engine.OpticalSystem3D()
    system.optical = lens.surfaces
    system.targets = [target]
    system.sources = [source]
    system.materials = [{"n": materials.vacuum}, {"n": materials.acrylic}]
    system.update()

    trace_engine = engine.OpticalEngine(
        3, [operation.StandardReaction()], compile_active_rays=False,
        simple_ray_inheritance={"wavelength"} if density_error else {"wavelength", "goal"},
        **engine_kw)
    trace_engine.optical_system = system
    trace_engine.validate_system()

    m = magnification
    if combined:
        # both objectives of the flags below, over the same goal and domain
        size = abs(m) * object_size
        half = 1.25 * size
        goal, domain = even_square(size, half, bins), ((-half, half), (-half, half))
        error_function = optimizer.SumError([
            optimizer.TransportError(("y_end", "z_end"), goal, domain, directions=directions),
            optimizer.DensityError(("y_end", "z_end"), goal, domain,
                                   oob_weight=1.0 / (ray_count * size ** 2))])
    elif transport_error:
        # the goal and the domain of --density-error; rays beyond the margin need no penalty,
        # their rank pulls them in
        size = abs(m) * object_size
        half = 1.25 * size
        error_function = optimizer.TransportError(
            ("y_end", "z_end"), even_square(size, half, bins), ((-half, half), (-half, half)),
            directions=directions)
    elif density_error:
        # the even square of half-width m * object_size inside a domain with a margin of a quarter;
        # a ray beyond the margin is pulled back by the penalty (weighted per ray: the histogram
        # part of the error is of order 1 whatever the ray count)
        size = abs(m) * object_size
        half = 1.25 * size
        error_function = optimizer.DensityError(
            ("y_end", "z_end"), even_square(size, half, bins), ((-half, half), (-half, half)),
            oob_weight=1.0 / (ray_count * size ** 2),
            weights=lambertian if lambertian_weights else None)
    else:
        error_function = optimizer.GoalError(("y_end", "z_end"), lambda s: -m * s["goal"],
                                             rowwise=rowwise)
    return dict(engine=trace_engine, system=system, lens=lens, source=source,
                start_points=start_points, error_function=error_function, accumulator=accumulator)


def run(ray_count=20000, steps=30, lens_res_scale=0.12, host=False, verbose=True,
        density_error=False, bins=64, generic=False, splat_variant=0, lambertian_weights=False,
        transport_error=False, directions=8, combined=False):
    if combined:
        if density_error or transport_error or lambertian_weights or host:
            raise ValueError("--combined runs both objectives itself: no other objective flag")
        return run_combined(ray_count, steps, lens_res_scale, verbose, bins, generic, directions)
    if lambertian_weights and (transport_error or not density_error):
        raise ValueError("--lambertian-weights weighs a DensityError: it needs --density-error")
    if transport_error and density_error:
        raise ValueError("--transport-error and --density-error are two objectives: choose one")
    distributions.set_device_random(not host)
    try:
        s = build(ray_count, lens_res_scale, density_error=density_error, bins=bins,
                  lambertian_weights=lambertian_weights, transport_error=transport_error,
                  directions=directions)
        if density_error:
            s["error_function"].splat_variant = splat_variant
        # (a DensityError is one term of order 1, not a sum over the rays: its own step size)
        lr = DENSITY_LEARNING_RATE if density_error else 2e-5 * (20000 / ray_count)
        if transport_error:
            # a sum over the rays like the GoalError's, of K terms per ray in units of the domain's
            # width w: a ray's gradient is K / w**2 times that of a squared distance
            erf = s["error_function"]
            width = erf.domain[0][1] - erf.domain[0][0]
            lr *= width ** 2 / erf.n_directions
        opt = optimizer.SGD_Optimizer(s["engine"], s["lens"].parameters, s["error_function"], 3,
                                      learning_rate=lr, grad_clip=1.0,
                                      fused=False if generic else "auto")
        opt.suppress_warnings = True
        errors, times = [], []
        for step in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            errors.append(float(opt.single_step(s["accumulator"] if step < steps // 2 else None)))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            if verbose and step % 5 == 0:
                name = "transport error" if transport_error else \
                    "density error" if density_error else "mean squared error"
                print(f"step {step:4d}: {name} {errors[-1]:.6g}  ({1e3 * times[-1]:.2f} ms)")
        fused = opt._fused_step
        s.update(errors=errors, times=times, device_source=s["source"]._device_program() is not None,
                 graph_replays=0 if fused is None else fused.graph_replays)
        return s
    finally:
        distributions.set_device_random(True)


def transport_weight(erf, ray_count):
    """The weight that gives a TransportError, as a term beside a DensityError stepped with
    DENSITY_LEARNING_RATE, the step it takes alone in ``run``."""
    width = erf.domain[0][1] - erf.domain[0][0]
    alone = 2e-5 * (20000 / ray_count) * width ** 2 / erf.n_directions
    return alone / DENSITY_LEARNING_RATE


def run_combined(ray_count=20000, steps=30, lens_res_scale=0.12, verbose=True, bins=64,
                 generic=False, directions=8):
    """``--combined``: SumError([TransportError, DensityError]), the balance moved from transport
    (nine tenths of its own step, a tenth of the density's) to density (the reverse) across the
    run."""
    s = build(ray_count, lens_res_scale, bins=bins, directions=directions, combined=True)
    erf = s["error_function"]
    w_t = transport_weight(erf.terms[0], ray_count)
    opt = optimizer.SGD_Optimizer(s["engine"], s["lens"].parameters, erf, 3,
                                  learning_rate=DENSITY_LEARNING_RATE, grad_clip=1.0,
                                  fused=False if generic else "auto")
    opt.suppress_warnings = True
    errors, times, transport, density, merit = [], [], [], [], []
    for step in range(steps):
        a = step / (steps - 1) if steps > 1 else 0.0
        erf.set_weights([w_t * (1.0 - 0.9 * a), 0.1 + 0.9 * a])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        errors.append(float(opt.single_step(s["accumulator"] if step < steps // 2 else None)))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        last = erf.last_errors.cpu()
        transport.append(float(last[0, 2]))
        density.append(float(last[1, 0]))
        # one number for the run, whatever the balance was: both terms at their full weights
        merit.append(w_t * float(last[0, 0]) + float(last[1, 0]))
        if verbose and (step % 5 == 0 or step == steps - 1):
            print(f"step {step:4d}: transport error (mean term) {transport[-1]:.6g}  density error "
                  f"{density[-1]:.6g}  weighted sum {errors[-1]:.6g}  ({1e3 * times[-1]:.2f} ms)")
    fused = opt._fused_step
    s.update(errors=errors, times=times, transport=transport, density=density, merit=merit,
             device_source=s["source"]._device_program() is not None,
             graph_replays=0 if fused is None else fused.graph_replays)
    return s


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--edge", type=float, default=0.12, help=f"lens mesh edge, up to {COARSEST_EDGE}")
    ap.add_argument("--host", action="store_true",
                    help="the density map on the host at every step (scipy), as before it had a program")
    ap.add_argument("--density-error", action="store_true",
                    help="optimise against the target density directly (DensityError), without ranks")
    ap.add_argument("--bins", type=int, default=64, help="bins per axis of the DensityError's grid")
    ap.add_argument("--transport-error", action="store_true",
                    help="optimise against the target density by sliced optimal transport (TransportError)")
    ap.add_argument("--directions", type=int, default=8,
                    help="projection directions of the TransportError")
    ap.add_argument("--generic", action="store_true", help="the generic path (fused=False)")
    ap.add_argument("--splat-variant", type=int, default=0, choices=(0, 1, 2),
                    help="tfrt_density_error's splat: 0 by the bin count, 1 LDS histogram, 2 global atomics")
    ap.add_argument("--lambertian-weights", action="store_true",
                    help="with --density-error: every ray carries cos theta of its start direction")
    ap.add_argument("--combined", action="store_true",
                    help="both objectives on one step: SumError([TransportError, DensityError])")
    a = ap.parse_args()
    out = run(a.rays, a.steps, a.edge, host=a.host, density_error=a.density_error, bins=a.bins,
              generic=a.generic, splat_variant=a.splat_variant,
              lambertian_weights=a.lambertian_weights, transport_error=a.transport_error,
              directions=a.directions, combined=a.combined)
    tail = sorted(out["times"][len(out["times"]) // 2:])
    print(f"source on the device: {out['device_source']}; steps replayed from the graph: "
          f"{out['graph_replays']} of {a.steps}; median step of the second half: "
          f"{1e3 * tail[len(tail) // 2]:.3f} ms")
    if a.combined:
        print(f"transport error (mean term): first {out['transport'][0]:.6g} -> last "
              f"{out['transport'][-1]:.6g}")
        print(f"density error: first {out['density'][0]:.6g} -> last {out['density'][-1]:.6g}")
        print(f"combined error at full weights: first {out['merit'][0]:.6g} -> last "
              f"{out['merit'][-1]:.6g}")
        sys.exit(0)
    name = "transport error" if a.transport_error else \
        "density error" if a.density_error else "mean squared illumination error"
    print(f"{name}: first {out['errors'][0]:.6g} -> last {out['errors'][-1]:.6g}")
