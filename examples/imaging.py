#!/usr/bin/env python3
"""
Imaging without a target in advance: a two-surface parametric acrylic lens is shaped so that the
rays of every object point meet in ONE point on the target plane -- wherever that point is.

The scene of the reference's dev/image_quality_3d.py (which can only LOOK at the result, as a
histogram of the target plane): P object points on a plane at x = -10 -- a small "F" --, from each
of them A rays in random directions inside a cone towards the lens (a non-dense ``AngularSource``
over a ``ManualBasePointDistribution`` of the points, tiled A times, and a
``RandomUniformSphere``), the lens of examples/hexalens.py, a target plane at x = +10.  The merit
function is the RMS spot size, ``optimizer.SpotError``: the rays carry the label of their object
point, and the error is the summed squared distance of every finished ray to the centroid of its
own label.  Magnification, distortion and field curvature are left to the lens.

The directions are re-drawn at every step; the labels stay (ray i is object point i mod P).  With a
``SpotError`` the optimiser runs the step as one fixed launch sequence replayed from a HIP graph
once the engine traces the source in place; ``--generic`` keeps the generic path (the same
kernels under torch.autograd).

``--apodize SIGMA`` weighs the rays by a Gaussian pupil: a ray that leaves its object point at the
angle theta to the axis carries ``exp(-(sin theta / (SIGMA * sin cone))**2 / 2)`` -- ``SIGMA`` in
units of the cone that fills the lens --, given to the ``SpotError`` as a callable on the source's
fields (the directions are re-drawn at every step, so are the weights).  The spot is then the
weighted one: centroid, RMS size and gradient.

    python examples/imaging.py [--rays 20000] [--steps 30] [--generic] [--adam] [--apodize SIGMA]

``--magnification M`` pins what the ``SpotError`` leaves to the lens: the image of an object point
at (y, z) must lie at (-M y, -M z).  The error is then a ``SumError`` of two terms on one step,
``SumError([SpotError, GoalError(("y_end", "z_end"), -M * object_coords)], reduce="mean")`` -- the
mean squared spot radius plus the mean squared distance to the image point, the error of the
reference's dev/hexalens.py --, one trace, two error evaluations, one combination and one reverse
sweep, replayed from the same graph.

    python examples/imaging.py --magnification 1.0 [--rays 20000] [--steps 30] [--generic]

``--focus`` frees the axial position too: an ``optimizer.FocusError`` over the same labels in the
place of the ``SpotError``.  The rays of an object point, taken as lines, must pass through one
common point of space, wherever along the beam that is; a ray counts while its end lies in a box
around the target.  Defocus and field curvature are then no longer charged to the lens as spot
size, and the solved foci are a read-out of the focal surface: the run ends with their spread
along x, the field curvature.  A line includes its backward extension, so a diverging bundle has
a (virtual) focus too: the flat starting lens reports the plate's image of the object plane, and
the error is the lens' aberration alone.  Where the focus should lie is a second term's business
(a ``SumError`` with a ``GoalError``, as ``--magnification`` builds for the ``SpotError``).

    python examples/imaging.py --focus [--rays 20000] [--steps 30] [--generic]

``--flat-field`` adds what a sensor asks of ``--focus``: the foci must lie in one plane across the
axis, wherever along the axis it has to stand --
``SumError([FocusError, FlatFieldError], reduce="mean")`` over the same labels and box, "a sharp
image on a flat sensor".  The ``FlatFieldError`` charges every ray the squared distance of its
object point's focus from the plane that fits the foci best (normal: the x axis; the offset is
free), so the spread of the foci along the axis -- the field curvature that ``--focus`` only
reports -- is now lowered.  The run prints that spread before and after, and the plane's offset.

    python examples/imaging.py --flat-field [--flat-weight W] [--rays 20000] [--steps 30] [--generic]

``--distortion [scale|affine]`` asks for an undistorted image without pinning its scale or place:
``SumError([SpotError, DistortionError], reduce="mean")``.  The ``DistortionError`` fits the
spots' centroids to ``A p + t`` over the object points p -- a free magnification (``scale``) or a
free 2 x 2 matrix (``affine``) and a free offset -- and charges every ray the squared distance of
its spot's centroid from the fitted image of its object point.  Every report prints the fitted
magnification and the largest residual.

    python examples/imaging.py --distortion scale [--rays 20000] [--steps 30] [--generic]

``--telecentric [WEIGHT]`` asks for an image-side telecentric lens: the MEAN direction of every
object point's bundle must be the axis, while the cone of each point stays as wide as it is --
``SumError([SpotError(("y_end", "z_end"), ...), CentroidError(("y_dir", "z_dir"), labels, domain,
targets=zeros)], weights=[1, WEIGHT], reduce="mean")``.  (A ``SpotError`` on the directions would
collimate the bundles, which is another objective.)  ``WEIGHT`` balances squared direction cosines
-- 4e-5 per term for the flat starting lens -- against squared spot radii of order 1: the default
is 1,000, and the step size is ``min(0.4, 100 / WEIGHT)``, because the term is stiff (at weight
1,000 and the step 0.4 of the other sums the combined error grows; at weight 100 the step is
stable, and the spot term wins: the lens focuses and the chief rays tilt).  The run prints the
largest ``|mean direction cosine|`` over the object points before and after.

    python examples/imaging.py --telecentric [WEIGHT] [--rays 20000] [--steps 30] [--generic]

``--round-spots [WEIGHT]`` adds the astigmatism term of an imaging merit function: the spot of
every object point must be ROUND -- equal and uncorrelated widths along y and z --, at whatever
size the ``SpotError`` beside it reaches:
``SumError([SpotError, MomentError(("y_end", "z_end"), labels, domain, shape="round")],
weights=[1, WEIGHT], reduce="mean")``.  The ``MomentError`` charges every ray the squared
anisotropic part of its spot's covariance, ``(Cxx - Cyy)**2 / 2 + 2 * Cxy**2``; the run prints the
largest anisotropy ``sqrt((Cxx - Cyy)**2 + 4 * Cxy**2) / (Cxx + Cyy)`` over the object points
before and after.  The term is stiff beside the spot term: at the step 0.4 of the other sums weight
10 is stable and weight 100 diverges, so the step is ``min(0.4, 4 / WEIGHT)``.

    python examples/imaging.py --round-spots [WEIGHT] [--rays 20000] [--steps 30] [--generic]
"""
import argparse
import math
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

LEARNING_RATE = 2e-5     # at 20,000 rays
MEAN_LEARNING_RATE = 0.4  # --magnification: LEARNING_RATE * 20,000 rays * 2 terms per ray, halved
                          # because two terms pull
TELECENTRIC_WEIGHT = 1000.0  # --telecentric: squared direction cosines against squared radii
TELECENTRIC_STEP = 100.0    # --telecentric: the largest weight * learning rate that is stable
FLAT_WEIGHT_CONES = 16.0  # --flat-field: the FlatFieldError's weight in units of sin(cone)^2
ROUND_WEIGHT = 1.0       # --round-spots: squared covariance residuals against squared radii
ROUND_STEP = 4.0         # --round-spots: the largest weight * learning rate that was stable
HALF_DIRECTION = 0.5     # --telecentric: the (y_dir, z_dir) of a finished ray that counts
HALF_DOMAIN = 3.0        # the target region: the unfocused cone of a ray bundle has radius ~1.6


def letter_f(size=0.2):
    """The object points: an "F" of height 2 * size in the (y, z) plane, (P, 3) with x = 0 --
    a backbone of 15 points, a top bar of 8 and a middle bar of 5."""
    backbone = [(-0.5 * size, z) for z in np.linspace(-size, size, 15)]
    top = [(y, size) for y in np.linspace(-0.5 * size, 0.75 * size, 9)[1:]]
    middle = [(y, 0.0) for y in np.linspace(-0.5 * size, 0.4 * size, 6)[1:]]
    yz = np.array(backbone + top + middle, dtype=np.float64)
    return np.concatenate([np.zeros((yz.shape[0], 1)), yz], axis=1)


def gaussian_pupil(sigma, cone):
    """The weights of ``--apodize``: a callable on the source's field dict."""
    scale = sigma * math.sin(cone)

    def weights(src):
        d = [src[a + "_end"].double() - src[a + "_start"].double() for a in "xyz"]
        sin2 = (d[1] * d[1] + d[2] * d[2]) / (d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        return torch.exp(-0.5 * sin2 / (scale * scale))
    return weights


def focus_spread(term):
    """The spread of the foci of ``term``'s last evaluation along its axis: the largest minus the
    smallest height of a group with a focus."""
    h = term.heights()
    h = h[torch.isfinite(h)]
    return float(h.max() - h.min())


def anisotropy(term):
    """The largest ``sqrt((Cxx - Cyy)**2 + 4 * Cxy**2) / (Cxx + Cyy)`` over the groups of
    ``term``'s last evaluation: 0 for a round spot, 1 for a line."""
    C = term.covariances()
    C = C[torch.isfinite(C).all(dim=1) & (C[:, 0] + C[:, 2] > 0)]
    d = C[:, 0] - C[:, 2]
    return float((torch.sqrt(d * d + 4.0 * C[:, 1] * C[:, 1]) / (C[:, 0] + C[:, 2])).max())


def build(ray_count=20000, lens_res_scale=0.12, source_distance=10.0, target_distance=10.0,
          object_size=0.2, lens_aperature=1.0, apodize=None, magnification=None, focus=False,
          distortion=None, flat_field=False, flat_weight=None, telecentric=None,
          round_spots=None):
    points = letter_f(object_size)
    P = points.shape[0]
    A = max(ray_count // P, 2)
    n_rays = P * A
    # ray i leaves object point i mod P: the points tiled A times, one random direction each
    base_points = distributions.ManualBasePointDistribution(3, points=np.tile(points, (A, 1)))
    # (the cone that just fills the lens from the farthest object point)
    cone = math.atan((0.95 * lens_aperature - 1.25 * object_size) / source_distance)
    directions = distributions.RandomUniformSphere(cone, n_rays)
    source = sources.AngularSource(3, (-source_distance, 0.0, 0.0), (1.0, 0.0, 0.0), directions,
                                   base_points, [drawing.YELLOW], dense=False)
    labels = np.arange(n_rays) % P

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
        center=(target_distance, 0, 0), direction=(1, 0, 0), i_size=100, j_size=100))
    target.frozen = True

    system = engine.OpticalSystem3D()
    system.optical = lens.surfaces
    system.targets = [target]
    system.sources = [source]
    system.materials = [{"n": materials.vacuum}, {"n": materials.acrylic}]
    system.update()

    trace_engine = engine.OpticalEngine(
        3, [operation.StandardReaction()], compile_active_rays=False,
        simple_ray_inheritance={"wavelength"})
    trace_engine.optical_system = system
    trace_engine.validate_system()

    # a ray that leaves the target region is pulled back instead of dragging its spot along
    error_function = optimizer.SpotError(
        ("y_end", "z_end"), labels, ((-HALF_DOMAIN, HALF_DOMAIN), (-HALF_DOMAIN, HALF_DOMAIN)),
        oob_weight=1.0, weights=None if apodize is None else gaussian_pupil(apodize, cone))
    flat_term = None
    if focus or flat_field:
        # the box contains the target plane: every ray that lands in the target region counts
        box = ((target_distance - 1.0, target_distance + 1.0),
               (-HALF_DOMAIN, HALF_DOMAIN), (-HALF_DOMAIN, HALF_DOMAIN))
        error_function = optimizer.FocusError(labels, box, min_det=1e-9)
    spot = error_function
    if flat_field:
        flat_term = optimizer.FlatFieldError(labels, box, axis=(1.0, 0.0, 0.0), min_det=1e-9)
        if flat_weight is None:
            # in units of sin(cone)^2: an axial distance dz blurs the image by dz * sin(cone), and
            # a focus moves along the axis about 1 / sin(cone) times as far as the rays that make
            # it move are displaced across -- the term is that much stiffer than the FocusError,
            # and at weight 1 the example's step size diverges.  16 sin(cone)^2 = 0.078 lowers
            # the spread of the foci at that step size; 4 and 1 do so more slowly
            flat_weight = FLAT_WEIGHT_CONES * math.sin(cone) ** 2
        error_function = optimizer.SumError([spot, flat_term], weights=[1.0, flat_weight],
                                            reduce="mean")
    if magnification is not None:
        # ray i leaves object point i mod P whatever direction is drawn for it: the image points
        # are a fixed table with one row per source ray
        image = -float(magnification) * np.tile(points, (A, 1))[:, 1:]
        error_function = optimizer.SumError(
            [spot, optimizer.GoalError(("y_end", "z_end"),
                                       torch.as_tensor(image).to(lens.parameters[0].device))],
            reduce="mean")
    distortion_term = None
    if distortion is not None:
        # the object points in the fields' order (y, z): one row per label
        distortion_term = optimizer.DistortionError(
            ("y_end", "z_end"), labels, points[:, 1:],
            ((-HALF_DOMAIN, HALF_DOMAIN), (-HALF_DOMAIN, HALF_DOMAIN)), fit=distortion)
        error_function = optimizer.SumError([spot, distortion_term], reduce="mean")
    tele_term = None
    if telecentric is not None:
        # one target per label: the mean (y_dir, z_dir) of every object point's bundle is 0
        tele_term = optimizer.CentroidError(
            ("y_dir", "z_dir"), labels,
            ((-HALF_DIRECTION, HALF_DIRECTION), (-HALF_DIRECTION, HALF_DIRECTION)),
            targets=np.zeros((P, 2)))
        error_function = optimizer.SumError([spot, tele_term], weights=[1.0, float(telecentric)],
                                            reduce="mean")
    round_term = None
    if round_spots is not None:
        round_term = optimizer.MomentError(
            ("y_end", "z_end"), labels,
            ((-HALF_DOMAIN, HALF_DOMAIN), (-HALF_DOMAIN, HALF_DOMAIN)), shape="round")
        error_function = optimizer.SumError([spot, round_term], weights=[1.0, float(round_spots)],
                                            reduce="mean")
    return dict(engine=trace_engine, system=system, lens=lens, source=source, n_rays=n_rays,
                n_points=P, error_function=error_function, spot=spot, accumulator=accumulator,
                distortion=distortion_term, flat_field=flat_term, telecentric=tele_term,
                round_spots=round_term)


def run(ray_count=20000, steps=30, lens_res_scale=0.12, generic=False, adam=False, verbose=True,
        learning_rate=None, apodize=None, magnification=None, focus=False, distortion=None,
        flat_field=False, flat_weight=None, telecentric=None, round_spots=None):
    s = build(ray_count, lens_res_scale, apodize=apodize, magnification=magnification, focus=focus,
              distortion=distortion, flat_field=flat_field, flat_weight=flat_weight,
              telecentric=telecentric, round_spots=round_spots)
    focus = focus or flat_field
    combined, erf = s["error_function"], s["spot"]
    if learning_rate is None:
        # (the error is a sum over the rays: the step size goes with 1 / rays)
        learning_rate = LEARNING_RATE * (20000 / s["n_rays"])
        if magnification is not None or distortion is not None or flat_field \
                or telecentric is not None or round_spots is not None:
            # (a mean over two terms per ray: the same step per ray as the sum's)
            learning_rate = MEAN_LEARNING_RATE
        if telecentric is not None and telecentric > 0.0:
            learning_rate = min(MEAN_LEARNING_RATE, TELECENTRIC_STEP / telecentric)
        if round_spots is not None and round_spots > 0.0:
            learning_rate = min(MEAN_LEARNING_RATE, ROUND_STEP / round_spots)
    kw = dict(learning_rate=learning_rate, grad_clip=1.0, fused=False if generic else "auto")
    if adam:
        opt = optimizer.Adam_Optimizer(s["engine"], s["lens"].parameters, combined, 3,
                                       adam_learning_rate=3e-4, **kw)
    else:
        opt = optimizer.SGD_Optimizer(s["engine"], s["lens"].parameters, combined, 3, **kw)
    opt.suppress_warnings = True
    rms, times, errors, place, fits, spreads, tilts, shapes = [], [], [], [], [], [], [], []
    summed = magnification is not None or distortion is not None or flat_field \
        or telecentric is not None or round_spots is not None
    for step in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mean = float(opt.single_step(s["accumulator"] if step < steps // 2 else None))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        if apodize is None:
            inside = light = int(erf.last_acc[:, 0].sum())
        else:
            # (weighted records: W = sum wq in units of 2^-wbits, the ray count in slot 5)
            inside = int(erf.last_acc[:, 5].sum())
            light = math.ldexp(int(erf.last_acc[:, 0].sum()), -erf.graph_key()[-1])
        errors.append(mean)
        if not summed:
            error_sum = mean * float(opt.last_error_terms)
        else:
            # (the terms' own triples {sum, terms, mean} of the step)
            error_sum = float(combined.last_errors[0, 0])
            place.append(float(combined.last_errors[1, 2]))
        rms.append(math.sqrt(error_sum / light) if inside else float("nan"))
        if flat_field:
            # (read outside the timed part of the step)
            spreads.append(focus_spread(s["flat_field"]))
        if telecentric is not None:
            # (read outside the timed part of the step)
            c = s["telecentric"].centroids()
            tilts.append(float(c[torch.isfinite(c).all(dim=1)].abs().max()))
        if round_spots is not None:
            # (read outside the timed part of the step)
            shapes.append(anisotropy(s["round_spots"]))
        if verbose and (step % 5 == 0 or step == steps - 1):
            extra = "" if magnification is None else \
                f"  mean squared image distance {place[-1]:.6g}  combined {mean:.6g}"
            if distortion is not None:
                fit = s["distortion"].fit_parameters()
                r = s["distortion"].residuals()
                worst = float(torch.linalg.norm(r[torch.isfinite(r).all(dim=1)], dim=1).max())
                scale = fit["magnification"] if distortion == "scale" else \
                    float(torch.linalg.det(fit["matrix"]))
                fits.append((scale, worst))
                extra = (f"  mean squared distortion {place[-1]:.6g}  combined {mean:.6g}  "
                         f"{'magnification' if distortion == 'scale' else 'det A'} {scale:.6g}  "
                         f"largest |r| {worst:.6g}")
            if flat_field:
                extra = (f"  mean squared distance to the plane {place[-1]:.6g}  combined "
                         f"{mean:.6g}  spread of the foci {spreads[-1]:.6g}")
            if telecentric is not None:
                extra = (f"  mean squared mean direction {place[-1]:.6g}  combined {mean:.6g}  "
                         f"largest |mean direction cosine| {tilts[-1]:.6g}")
            if round_spots is not None:
                extra = (f"  mean squared covariance residual {place[-1]:.6g}  combined "
                         f"{mean:.6g}  largest anisotropy {shapes[-1]:.6g}")
            what = "rms distance to the focus" if focus else "rms spot"
            print(f"step {step:4d}: {what} {rms[-1]:.6g}{extra}  ({inside} rays inside, "
                  f"{1e3 * times[-1]:.2f} ms)")
    fused = opt._fused_step
    s.update(rms=rms, times=times, errors=errors, place=place, fits=fits, spreads=spreads,
             tilts=tilts, shapes=shapes,
             graph_replays=0 if fused is None else fused.graph_replays,
             centroids=erf.foci() if focus else erf.centroids())
    return s


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--edge", type=float, default=0.12, help="lens mesh edge")
    ap.add_argument("--generic", action="store_true", help="the generic path (fused=False)")
    ap.add_argument("--adam", action="store_true", help="an Adam_Optimizer instead of plain SGD")
    ap.add_argument("--lr", type=float, default=None,
                    help=f"learning rate (default {LEARNING_RATE} * 20000 / rays)")
    ap.add_argument("--apodize", type=float, default=None, metavar="SIGMA",
                    help="Gaussian pupil weights, SIGMA in units of the cone that fills the lens")
    ap.add_argument("--magnification", type=float, default=None, metavar="M",
                    help="pin the image of (y, z) to (-M y, -M z): SumError([SpotError, GoalError])")
    ap.add_argument("--focus", action="store_true",
                    help="a FocusError in the place of the SpotError: the axial position is free")
    ap.add_argument("--flat-field", action="store_true",
                    help="SumError([FocusError, FlatFieldError]): a sharp image on a flat sensor, "
                         "wherever along the axis it has to stand")
    ap.add_argument("--flat-weight", type=float, default=None, metavar="W",
                    help="--flat-field: the weight of the FlatFieldError beside the FocusError "
                         f"(default {FLAT_WEIGHT_CONES} * sin(cone)^2)")
    ap.add_argument("--distortion", nargs="?", const="scale", default=None,
                    choices=("scale", "affine"),
                    help="SumError([SpotError, DistortionError]): an undistorted image at a free "
                         "magnification (scale) or under a free 2 x 2 matrix (affine)")
    ap.add_argument("--telecentric", nargs="?", type=float, const=TELECENTRIC_WEIGHT, default=None,
                    metavar="WEIGHT",
                    help="SumError([SpotError, CentroidError((y_dir, z_dir), targets=0)]): the mean "
                         "direction of every object point's bundle along the axis (default "
                         f"WEIGHT {TELECENTRIC_WEIGHT:g}; the step is min({MEAN_LEARNING_RATE}, "
                         f"{TELECENTRIC_STEP:g} / WEIGHT))")
    ap.add_argument("--round-spots", nargs="?", type=float, const=ROUND_WEIGHT, default=None,
                    metavar="WEIGHT",
                    help="SumError([SpotError, MomentError((y_end, z_end), shape='round')]): every "
                         f"object point's spot round at whatever size (default WEIGHT "
                         f"{ROUND_WEIGHT:g}; the step is min({MEAN_LEARNING_RATE}, "
                         f"{ROUND_STEP:g} / WEIGHT))")
    a = ap.parse_args()
    if a.focus and (a.apodize is not None or a.magnification is not None):
        ap.error("--focus takes neither --apodize nor --magnification")
    if a.distortion is not None and (a.focus or a.magnification is not None):
        ap.error("--distortion takes neither --magnification nor --focus")
    if a.flat_field and (a.apodize is not None or a.magnification is not None
                         or a.distortion is not None):
        ap.error("--flat-field takes neither --apodize nor --magnification nor --distortion")
    if a.telecentric is not None:
        if a.focus or a.flat_field or a.magnification is not None or a.distortion is not None:
            ap.error("--telecentric takes none of --focus, --flat-field, --magnification and "
                     "--distortion")
        if not (a.telecentric >= 0.0 and math.isfinite(a.telecentric)):
            ap.error("--telecentric WEIGHT must be finite and >= 0")
    if a.round_spots is not None:
        if a.focus or a.flat_field or a.magnification is not None or a.distortion is not None \
                or a.telecentric is not None or a.apodize is not None:
            ap.error("--round-spots takes none of --focus, --flat-field, --magnification, "
                     "--distortion, --telecentric and --apodize")
        if not (a.round_spots >= 0.0 and math.isfinite(a.round_spots)):
            ap.error("--round-spots WEIGHT must be finite and >= 0")
    out = run(a.rays, a.steps, a.edge, generic=a.generic, adam=a.adam, learning_rate=a.lr,
              apodize=a.apodize, magnification=a.magnification, focus=a.focus,
              distortion=a.distortion, flat_field=a.flat_field, flat_weight=a.flat_weight,
              telecentric=a.telecentric, round_spots=a.round_spots)
    tail = sorted(out["times"][len(out["times"]) // 2:])
    print(f"{out['n_points']} object points, {out['n_rays']} rays; steps replayed from the graph: "
          f"{out['graph_replays']} of {a.steps}; median step of the second half: "
          f"{1e3 * tail[len(tail) // 2]:.3f} ms")
    if a.flat_field:
        print(f"spread of the foci along the axis: first {out['spreads'][0]:.6g} last "
              f"{out['spreads'][-1]:.6g}")
        plane = out["flat_field"].plane()
        print(f"plane of the foci: offset {plane['offset']:.6g} along {plane['axis']}, "
              f"{plane['groups_used']} object points")
        print(f"mean squared distance to the plane: first {out['place'][0]:.6g} last "
              f"{out['place'][-1]:.6g}")
        print(f"combined error: first {out['errors'][0]:.6g} last {out['errors'][-1]:.6g}")
    if a.focus or a.flat_field:
        # (the mean squared distance of a group's focus from its rays' lines)
        first, last = (out["rms"][0] ** 2, out["rms"][-1] ** 2) if a.flat_field else \
            (out["errors"][0], out["errors"][-1])
        print(f"focus error: first {first:.6g} last {last:.6g}")
        x = out["centroids"][:, 0]
        x = x[torch.isfinite(x)]
        print(f"foci of {x.numel()} object points: x from {float(x.min()):.6g} to "
              f"{float(x.max()):.6g}, spread {float(x.max() - x.min()):.6g} (field curvature)")
    else:
        print(f"rms spot: first {out['rms'][0]:.6g} last {out['rms'][-1]:.6g}")
    if a.distortion is not None:
        print(f"mean squared distortion: first {out['place'][0]:.6g} last {out['place'][-1]:.6g}")
        print(f"combined error: first {out['errors'][0]:.6g} last {out['errors'][-1]:.6g}")
        scale, worst = out["fits"][-1]
        print(f"fitted {'magnification' if a.distortion == 'scale' else 'det A'} {scale:.6g}, "
              f"largest |r| {worst:.6g}")
    if a.magnification is not None:
        print(f"mean squared image distance: first {out['place'][0]:.6g} last "
              f"{out['place'][-1]:.6g}")
        print(f"combined error: first {out['errors'][0]:.6g} last {out['errors'][-1]:.6g}")
    if a.telecentric is not None:
        print(f"mean squared mean direction: first {out['place'][0]:.6g} last "
              f"{out['place'][-1]:.6g}")
        print(f"combined error: first {out['errors'][0]:.6g} last {out['errors'][-1]:.6g}")
        print(f"largest |mean direction cosine| over {out['n_points']} object points: first "
              f"{out['tilts'][0]:.6g} last {out['tilts'][-1]:.6g}")
    if a.round_spots is not None:
        print(f"mean squared covariance residual: first {out['place'][0]:.6g} last "
              f"{out['place'][-1]:.6g}")
        print(f"combined error: first {out['errors'][0]:.6g} last {out['errors'][-1]:.6g}")
        print(f"largest anisotropy over {out['n_points']} object points: first "
              f"{out['shapes'][0]:.6g} last {out['shapes'][-1]:.6g}")
