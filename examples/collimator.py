#!/usr/bin/env python3
"""
Collimation: a two-surface parametric acrylic lens is shaped so that the rays of every object
point leave it PARALLEL -- an eyepiece, a beam expander, the collimator of a light source.

The scene is that of examples/imaging.py: P object points on a plane at x = -10 -- a small "F" --,
from each of them A rays in random directions inside a cone towards the lens, the lens of
examples/hexalens.py, a plane at x = +10 that merely ends the rays.  The merit function is stated
in the DIRECTION of the outgoing rays, not in where they land: ``optimizer.SpotError`` over
``("y_dir", "z_dir")``, the direction cosines of a finished ray's last link.  The rays carry the
label of their object point, and the error is the summed squared distance of every ray's direction
to the mean direction of its own label: a spot in direction space, the squared RMS angular spot
times the ray count.  Which way each bundle leaves (the angular magnification) is left to the lens.

``--density-error`` swaps in a far-field intensity goal: a ``DensityError`` over
``("y_dir", "z_dir")`` whose goal is a smooth (Gaussian) distribution over the outgoing direction,
whatever plane catches the rays -- how a headlamp or a beam shaper is specified.

The directions are re-drawn at every step.  With either error the optimiser runs the step as one
fixed launch sequence replayed from a HIP graph once the engine traces the source in place;
``--generic`` keeps the generic path (the same kernels under torch.autograd).

    python examples/collimator.py [--rays 20000] [--steps 30] [--adam] [--density-error [--bins 32]] [--generic]
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tfrt.optimizer as optimizer            # noqa: E402
import imaging                                # noqa: E402

# (a direction is a position over the length of the link, ~10 here: the residuals and their
# derivatives are both a tenth of examples/imaging.py's, the step size a hundred times its)
LEARNING_RATE = 2e-3           # at 20,000 rays
HALF_DOMAIN = 0.25             # direction cosines: the unfocused bundles stay within ~0.1
DENSITY_LEARNING_RATE = 0.05
DENSITY_HALF_DOMAIN = 0.12
DENSITY_SIGMA = 0.03
DENSITY_BINS = 32


def far_field_goal(gy, gz):
    """The goal of ``--density-error``: a Gaussian beam around the axis."""
    return torch.exp(-(gy ** 2 + gz ** 2) / (2 * DENSITY_SIGMA ** 2))


def build(ray_count=20000, lens_res_scale=0.12, density_error=False, bins=DENSITY_BINS):
    s = imaging.build(ray_count, lens_res_scale)
    fields = ("y_dir", "z_dir")
    if density_error:
        h = DENSITY_HALF_DOMAIN
        s["error_function"] = optimizer.DensityError(
            fields, far_field_goal, ((-h, h), (-h, h)), oob_weight=1.0 / (s["n_rays"] * h ** 2),
            bins=bins)
    else:
        labels = torch.arange(s["n_rays"]) % s["n_points"]
        # a ray that leaves the domain is pulled back instead of dragging its spot along
        s["error_function"] = optimizer.SpotError(
            fields, labels, ((-HALF_DOMAIN, HALF_DOMAIN), (-HALF_DOMAIN, HALF_DOMAIN)),
            oob_weight=1.0)
    return s


def run(ray_count=20000, steps=30, lens_res_scale=0.12, generic=False, adam=False,
        density_error=False, verbose=True, learning_rate=None, bins=DENSITY_BINS):
    s = build(ray_count, lens_res_scale, density_error, bins)
    erf = s["error_function"]
    if learning_rate is None:
        # (a SpotError is a sum over the rays: the step size goes with 1 / rays; a DensityError is
        # one term of order 1)
        learning_rate = DENSITY_LEARNING_RATE if density_error \
            else LEARNING_RATE * (20000 / s["n_rays"])
    kw = dict(learning_rate=learning_rate, grad_clip=1.0, fused=False if generic else "auto")
    if adam:
        opt = optimizer.Adam_Optimizer(s["engine"], s["lens"].parameters, erf, 3,
                                       adam_learning_rate=3e-4, **kw)
    else:
        opt = optimizer.SGD_Optimizer(s["engine"], s["lens"].parameters, erf, 3, **kw)
    opt.suppress_warnings = True
    errors, times = [], []
    name = "density error" if density_error else "rms angular spot"
    for step in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mean = float(opt.single_step(s["accumulator"] if step < steps // 2 else None))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        if density_error:
            inside = int(round(float(erf.last_hq.sum()) / 2 ** 32))
            errors.append(mean)
        else:
            inside = int(erf.last_acc[:, 0].sum())
            error_sum = mean * float(opt.last_error_terms)
            errors.append(math.sqrt(error_sum / inside) if inside else float("nan"))
        if verbose and (step % 5 == 0 or step == steps - 1):
            print(f"step {step:4d}: {name} {errors[-1]:.6g}  ({inside} rays inside, "
                  f"{1e3 * times[-1]:.2f} ms)")
    fused = opt._fused_step
    s.update(errors=errors, times=times, name=name,
             graph_replays=0 if fused is None else fused.graph_replays)
    return s


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--edge", type=float, default=0.12, help="lens mesh edge")
    ap.add_argument("--generic", action="store_true", help="the generic path (fused=False)")
    ap.add_argument("--adam", action="store_true", help="an Adam_Optimizer instead of plain SGD")
    ap.add_argument("--density-error", action="store_true",
                    help="a far-field DensityError over (y_dir, z_dir) instead of the SpotError")
    ap.add_argument("--bins", type=int, default=DENSITY_BINS,
                    help="bins per axis of the DensityError's grid")
    ap.add_argument("--lr", type=float, default=None, help="learning rate")
    a = ap.parse_args()
    out = run(a.rays, a.steps, a.edge, generic=a.generic, adam=a.adam,
              density_error=a.density_error, learning_rate=a.lr, bins=a.bins)
    tail = sorted(out["times"][len(out["times"]) // 2:])
    print(f"{out['n_points']} object points, {out['n_rays']} rays; steps replayed from the graph: "
          f"{out['graph_replays']} of {a.steps}; median step of the second half: "
          f"{1e3 * tail[len(tail) // 2]:.3f} ms")
    print(f"{out['name']}: first {out['errors'][0]:.6g} last {out['errors'][-1]:.6g}")
