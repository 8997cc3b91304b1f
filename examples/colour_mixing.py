#!/usr/bin/env python3
"""
Colour mixing: the four dies of an RGBW emitter behind one collimating lens must fill the far
field in the same way -- no coloured fringes --, while all of them together make a given beam.

The scene is that of examples/collimator.py: P object points on a plane at x = -10, from each of
them A rays in random directions inside a cone towards the lens, the two-surface parametric lens
of examples/hexalens.py, a plane at x = +10 that merely ends the rays.  The object points are dealt
to four "dies" by the quadrant of the object plane they lie in; a ray carries the label of its
object point's die.  The objective is

    SumError([DensityError(("y_dir", "z_dir"), far_field_goal, ...),
              MixingError(("y_dir", "z_dir"), dies, ...)], weights=[1, MIX], reduce="mean")

-- the pooled far field must be the Gaussian beam of ``collimator.py --density-error``, and every
die's far field must be the pooled one, whatever that is.  A lens that collimates turns the place
of a die into a direction: the better the beam, the further the colours separate.  The run shows
that and what the ``MixingError`` does about it, in two phases on one captured step: the first half
of the steps with ``MIX = 0`` (``SumError.set_weights``; the term is still evaluated, so its
read-outs show the colours separating), the second half with ``MIX = --mix-weight``.  It prints
``max(group_errors())`` -- the mean squared difference of the worst die's far field from the pooled
one, in units of the uniform density -- when the term is switched on and at the end, and what it
was on the slab the lens starts as.

The directions are re-drawn at every step; the labels stay.  ``--lambertian-weights`` weighs
every ray by the cosine of its angle to the axis (a Lambertian die sampled uniformly in solid
angle): both terms then work on radiant power.  The optimiser runs the step as one fixed launch
sequence replayed from a HIP graph once the engine traces the source in place; ``--generic`` keeps
the generic path (the same kernels under torch.autograd).

    python examples/colour_mixing.py [--rays 20000] [--steps 30] [--bins 16] [--mix-weight 0.5]
                                     [--generic] [--lambertian-weights]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tfrt.optimizer as optimizer            # noqa: E402
import collimator                             # noqa: E402
import imaging                                # noqa: E402

BINS = 16                # per axis: a die's share of 20,000 rays still fills the beam's bins
MIX_WEIGHT = 0.5         # a squared density difference in units of the uniform density against
#                          the DensityError's unit-norm one


def dies_of(points):
    """The die of every object point: the quadrant of the (y, z) plane it lies in, 0 .. 3."""
    return (points[:, 1] > 0).astype(np.int64) * 2 + (points[:, 2] > 0).astype(np.int64)


def lambertian(src):
    """The weights of ``--lambertian-weights``: the cosine of a source ray's angle to the x axis."""
    d = [src[a + "_end"].double() - src[a + "_start"].double() for a in "xyz"]
    return d[0] / torch.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def build(ray_count=20000, lens_res_scale=0.12, bins=BINS, mix_weight=MIX_WEIGHT,
          lambertian_weights=False):
    s = imaging.build(ray_count, lens_res_scale)
    fields = ("y_dir", "z_dir")
    h = collimator.DENSITY_HALF_DOMAIN
    domain = ((-h, h), (-h, h))
    oob = 1.0 / (s["n_rays"] * h ** 2)
    weights = lambertian if lambertian_weights else None
    # ray i leaves object point i mod P: one die label per source ray
    dies = dies_of(imaging.letter_f())[np.arange(s["n_rays"]) % s["n_points"]]
    density = optimizer.DensityError(fields, collimator.far_field_goal, domain, oob_weight=oob,
                                     bins=bins, weights=weights)
    mixing = optimizer.MixingError(fields, dies, domain, bins, oob_weight=oob, n_groups=4,
                                   weights=weights)
    s["density"], s["mixing"], s["mix_weight"] = density, mixing, float(mix_weight)
    s["error_function"] = optimizer.SumError([density, mixing], weights=[1.0, 0.0], reduce="mean")
    return s


def run(ray_count=20000, steps=30, lens_res_scale=0.12, generic=False, bins=BINS,
        mix_weight=MIX_WEIGHT, lambertian_weights=False, verbose=True, learning_rate=None):
    s = build(ray_count, lens_res_scale, bins, mix_weight, lambertian_weights)
    erf, mixing = s["error_function"], s["mixing"]
    if learning_rate is None:
        learning_rate = collimator.DENSITY_LEARNING_RATE
    opt = optimizer.SGD_Optimizer(s["engine"], s["lens"].parameters, erf, 3,
                                  learning_rate=learning_rate, grad_clip=1.0,
                                  fused=False if generic else "auto")
    opt.suppress_warnings = True
    switch = steps // 2
    errors, worst, times = [], [], []
    for step in range(steps):
        if step == switch:
            erf.set_weights([1.0, s["mix_weight"]])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        errors.append(float(opt.single_step(s["accumulator"] if step < switch else None)))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        e = mixing.group_errors()
        worst.append(float(e[torch.isfinite(e)].max()))
        if verbose and (step % 5 == 0 or step in (switch, steps - 1)):
            density, mix = (float(v) for v in erf.last_errors[:, 0])
            print(f"step {step:4d}: density error {density:.6g}  mixing error {mix:.6g}  "
                  f"max group error {worst[-1]:.6g}  ({1e3 * times[-1]:.2f} ms)")
    fused = opt._fused_step
    s.update(errors=errors, worst=worst, times=times, switch=switch,
             graph_replays=0 if fused is None else fused.graph_replays)
    return s


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--edge", type=float, default=0.12, help="lens mesh edge")
    ap.add_argument("--bins", type=int, default=BINS, help="bins per axis of both terms' grids")
    ap.add_argument("--mix-weight", type=float, default=MIX_WEIGHT,
                    help="the MixingError's weight in the second half of the steps")
    ap.add_argument("--generic", action="store_true", help="the generic path (fused=False)")
    ap.add_argument("--lambertian-weights", action="store_true",
                    help="weigh every ray by the cosine of its angle to the axis")
    ap.add_argument("--lr", type=float, default=None, help="learning rate")
    a = ap.parse_args()
    out = run(a.rays, a.steps, a.edge, generic=a.generic, bins=a.bins, mix_weight=a.mix_weight,
              lambertian_weights=a.lambertian_weights, learning_rate=a.lr)
    tail = sorted(out["times"][len(out["times"]) // 2:])
    print(f"{out['n_points']} object points on 4 dies, {out['n_rays']} rays; steps replayed from "
          f"the graph: {out['graph_replays']} of {a.steps}; median step of the second half: "
          f"{1e3 * tail[len(tail) // 2]:.3f} ms")
    print(f"max group error on the slab: {out['worst'][0]:.6g}")
    print(f"max group error: first {out['worst'][out['switch']]:.6g} last {out['worst'][-1]:.6g}")
