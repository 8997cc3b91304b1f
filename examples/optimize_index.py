#!/usr/bin/env python3
"""
A 2-D lens whose refractive index is the parameter: the single acrylic-like arc of
optimize_arc.py (centre (5, 0), radius 5, facing the beam), now with StandardReaction("value"):
the arc carries its n_in / n_out as plain fields, and n_in -- the glass behind the surface -- is
the parameter.  Gradient descent on it focuses a collimated beam on the point (10, 0) of a target
wall inside the glass (error = finished["y_end"] ** 2; paraxially n R / (n - 1) = 10 at n = 2).
The arc's shape stays fixed.

With a GoalError the fused 2-D step runs -- update, tfrt_trace2d_forward, tfrt_trace2d_backward_goal
with the index terms (tfrt_scene2d.grad_arc_n_in), parameter update -- captured in one HIP graph
after a few eager steps.  ``--generic`` forces the generic path for comparison.

    python examples/optimize_index.py [--rays 1000] [--steps 40] [--generic]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tfrt.boundaries as boundaries          # noqa: E402
import tfrt.engine as engine                  # noqa: E402
import tfrt.operation as operation            # noqa: E402
import tfrt.optimizer as optimizer            # noqa: E402
import tfrt.sources as sources                # noqa: E402

PI = math.pi


def build(ray_count=1000, n_start=1.5, ray_dtype=torch.float64, device="cuda:0"):
    index = torch.tensor([n_start], dtype=torch.float64, device=device, requires_grad=True)
    arc = boundaries.ManualArcBoundary()
    arc["x_center"] = np.array([5.0])
    arc["y_center"] = np.array([0.0])
    arc["angle_start"] = np.array([3 * PI / 4])
    arc["angle_end"] = np.array([5 * PI / 4])
    arc["radius"] = np.array([5.0])
    arc["n_in"] = index                     # the glass inside the arc's circle
    arc["n_out"] = np.array([1.0])

    target = boundaries.ManualSegmentBoundary()
    target.feed_segments(np.array([[10, -5, 10, 5]], dtype=np.float64))
    target.frozen = True

    ys = np.linspace(-1.5, 1.5, ray_count)
    source = sources.ManualSource(2)
    source["x_start"] = np.full(ray_count, -1.0)
    source["y_start"] = ys
    source["x_end"] = np.zeros(ray_count)
    source["y_end"] = ys
    source["wavelength"] = np.full(ray_count, 550.0)

    system = engine.OpticalSystem2D()
    system.optical_arcs = [arc]
    system.sources = [source]
    system.target_segments = [target]

    trace_engine = engine.OpticalEngine(2, [operation.StandardReaction("value")],
                                        ray_dtype=ray_dtype)
    trace_engine.optical_system = system
    system.update()
    trace_engine.validate_system()
    return dict(parameter=index, system=system, engine=trace_engine)


def make_optimizer(scene, generic=False):
    n = scene["system"].sources["x_start"].shape[0]
    goal = torch.zeros(n, dtype=torch.float64, device=scene["parameter"].device)
    erf = optimizer.GoalError(("y_end",), goal)
    return optimizer.SGD_Optimizer(scene["engine"], [scene["parameter"]], erf, 2,
                                   learning_rate=1.0, grad_clip=0.02, sgd_learning_rate=1.0,
                                   fused=not generic)


def run(ray_count=1000, steps=40, generic=False, verbose=True):
    scene = build(ray_count)
    opt = make_optimizer(scene, generic)
    errors = []
    for i in range(steps):
        errors.append(float(opt.single_step(None)))
        if verbose:
            print(f"step {i + 1}: error {errors[-1]:.6e}  index {float(scene['parameter']):.6f}")
    return errors, dict(scene, optimizer=opt)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rays", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--generic", action="store_true",
                    help="force the generic optimiser step (for comparison)")
    a = ap.parse_args()
    errors, s = run(a.rays, a.steps, a.generic)
    fs = s["optimizer"]._fused_step
    path = ("generic" if fs is None else
            f"fused, {fs.graph_replays} of {fs.steps} steps replayed from a HIP graph")
    print(f"error {errors[0]:.6e} -> {errors[-1]:.6e}, index {float(s['parameter']):.6f} ({path})")


if __name__ == "__main__":
    main()
