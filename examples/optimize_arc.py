#!/usr/bin/env python3
"""
Counterpart of the reference's dev/optimize_single_arc.py: one acrylic arc whose centre and
radius are the SAME parameter (``arc["x_center"] = parameter; arc["radius"] = parameter``) is
shaped by gradient descent so that a beam focuses on a target wall at x = 10
(error = finished["y_end"] ** 2).

The reference's error is a GoalError (goal: y_end = 0), so on the GPU SGD_Optimizer runs the fused
2-D step -- update, tfrt_trace2d_forward, tfrt_trace2d_backward_goal, parameter update -- captured
in one HIP graph after a few eager steps.  The reference's optimiser is Keras SGD with learning
rate 1, Nesterov momentum 0.8 and the gradient clipped to 0.1; ``--momentum`` runs that rule
(without it: plain SGD); ``--adam`` runs an ``Adam_Optimizer`` instead (the Keras Adam rule,
adam_learning_rate 0.05, on the same clipped gradient and the same fused step).  ``--rowwise`` states the same error as
``RowwiseError(lambda r: r["y_end"] ** 2)``, any element-wise torch function's form: the fused step
then evaluates it on fixed-shape columns (tfrt_trace2d_rows, tfrt_trace2d_backward_rows) inside
the same graph.  ``--generic`` forces the generic path (user error function, autograd) for
comparison.  ``--deterministic`` sums the reverse sweep's gradients in an order-independent way
(``OpticalEngine(deterministic=True)``): the whole run is bit-identical from one run to the next.
``--random-source`` shapes the same lens over a beam that is re-drawn at every step (a
``RandomUniformBeam``, one wavelength, one ray per beam point: stochastic gradient descent proper).
On the GPU the source is a device program -- ``update()`` steps a counter, one launch writes the
rays of the new draw into the same buffers --, so the step is captured like the static one; the
run prints whether it was, and the mean step time by device events after ``--warmup`` steps.
``--pool-source`` is the staged workflow of the reference's dev/precompile_*.py in 2-D: stage 1 traces
a static fan through a FIXED biconvex front lens once and stores the finished rays in a
``PrecompiledSource`` (``from_samples``); stage 2 shapes the arc over ``--rays`` rays re-sampled
from that pool at every step, their end points jittered by a small normal perturbation.  On the GPU
the pool is a device program too (TFRT_SRC_POOL: uploaded once, rows and jitter drawn inside the
step's graph); ``--host`` switches that off (``distributions.set_device_random(False)``: the rows
are drawn and the pool indexed on the host every step) for comparison.  This mode prints one JSON
line: ms_per_step, graph_replays and whether the step was replayed from a graph, device_mode, and
the error of the first and the last step.
No GUI.

    python examples/optimize_arc.py [--rays 10] [--steps 30] [--momentum | --adam] [--rowwise] [--generic]
                                    [--deterministic] [--random-source [--warmup 5]]
                                    [--pool-source [--host] [--pool-rays 16384] [--sigma 1e-3]]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tfrt.boundaries as boundaries          # noqa: E402
import tfrt.distributions as distributions    # noqa: E402
import tfrt.drawing as drawing                # noqa: E402
import tfrt.engine as engine                  # noqa: E402
import tfrt.materials as materials            # noqa: E402
import tfrt.operation as operation            # noqa: E402
import tfrt.optimizer as optimizer            # noqa: E402
import tfrt.sources as sources                # noqa: E402

PI = math.pi
POOL_FIELDS = ("x_start", "y_start", "x_end", "y_end", "wavelength")


def stage_one(pool_rays=16384, ray_dtype=torch.float64):
    """The pool of ``--pool-source``: a static fan from (-14, 0) through a fixed biconvex acrylic
    lens (vertices at x = -8 and x = -7.4, radii 6: the fan leaves it roughly collimated) onto a
    wall at x = -4; the finished rays, with their wavelength."""
    def lens_arc(x_center, angle_start, angle_end):
        arc = boundaries.ManualArcBoundary()
        arc["x_center"] = np.array([x_center])
        arc["y_center"] = np.array([0.0])
        arc["angle_start"] = np.array([angle_start])
        arc["angle_end"] = np.array([angle_end])
        arc["radius"] = np.array([6.0])
        arc["mat_in"] = np.array([1], dtype=np.int64)
        arc["mat_out"] = np.array([0], dtype=np.int64)
        arc.frozen = True
        return arc

    wall = boundaries.ManualSegmentBoundary()
    wall.feed_segments(np.array([[-4, -5, -4, 5]], dtype=np.float64))
    wall.frozen = True
    fan = distributions.StaticUniformAngularDistribution(-0.17, 0.17, pool_rays)
    source = sources.PointSource(2, (-14.0, 0.0), 0.0, fan, drawing.RAINBOW_6[3:4])
    source.frozen = True
    system = engine.OpticalSystem2D()
    system.optical_arcs = [lens_arc(-2.0, 3 * PI / 4, 5 * PI / 4), lens_arc(-13.4, -PI / 4, PI / 4)]
    system.sources = [source]
    system.target_segments = [wall]
    system.materials = [{"n": materials.vacuum}, {"n": materials.acrylic}]
    eng = engine.OpticalEngine(2, [operation.StandardReaction()],
                               simple_ray_inheritance={"wavelength"}, ray_dtype=ray_dtype,
                               compile_active_rays=False)
    eng.optical_system = system
    system.update()
    eng.validate_system()
    eng.ray_trace(3)
    fin = eng.finished_rays
    return {f: fin[f].detach().clone() for f in POOL_FIELDS}


def build(ray_count=10, ray_dtype=torch.float64, device="cuda:0", deterministic=False,
          random_source=False, pool_source=False, pool_rays=16384, sigma=1e-3):
    parameter = torch.tensor([5.0], dtype=torch.float64, device=device, requires_grad=True)
    arc = boundaries.ManualArcBoundary()
    arc["x_center"] = parameter
    arc["y_center"] = np.array([0.0])
    arc["angle_start"] = np.array([3 * PI / 4])
    arc["angle_end"] = np.array([5 * PI / 4])
    arc["radius"] = parameter
    engine.annotation_helper(arc, "mat_in", 1, "x_center", dtype=torch.int64)
    engine.annotation_helper(arc, "mat_out", 0, "x_center", dtype=torch.int64)

    target = boundaries.ManualSegmentBoundary()
    target.feed_segments(np.array([[10, -5, 10, 5]], dtype=np.float64))
    target.frozen = True

    angles = distributions.StaticUniformAngularDistribution(0, 0, 1)
    if pool_source:
        # re-sampled with replacement by every update(), the end points jittered along y
        source = sources.PrecompiledSource(2, sample_count=ray_count,
                                           end_perturbation=None if sigma == 0 else (0.0, sigma))
        source.from_samples([stage_one(pool_rays, ray_dtype)])
    elif random_source:
        # re-drawn by every update(): one ray per beam point (an undense source), one wavelength
        beam_points = distributions.RandomUniformBeam(-1.5, 1.5, ray_count)
        source = sources.AngularSource(2, (-1.0, 0.0), 0.0, angles, beam_points,
                                       drawing.RAINBOW_6[3:4], dense=False)
    else:
        beam_points = distributions.StaticUniformBeam(-1.5, 1.5, ray_count)
        source = sources.AngularSource(2, (-1.0, 0.0), 0.0, angles, beam_points, drawing.RAINBOW_6)
        source.frozen = True

    system = engine.OpticalSystem2D()
    system.optical_arcs = [arc]
    system.sources = [source]
    system.target_segments = [target]
    system.materials = [{"n": materials.vacuum}, {"n": materials.acrylic}]

    trace_engine = engine.OpticalEngine(2, [operation.StandardReaction()],
                                        simple_ray_inheritance={"wavelength"},
                                        ray_dtype=ray_dtype, deterministic=deterministic)
    trace_engine.optical_system = system
    system.update()
    trace_engine.validate_system()
    return dict(parameter=parameter, arc=arc, system=system, engine=trace_engine, source=source)


def make_optimizer(scene, momentum=False, generic=False, rowwise=False, adam=False):
    if rowwise:
        erf = optimizer.RowwiseError(lambda r: r["y_end"] ** 2)
    else:
        n = scene["system"].sources["x_start"].shape[0]
        goal = torch.zeros(n, dtype=torch.float64, device=scene["parameter"].device)
        erf = optimizer.GoalError(("y_end",), goal)
    if adam:
        return optimizer.Adam_Optimizer(scene["engine"], [scene["parameter"]], erf, 2,
                                        learning_rate=1.0, grad_clip=0.1, adam_learning_rate=0.05,
                                        fused=not generic)
    # Keras SGD(learning_rate=1.0, momentum=0.8, nesterov=True) of the reference, gradient clipped
    # to 0.1 before it is applied
    return optimizer.SGD_Optimizer(scene["engine"], [scene["parameter"]], erf, 2,
                                   learning_rate=1.0, grad_clip=0.1, sgd_learning_rate=1.0,
                                   apply_momentum=momentum, fused=not generic)


def run(ray_count=10, steps=30, momentum=False, generic=False, verbose=True, rowwise=False,
        deterministic=False, random_source=False, warmup=0, adam=False):
    """``warmup`` > 0: that many untimed steps first; the mean time of the ``steps`` after them (device
    events around the loop, no host read inside it) is returned as ``ms_per_step``."""
    scene = build(ray_count, deterministic=deterministic, random_source=random_source)
    opt = make_optimizer(scene, momentum, generic, rowwise, adam)
    errors = []
    if warmup > 0:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(warmup + steps):
            if i == warmup:
                t0.record()
            err = opt.single_step(None, momentum=0.8 if momentum else 0.0)
            if i == 0 or i == warmup + steps - 1:
                errors.append(float(err))
        t1.record()
        torch.cuda.synchronize()
        return errors, dict(scene, optimizer=opt, ms_per_step=t0.elapsed_time(t1) / max(steps, 1))
    for i in range(steps):
        # the reference's schedule: 30 steps at learning rate 1, then 0.1 (its momentum stays 0.8:
        # the script's set_momentum call is commented out)
        err = opt.single_step(None, lr_scale=0.1 if i >= 30 else 1.0,
                              momentum=0.8 if momentum else 0.0)
        errors.append(float(err))
        if verbose:
            print(f"step {i + 1}: error {errors[-1]:.6e}  parameter {float(scene['parameter']):.6f}")
    return errors, dict(scene, optimizer=opt)


def run_pool(ray_count=4096, steps=30, warmup=5, host=False, momentum=False, generic=False,
             rowwise=False, pool_rays=16384, sigma=1e-3, verbose=False):
    """``--pool-source``: ``warmup`` untimed steps, then ``steps`` timed ones (device events around
    the loop, no host read inside it).  Returns (result, errors, scene): ``errors`` holds the error
    of every warm-up step and of the last timed one."""
    if host:
        distributions.set_device_random(False)
    scene = build(ray_count, pool_source=True, pool_rays=pool_rays, sigma=sigma)
    opt = make_optimizer(scene, momentum, generic, rowwise)
    kw = dict(momentum=0.8 if momentum else 0.0)
    errors = [float(opt.single_step(None, **kw)) for _ in range(max(warmup, 1))]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    err = None
    for _ in range(steps):
        err = opt.single_step(None, **kw)
    t1.record()
    torch.cuda.synchronize()
    if err is not None:
        errors.append(float(err))
    fs = opt._fused_step
    replays = 0 if fs is None else int(fs.graph_replays)
    pool = scene["source"]
    result = {"ms_per_step": t0.elapsed_time(t1) / max(steps, 1), "graph_replays": replays,
              "graph_replayed": bool(replays > 0 and fs.capture_error is None),
              "device_mode": bool(pool.device_mode), "rays": int(ray_count), "steps": int(steps),
              "pool_rays": int(pool.sampling_domain_size), "error_first": errors[0],
              "error_last": errors[-1], "parameter": float(scene["parameter"].detach())}
    if verbose:
        print(json.dumps(result))
    return result, errors, dict(scene, optimizer=opt)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rays", type=int, default=10,
                    help="beam points (the reference's 10); each is traced at six wavelengths")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--momentum", action="store_true",
                    help="the reference's Nesterov momentum 0.8")
    ap.add_argument("--adam", action="store_true",
                    help="the Keras Adam rule (Adam_Optimizer) instead of SGD")
    ap.add_argument("--rowwise", action="store_true",
                    help="the same error as a RowwiseError (any element-wise error function)")
    ap.add_argument("--generic", action="store_true",
                    help="force the generic optimiser step (for comparison)")
    ap.add_argument("--deterministic", action="store_true",
                    help="bit-reproducible gradients (ordered reverse-sweep sums)")
    ap.add_argument("--random-source", action="store_true",
                    help="re-draw the beam at every step (RandomUniformBeam) and time the steps")
    ap.add_argument("--warmup", type=int, default=5,
                    help="untimed steps before the timed ones (--random-source, --pool-source)")
    ap.add_argument("--pool-source", action="store_true",
                    help="two stages: store the rays behind a fixed front lens, then shape the arc "
                         "over --rays rays re-sampled from them at every step; prints a JSON line")
    ap.add_argument("--host", action="store_true",
                    help="--pool-source: re-sample the pool on the host every step (no device program)")
    ap.add_argument("--pool-rays", type=int, default=16384, help="rays traced in stage 1")
    ap.add_argument("--sigma", type=float, default=1e-3,
                    help="standard deviation of the end points' jitter in y (0: none)")
    a = ap.parse_args()
    if a.pool_source:
        run_pool(a.rays, a.steps, a.warmup, a.host, a.momentum, a.generic, a.rowwise, a.pool_rays,
                 a.sigma, verbose=True)
        return
    errors, s = run(a.rays, a.steps, a.momentum, a.generic, rowwise=a.rowwise,
                    deterministic=a.deterministic, random_source=a.random_source,
                    warmup=max(a.warmup, 1) if a.random_source else 0, verbose=not a.random_source,
                    adam=a.adam)
    fs = s["optimizer"]._fused_step
    path = ("generic" if fs is None else
            f"fused, {fs.graph_replays} of {fs.steps} steps replayed from a HIP graph")
    print(f"error {errors[0]:.6e} -> {errors[-1]:.6e} ({path})")
    if a.random_source:
        captured = fs is not None and fs.graph_replays > 0 and fs.capture_error is None
        made = "device program" if hasattr(s["source"]._fields, "ray_block") else \
            "host draw (torch)"
        print(f"random source: {made}; step captured: {'yes' if captured else 'no'}; "
              f"mean step {s['ms_per_step']:.3f} ms over {a.steps} steps")


if __name__ == "__main__":
    main()
