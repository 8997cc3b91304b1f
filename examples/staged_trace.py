#!/usr/bin/env python3
"""
Counterpart of the reference's dev/precompile_save.py / precompile_load.py / precompile_sample.py:
a staged design.  The fixed front part of a system is traced once and the rays that leave it are
stored; the parametric back part is then optimised against a random re-sample of that pool, jittered
by a normal perturbation of the end points, at every step.

    stage 1   a random aperture source (object disc at x = -10) through a FIXED weak lens at x = -5
              onto an intermediate plane at x = -2, a few draws; the finished rays -- with the
              object coordinates they inherit -- go into a PrecompiledSource with from_samples()
    stage 2   the parametric two-surface lens of examples/hexalens.py at x = 0 is shaped so that the
              stored rays image the object onto the plane at x = +10 (a GoalError on the inherited
              object coordinates), the source being PrecompiledSource(sample_count=N,
              end_perturbation=...)

On a HIP device the pool is uploaded once and re-sampled by a device program inside the step's launch
graph (tensorflowraytrace_amd/sources.py, TFRT_SRC_POOL); ``--host`` draws the rows and indexes the
pool on the host every step instead, for comparison.

    python examples/staged_trace.py [--rays 20000] [--steps 30] [--host] [--momentum]

Prints one JSON line: ms_per_step (device events around the timed steps, after a warm-up),
graph_replays, device_mode, and the mean squared image error of the first and last steps.
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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

import hexalens                               # noqa: E402

FIELDS = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end", "wavelength", "object_coords")
# the fixed lens (focal length ~ 20) turns the object at distance 5 into a virtual one at distance
# 6.7 from it, 1.33 times the size; the parametric lens images that, 11.7 in front of it, onto the
# plane 10 behind it
MAGNIFICATION = -(20.0 / 15.0) * (10.0 / (5.0 + 20.0 / 3.0))


def stage_one(rays_per_draw, draws):
    """The pool: finished rays of ``draws`` traces of the fixed front part, as field mappings."""
    start = distributions.RandomUniformCircle(rays_per_draw, 0.2)
    distributions.BasePointTransformation(start, translation=(-10, 0, 0))
    end = distributions.RandomUniformCircle(rays_per_draw, 0.4)
    distributions.BasePointTransformation(end, translation=(-5, 0, 0))
    source = sources.AperatureSource(
        3, start, end, [drawing.YELLOW], dense=False,
        extra_fields={"object_coords": ("start_point", start, "points")})
    zero_points = mt.hexagonal_mesh(1.0, 6)
    zero_points.rotate_y(90)
    zero_points.rotate_x(90)
    r2 = zero_points.points[:, 1] ** 2 + zero_points.points[:, 2] ** 2
    zero_points.translate((-5, 0, 0))
    front = boundaries.ParametricMultiTriangleBoundary(
        zero_points, boundaries.FromVectorVG((1, 0, 0)),
        [boundaries.ThicknessConstraint(0.0, "min"), boundaries.ThicknessConstraint(0.2, "min")],
        [True, False], initial_parameters=[-0.025 * (1 - r2), 0.025 * (1 - r2)],
        material_list=[{"mat_in": 1, "mat_out": 0}] * 2)
    plane = boundaries.ManualTriangleBoundary(
        mesh=mt.plane(center=(-2, 0, 0), direction=(1, 0, 0), i_size=100, j_size=100))
    plane.frozen = True
    system = engine.OpticalSystem3D()
    system.optical = front.surfaces
    system.targets = [plane]
    system.sources = [source]
    system.materials = [{"n": materials.vacuum}, {"n": materials.acrylic}]
    system.update()
    eng = engine.OpticalEngine(3, [operation.StandardReaction()], compile_active_rays=False,
                               simple_ray_inheritance={"wavelength", "object_coords"})
    eng.optical_system = system
    eng.validate_system()
    samples = []
    for _ in range(draws):
        system.update()
        eng.ray_trace(3)
        fin = eng.finished_rays
        samples.append({f: fin[f].detach().clone() for f in FIELDS})
    return samples


def save_pool(samples, filename):
    """The pool as the file a PrecompiledSource loads (tfrt/sources.py:1174-1181, 1207-1218)."""
    fields = {f: np.concatenate([np.asarray(s[f].cpu()) for s in samples], axis=0) for f in FIELDS}
    with open(filename, "wb") as f:
        pickle.dump({"dimension": 3, "standard_domains": set(), "fields": fields}, f,
                    pickle.HIGHEST_PROTOCOL)


def run(ray_count=20000, steps=30, warmup=10, host=False, momentum=False, lens_res_scale=0.12,
        pool_rays=65536, sigma=1e-3, pool_file=None, save_pool_to=None, verbose=False):
    if host:
        distributions.set_device_random(False)
    perturbation = None if sigma == 0 else (0.0, sigma, sigma)      # (the plane's own coordinates)
    if pool_file is None:
        draws = 4
        samples = stage_one(max(pool_rays // draws, 1), draws)
        if save_pool_to:
            save_pool(samples, save_pool_to)
        pool = sources.PrecompiledSource(3, sample_count=ray_count, end_perturbation=perturbation)
        pool.from_samples(samples)
    else:
        pool = sources.PrecompiledSource(pool_file, sample_count=ray_count,
                                         end_perturbation=perturbation)
    s = hexalens.build(64, lens_res_scale)
    system, eng = s["system"], s["engine"]
    system.sources = [pool]
    system.update()
    eng.validate_system()
    erf = optimizer.GoalError(("y_end", "z_end"),
                              lambda src: src["object_coords"][:, 1:] * MAGNIFICATION, rowwise=True)
    learning_rate = 2e-5 * (20000 / ray_count)
    if momentum:
        opt = optimizer.SGD_Optimizer(eng, s["lens"].parameters, erf, 3,
                                      learning_rate=(1 - 0.6) * learning_rate, grad_clip=0.1,
                                      apply_momentum=True, nesterov=True)
    else:
        opt = optimizer.SGD_Optimizer(eng, s["lens"].parameters, erf, 3,
                                      learning_rate=learning_rate, grad_clip=1.0)
    opt.suppress_warnings = True
    kw = dict(momentum=0.6) if momentum else {}
    errors = [opt.single_step(None, **kw) for _ in range(warmup)]
    gpu = torch.cuda.is_available()
    if gpu:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
    errors += [opt.single_step(None, **kw) for _ in range(steps)]
    ms = float("nan")
    if gpu:
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / max(steps, 1)
    errors = [float(e) for e in errors]
    fs = opt._fused_step
    result = {"ms_per_step": ms, "graph_replays": 0 if fs is None else int(fs.graph_replays),
              "device_mode": bool(getattr(pool, "device_mode", False)), "rays": int(ray_count),
              "steps": int(steps), "pool_rays": int(pool.sampling_domain_size),
              "error_first": float(np.mean(errors[:3])), "error_last": float(np.mean(errors[-3:]))}
    if verbose:
        print(json.dumps(result))
    return result, errors, dict(s, pool=pool, optimizer=opt)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20000, help="rays drawn from the pool per step")
    ap.add_argument("--steps", type=int, default=30, help="timed optimiser steps")
    ap.add_argument("--warmup", type=int, default=10, help="steps before the timed ones")
    ap.add_argument("--host", action="store_true",
                    help="re-sample the pool on the host every step (no device program)")
    ap.add_argument("--momentum", action="store_true", help="Nesterov SGD, momentum 0.6")
    ap.add_argument("--edge", type=float, default=0.12, help="edge length of the lens mesh")
    ap.add_argument("--pool-rays", type=int, default=65536, help="rays traced in stage 1")
    ap.add_argument("--sigma", type=float, default=1e-3,
                    help="standard deviation of the end points' jitter in y and z (0: none)")
    ap.add_argument("--pool-file", default=None, help="load the pool from this file (skips stage 1)")
    ap.add_argument("--save-pool", default=None, help="write the pool of stage 1 to this file")
    a = ap.parse_args()
    run(a.rays, a.steps, a.warmup, a.host, a.momentum, a.edge, a.pool_rays, a.sigma, a.pool_file,
        a.save_pool, verbose=True)
