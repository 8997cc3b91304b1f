"""
The yardstick of tests/test_gpu_trace2d_sweep.py checked on its own, without a GPU: the oracle's
2-D gradient with respect to the source rays (and with it the dead_ray_length scaling of the dead
class, the stopped class and the start rows of the active class) against central differences of
the same all-class error.
"""
import numpy as np
import pytest
import torch

from oracle import tracer
from test_gpu_trace2d import _oracle_system, _src2
from test_gpu_trace2d_sweep import (BLOCK, CLASSES, EDGE, NAMES, _error_columns, _scene_for,
                                    block_size_in_the_sources)

PASSES = 4
H = 1e-6            # test_index_gradient_2d_central_difference's step ...
BAR = 1e-5          # ... and its bar, relative to the entry itself


def test_the_block_size_the_gpu_cases_state_is_the_sources():
    assert block_size_in_the_sources() == BLOCK


def _tagged(sets):
    """The scene's sets with a primitive number on every optical primitive (it travels into the
    projection's optical data, like mat_in)."""
    out = {k: dict(s) for k, s in sets.items()}
    for base, name in ((0, "optical_segments"), (1000, "optical_arcs")):
        n = out[name]["mat_in"].shape[0]
        out[name]["prim"] = base + torch.arange(n)
    return out


def _trace(system, src, dead_len):
    """tracer.ray_trace's loop; returns the error ray by ray (a source ray's own links and
    descendants: the error is a sum over source rays) and the trace's signature: which rays were
    put in which class by which kind of primitive in every pass, and the optical primitive every
    active ray met."""
    n = src["x_start"].shape[0]
    history = {c: [] for c in CLASSES}
    signature = []
    rays = dict(src)
    for p in range(PASSES):
        before = {c: len(history[c]) for c in CLASSES}
        rays, proj = tracer.single_pass(
            system, rays, history, inherit=("wavelength", "ray_id"), finite_tir_gradient=True,
            flags=dict(compile_dead_rays=True, compile_stopped_rays=True,
                       dead_ray_length=dead_len))
        for c in CLASSES:
            for j, entry in enumerate(history[c][before[c]:]):      # (segments, then arcs)
                signature.append((p, c, j, tuple(entry["ray_id"].tolist()) if entry else ()))
        prim = proj["optical"].get("prim")
        signature.append((p, "prim", tuple(prim.tolist()) if prim is not None else ()))
        if not rays:
            break
    per_ray = torch.zeros(n, dtype=torch.float64)
    seen = {"under way": rays["ray_id"].long() if rays else torch.zeros(0, dtype=torch.long)}
    for k, c in enumerate(CLASSES):
        h = tracer.amalgamate(history[c])
        seen[c] = h["ray_id"].long() if h else torch.zeros(0, dtype=torch.long)
        if h:
            b = torch.stack([h[f] for f in NAMES])
            per_ray = per_ray.index_add(0, seen[c], _error_columns(b, k))
    return per_ray, signature, seen


def _source(rays, wl, shift=None):
    src = _src2(rays, wl, False)
    if shift is not None:
        row, h = shift
        src[NAMES[row]] = src[NAMES[row]] + h
    return src


@pytest.mark.parametrize("dead_len", [0.25, None])
def test_oracle_source_gradient_against_central_differences(dead_len):
    sets, rays, wl = _scene_for(*EDGE)
    system = _oracle_system(_tagged(sets))
    # two rays that end in each class (the active ones: still under way after the last pass),
    # the first of the scene whose path -- classes and primitives met -- is the same at +-H
    _, _, seen = _trace(system, _source(rays, wl), dead_len)
    ends = {"finished": seen["finished"], "stopped": seen["stopped"], "dead": seen["dead"],
            "active": seen["under way"]}
    chosen = []
    for cls in CLASSES:
        took = 0
        for j in sorted(set(ends[cls].tolist())):
            one = (rays[:, j:j + 1], wl[j:j + 1])
            base = _trace(system, _source(*one), dead_len)[1]
            if all(_trace(system, _source(*one, shift=(r, s * H)), dead_len)[1] == base
                   for r in range(4) for s in (1.0, -1.0)):
                chosen.append(j)
                took += 1
            if took == 2:
                break
        assert took == 2, f"no two steady rays ending {cls}"
    assert len(set(chosen)) == 8
    sub, sub_wl = rays[:, chosen], wl[chosen]

    src = _source(sub, sub_wl)
    leaves = [src[f].requires_grad_(True) for f in NAMES]
    per_ray, base, seen = _trace(system, src, dead_len)
    assert all(len(seen[c]) > 0 for c in CLASSES)
    grad = torch.stack(torch.autograd.grad(per_ray.sum(), leaves))
    assert bool(torch.isfinite(grad).all()) and bool((grad != 0).all())
    for row in range(4):
        vals = []
        for sgn in (1.0, -1.0):
            v, sig, _ = _trace(system, _source(sub, sub_wl, shift=(row, sgn * H)), dead_len)
            assert sig == base, "a ray changed its path within the step"
            vals.append(v)
        fd = (vals[0] - vals[1]) / (2 * H)
        err = ((fd - grad[row]).abs() / grad[row].abs()).numpy()
        print(f"{NAMES[row]}: central difference rel err {np.array2string(err, precision=2)}")
        assert float(err.max()) <= BAR, (NAMES[row], err)
