"""
The beam walk's face records as DPP operands (face_edges, tfrt_trace3d.hip): the per-pass beam trace
(k_intersect_beam) and the in-place trace (k_trace_inplace) against the ALL-PAIRS trace (every ray
against every face, the arithmetic tests/test_gpu_stress.py pins to the oracle), BIT FOR BIT --
counts, ids, rows and faces of every class (test_gpu_fuzz_inplace._same).

A record word that a lane reads from a lane of its row that is switched off, or from a row that
holds no copy of the record, culls valid (ray, face) pairs: a missing hit in almost every wavefront.

Scenes are small lenses (scene_util.lens_scene), float32 and float64 ray state, 3 passes:

  * 65, 127 and 4,096 rays: a last wavefront with one lane, with all but one, and full wavefronts --
    of 64 rays in the per-pass trace without coherent_only, of 32 rays (lanes 32..63 carry no ray
    and still hand the record round in their rows) with coherent_only and in every in-place trace
    of up to 160k rays; one in-place trace of 163,905 rays has 64-ray wavefronts, the last with one;
  * (k_front, k_back) = (1, 1), (2, 1), (5, 3) and (3, 2).  The first two have 14 and 32 faces --
    below the 64 faces the sphere hierarchy starts at, so the library traces them per pass without
    the walk (they pin that route to the same results); (3, 2), 80 faces, is the smallest lens that
    is walked, (5, 3) has 206.  A wavefront's chunk holds a handful of faces there, an odd number
    in some wavefronts and an even one in others (the target alone: two), so rounds of two records
    and a last round of one both run;
  * rays that start 1,000 units from the lens (a large Perr), and a negative ray_start_epsilion;
  * a triangle soup (test_gpu_stress._soup) at 256 rays: bundles are cut down to single rays.
"""
import functools

import pytest
import torch

import scene_util
import test_gpu_stress as st
from test_gpu_fuzz_inplace import _same
from test_gpu_inplace import _flags, _lens_args, assert_in_place
from test_gpu_trace3d import _gpu_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PASSES = 3
WALKED = 64   # faces from which a scene has a sphere hierarchy (has_hierarchy, tfrt_trace3d.hip)


@functools.lru_cache(maxsize=None)
def _lens(n_rays, k_front, k_back, dtype, source_distance, eps_start):
    """The scene on the device, its all-pairs trace (natural order) and the Hilbert order."""
    from tensorflowraytrace_amd import ops
    scene = scene_util.lens_scene(n_rays, k_front=k_front, k_back=k_back,
                                  source_distance=source_distance)
    src, fv, sc, _ = _gpu_scene(scene, dtype)
    fv = fv.detach()
    eps = None if eps_start is None else (sc.eps[0], sc.eps[1], eps_start)
    if eps is not None:
        sc.eps = eps
    ref = ops.trace3d(src, fv, sc, max_passes=PASSES, flags=_flags())
    return src, fv, sc, eps, ops.ray_order(src), ref


def _check_routes(n_rays, k_front, k_back, dtype, source_distance=10.0, eps_start=None,
                  routes=("beam64", "beam32", "inplace")):
    from tensorflowraytrace_amd import ops
    src, fv, sc, eps, order, ref = _lens(n_rays, k_front, k_back, dtype, source_distance, eps_start)
    assert int(ref["counts"][:, 1].sum()) > 0          # rays reach the target
    rays = src[:, order.long()].contiguous()
    for route in routes:
        args = _lens_args(sc, fv, order, route == "inplace", eps)
        args.coherent_only = route != "beam64"
        if route == "inplace" and fv.shape[0] >= WALKED:
            assert_in_place(args, fv, n_rays, PASSES)
        out = ops.trace3d(rays, fv, args, max_passes=PASSES, flags=_flags())
        _same(ops.restore_order(out, order), ref, (route, n_rays, k_front, k_back, dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k_front,k_back", [(1, 1), (2, 1), (5, 3), (3, 2)])
@pytest.mark.parametrize("n_rays", [65, 127, 4096])
def test_beam_and_in_place_traces_equal_the_all_pairs_trace(n_rays, k_front, k_back, dtype):
    _check_routes(n_rays, k_front, k_back, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rays_that_start_far_from_the_lens(dtype):
    _check_routes(4096, 5, 3, dtype, source_distance=1000.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_negative_ray_start_epsilion(dtype):
    _check_routes(4096, 5, 3, dtype, eps_start=-1e-3)


def test_in_place_wavefronts_of_64_rays():
    _check_routes(160 * 1024 + 65, 5, 3, torch.float32, routes=("inplace",))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_soup_cut_down_to_single_rays(dtype):
    from tensorflowraytrace_amd import ops
    sc0 = st._soup(21)                                  # 97 faces, 700 rays
    fv = sc0["P"].to(DEV)
    cat = sc0["cat"].int().to(DEV)
    base = dict(n_in=sc0["n_in"].to(DEV), n_out=sc0["n_out"].to(DEV))
    r = sc0["rays"][:, :256].to(DEV).to(dtype).contiguous()
    kw = dict(max_passes=PASSES, flags=_flags(), new_ray_length=sc0["L"])
    ref = ops.trace3d(r, fv, ops.Scene3DArgs(fv, cat, **base), **kw)
    assert int(ref["counts"][:, :3].sum()) > 0          # rays hit faces
    order = ops.ray_order(r)
    for route in ("beam64", "beam32", "inplace"):
        args = ops.Scene3DArgs(fv, cat, cluster_order=ops.cluster_order(fv), coherent_rays=True, **base)
        args.coherent_only = route != "beam64"
        args.in_place = route == "inplace"
        if args.in_place:
            assert_in_place(args, fv, r.shape[1], PASSES)
        out = ops.trace3d(r[:, order.long()].contiguous(), fv, args, **kw)
        _same(ops.restore_order(out, order), ref, (route, dtype))
