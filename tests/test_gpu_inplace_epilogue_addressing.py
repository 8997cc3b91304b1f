"""
The in-place trace's pass epilogue -- the reaction and the tape (trace_inplace, tfrt_trace3d.hip)
-- asks for everything it reads of the hit face (catagory, the unit normal, the index ratios) as
soon as the face is known and classifies and reacts behind one wait, and the frame origin is read
once per launch instead of once per pass.  A table row read for the wrong face, a row of the tape
or of the child block written at the wrong place or with the wrong stride moves a child ray, a
tape record or a count: the in-place trace against the ALL-PAIRS trace (every ray against every
face, per pass), BIT FOR BIT -- counts, ids, rows and faces of every class
(test_gpu_fuzz_inplace._same).  The tape itself (rec_tri, rec_t, rec_cls) lives in the workspace;
an in-place trace's ray sets are gathered from it (k_inplace_gather recomputes every row from
rec_tri / rec_t and cuts the classes by rec_cls), so the sets are the tape's image, and the branch
bits of rec_cls are read by the reverse sweep: gradients against the per-pass tape's.

  * 65 and 127 rays: a last wavefront with one lane and with all but one, 32-ray bundles; one trace
    of 163,905 rays has 64-ray bundles (the scene and reference of test_gpu_beam_walk_records);
  * 1, 3 and 5 passes (row p of every tape array, child rows (6 p + k));
  * float32, float64 and float16 ray state;
  * per-face indices absent -- a lens in "index" mode, one n_table column per ray: mat_in / mat_out
    by face, n_table by (material, ray) -- and present -- a triangle soup with n_in / n_out per
    face (feta);
  * the kernel that also writes every ray's finished row at the ray's own column
    (tfrt_scene3d.in_place == 2), called through the C ABI with a source stride and a finished
    capacity LARGER than the ray count (the workspace's own slot stride is the ray count by
    construction: Tape3.n), against the in-place trace's finished set, 1, 3 and 5 passes.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import scene_util
import test_gpu_stress as st
from test_gpu_beam_walk_records import _check_routes
from test_gpu_fuzz_inplace import _same
from test_gpu_inplace import _flags, _lens_args, assert_in_place
from test_gpu_trace3d import _gpu_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.float16]


@functools.lru_cache(maxsize=None)
def _lens(n_rays, dtype, passes):
    """A small lens (206 faces) on the device, its all-pairs trace and the Hilbert order."""
    from tensorflowraytrace_amd import ops
    scene = scene_util.lens_scene(n_rays, k_front=5, k_back=3)
    src, fv, sc, _ = _gpu_scene(scene, dtype)
    fv = fv.detach()
    ref = ops.trace3d(src, fv, sc, max_passes=passes, flags=_flags())
    return src, fv, sc, ops.ray_order(src), ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("passes", [1, 3, 5])
@pytest.mark.parametrize("n_rays", [65, 127])
def test_lens_in_index_mode(n_rays, passes, dtype):
    from tensorflowraytrace_amd import ops
    src, fv, sc, order, ref = _lens(n_rays, dtype, passes)
    assert int(ref["counts"][:, :3].sum()) > 0                 # rays meet faces
    if passes >= 3 and dtype != torch.float16:
        assert int(ref["counts"][:, 1].sum()) > 0              # ... and reach the target
    args = _lens_args(sc, fv, order, True)
    assert_in_place(args, fv, n_rays, passes)
    out = ops.trace3d(src[:, order.long()].contiguous(), fv, args, max_passes=passes, flags=_flags())
    _same(ops.restore_order(out, order), ref, (n_rays, passes, dtype))


def test_wavefronts_of_64_rays():
    _check_routes(160 * 1024 + 65, 5, 3, torch.float32, routes=("inplace",))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("passes", [1, 3, 5])
@pytest.mark.parametrize("n_rays", [65, 127])
def test_soup_with_per_face_indices(n_rays, passes, dtype):
    from tensorflowraytrace_amd import ops
    sc0 = st._soup(21)                                          # 97 faces
    fv = sc0["P"].to(DEV)
    cat = sc0["cat"].int().to(DEV)
    base = dict(n_in=sc0["n_in"].to(DEV), n_out=sc0["n_out"].to(DEV))
    r = sc0["rays"][:, :n_rays].to(DEV).to(dtype).contiguous()
    kw = dict(max_passes=passes, flags=_flags(), new_ray_length=sc0["L"])
    ref = ops.trace3d(r, fv, ops.Scene3DArgs(fv, cat, **base), **kw)
    assert int(ref["counts"][:, 0].sum()) > 0                   # rays are refracted / reflected
    order = ops.ray_order(r)
    args = ops.Scene3DArgs(fv, cat, cluster_order=ops.cluster_order(fv), coherent_rays=True, **base)
    args.coherent_only = args.in_place = True
    assert_in_place(args, fv, n_rays, passes)
    out = ops.trace3d(r[:, order.long()].contiguous(), fv, args, **kw)
    _same(ops.restore_order(out, order), ref, (n_rays, passes, dtype))


def test_tape_branch_bits_give_the_per_pass_gradients():
    from tensorflowraytrace_amd import ops
    scene = scene_util.lens_scene(127, k_front=5, k_back=3)
    src, fv0, sc, _ = _gpu_scene(scene, torch.float64, cluster="group")
    order = ops.ray_order(src)
    rays0 = src[:, order.long()].contiguous()
    grads = {}
    for in_place in (False, True):
        fv = fv0.detach().clone().requires_grad_(True)
        rays = rays0.detach().clone().requires_grad_(True)
        args = _lens_args(sc, fv.detach(), order, in_place)
        if in_place:
            assert_in_place(args, fv.detach(), 127, 3)
        out = ops.trace3d(rays, fv, args, max_passes=3, flags=_flags())
        assert out["finished"].shape[1] > 0
        err = (out["finished"][4].double() ** 2 + out["finished"][5].double() ** 2).sum()
        err = err + (out["active"][3].double() * out["active"][0].double()).sum() * 1e-3
        grads[in_place] = torch.autograd.grad(err, [fv, rays])
    for a, b in zip(grads[True], grads[False]):
        scale = float(b.abs().max())
        assert scale > 0
        # (the same float64 terms summed in another order, as in test_gpu_inplace)
        assert float((a - b).abs().max()) <= 1e-12 * scale


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 3, 5])
@pytest.mark.parametrize("n_rays", [65, 127])
def test_finished_rows_at_the_rays_own_columns(n_rays, P, dtype):
    from tensorflowraytrace_amd import ops, _lib
    L = _lib.lib()
    src, fv, sc, order, _ = _lens(n_rays, dtype, P)
    N, M = n_rays, fv.shape[0]
    stride, cap = N + 37, N + 5
    wide = torch.full((6, stride), float("nan"), dtype=dtype, device=DEV)
    wide[:, :N] = src[:, order.long()]
    rays = wide[:, :N].contiguous()
    args = _lens_args(sc, fv, order, True)
    assert_in_place(args, fv, N, P)
    ref = ops.trace3d(rays, fv, args, max_passes=P, flags=_flags())
    dt = {torch.float32: _lib.F32, torch.float64: _lib.F64, torch.float16: _lib.F16}[dtype]
    wsb = L.tfrt_trace3d_workspace_bytes(N, M, P, dt)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(_lib.COUNTS_PER_PASS * (P + 1), dtype=torch.int32, device=DEV)
    rows = torch.full((6, cap), 7.0, dtype=dtype, device=DEV)
    passes = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    face = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    fin = ops._ray_out(rows, passes, face)
    none = [ops._ray_out(None, None, None) for _ in range(3)]
    st_ = args.struct(fv)
    st_.in_place = 2
    try:
        _lib.check(L.tfrt_trace3d_forward(ops._p(wide), stride, N, ctypes.byref(st_), 1.0, 0.0, P, dt,
                                          _flags(), ctypes.byref(fin), *[ctypes.byref(o) for o in none],
                                          None, None, ops._p(counts), ops._p(ws), wsb,
                                          ops._stream(wide)), "forward")
        torch.cuda.synchronize()
    finally:
        st_.in_place = 1
    ids = ref["finished_id"].long()
    assert ids.numel() > 0 or dtype == torch.float16 or P < 3     # (the target is the third face met)
    assert torch.equal(rows[:, ids], ref["finished"])
    assert torch.equal(face[ids], ref["finished_face"])
    # the pass a ray finished in: the finished set lists pass after pass
    per_pass = torch.tensor(ref["counts"][:, 1].astype(np.int64))
    assert torch.equal(passes[ids].cpu().long(), torch.repeat_interleave(torch.arange(1, P + 1), per_pass))
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[ids] = False
    assert torch.equal(rows[:, :N][:, rest], rays[:, rest])     # the source ray stands in
    assert bool((face[:N][rest] == -1).all())
    assert bool(((passes[:N][rest] >= 1) & (passes[:N][rest] <= P)).all())
    # nothing beyond the ray count
    assert bool((rows[:, N:] == 7.0).all()) and bool((face[N:] == -7).all()) and bool((passes[N:] == -7).all())

