"""
The in-place goal sweep (k_backward_chain_goal_inplace) forms no face terms for a face nobody
differentiates (csrc/trace_math.h adjoint3d, face_terms = false): the k = 3 lens of
tests/test_gpu_chain_goal_inplace.py with surfaces frozen like the target (parameters that take no
gradient, and ``frozen`` keeps the system's updates from rebuilding the surface in one launch with
the others, so its bytes of tfrt_scene3d.face_grad_mask are zero) --

  frozen    the front surface (the rays' first pass), the back surface (their second), both
  depth     2 (nobody reaches the target through the lens: every gradient is exactly zero) and 3
  aperture  0.8, and 1.6: rays that miss the lens finish on the target in the first pass --
            frozen finished lanes below the wavefront's top pass, next to lanes with a child

With both frozen the optimiser's only parameters are those of a third, small surface far off the
rays' way: it keeps the reverse sweep running (somebody wants face gradients) while every lane of
every pass runs the adjoint without face terms.

Eager fused steps, float64 ray state.  Checked against torch.autograd through the oracle at 1e-8
(the sweep's stated tolerance, as tests/test_gpu_sweep_one_round_trip.py applies it): the optimised
surface's parameter gradient, exactly zero where the oracle's is; error and term count; and the
sweep's gradient with respect to the SOURCE rays, which sweep_drive.capture_source_gradient asks the
goal step's entry for (gs and ge: what a frozen face's adjoint still has to deliver).  The rows of
the step's face-gradient block that belong to frozen surfaces and to the target are exactly 0.0,
the optimised surface's not all zero at depth 3.
"""
import numpy as np
import pytest
import torch

from oracle import tracer
from sweep_drive import capture_source_gradient, natural_order
from test_gpu_chain_goal_inplace import SLICE, WARM, _case
from test_gpu_engine import _oracle_for

pytestmark = pytest.mark.gpu

TOL = 1e-8
CASES = [(frozen, depth, aperture) for frozen in ("front", "back", "both") for depth in (2, 3)
         for aperture in (0.8, 1.6)]


_GEO = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")


def _frozen_case(frozen, depth, aperture):
    import tfrt.boundaries as boundaries
    import tfrt.mesh_tools as mt
    import tfrt.optimizer as optimizer
    c = _case(4161, depth, aperture=aperture)
    surfaces = c["lens"].surfaces
    ks = {"front": [0], "back": [1], "both": [0, 1]}[frozen]
    # faces built once from parameters that take no gradient, then left alone (a surface that the
    # system updates is built in one launch with the others and shares their gradient block)
    for k in ks:
        surfaces[k].parameters.requires_grad_(False)
        surfaces[k].update()
        surfaces[k].frozen = True
        assert not surfaces[k].face_verts.requires_grad
    live = [s for k, s in enumerate(surfaces) if k not in ks]
    c["optical"] = list(surfaces)
    if not live:
        mesh = mt.hexagonal_mesh(0.1, 1)
        mesh.rotate_y(90)
        mesh.rotate_x(90)
        mesh.translate((0.0, 50.0, 0.0))
        far = boundaries.ParametricTriangleBoundary(mesh, boundaries.FromVectorVG((1, 0, 0)),
                                                    material_dict={"mat_in": 1, "mat_out": 0})
        c["optical"] = list(surfaces) + [far]
        c["system"].optical = c["optical"]
        live = [far]
    c["system"].update()
    opt = optimizer.SGD_Optimizer(c["eng"], [s.parameters for s in live], c["opt"].error_function,
                                  depth, learning_rate=3e-4, grad_clip=1e9, fused="auto",
                                  graph=False, speculative=False)
    opt.suppress_warnings = True
    c["opt"], c["frozen"], c["live"] = opt, ks, live
    return c


def _oracle(c, used, depth):
    """Error sum, terms, d / d (the lens's parameters) and d / d (source rays, (6, N))."""
    q = [u.clone().requires_grad_(True) for u in used]
    osys, src = _oracle_for(c["system"], c["lens"], c["target"], c["source"], q)
    n = src["x_start"].shape[0]
    total = [torch.zeros_like(u) for u in used]
    g_src = torch.zeros((6, n), dtype=torch.float64)
    err_sum, terms = 0.0, 0
    for a in range(0, n, SLICE):
        part = {k: v[a:a + SLICE] for k, v in src.items()}
        leaves = [part[k].clone().requires_grad_(True) for k in _GEO]
        part.update(zip(_GEO, leaves))
        ref = tracer.ray_trace(osys, part, max_iterations=depth,
                               inherit=("wavelength", "object_coords"))
        rf = ref.get("finished")
        if not rf or rf["y_end"].shape[0] == 0:
            continue
        rerr = (torch.stack([rf["y_end"], rf["z_end"]], 1) + rf["object_coords"][:, 1:]) ** 2
        err_sum += float(rerr.sum().detach())
        terms += rerr.numel()
        if not rerr.requires_grad:
            continue
        got = torch.autograd.grad(rerr.sum(), q + leaves, retain_graph=True, allow_unused=True)
        for t, g in zip(total, got[:len(q)]):
            if g is not None:
                t += g
        for i, g in enumerate(got[len(q):]):
            if g is not None:
                g_src[i, a:a + SLICE] = g
    return err_sum, terms, total, g_src


@pytest.mark.parametrize("frozen,depth,aperture", CASES)
def test_frozen_surfaces(frozen, depth, aperture, monkeypatch):
    c = _frozen_case(frozen, depth, aperture)
    box = capture_source_gradient(monkeypatch)
    opt, ks = c["opt"], c["frozen"]
    live = [s.parameters for s in c["live"]]
    for _ in range(WARM):
        opt.single_step(None, lr_scale=0.0)
    c["system"].update()
    used = [p.detach().cpu().clone() for p in c["lens"].parameters]
    before = [p.detach().cpu().clone() for p in live]
    err = float(opt.single_step(None))
    terms = int(float(opt.last_error_terms))
    fs = opt._fused_step
    assert fs is not None and fs.graph_replays == 0
    assert fs.in_place and fs.folded_backward          # the kernel under test is the one that ran
    grads = [(u - p.detach().cpu()) / (0.01 * opt.learning_rate) for u, p in zip(before, live)]

    # the step's face-gradient block: optical surfaces in the system's order, then the target
    n_faces = [s.face_verts.shape[0] for s in c["optical"]]
    g_fv = fs._state.g_fv.detach().cpu().reshape(-1, 9)
    assert g_fv.shape[0] == sum(n_faces) + c["target"].face_verts.shape[0]
    rows = np.cumsum([0] + n_faces)
    block = lambda i: g_fv[rows[i]:rows[i + 1]]
    top = [float(block(i).abs().max()) for i in range(len(n_faces))]
    print(f"{frozen} frozen, depth {depth}, aperture {aperture}: error {err!r}, terms {terms}, "
          f"max |face gradient| per surface {top}, target {float(g_fv[rows[-1]:].abs().max()):.3e}")
    for k in ks:
        assert top[k] == 0.0
    assert float(g_fv[rows[-1]:].abs().max()) == 0.0

    err_o, terms_o, g_o, g_src_o = _oracle(c, used, depth)
    assert terms == terms_o
    if terms_o:
        assert abs(err - err_o / terms_o) <= TOL * (err_o / terms_o)
    if frozen == "both":
        assert top[2] == 0.0 and float(grads[0].abs().max()) == 0.0     # (no ray meets that surface)
    else:
        k = 1 - ks[0]
        want, grad = g_o[k], grads[0]
        diff, ref = float((grad - want).abs().max()), float(want.abs().max())
        print(f"  parameter gradient: max |d| {diff:.3e}, max |ref| {ref:.3e}")
        if depth == 3:
            assert ref > 0.0 and top[k] > 0.0
        else:
            assert ref == 0.0
        assert diff <= TOL * ref
        assert bool((grad[want == 0.0] == 0.0).all())

    g_src = natural_order(box["g_src"].cpu(), fs._state.perm.cpu() if fs._state.perm is not None else None)
    diff, ref = float((g_src - g_src_o).abs().max()), float(g_src_o.abs().max())
    print(f"  source-ray gradient: max |d| {diff:.3e}, max |ref| {ref:.3e}")
    assert ref > 0.0 or terms_o == 0
    assert diff <= TOL * ref
    assert bool((g_src[g_src_o == 0.0] == 0.0).all())
