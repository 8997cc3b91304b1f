"""
The in-place goal sweep takes a reaction's index ratio from the per-face table of the trace's set-up
launch (feta[4f], feta[4f + 1] = snell_ratios(n_in, n_out)) instead of dividing n_in and n_out
again.  The k = 3 lens of tests/test_gpu_chain_goal_inplace.py in "value" mode with per-face indices
that take no gradient --

  mirror         faces with n_in == 0 (both ratios' safe values; the reverse of a reflection)
  n_out_zero     faces whose outer index is zero: a ratio of exactly 0 from inside, n_out taken as 1
                 from outside
  total_internal_reflection   faces of n_in = 4, met from inside beyond 14.5 degrees
  all_of_them    the three mixed on one lens
  mixed_indices  a different pair (n_in, n_out) on every face: every lane picks another entry

and a flat glass face met from inside within 1e-12 .. 0.2 rad of the critical angle on both sides
(the scene of tests/test_gpu_inplace_oracle.py::test_in_place_gradients_at_the_critical_angle as a
parametric surface of an optimiser).

Reflecting lenses are traced at depth 5: a ray reflected at the back surface and again at the front
one still reaches the target, so reflected records carry a gradient.  The engine would leave such
sources to the per-pass kernels (their wavefronts are no narrow bundles); sweep_drive.force_in_place
keeps them on the in-place route, and every case asserts that the step ran in place with the goal
folded into the sweep.  Eager fused steps, float64 ray state; error, term count and parameter
gradients against torch.autograd through the oracle at 1e-8; an entry that is not finite in the
oracle's gradient is one the optimiser zeroed (optimizer.py:226-229).
"""
import numpy as np
import pytest
import torch

from oracle import tracer
from test_gpu_chain_goal_inplace import SLICE, WARM, _case
from test_gpu_engine import _oracle_surface
from sweep_drive import force_in_place

pytestmark = pytest.mark.gpu

TOL = 1e-8
# kind: trace depth, per-face (n_in, n_out) drawn with these probabilities (None: uniform pairs)
KINDS = {
    "mirror": (5, [((1.49, 1.0), 0.6), ((0.0, 1.0), 0.4)]),
    "n_out_zero": (3, [((1.49, 1.0), 0.7), ((1.49, 0.0), 0.3)]),
    "total_internal_reflection": (5, [((1.49, 1.0), 0.5), ((4.0, 1.0), 0.5)]),
    "all_of_them": (5, [((1.49, 1.0), 0.4), ((0.0, 1.0), 0.25), ((1.49, 0.0), 0.1), ((4.0, 1.0), 0.25)]),
    "mixed_indices": (3, None),
}


def _ratio_case(kind, monkeypatch):
    import tfrt.optimizer as optimizer
    depth, drawn = KINDS[kind]
    c = _case(4161, depth, value=True)
    force_in_place(monkeypatch, c["eng"])
    rng = np.random.default_rng(11)
    index = []
    for surface in c["lens"].surfaces:
        n = surface.face_verts.shape[0]
        if drawn is None:
            vin, vout = rng.uniform(1.2, 1.7, size=n), rng.uniform(1.0, 1.4, size=n)
        else:
            pairs = [p for p, _ in drawn]
            pick = rng.choice(len(pairs), size=n, p=[w for _, w in drawn])
            vin, vout = [np.array([pairs[i][j] for i in pick]) for j in (0, 1)]
        n_in = torch.tensor(vin, dtype=torch.float64, device="cuda")
        n_out = torch.tensor(vout, dtype=torch.float64, device="cuda")
        surface.material_dict = {"n_in": n_in, "n_out": n_out}
        surface.update_materials()
        index.append((n_in.cpu(), n_out.cpu()))
    c["system"].update()
    opt = optimizer.SGD_Optimizer(c["eng"], list(c["lens"].parameters), c["opt"].error_function,
                                  depth, learning_rate=3e-4, grad_clip=1e9, fused="auto",
                                  graph=False, speculative=False)
    opt.suppress_warnings = True
    c["opt"], c["index"], c["depth"] = opt, index, depth
    return c


def _oracle(c, used):
    q = [u.clone().requires_grad_(True) for u in used]
    surfs = []
    for s, p, (n_in, n_out) in zip(c["lens"].surfaces, q, c["index"]):
        f = _oracle_surface(s, p)
        del f["mat_in"], f["mat_out"]
        f["n_in"], f["n_out"] = n_in, n_out
        surfs.append(f)
    tgt = tracer.faces_from_vertices(c["target"]._vertices.detach().cpu(), c["target"]._faces[:, 1:])
    osys = tracer.System(3, materials=[], optical=tracer.amalgamate(surfs), target=tgt)
    src = {k: v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu()
           for k, v in c["system"]._amalgamated_sources.items()}
    total = [torch.zeros_like(u) for u in used]
    err_sum, terms = 0.0, 0
    for a in range(0, src["x_start"].shape[0], SLICE):
        part = {k: v[a:a + SLICE] for k, v in src.items()}
        ref = tracer.ray_trace(osys, part, max_iterations=c["depth"],
                               inherit=("wavelength", "object_coords"), index_type="value")
        rf = ref.get("finished")
        if not rf or rf["y_end"].shape[0] == 0:
            continue
        rerr = (torch.stack([rf["y_end"], rf["z_end"]], 1) + rf["object_coords"][:, 1:]) ** 2
        for t, g in zip(total, torch.autograd.grad(rerr.sum(), q, retain_graph=True,
                                                   allow_unused=True)):
            if g is not None:
                t += g
        err_sum += float(rerr.sum().detach())
        terms += rerr.numel()
    return err_sum, terms, total


@pytest.mark.parametrize("kind", list(KINDS))
def test_goal_sweep_with_ratios_from_the_table(kind, monkeypatch):
    c = _ratio_case(kind, monkeypatch)
    opt, params = c["opt"], list(c["lens"].parameters)
    for _ in range(WARM):
        opt.single_step(None, lr_scale=0.0)
    c["system"].update()
    used = [p.detach().cpu().clone() for p in params]
    err = float(opt.single_step(None))
    terms = int(float(opt.last_error_terms))
    fs = opt._fused_step
    assert fs is not None and fs.graph_replays == 0
    assert fs.in_place and fs.folded_backward
    counts = np.stack([np.asarray(x) for x in c["eng"].last_trace["counts"]])
    grads = [(u - p.detach().cpu()) / (0.01 * opt.learning_rate) for u, p in zip(used, params)]
    err_o, terms_o, g_o = _oracle(c, used)
    print(f"{kind}: error {err!r} / {err_o / max(terms_o, 1)!r}, terms {terms} / {terms_o}, "
          f"ray counts per pass\n{counts}")
    assert terms == terms_o and terms_o > 0
    if np.isfinite(err_o):
        assert abs(err - err_o / terms_o) <= TOL * abs(err_o / terms_o)
    for i, (g, w) in enumerate(zip(grads, g_o)):
        # (the optimiser zeroes the non-finite entries of a gradient, optimizer.py:226-229: where
        # the oracle's entry is not finite the step must have left the parameter where it was)
        fin_w = torch.isfinite(w)
        assert bool(torch.isfinite(g).all()) and bool((g[~fin_w] == 0.0).all()), \
            f"parameter {i}: other non-finite entries than the oracle's"
        diff = float((g[fin_w] - w[fin_w]).abs().max())
        ref = float(w[fin_w].abs().max())
        print(f"  parameter {i}: max |d| {diff:.3e}, max |ref| {ref:.3e}, "
              f"non-finite {int((~fin_w).sum())}")
        assert ref > 0.0
        assert diff <= TOL * ref, f"parameter {i}: {diff:.3e} against {ref:.3e}"


# ------------------------------------------------------------------------------ critical angle

def _critical_case(monkeypatch):
    """A flat parametric face in the plane x = 0 (96 triangles, glass on one side), 4,224 rays that
    meet it at the critical angle + {-1e-9, -1e-12, 1e-12, 1e-9, -0.2, 0.1} rad, half of them from
    either side (from the glass side they are refracted out at grazing angles or reflected back,
    from the other they enter the glass); targets at x = +-40 and, for the grazing ones, y = 60."""
    import tfrt.boundaries as boundaries
    import tfrt.distributions as distributions
    import tfrt.drawing as drawing
    import tfrt.engine as engine
    import tfrt.mesh_tools as mt
    import tfrt.operation as operation
    import tfrt.optimizer as optimizer
    import tfrt.sources as sources

    n_glass, n_rays = 1.5, 4224
    rng = np.random.default_rng(5)
    ang = np.arcsin(1.0 / n_glass) + np.resize([-1e-9, -1e-12, 1e-12, 1e-9, -0.2, 0.1], n_rays)
    side = np.where(np.arange(n_rays) % 2 == 0, 1.0, -1.0)
    rad, phi = 12.0 * np.sqrt(rng.random(n_rays)), 2 * np.pi * rng.random(n_rays)
    hit = np.stack([np.zeros(n_rays), rad * np.cos(phi), rad * np.sin(phi)], 1)
    d = np.stack([side * np.cos(ang), np.sin(ang), np.zeros(n_rays)], 1)       # towards the face
    start_points = distributions.ManualBasePointDistribution(3, points=hit - d)
    end_points = distributions.ManualBasePointDistribution(3, points=hit - 0.5 * d)
    source = sources.AperatureSource(
        3, start_points, end_points, [drawing.YELLOW], dense=False,
        extra_fields={"object_coords": ("start_point", start_points, "points")})

    mesh = mt.hexagonal_mesh(25.0, 4)
    mesh.rotate_y(90)
    mesh.rotate_x(90)
    face = boundaries.ParametricTriangleBoundary(
        mesh, boundaries.FromVectorVG((1, 0, 0)), initial_parameters=0.0,
        material_dict={"n_in": n_glass, "n_out": 1.0})
    targets = []
    for center, direction in (((40, 0, 0), (1, 0, 0)), ((-40, 0, 0), (1, 0, 0)), ((0, 60, 0), (0, 1, 0))):
        t = boundaries.ManualTriangleBoundary(
            mesh=mt.plane(center=center, direction=direction, i_size=4000, j_size=4000))
        t.frozen = True
        targets.append(t)
    system = engine.OpticalSystem3D()
    system.optical = [face]
    system.targets = targets
    system.sources = [source]
    system.update()
    eng = engine.OpticalEngine(3, [operation.StandardReaction("value")],
                               simple_ray_inheritance={"wavelength", "object_coords"},
                               ray_dtype=torch.float64)
    eng.optical_system = system
    eng.validate_system()
    force_in_place(monkeypatch, eng)
    erf = optimizer.GoalError(("y_end", "z_end"), lambda src: -src["object_coords"][:, 1:])
    opt = optimizer.SGD_Optimizer(eng, [face.parameters], erf, 2, learning_rate=3e-4, grad_clip=1e9,
                                  fused="auto", graph=False, speculative=False)
    opt.suppress_warnings = True
    return dict(opt=opt, eng=eng, system=system, face=face, targets=targets, n_glass=n_glass)


def test_goal_sweep_at_the_critical_angle(monkeypatch):
    c = _critical_case(monkeypatch)
    opt, face = c["opt"], c["face"]
    for _ in range(WARM):
        opt.single_step(None, lr_scale=0.0)
    c["system"].update()
    used = face.parameters.detach().cpu().clone()
    err = float(opt.single_step(None))
    terms = int(float(opt.last_error_terms))
    fs = opt._fused_step
    assert fs is not None and fs.graph_replays == 0
    assert fs.in_place and fs.folded_backward
    grad = (used - face.parameters.detach().cpu()) / (0.01 * opt.learning_rate)

    q = used.clone().requires_grad_(True)
    f = _oracle_surface(face, q)
    del f["mat_in"], f["mat_out"]
    n = f["xp"].shape[0]
    f["n_in"] = torch.full((n,), c["n_glass"], dtype=torch.float64)
    f["n_out"] = torch.ones(n, dtype=torch.float64)
    tgt = tracer.amalgamate([tracer.faces_from_vertices(t._vertices.detach().cpu(), t._faces[:, 1:])
                             for t in c["targets"]])
    osys = tracer.System(3, materials=[], optical=f, target=tgt)
    src = {k: v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu()
           for k, v in c["system"]._amalgamated_sources.items()}
    ref = tracer.ray_trace(osys, src, max_iterations=2, inherit=("wavelength", "object_coords"),
                           index_type="value")
    rf = ref["finished"]
    rerr = (torch.stack([rf["y_end"], rf["z_end"]], 1) + rf["object_coords"][:, 1:]) ** 2
    (want,) = torch.autograd.grad(rerr.sum(), [q])
    back = int(((rf["x_end"] - rf["x_start"]) * rf["object_coords"][:, 0] > 0).sum())
    print(f"critical angle: error {err!r} / {float(rerr.sum().detach()) / rerr.numel()!r}, terms {terms} / "
          f"{rerr.numel()}, {back} of {rf['x_end'].shape[0]} finished rays on their own side")
    assert terms == rerr.numel() > 0
    assert 0 < back < rf["x_end"].shape[0]                     # reflected back and passed through
    fin_w = torch.isfinite(want)
    assert bool(torch.isfinite(grad).all()) and bool((grad[~fin_w] == 0.0).all())
    diff, top = float((grad[fin_w] - want[fin_w]).abs().max()), float(want[fin_w].abs().max())
    print(f"  parameter gradient: max |d| {diff:.3e}, max |ref| {top:.3e}, non-finite {int((~fin_w).sum())}")
    assert top > 0.0
    assert diff <= TOL * top, f"{diff:.3e} against {top:.3e}"
