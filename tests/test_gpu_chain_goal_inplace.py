"""
The reverse sweep of the in-place goal step (k_backward_chain_goal_inplace: the in-place tape, the
built-in goal as the only gradient, the chain's records in LDS, per-face indices from the set-up
launch's table) against the per-pass fused step (``eng.in_place = False``)
and against torch.autograd through the oracle -- on the cases that take the kernel and on the
ones its dispatch must leave to the general kernels (more passes than the LDS columns hold, index
gradients, indices that depend on the ray).

The lens is test_gpu_fused_step._make's (k = 3), the steps are eager fused steps, the ray state is
float64: the gradients are compared at 1e-8, the reverse sweep's stated tolerance
(csrc/trace_math.h) and the one tests/test_gpu_fullsize.py uses for float64 state.
"""
import numpy as np
import pytest
import torch

from oracle import tracer
from test_gpu_engine import _oracle_for, _oracle_surface

pytestmark = pytest.mark.gpu

TOL = 1e-8
WARM = 8          # steps before the measured one: ray order, the visit-all note, the in-place trace
SLICE = 512       # rays per oracle trace


def _case(n_rays, depth, aperture=0.8, two_wavelengths=False, value=False):
    import tfrt.boundaries as boundaries
    import tfrt.distributions as distributions
    import tfrt.drawing as drawing
    import tfrt.engine as engine
    import tfrt.materials as materials
    import tfrt.mesh_tools as mt
    import tfrt.operation as operation
    import tfrt.optimizer as optimizer
    import tfrt.sources as sources

    start_points = distributions.StaticUniformCircle(n_rays, 0.2)
    distributions.BasePointTransformation(start_points, translation=(-10, 0, 0))
    end_points = distributions.StaticUniformCircle(n_rays, aperture)
    distributions.BasePointTransformation(end_points)
    wavelengths = [drawing.YELLOW]
    if two_wavelengths:   # (an undense source matches its inputs 1:1)
        wavelengths = np.where(np.arange(n_rays) % 2 == 0, drawing.YELLOW, 650.0)
    source = sources.AperatureSource(
        3, start_points, end_points, wavelengths, dense=False,
        extra_fields={"object_coords": ("start_point", start_points, "points")})

    zero_points = mt.hexagonal_mesh(1.0, 3)
    zero_points.rotate_y(90)
    zero_points.rotate_x(90)
    r2 = (zero_points.points[:, 1] ** 2 + zero_points.points[:, 2] ** 2)
    vmap = np.random.default_rng(0).uniform(size=(zero_points.n_faces, 3)) > 0.25
    if value:
        material_list = [{"n_in": 1.49, "n_out": 1.0}] * 2
    else:
        material_list = [{"mat_in": 1, "mat_out": 0}] * 2
    lens = boundaries.ParametricMultiTriangleBoundary(
        zero_points, boundaries.FromVectorVG((1, 0, 0)),
        [boundaries.ThicknessConstraint(0.0, "min"), boundaries.ThicknessConstraint(0.2, "min")],
        [True, False], initial_parameters=[-0.15 * (1 - r2), 0.15 * (1 - r2)],
        material_list=material_list, vertex_update_map=vmap)
    target = boundaries.ManualTriangleBoundary(
        mesh=mt.plane(center=(10, 0, 0), direction=(1, 0, 0), i_size=100, j_size=100))
    target.frozen = True
    system = engine.OpticalSystem3D()
    system.optical = lens.surfaces
    system.targets = [target]
    system.sources = [source]
    if not value:
        system.materials = [{"n": materials.vacuum}, {"n": materials.acrylic}]
    system.update()
    index = []
    if value:   # tests/test_gpu_index_gradients._lens3d: per-face n_in as parameters
        rng = np.random.default_rng(3)
        for surface in lens.surfaces:
            n_in = torch.tensor(1.49 + 0.02 * rng.random(surface.face_verts.shape[0]),
                                dtype=torch.float64, device="cuda", requires_grad=True)
            surface.material_dict = {"n_in": n_in, "n_out": 1.0}
            surface.update_materials()
            index.append(n_in)
        system.update()
    eng = engine.OpticalEngine(
        3, [operation.StandardReaction("value" if value else "index")],
        simple_ray_inheritance={"wavelength", "object_coords"}, ray_dtype=torch.float64)
    eng.optical_system = system
    eng.validate_system()
    params = list(lens.parameters) + index
    erf = optimizer.GoalError(("y_end", "z_end"), lambda src: -src["object_coords"][:, 1:])
    opt = optimizer.SGD_Optimizer(eng, params, erf, depth, learning_rate=3e-5 if value else 3e-4,
                                  grad_clip=1e9, fused="auto", graph=False, speculative=False)
    opt.suppress_warnings = True
    return dict(opt=opt, eng=eng, system=system, lens=lens, target=target, source=source,
                params=params)


def _step(c):
    """WARM steps that move nothing (lr_scale = 0: the two runs of a case keep identical
    parameters), then one real step -> (error, terms, ray counts, parameters used, gradients)."""
    opt, params = c["opt"], c["params"]
    for _ in range(WARM):
        opt.single_step(None, lr_scale=0.0)
    c["system"].update()
    used = [p.detach().cpu().clone() for p in params]
    err = float(opt.single_step(None))
    terms = int(float(opt.last_error_terms))
    counts = np.stack([np.asarray(x) for x in c["eng"].last_trace["counts"]])
    scale = 0.01 * opt.learning_rate
    grads = [(u - p.detach().cpu()) / scale for u, p in zip(used, params)]
    return err, terms, counts, used, grads


def _oracle(c, used, depth, value):
    """Error sum, term count and parameter gradients by torch.autograd through the oracle, the
    source in contiguous slices of SLICE rays (tests/test_gpu_fullsize.py)."""
    q = [u.clone().requires_grad_(True) for u in used]
    if value:
        surfs = []
        for s, p, n_in in zip(c["lens"].surfaces, q[:2], q[2:]):
            f = _oracle_surface(s, p)
            del f["mat_in"], f["mat_out"]
            f["n_in"] = n_in
            f["n_out"] = torch.ones_like(n_in)
            surfs.append(f)
        tgt = tracer.faces_from_vertices(c["target"]._vertices.detach().cpu(),
                                         c["target"]._faces[:, 1:])
        osys = tracer.System(3, materials=[], optical=tracer.amalgamate(surfs), target=tgt)
        src = {k: v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu()
               for k, v in c["system"]._amalgamated_sources.items()}
    else:
        osys, src = _oracle_for(c["system"], c["lens"], c["target"], c["source"], q)
    n = src["x_start"].shape[0]
    total = [torch.zeros_like(u) for u in used]
    err_sum, terms = 0.0, 0
    for a in range(0, n, SLICE):
        part = {k: v[a:a + SLICE] for k, v in src.items()}
        ref = tracer.ray_trace(osys, part, max_iterations=depth,
                               inherit=("wavelength", "object_coords"),
                               index_type="value" if value else "index")
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


def _close(got, want, what):
    """max |got - want| <= TOL max |want|: test_gpu_fullsize's relative measure (a gradient that is
    zero must be met exactly)."""
    for k, (g, w) in enumerate(zip(got, want)):
        diff, ref = float((g - w).abs().max()), float(w.abs().max())
        print(f"{what}, parameter {k}: max |d| {diff:.3e}, max |ref| {ref:.3e}")
        assert diff <= TOL * ref, f"{what}, parameter {k}: {diff:.3e} against {ref:.3e}"


# rays, trace_depth, source aperture, two wavelengths, "value" mode with index gradients, and
# whether the step's sweep is the in-place goal kernel's
CASES = {
    "base_8192_depth_3": (8192, 3, 0.8, False, False, True),
    "last_wavefront_of_one_ray": (4161, 3, 0.8, False, False, True),
    "depth_1_no_child": (8192, 1, 0.8, False, False, True),
    "aperture_wider_than_the_lens": (8192, 3, 1.6, False, False, True),
    "depth_9_more_passes_than_lds_columns": (8192, 9, 0.8, False, False, False),
    "value_mode_index_gradients": (8192, 3, 0.8, False, True, False),
    "two_wavelengths_no_ratio_table": (8192, 3, 0.8, True, False, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_in_place_goal_sweep_equals_the_per_pass_step_and_the_oracle(name):
    """One eager fused step in place and one per pass from the same parameters: error, term count
    and ray counts equal exactly; parameter gradients ((p_before - p_after) / (0.01 * rate), the
    clip inactive) within 1e-8 of each other and of torch.autograd through the oracle.  The cases
    the in-place goal kernel's dispatch leaves to the general kernels are told by their results."""
    n_rays, depth, aperture, two_wl, value, own_kernel = CASES[name]
    kw = dict(aperture=aperture, two_wavelengths=two_wl, value=value)
    a = _case(n_rays, depth, **kw)
    b = _case(n_rays, depth, **kw)
    b["eng"].in_place = False                      # the per-pass fused step
    err_a, terms_a, counts_a, used_a, g_a = _step(a)
    err_b, terms_b, counts_b, used_b, g_b = _step(b)
    fs_a, fs_b = a["opt"]._fused_step, b["opt"]._fused_step
    assert fs_a is not None and fs_b is not None and fs_a.graph_replays == 0
    assert not fs_b.in_place
    if own_kernel:
        assert fs_a.in_place and fs_a.folded_backward
    for u, v in zip(used_a, used_b):
        assert torch.equal(u, v)                   # the two steps started from the same parameters
    print(f"{name}: error {err_a!r} / {err_b!r}, terms {terms_a} / {terms_b}")
    assert np.array_equal(np.float64(err_a), np.float64(err_b), equal_nan=True)
    assert terms_a == terms_b
    assert np.array_equal(counts_a, counts_b)
    _close(g_a, g_b, "in place against per pass")
    err_o, terms_o, g_o = _oracle(a, used_a, depth, value)
    assert terms_a == terms_o
    if terms_o:
        assert abs(err_a - err_o / terms_o) <= TOL * (err_o / terms_o)
    else:                                          # (trace_depth 1: no ray has reached the target)
        assert all(float(g.abs().max()) == 0.0 for g in g_o)
    _close(g_a, g_o, "in place against oracle autograd")
    _close(g_b, g_o, "per pass against oracle autograd")
