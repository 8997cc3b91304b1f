"""
The in-place trace (tfrt_scene3d.in_place: all passes in one launch, rays kept in their slots) and
its reverse sweep (k_backward_chain on the in-place tape) against torch.autograd through the float64
oracle -- not against another HIP path.  Each test covers one mode of the sweep:

* chain records re-read from HBM (a trace of more than CHAIN_MAXP = 8 passes: chain_in_lds = 0),
  with P = 8 and P = 9 on both sides of the limit: a lens, a mirrored light guide whose rays bounce
  more than ten times, and reference-fixture soups (stops, dead rays, mirrors, TIR, coplanar ties);
* the gradient with respect to the source rays (slot = ray in place, no rayid table);
* index gradients on an in-place tape (GN: grad_n_in / grad_n_out) -- in tests/test_gpu_trace3d.py,
  test_value_mode_gradient_with_respect_to_the_refractive_indices[in_place];
* the refract / total-internal-reflection branch bits recorded on the in-place tape, at the
  critical angle.

Every trace here first asserts that it takes the in-place route (assert_in_place).
"""
import numpy as np
import pytest
import torch

import oracle_util
import scene_util
from oracle import tracer
from test_gpu_inplace import assert_in_place
from test_gpu_trace3d import _gpu_scene
from test_reference_golden import SOUP, _check_grad, _soup_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
CLASSES = ("finished", "active", "stopped", "dead")


def _flags():
    from tensorflowraytrace_amd import _lib
    return _lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_DEAD | _lib.COMPILE_STOPPED


def _error(blocks):
    """A scalar of every class's rays (6 x n blocks, float64): every row of every class carries a
    gradient, the classes weighted differently."""
    tot = 0.0
    for k, cls in enumerate(CLASSES):
        r = blocks.get(cls)
        if r is None or r.shape[1] == 0:
            continue
        w = torch.arange(1, 7, dtype=torch.float64, device=r.device)[:, None] * (0.3 + k)
        tot = tot + (w * r * r).sum() * 1e-2 + (r[3:] * r[:3]).sum()
    return tot


def _oracle_blocks(ref):
    return {cls: torch.stack([ref[cls][n] for n in NAMES]) for cls in CLASSES
            if ref.get(cls) and ref[cls]["x_start"].shape[0]}


def _in_place(src, fv, args, passes, order=None, **kw):
    """In-place trace of the natural-order rays `src` over `order` (default ops.ray_order; ids and
    classes handed back in the natural numbering through perm=); gradients reach `src` through the
    permutation."""
    from tensorflowraytrace_amd import ops
    order = ops.ray_order(src.detach()) if order is None else order
    args.coherent_rays = True
    args.coherent_only = args.in_place = True
    assert_in_place(args, fv.detach(), src.shape[1], passes)
    return ops.trace3d(src[:, order.long()].contiguous(), fv, args, max_passes=passes,
                       flags=_flags(), perm=order, **kw)


def _same_sets(out, ref, tol, tag):
    """Same rays in the same classes and order; coordinates to `tol` of the class's magnitude."""
    for cls in CLASSES:
        rs = ref.get(cls) or {}
        n = rs["x_start"].shape[0] if "x_start" in rs else 0
        assert out[cls].shape[1] == n, (tag, cls, out[cls].shape[1], n)
        if n:
            assert np.array_equal(out[cls + "_id"].cpu().numpy().astype(np.int64),
                                  rs["ray_id"].numpy().astype(np.int64)), (tag, cls)
            want = torch.stack([rs[k] for k in NAMES]).detach().numpy()
            got = out[cls].detach().cpu().double().numpy()
            assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) <= tol, (tag, cls)


def _rel(got, want):
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())


# ------------------------------------------------------------------------------------------ lens

@pytest.mark.parametrize("passes,dtype,tol", [
    (8, torch.float64, 1e-8), (9, torch.float64, 1e-8), (10, torch.float64, 1e-8),
    (12, torch.float64, 1e-8), (10, torch.float32, 1e-5), (12, torch.float32, 1e-5)])
def test_in_place_lens_gradients_against_oracle_autograd(passes, dtype, tol):
    """6,000 rays through the lens, P on both sides of CHAIN_MAXP: d error / d (lens parameters,
    source rays) of an error over the finished and active rays."""
    from tensorflowraytrace_amd import ops
    scene = scene_util.lens_scene(6000, k_front=6, k_back=4)
    src0, fv, sc, (p_f, p_b) = _gpu_scene(scene, dtype, cluster="group")
    src = src0.detach().clone().requires_grad_(True)
    order = ops.ray_order(src.detach())
    args = ops.Scene3DArgs(fv.detach(), sc.catagory, mat_in=sc.mat_in, mat_out=sc.mat_out,
                           n_table=sc.n_table[:, order.long()].contiguous(),
                           face_grad_mask=sc.face_grad_mask, cluster_order=sc.cluster_order)
    out = _in_place(src, fv, args, passes, order)
    assert out["finished"].shape[1] > 4000
    err = _error({c: out[c].double() for c in CLASSES})
    g_f, g_b, g_src = torch.autograd.grad(err, [p_f, p_b, src])

    system, (q_f, q_b), _ = oracle_util.lens_oracle(scene)
    osrc = oracle_util.source_dict(scene["rays"], scene["wavelength"],
                                   np.float32 if dtype == torch.float32 else None)
    leaves = [osrc[n].requires_grad_(True) for n in NAMES]
    ref = tracer.ray_trace(system, osrc, max_iterations=passes, inherit=("wavelength", "ray_id"),
                           flags=dict(compile_dead_rays=True, compile_stopped_rays=True))
    _same_sets(out, ref, 1e-9 if dtype == torch.float64 else 1e-5, passes)
    rerr = _error(_oracle_blocks(ref))
    assert abs(float(err) - float(rerr)) <= tol * abs(float(rerr))
    r_f, r_b, *r_src = torch.autograd.grad(rerr, [q_f, q_b] + leaves)
    assert _rel(g_f, r_f) <= tol and _rel(g_b, r_b) <= tol
    assert _rel(g_src, torch.stack(r_src)) <= tol


# --------------------------------------------------------------------------------- light guide

def _light_guide(n_rays, seed, length=12):
    """A square tube along +x (|y|, |z| < 1) whose y walls are mirrors (n_in = 0) and whose z walls
    are glass (the tube is inside: rays meet them from the glass side, most are totally
    reflected, steep ones refract out), 24 triangles per wall; a target caps the far end, a stop
    plane above catches what leaves through the top wall, what leaves through the bottom dies.
    Rays start inside near x = 0 heading +x at steep transverse angles: many bounce ten times and
    more.  Returns (faces (M,9), category, n_in, n_out, rays (6,N)) as float64 / int64 tensors."""
    tris, cat, n_in, n_out = [], [], [], []
    xs = np.linspace(0.0, length, length + 1)
    for x0, x1 in zip(xs[:-1], xs[1:]):
        for s in (-1.0, 1.0):
            # y = s walls: mirrors (orientation irrelevant)
            tris += [[(x0, s, -1), (x1, s, -1), (x0, s, 1)], [(x1, s, -1), (x1, s, 1), (x0, s, 1)]]
            cat += [0, 0]
            n_in += [0.0, 0.0]
            n_out += [1.0, 1.0]
            # z = s walls: normal pointing out of the tube (+z on top, -z at the bottom), glass in
            a, b, c = (x0, -1, s), (x1, -1, s), (x0, 1, s)
            d, e, f = (x1, -1, s), (x1, 1, s), (x0, 1, s)
            tris += ([[a, b, c], [d, e, f]] if s > 0 else [[a, c, b], [d, f, e]])
            cat += [0, 0]
            n_in += [1.5, 1.5]
            n_out += [1.0, 1.0]
    L = float(length)
    tris += [[(L, -2, -2), (L, 2, -2), (L, -2, 2)], [(L, 2, -2), (L, 2, 2), (L, -2, 2)]]
    cat += [2, 2]
    tris += [[(-5, -30, 3), (30, -30, 3), (-5, 30, 3)], [(30, -30, 3), (30, 30, 3), (-5, 30, 3)]]
    cat += [1, 1]
    n_in += [1.0] * 4
    n_out += [1.0] * 4
    rng = np.random.default_rng(seed)
    s = np.stack([rng.uniform(0.1, 0.5, n_rays), rng.uniform(-0.9, 0.9, n_rays),
                  rng.uniform(-0.9, 0.9, n_rays)])
    d = np.stack([np.ones(n_rays), rng.uniform(-1.6, 1.6, n_rays), rng.uniform(-2.0, 2.0, n_rays)])
    rays = np.concatenate([s, s + 0.5 * d])
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return (t(np.asarray(tris).reshape(-1, 9)), torch.tensor(cat), t(n_in), t(n_out), t(rays))


def _oracle_soup(P, cat, n_in, n_out, rays, passes, L, dead=None):
    """torch.autograd-ready oracle trace of a triangle soup (value mode); P and rays are leaves."""
    def sub(mask):
        verts = P[mask].reshape(-1, 3)
        d = tracer.faces_from_vertices(verts, torch.arange(verts.shape[0]).reshape(-1, 3))
        d["n_in"], d["n_out"] = n_in[mask], n_out[mask]
        return d
    system = tracer.System(3, optical=sub(cat == 0), stop=sub(cat == 1), target=sub(cat == 2))
    src = {n: rays[i] for i, n in enumerate(NAMES)}
    src["ray_id"] = torch.arange(rays.shape[1], dtype=torch.float64)
    return tracer.ray_trace(system, src, max_iterations=passes, inherit=("ray_id",),
                            index_type="value", new_ray_length=L,
                            flags=dict(compile_dead_rays=True, compile_stopped_rays=True,
                                       dead_ray_length=dead))


def _soup_against_oracle(P0, cat, n_in, n_out, rays0, passes, L, dead, tag):
    """In-place trace + reverse sweep of a soup (float64 state) against the oracle: the same
    classes, ids and rays; d error / d (face vertices, source rays) to 1e-8 (same non-finite
    entries).  Returns the trace's per-pass counts."""
    from tensorflowraytrace_amd import ops
    fv = P0.to(DEV).requires_grad_(True)
    src = rays0.to(DEV).requires_grad_(True)
    args = ops.Scene3DArgs(fv.detach(), cat.int().to(DEV), n_in=n_in.to(DEV), n_out=n_out.to(DEV),
                           cluster_order=ops.cluster_order(fv.detach()))
    out = _in_place(src, fv, args, passes, new_ray_length=L, dead_ray_length=dead)
    err = _error({c: out[c] for c in CLASSES})
    g_fv, g_src = torch.autograd.grad(err, [fv, src])

    P = P0.clone().requires_grad_(True)
    rays = rays0.clone().requires_grad_(True)
    ref = _oracle_soup(P, cat, n_in, n_out, rays, passes, L, dead)
    _same_sets(out, ref, 1e-9, tag)
    rerr = _error(_oracle_blocks(ref))
    assert abs(float(err) - float(rerr)) <= 1e-8 * abs(float(rerr)), tag
    r_fv, r_src = torch.autograd.grad(rerr, [P, rays])
    _check_grad(g_fv.cpu().numpy(), r_fv.numpy(), tag, "face vertices", 1e-8)
    _check_grad(g_src.cpu().numpy(), r_src.numpy(), tag, "source rays", 1e-8)
    return out["counts"]


@pytest.mark.parametrize("passes", [8, 9, 10, 12])
def test_in_place_light_guide_against_oracle_autograd(passes):
    """Chains longer than the LDS columns hold: from P = 9 on the reverse sweep re-reads every
    record of a ray's chain from HBM at the ray's own slot."""
    P0, cat, n_in, n_out, rays = _light_guide(3000, seed=passes)
    counts = _soup_against_oracle(P0, cat, n_in, n_out, rays, passes, 1.0, None, f"guide P={passes}")
    assert counts[passes - 1, 0] > 100                 # rays still bouncing after the last pass
    assert counts[:, 1].sum() > 100 and counts[:, 2].sum() > 10 and counts[:, 3].sum() > 10


@pytest.mark.parametrize("seed", [2, 16, 25])
def test_in_place_reference_soups_at_ten_passes_against_oracle_autograd(seed):
    """The adversarial soups of tests/golden/reference_soup3d.npz (coplanar ties, mirrors, total
    internal reflection, stops) traced over ten passes -- chain records from HBM -- with their
    rays cut to dead_ray_length when they die."""
    sc = _soup_case(np.load(SOUP), seed)
    _soup_against_oracle(sc["P"], sc["cat"], sc["n_in"], sc["n_out"], sc["rays"], 10, sc["L"],
                         sc["dead"], f"soup {seed}")


# ------------------------------------------------------------------------------ critical angle

def test_in_place_gradients_at_the_critical_angle():
    """test_gpu_trace3d.test_gradients_at_the_critical_angle_and_float32_against_float64_state (i)
    made large enough to go in place: the flat glass face is 128 coplanar triangles, every ray meets
    it inside its own triangle, within 1e-12 .. 0.2 rad of the critical angle on both sides.  The
    branch the reverse sweep takes is the one recorded on the in-place tape: ids and gradients
    those of the oracle (same bar as the small scene)."""
    from tensorflowraytrace_amd import ops
    n_glass = 1.5
    crit = np.arcsin(1.0 / n_glass)
    k, h = 8, 5.0                                   # 8 x 8 cells of 5 x 5 in the plane x = 0
    tris = []
    for i in range(k):
        for j in range(k):
            y0, z0 = -20.0 + i * h, -20.0 + j * h
            # (normals +x: n_in = glass on the -x side)
            tris += [[0, y0, z0, 0, y0 + h, z0, 0, y0, z0 + h],
                     [0, y0 + h, z0, 0, y0 + h, z0 + h, 0, y0, z0 + h]]
    tris += [[40.0, -500.0, -500.0, 40.0, 500.0, -500.0, 40.0, 0.0, 800.0],
             [-40.0, -500.0, -500.0, -40.0, 0.0, 800.0, -40.0, 500.0, -500.0],
             [-100.0, 30.0, -300.0, 100.0, 30.0, -300.0, 0.0, 30.0, 600.0]]
    M = len(tris)
    P = torch.tensor(tris, dtype=torch.float64, device=DEV, requires_grad=True)
    cat = torch.tensor([0] * (M - 3) + [2] * 3, dtype=torch.int32, device=DEV)
    n_in = torch.tensor([n_glass] * (M - 3) + [1.0] * 3, dtype=torch.float64, device=DEV)
    n_out = torch.ones(M, dtype=torch.float64, device=DEV)
    off = np.array([-1e-9, -1e-12, 1e-12, 1e-9, -0.2, 0.1])
    # every cell's lower triangle is hit at its centroid, by each of the six angles in turn
    hits = [(-20.0 + i * h + h / 3, -20.0 + j * h + h / 3) for i in range(k) for j in range(k)]
    ang = crit + np.resize(off, len(hits) * 2)
    hy = np.repeat([y for y, _ in hits], 2)
    hz = np.repeat([z for _, z in hits], 2)
    d = np.stack([-np.cos(ang), -np.sin(ang), np.zeros_like(ang)])       # from inside the glass
    s = np.stack([d[0], hy + d[1], hz])
    e = np.stack([0.5 * d[0], hy + 0.5 * d[1], hz])
    rays = torch.tensor(np.concatenate([s, e]), dtype=torch.float64, device=DEV)
    N = rays.shape[1]
    args = ops.Scene3DArgs(P.detach(), cat, n_in=n_in, n_out=n_out,
                           cluster_order=ops.cluster_order(P.detach()))
    out = _in_place(rays, P, args, 2)
    assert out["finished"].shape[1] == N                               # refracted out or reflected back
    back = int((out["finished"][3] < 0).sum())
    assert 0 < back < N                                                # both branches taken
    loss = (out["finished"][4] ** 2).sum() + out["finished"][5].sum()
    (g,) = torch.autograd.grad(loss, [P])
    assert bool(torch.isfinite(g).all())

    Pc = P.detach().cpu().clone().requires_grad_(True)
    faces = tracer.faces_from_vertices(Pc.reshape(-1, 3), torch.arange(3 * M).reshape(M, 3))
    optical = torch.arange(M) < M - 3
    sub = lambda m: {key: v[m] for key, v in faces.items()}
    opt_f = sub(optical)
    opt_f["n_in"], opt_f["n_out"] = n_in.cpu()[optical], n_out.cpu()[optical]
    system = tracer.System(3, optical=opt_f, target=sub(~optical))
    src = {key: rays[i].cpu() for i, key in enumerate(NAMES)}
    src["ray_id"] = torch.arange(N, dtype=torch.float64)
    ref = tracer.ray_trace(system, src, max_iterations=2, inherit=("ray_id",), index_type="value")
    assert np.array_equal(out["finished_id"].cpu().numpy(),
                          ref["finished"]["ray_id"].numpy().astype(np.int32))
    assert int((ref["finished"]["x_end"] < 0).sum()) == back
    rloss = (ref["finished"]["y_end"] ** 2).sum() + ref["finished"]["z_end"].sum()
    (rg,) = torch.autograd.grad(rloss, [Pc])
    assert float((g.cpu() - rg).abs().max() / rg.abs().max()) < 1e-7
