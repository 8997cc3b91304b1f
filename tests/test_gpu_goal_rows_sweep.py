"""
k_backward_chain_goal_inplace with the goal's rows as a compile-time fact (its ROWS parameter,
tfrt_trace3d.hip): a goal on ("y_end", "z_end") -- rows 4 and 5, ascending -- takes the instantiation
that knows them, every other goal the one that reads them from its arguments.  The route is chosen
from the goal alone, so the tests choose it by the goal they state.

The scene is scene_util.lens_scene with k_front = 5, k_back = 3 (the smallest lens the in-place tests
use, 206 faces) and a source wider than the lens (aperture 1.6): rays outside the lens finish on the
target in the FIRST pass, rays through it in the third, so a trace holds wavefronts that finish in
one pass, in three, and mixed ones.  tfrt_trace3d_forward (in place, no ray sets) and
tfrt_trace3d_backward_goal are called through the C ABI, with a block for the source rays' gradient.

  rays     64 (one wavefront: the in-place route starts there), 65, 128 and 191
  passes   1, 2, 3
  state    float32 and float64
  faces    nine terms per face, and the four sums (tfrt_scene3d.face_sums) expanded here by
           trace_math.h's face_sums_expand formulas
  frozen   with and without a frozen front surface (zero bytes of face_grad_mask)
  goals    ("y_end", "z_end"): the instantiated rows; ("z_end",) and ("x_end", "y_end", "z_end"):
           ascending rows decided at run time; ("z_end", "y_end") with the columns swapped: not
           ascending, the run-time loop over the columns

1. every goal against torch.autograd through the oracle: error, term count, face-vertex gradient
   pulled back to the lens parameters, and the source rays' gradient, at 1e-8 of the largest entry
   (float64 state) and 1e-5 (float32) -- the tolerances of tests/test_gpu_sweep_one_round_trip.py;
2. ("y_end", "z_end") against ("z_end", "y_end") with swapped columns: a lane adds its two squared
   residuals to zero in either order, so the error and the seeds have the same bits.  The error is
   equal bit for bit at every size, the source gradient (one lane per ray) too; the face gradients
   bit for bit at 64 rays (one wavefront: one adder per face), and at the other sizes no further
   from a run of the run-time route than three runs of that route are from each other;
3. the same goal through the general chain kernel (k_backward_chain<..., GOAL = true, ...>, taken when
   the indices are one table column per ray): error equal bit for bit and gradients at 1e-8 in
   float64 state, as tests/test_gpu_chain_goal_inplace.py keeps these two routes together; 1e-5 in
   float32 state.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle_util
import scene_util
from oracle import tracer
from test_gpu_inplace import assert_in_place
from test_gpu_trace3d import _gpu_scene

pytestmark = pytest.mark.gpu

NAMES = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
RAYS = (64, 65, 128, 191)
DEPTHS = (1, 2, 3)
K_FRONT, K_BACK = 5, 3

# name: (fields, column of _goal_table holding each field's goal)
GOALS = {
    "y_end-z_end": (("y_end", "z_end"), (0, 1)),
    "z_end": (("z_end",), (1,)),
    "x_end-y_end-z_end": (("x_end", "y_end", "z_end"), (2, 0, 1)),
    "z_end-y_end": (("z_end", "y_end"), (1, 0)),
}


def _goal_table(scene):
    """(N, 3) float64: the image point of every ray's object point (y, z) and, for x_end, a plane
    a little in front of the target -- a residual that is not zero."""
    g = np.asarray(scene["goal"], dtype=np.float64)
    x = 9.5 + 0.25 * np.cos(np.arange(g.shape[0]))
    return np.concatenate([g, x[:, None]], axis=1)


@functools.lru_cache(maxsize=None)
def _scene(n_rays):
    return scene_util.lens_scene(n_rays, k_front=K_FRONT, k_back=K_BACK, aperture=1.6)


_oracle_traces = {}


def _oracle(n_rays, depth, f32, goal_name):
    """(error sum, terms, d / d front parameters, d / d back parameters, d / d source rays (6, N))
    by autograd through the oracle; the trace is made once per (rays, depth, rounding) and shared,
    the results are never written to."""
    key = (n_rays, depth, f32)
    if key not in _oracle_traces:
        scene = _scene(n_rays)
        system, (q_f, q_b), _ = oracle_util.lens_oracle(scene)
        src = oracle_util.source_dict(scene["rays"], scene["wavelength"], np.float32 if f32 else None)
        leaves = [src[n].requires_grad_(True) for n in NAMES]
        ref = tracer.ray_trace(system, src, max_iterations=depth, inherit=("wavelength", "ray_id"))
        _oracle_traces[key] = (ref.get("finished"), q_f, q_b, leaves, {})
    rf, q_f, q_b, leaves, done = _oracle_traces[key]
    if goal_name not in done:
        fields, cols = GOALS[goal_name]
        zero = lambda: (torch.zeros_like(q_f), torch.zeros_like(q_b), torch.zeros(6, n_rays, dtype=torch.float64))
        if not rf or rf["y_end"].shape[0] == 0:
            done[goal_name] = (0.0, 0) + zero()
        else:
            table = torch.tensor(_goal_table(_scene(n_rays)))[rf["ray_id"].long()]
            out = torch.stack([rf[f] for f in fields], 1)
            sq = (out - table[:, list(cols)]) ** 2
            grads = torch.autograd.grad(sq.sum(), [q_f, q_b] + leaves, retain_graph=True,
                                        allow_unused=True)
            z = zero()
            g_f = z[0] if grads[0] is None else grads[0]
            g_b = z[1] if grads[1] is None else grads[1]
            g_src = torch.stack([torch.zeros(n_rays, dtype=torch.float64) if g is None else g
                                 for g in grads[2:]])
            done[goal_name] = (float(sq.sum().detach()), sq.numel(), g_f, g_b, g_src)
    return done[goal_name]


class _Lens:
    """The lens on the device, its rays in a coherent order, and the buffers of one in-place trace
    and its goal sweep; sweep() runs both through the C ABI."""

    def __init__(self, n_rays, depth, dtype, frozen, per_ray_indices=False):
        from tensorflowraytrace_amd import _lib, ops
        self.n, self.depth, self.dtype = n_rays, depth, dtype
        scene = _scene(n_rays)
        src, fv, sc, (self.p_f, self.p_b) = _gpu_scene(scene, dtype, cluster="group")
        self.fv = fv
        self.fvd = fv.detach().contiguous()
        self.order = ops.ray_order(src)
        o = self.order.long()
        self.rays = src[:, o].contiguous()
        self.n_front = 6 * K_FRONT * K_FRONT
        mask = sc.face_grad_mask.clone()
        if frozen:
            mask[:self.n_front] = 0
        if per_ray_indices:      # one table column per ray: no per-face index table (feta)
            table = sc.n_table[:, o].contiguous()
        else:                    # one wavelength, one column: the indices are per face
            table = sc.n_table[:, :1].contiguous()
        self.args = ops.Scene3DArgs(self.fvd, sc.catagory, mat_in=sc.mat_in, mat_out=sc.mat_out,
                                    n_table=table, face_grad_mask=mask,
                                    cluster_order=sc.cluster_order, coherent_rays=True)
        self.args.n_table_uniform = not per_ray_indices
        self.args.coherent_only = self.args.in_place = True
        assert_in_place(self.args, self.fvd, n_rays, depth)
        self.table = torch.tensor(_goal_table(scene), device="cuda")[o]      # (N, 3), trace order
        L = _lib.lib()
        self.M, self.dt = self.fvd.shape[0], ops._DT[dtype]
        self.wsb = L.tfrt_trace3d_workspace_bytes(n_rays, self.M, depth, self.dt)
        self.ws = torch.zeros(max(self.wsb, 1), dtype=torch.uint8, device="cuda")
        self.gwb = L.tfrt_trace3d_backward_goal_workspace_bytes(n_rays)
        self.gws = torch.zeros(max(self.gwb, 1), dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros(_lib.COUNTS_PER_PASS * (depth + 1), dtype=torch.int32, device="cuda")
        self.fin = torch.zeros((6, n_rays), dtype=dtype, device="cuda")
        self.fin_id = torch.zeros(n_rays, dtype=torch.int32, device="cuda")
        self.fin_face = torch.zeros(n_rays, dtype=torch.int32, device="cuda")

    def sweep(self, goal_name, face_sums):
        """-> (error sum, terms, (M, 9) face-vertex gradient, (6, N) source gradient in the trace's
        order), float64 on the host."""
        from tensorflowraytrace_amd import _lib, ops
        L = _lib.lib()
        fields, cols = GOALS[goal_name]
        rows = (ctypes.c_int32 * 6)(*([NAMES.index(f) for f in fields] + [0] * 6)[:6])
        goal = self.table[:, list(cols)].t().contiguous()                   # (fields, N) columns
        n, P = self.n, self.depth
        st = self.args.struct(self.fvd)
        stream = ops._stream(self.rays)
        none = ops._ray_out(None, None, None)
        g_fv = torch.zeros((self.M, 9), dtype=torch.float64, device="cuda")
        g_src = torch.zeros((6, n), dtype=torch.float64, device="cuda")
        err = torch.zeros(3, dtype=torch.float64, device="cuda")
        tests = torch.zeros(1, dtype=torch.int64, device="cuda")
        pending = _lib.GoalPending()
        old = st.face_sums
        try:
            st.face_sums = 1 if face_sums else 0
            _lib.check(L.tfrt_trace3d_forward(
                ops._p(self.rays), n, n, ctypes.byref(st), 1.0, 0.0, P, self.dt, _lib.COMPILE_FINISHED,
                ctypes.byref(none), ctypes.byref(none), ctypes.byref(none), ctypes.byref(none),
                None, None, ops._p(self.counts), ops._p(self.ws), self.wsb, stream), "forward")
            _lib.check(L.tfrt_trace3d_backward_goal(
                ops._p(self.rays), n, n, ctypes.byref(st), 1.0, 0.0, P, self.dt,
                ctypes.byref(ops._ray_out(self.fin, self.fin_id, self.fin_face)), rows, len(fields),
                ops._p(goal), n, 1, ops._p(err), ops._p(tests), ops._p(self.gws), self.gwb,
                ctypes.byref(pending), None, 0, None, 0, None, 0, ops._p(g_fv), ops._p(g_src),
                ops._p(self.counts), ops._p(self.ws), self.wsb, stream), "backward_goal")
            _lib.check(L.tfrt_goal_finish(ctypes.byref(pending), stream), "goal_finish")
            torch.cuda.synchronize()
        finally:
            st.face_sums = old
        g = g_fv.cpu()
        if face_sums:
            assert float(g[:, 4:].abs().max()) == 0.0      # four sums and five zeros per face
            g = _expand(self.fvd.cpu(), g[:, :4])
        e = err.cpu()
        return float(e[0]), int(e[1]), g, g_src.cpu()

    def to_parameters(self, g_fv):
        """The face-vertex gradient pulled back to the two surfaces' parameters."""
        g = torch.autograd.grad(self.fv, [self.p_f, self.p_b], grad_outputs=g_fv.to(self.fv.device),
                                retain_graph=True)
        return [x.cpu() for x in g]

    def natural(self, g_src):
        out = torch.zeros_like(g_src)
        out[:, self.order.cpu().long()] = g_src
        return out


def _expand(P, S):
    """csrc/trace_math.h face_sums_expand: the nine vertex gradients of every face from its four
    sums (the gradient w.r.t. C = E1 x E2 and w.r.t. the hit parameter's numerator)."""
    E1, E2 = P[:, 3:6] - P[:, 0:3], P[:, 6:9] - P[:, 0:3]
    C = torch.cross(E1, E2, dim=1)
    Cb, numb = S[:, :3], S[:, 3:4]
    E1b, E2b = torch.cross(E2, Cb, dim=1), torch.cross(Cb, E1, dim=1)
    return torch.cat([numb * C - (E1b + E2b), E1b, E2b], dim=1)


def _close(got, want, tol, what):
    """max |got - want| <= tol max |want| (a gradient that is zero must be met exactly)."""
    diff, ref = float((got - want).abs().max()), float(want.abs().max())
    print(f"  {what}: max |d| {diff:.3e}, max |ref| {ref:.3e}, bound {tol * ref:.3e}")
    assert diff <= tol * ref, f"{what}: {diff:.3e} against {ref:.3e}"


# every (rays, passes) with both state types; four sums and the frozen surface alternate so that
# each meets every ray count, every depth and both state types
CASES = [(n, d, dt, (i + j + k) % 2 == 0, (i + (j + k) // 2) % 2 == 1)
         for i, n in enumerate(RAYS) for j, d in enumerate(DEPTHS)
         for k, dt in enumerate((torch.float64, torch.float32))]


def _id(case):
    n, d, dt, four, frozen = case
    return (f"{n}_rays-depth_{d}-{'f32' if dt == torch.float32 else 'f64'}-"
            f"{'four_sums' if four else 'nine_terms'}{'-frozen_front' if frozen else ''}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_goal_against_oracle_autograd(case):
    n, depth, dtype, four, frozen = case
    f32 = dtype == torch.float32
    tol = 1e-5 if f32 else 1e-8
    lens = _Lens(n, depth, dtype, frozen)
    for name in GOALS:
        err, terms, g_fv, g_src = lens.sweep(name, four)
        err_o, terms_o, r_f, r_b, r_src = _oracle(n, depth, f32, name)
        print(f"{_id(case)} {name}: error {err!r} / {err_o!r}, terms {terms} / {terms_o}")
        assert terms == terms_o and terms_o > 0
        assert abs(err - err_o) <= tol * err_o
        g_f, g_b = lens.to_parameters(g_fv)
        if frozen:
            assert float(g_fv[:lens.n_front].abs().max()) == 0.0
            assert float(g_f.abs().max()) == 0.0
        else:
            _close(g_f, r_f, tol, "front parameters")
        # (before the third pass next to no ray has reached the target through the lens: a
        # gradient that is zero in the oracle is zero here)
        _close(g_b, r_b, tol, "back parameters")
        if depth == 3:
            assert float(r_b.abs().max()) > 0.0
        assert float(g_fv[lens.n_front + 6 * K_BACK * K_BACK:].abs().max()) == 0.0   # the target
        _close(lens.natural(g_src), r_src, tol, "source rays")


@pytest.mark.parametrize("four", [False, True], ids=["nine_terms", "four_sums"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", RAYS)
def test_known_rows_against_the_same_goal_with_swapped_columns(n, dtype, four):
    lens = _Lens(n, 3, dtype, False)
    err_k, terms_k, fv_k, src_k = lens.sweep("y_end-z_end", four)
    runs = [lens.sweep("z_end-y_end", four) for _ in range(3)]
    assert terms_k > 0
    for err_r, terms_r, _, src_r in runs:
        assert terms_r == terms_k
        assert np.float64(err_r).tobytes() == np.float64(err_k).tobytes()
        assert torch.equal(src_r, src_k)
    spread = max(float((runs[a][2] - runs[b][2]).abs().max()) for a in range(3) for b in range(a))
    away = min(float((fv_k - r[2]).abs().max()) for r in runs)
    print(f"{n} rays: run-time route's spread {spread:.3e}, known rows from the nearest run {away:.3e}")
    if n == 64:
        assert all(torch.equal(fv_k, r[2]) for r in runs)
    assert away <= spread


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("n", RAYS)
def test_known_rows_against_the_general_chain_kernel(n, depth, dtype):
    f32 = dtype == torch.float32
    tol = 1e-5 if f32 else 1e-8
    four = (n + depth) % 2 == 0
    own = _Lens(n, depth, dtype, False).sweep("y_end-z_end", four)
    general = _Lens(n, depth, dtype, False, per_ray_indices=True).sweep("y_end-z_end", four)
    print(f"{n} rays, depth {depth}: error {own[0]!r} / {general[0]!r}, terms {own[1]} / {general[1]}")
    assert own[1] == general[1] > 0
    if f32:
        assert abs(own[0] - general[0]) <= tol * general[0]
    else:
        assert np.float64(own[0]).tobytes() == np.float64(general[0]).tobytes()
    _close(own[2], general[2], tol, "face vertices")
    if depth == 3:
        assert float(general[2].abs().max()) > 0.0
    _close(own[3], general[3], tol, "source rays")
