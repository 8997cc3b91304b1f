"""
What k_backward_chain_goal_inplace (tfrt_trace3d.hip) forms behind its walk back since it keeps five
wavefronts per SIMD: the wavefront's error sum (`partial`), its two counts (`partial_cnt`: finished
rays, passes its rays entered) and the rays' columns of `grad_src_rays` -- their addresses are made
of the wavefront's index and the lane after the walk, not ahead of it.

tfrt_trace3d_forward (in place, no ray sets) and tfrt_trace3d_backward_goal are called through the
C ABI as tests/test_gpu_goal_rows_sweep.py calls them, and the goal workspace is read back before
tfrt_goal_finish folds it: one float64 per 64 rays, then (256-byte aligned) two int32 per 64 rays.

The scene is scene_util.lens_scene with k_front = 5, k_back = 3 and a source a little wider than the
lens (aperture 1.3).  The rays are traced in the source's own order, in which the end points spiral
outwards: at 191 rays and two passes the first wavefront's rays all go through the lens (nobody
finishes, every ray enters both passes), the third's all miss it (everybody finishes in pass 1) and
the second is mixed; at three passes the first finishes in pass 3.  test_wavefront_roles asserts that
the oracle sees these roles.

  rays     1 and 63 (fewer than 64: not an in-place trace, the per-pass path and k_backward_chain
           write `partial` and no counts), 64, 65, 129 (a last wavefront of one ray), 191
  passes   2 and 3
  state    float32 and float64
  goals    ("y_end", "z_end"): the instantiated rows; ("x_end", "y_end", "z_end"): rows decided at
           run time
  faces    the four sums (the instantiation that keeps five wavefronts with known rows) and the
           nine terms, alternating
  g_src    requested and not requested

Checked per wavefront against host sums of the oracle's per-ray values: the error sum at 1e-8 of
the wavefront's sum (float64 state) and 1e-5 (float32) -- the tolerances of
tests/test_gpu_goal_rows_sweep.py --, exactly zero where no ray of the wavefront finishes; the two
counts exactly.  The source gradient against autograd through the oracle at the same tolerances;
without it the sums and counts must keep their bits and the face gradient stay within tolerance.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle_util
import scene_util
from oracle import tracer
from test_gpu_goal_rows_sweep import _expand, _close, NAMES
from test_gpu_trace3d import _gpu_scene

pytestmark = pytest.mark.gpu

RAYS = (1, 63, 64, 65, 129, 191)
DEPTHS = (2, 3)
K_FRONT, K_BACK = 5, 3
APERTURE = 1.3

# name: (fields, column of _goal_table holding each field's goal)
GOALS = {
    "y_end-z_end": (("y_end", "z_end"), (0, 1)),
    "x_end-y_end-z_end": (("x_end", "y_end", "z_end"), (2, 0, 1)),
}


@functools.lru_cache(maxsize=None)
def _scene(n_rays):
    return scene_util.lens_scene(n_rays, k_front=K_FRONT, k_back=K_BACK, aperture=APERTURE)


def _goal_table(scene):
    g = np.asarray(scene["goal"], dtype=np.float64)
    x = 9.5 + 0.25 * np.cos(np.arange(g.shape[0]))
    return np.concatenate([g, x[:, None]], axis=1)


_oracle_runs = {}


def _oracle(n_rays, depth, f32, goal_name):
    """Per ray, in source order, from the oracle: (finished (N,) bool, squared residuals summed over
    the goal's fields (N,) float64, passes entered (N,) int, d error / d source rays (6, N)).  The
    traces are made once per (rays, depth, rounding), shared and never written to."""
    key = (n_rays, depth, f32)
    if key not in _oracle_runs:
        scene = _scene(n_rays)
        system, _, _ = oracle_util.lens_oracle(scene)
        src = oracle_util.source_dict(scene["rays"], scene["wavelength"], np.float32 if f32 else None)
        leaves = [src[n].requires_grad_(True) for n in NAMES]
        ref = tracer.ray_trace(system, src, max_iterations=depth, inherit=("wavelength", "ray_id"))
        # a ray enters pass p + 1 when pass p leaves it active: once, plus once per pass before the
        # last that lists it among its active rays
        entered = np.ones(n_rays, dtype=np.int64)
        src1 = oracle_util.source_dict(scene["rays"], scene["wavelength"], np.float32 if f32 else None)
        before = tracer.ray_trace(system, src1, max_iterations=depth - 1,
                                  inherit=("wavelength", "ray_id")).get("active")
        if before and before["x_start"].shape[0]:
            entered += np.bincount(before["ray_id"].long().numpy(), minlength=n_rays)
        _oracle_runs[key] = (ref.get("finished"), leaves, entered, {})
    rf, leaves, entered, done = _oracle_runs[key]
    if goal_name not in done:
        fields, cols = GOALS[goal_name]
        fin = np.zeros(n_rays, dtype=bool)
        sq_ray = np.zeros(n_rays, dtype=np.float64)
        g_src = torch.zeros(6, n_rays, dtype=torch.float64)
        if rf and rf["y_end"].shape[0] > 0:
            ids = rf["ray_id"].long()
            table = torch.tensor(_goal_table(_scene(n_rays)))[ids]
            sq = (torch.stack([rf[f] for f in fields], 1).double() - table[:, list(cols)]) ** 2
            grads = torch.autograd.grad(sq.sum(), leaves, retain_graph=True, allow_unused=True)
            g_src = torch.stack([torch.zeros(n_rays, dtype=torch.float64) if g is None else g.double()
                                 for g in grads])
            fin[ids.numpy()] = True
            # (a ray's terms in the goal's field order, as the sweep adds them to zero)
            sq_ray[ids.numpy()] = sq.detach().numpy().sum(axis=1)
        done[goal_name] = (fin, sq_ray, entered, g_src)
    return done[goal_name]


def _per_wave(x, n):
    return np.array([x[a:a + 64].sum() for a in range(0, n, 64)])


class _Lens:
    """The lens on the device, its rays in the source's order, the buffers of one trace and its
    goal sweep; sweep() runs both through the C ABI and reads the goal workspace back."""

    def __init__(self, n_rays, depth, dtype):
        from tensorflowraytrace_amd import _lib, ops
        self.n, self.depth, self.dtype = n_rays, depth, dtype
        scene = _scene(n_rays)
        src, fv, sc, _ = _gpu_scene(scene, dtype, cluster="group")
        self.fvd = fv.detach().contiguous()
        self.rays = src.contiguous()
        self.args = ops.Scene3DArgs(self.fvd, sc.catagory, mat_in=sc.mat_in, mat_out=sc.mat_out,
                                    n_table=sc.n_table[:, :1].contiguous(),
                                    face_grad_mask=sc.face_grad_mask,
                                    cluster_order=sc.cluster_order, coherent_rays=True)
        self.args.n_table_uniform = True
        self.args.coherent_only = self.args.in_place = True
        L = _lib.lib()
        self.in_place = L.tfrt_trace3d_in_place(ctypes.byref(self.args.struct(self.fvd)), n_rays, depth) == 1
        assert self.in_place == (n_rays >= 64)
        self.table = torch.tensor(_goal_table(scene), device="cuda")
        self.M, self.dt = self.fvd.shape[0], ops._DT[dtype]
        self.wsb = L.tfrt_trace3d_workspace_bytes(n_rays, self.M, depth, self.dt)
        self.ws = torch.zeros(max(self.wsb, 1), dtype=torch.uint8, device="cuda")
        self.gwb = L.tfrt_trace3d_backward_goal_workspace_bytes(n_rays)
        self.counts = torch.zeros(_lib.COUNTS_PER_PASS * (depth + 1), dtype=torch.int32, device="cuda")
        self.fin = torch.zeros((6, n_rays), dtype=dtype, device="cuda")
        self.fin_id = torch.zeros(n_rays, dtype=torch.int32, device="cuda")
        self.fin_face = torch.zeros(n_rays, dtype=torch.int32, device="cuda")

    def sweep(self, goal_name, face_sums, with_src):
        """-> (partial (W,) float64, partial_cnt (W, 2) int32 or None, error sum, terms, (M, 9)
        face-vertex gradient, (6, N) source gradient or None), on the host."""
        from tensorflowraytrace_amd import _lib, ops
        L = _lib.lib()
        fields, cols = GOALS[goal_name]
        rows = (ctypes.c_int32 * 6)(*([NAMES.index(f) for f in fields] + [0] * 6)[:6])
        goal = self.table[:, list(cols)].t().contiguous()                   # (fields, N) columns
        n, P = self.n, self.depth
        st = self.args.struct(self.fvd)
        stream = ops._stream(self.rays)
        none = ops._ray_out(None, None, None)
        fin_out = ops._ray_out(self.fin, self.fin_id, self.fin_face)
        g_fv = torch.zeros((self.M, 9), dtype=torch.float64, device="cuda")
        g_src = torch.zeros((6, n), dtype=torch.float64, device="cuda") if with_src else None
        err = torch.zeros(3, dtype=torch.float64, device="cuda")
        tests = torch.zeros(1, dtype=torch.int64, device="cuda")
        # (poisoned: what the sweep leaves in it is what it wrote)
        gws = torch.full((max(self.gwb, 1),), 0xA5, dtype=torch.uint8, device="cuda")
        pending = _lib.GoalPending()
        old = st.face_sums
        try:
            st.face_sums = 1 if face_sums else 0
            _lib.check(L.tfrt_trace3d_forward(
                ops._p(self.rays), n, n, ctypes.byref(st), 1.0, 0.0, P, self.dt, _lib.COMPILE_FINISHED,
                ctypes.byref(none if self.in_place else fin_out), ctypes.byref(none),
                ctypes.byref(none), ctypes.byref(none),
                None, None, ops._p(self.counts), ops._p(self.ws), self.wsb, stream), "forward")
            _lib.check(L.tfrt_trace3d_backward_goal(
                ops._p(self.rays), n, n, ctypes.byref(st), 1.0, 0.0, P, self.dt,
                ctypes.byref(fin_out), rows, len(fields),
                ops._p(goal), n, 1, ops._p(err), ops._p(tests), ops._p(gws), self.gwb,
                ctypes.byref(pending), None, 0, None, 0, None, 0, ops._p(g_fv),
                None if g_src is None else ops._p(g_src),
                ops._p(self.counts), ops._p(self.ws), self.wsb, stream), "backward_goal")
            torch.cuda.synchronize()
            raw = gws.cpu().numpy()
            _lib.check(L.tfrt_goal_finish(ctypes.byref(pending), stream), "goal_finish")
            torch.cuda.synchronize()
        finally:
            st.face_sums = old
        W = (n + 63) // 64
        partial = raw[:8 * W].view(np.float64).copy()
        cnt = None
        if self.in_place:
            at = (8 * W + 255) // 256 * 256
            cnt = raw[at:at + 8 * W].view(np.int32).reshape(W, 2).copy()
        g = g_fv.cpu()
        if face_sums:
            assert float(g[:, 4:].abs().max()) == 0.0      # four sums and five zeros per face
            g = _expand(self.fvd.cpu(), g[:, :4])
        e = err.cpu()
        return partial, cnt, float(e[0]), int(e[1]), g, None if g_src is None else g_src.cpu()


CASES = [(n, d, dt, (i + j + k) % 2 == 0)
         for i, n in enumerate(RAYS) for j, d in enumerate(DEPTHS)
         for k, dt in enumerate((torch.float32, torch.float64))]


def _id(case):
    n, d, dt, four = case
    return f"{n}_rays-depth_{d}-{'f32' if dt == torch.float32 else 'f64'}-{'four_sums' if four else 'nine_terms'}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_partials_counts_and_source_gradient_per_wavefront(case):
    n, depth, dtype, four_first = case
    f32 = dtype == torch.float32
    tol = 1e-5 if f32 else 1e-8
    lens = _Lens(n, depth, dtype)
    for g, name in enumerate(GOALS):
        four = four_first == (g == 0)       # (both goals meet both forms over the cases)
        fin, sq_ray, entered, r_src = _oracle(n, depth, f32, name)
        want_err, want_fin, want_ent = _per_wave(sq_ray, n), _per_wave(fin, n), _per_wave(entered, n)
        partial, cnt, err, terms, g_fv, g_src = lens.sweep(name, four, True)
        print(f"{_id(case)} {name} four_sums={four}: partial {partial} / {want_err}, counts "
              f"{None if cnt is None else cnt.tolist()} / {want_fin.tolist()} {want_ent.tolist()}")
        assert partial.shape == want_err.shape
        for w in range(partial.shape[0]):
            if want_fin[w] == 0:
                assert partial[w] == 0.0, (w, partial[w])
            else:
                assert abs(partial[w] - want_err[w]) <= tol * want_err[w], (w, partial[w], want_err[w])
        if cnt is not None:
            assert cnt[:, 0].tolist() == want_fin.tolist()
            assert cnt[:, 1].tolist() == want_ent.tolist()
        assert terms == int(fin.sum()) * len(GOALS[name][0])
        assert abs(err - sq_ray.sum()) <= tol * sq_ray.sum()
        if float(r_src.abs().max()) > 0.0:
            _close(g_src, r_src, tol, "source rays")
        else:
            assert float(g_src.abs().max()) == 0.0
        # the same sweep without a block for the source gradient
        partial2, cnt2, err2, terms2, g_fv2, none = lens.sweep(name, four, False)
        assert none is None and terms2 == terms
        assert partial2.tobytes() == partial.tobytes()
        assert (cnt is None and cnt2 is None) or cnt2.tolist() == cnt.tolist()
        assert np.float64(err2).tobytes() == np.float64(err).tobytes()
        if float(g_fv.abs().max()) > 0.0:
            _close(g_fv2, g_fv, tol, "face vertices, no source gradient asked for")
        else:
            assert float(g_fv2.abs().max()) == 0.0


def test_wavefront_roles():
    """191 rays: the oracle sees a wavefront in which no ray finishes, one in which every ray
    finishes in pass 1 and a mixed one (two passes), and one that finishes in pass 3 (three)."""
    fin, _, entered, _ = _oracle(191, 2, True, "y_end-z_end")
    fw, ew = _per_wave(fin, 191), _per_wave(entered, 191)
    assert fw[0] == 0 and ew[0] == 128                    # through the lens: nobody finishes
    assert 0 < fw[1] < 64 and 64 < ew[1] < 128            # mixed
    assert fw[2] == 63 and ew[2] == 63                    # past the lens: all finish in pass 1
    fin3, _, entered3, _ = _oracle(191, 3, True, "y_end-z_end")
    fw3, ew3 = _per_wave(fin3, 191), _per_wave(entered3, 191)
    assert fw3[0] == 64 and ew3[0] == 192                 # ... and in pass 3
    assert fw3[2] == 63 and ew3[2] == 63
