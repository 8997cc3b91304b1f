"""
wave_face_sums (csrc/tfrt_trace3d.hip) in every tier of its LDS layout: a wavefront's face
gradients are summed per distinct face in LDS, eight copies of every sum for up to 8 faces, four for
up to 16, two for up to 32; beyond 32 slots the remaining faces' lanes go straight to memory while
the 32 slots are folded.  The lens of tests/test_gpu_chain_goal_inplace.py with meshes of different
density, so that 64-ray wavefronts meet 1 .. 8, 9 .. 16, 17 .. 32 and more than 32 faces in a pass:

  kernel    k_backward_chain_goal_inplace (one wavelength) and the general k_backward_chain (two
            wavelengths: no per-face ratio table, tests/test_gpu_chain_goal_inplace.py)
  rays      4,161 (a last wavefront of one ray) and 8,192
  mesh      hexagonal_mesh(1.0, k), k = 3, 6, 9, 13, source aperture 0.8 or 1.6

From k = 10 on the engine would no longer trace such a source in place (its wavefronts are no narrow
bundles); sweep_drive.force_in_place keeps it there.

Tier check: the recorded hit faces are read back from the step's tape -- tfrt_trace3d_compact cuts
every class's records, with their faces and ray positions, out of the workspace the sweep has just
read -- and the faces a pass's wave_face_sums is handed are counted on the host per 64-ray group:
those of the records of rays that reach the target (the others carry no gradient), on surfaces whose
gradient is wanted (not the target).  The case's tier must hold a (wavefront, pass); over the cases
every tier does, a count of exactly 8 or 9 occurs, both lens surfaces' passes are counted, and 4,161
rays leave a last wavefront of one ray.

Gradient check: parameter gradients against torch.autograd through the oracle, float64 state at 1e-8
of the largest entry (the sweep's stated tolerance, as test_gpu_sweep_one_round_trip._close applies
it), float32 state at 1e-5; exactly zero where the oracle's gradient is exactly zero.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sweep_drive import force_in_place
from test_gpu_chain_goal_inplace import _case, _oracle, _step
from test_gpu_sweep_one_round_trip import _oracle_of

pytestmark = pytest.mark.gpu

TIERS = ("1-8", "9-16", "17-32", "33+")
DEPTH = 3
# name: rays, mesh k, aperture, two wavelengths (the general kernel), float32 state, the tier aimed at
CASES = {
    "goal_inplace-8192-k3": (8192, 3, 0.8, False, False, "1-8"),
    "goal_inplace-4161-k6-wide": (4161, 6, 1.6, False, False, "9-16"),
    "goal_inplace-4161-k9-wide": (4161, 9, 1.6, False, False, "17-32"),
    "goal_inplace-4161-k13-wide": (4161, 13, 1.6, False, False, "33+"),
    "goal_inplace-4161-k9-wide-float32": (4161, 9, 1.6, False, True, "17-32"),
    "chain-4161-k3": (4161, 3, 0.8, True, False, "1-8"),
    "chain-8192-k6-wide": (8192, 6, 1.6, True, False, "9-16"),
    "chain-4161-k9-wide": (4161, 9, 1.6, True, False, "17-32"),
    "chain-4161-k13-wide": (4161, 13, 1.6, True, False, "33+"),
}


def _tier(n):
    return TIERS[0 if n <= 8 else (1 if n <= 16 else (2 if n <= 32 else 3))]


def _tape_faces(fs):
    """(P, N) recorded hit face of every ray position and pass (-1: no record or no hit) and (N,)
    whether the ray reached the target, from the tape in the step's workspace."""
    from tensorflowraytrace_amd import _lib, ops
    st = fs._state
    N, P, dev = st.N, st.P, st.block.device
    caps = {"finished": N, "active": N * P, "stopped": N, "dead": N}
    buf, outs = {}, []
    for name in ("finished", "active", "stopped", "dead"):
        rays = torch.empty((6, caps[name]), dtype=st.block.dtype, device=dev)
        ids = torch.full((caps[name],), -1, dtype=torch.int32, device=dev)
        faces = torch.full((caps[name],), -1, dtype=torch.int32, device=dev)
        buf[name] = (rays, ids, faces)
        outs.append(ops._ray_out(rays, ids, faces))
    unf = torch.empty((6, N), dtype=st.block.dtype, device=dev)
    unf_id = torch.empty(N, dtype=torch.int32, device=dev)
    counts = torch.zeros(_lib.COUNTS_PER_PASS * (P + 1), dtype=torch.int32, device=dev)
    flags = (_lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_STOPPED | _lib.COMPILE_DEAD)
    rc = _lib.lib().tfrt_trace3d_compact(
        ops._p(st.block), st.block.shape[1], N, 0.0, P, st.dt, flags, ctypes.byref(outs[0]),
        ctypes.byref(outs[1]), ctypes.byref(outs[2]), ctypes.byref(outs[3]), ops._p(unf),
        ops._p(unf_id), ops._p(counts), st.M, None, ops._p(st.ws), st.wsb, ops._stream(st.block))
    assert rc == 0
    torch.cuda.synchronize()
    cnt = counts.cpu().numpy().reshape(P + 1, _lib.COUNTS_PER_PASS)
    face = np.full((P, N), -1, dtype=np.int64)
    finished = np.zeros(N, dtype=bool)
    for name, col in (("active", _lib.CLS_ACTIVE), ("finished", _lib.CLS_FINISHED),
                      ("stopped", _lib.CLS_STOPPED)):
        ids, faces = buf[name][1].cpu().numpy(), buf[name][2].cpu().numpy()
        for p in range(P):
            n, base = int(cnt[p, col]), int(cnt[p, 4 + col])
            face[p, ids[base:base + n]] = faces[base:base + n]
            if name == "finished":
                finished[ids[base:base + n]] = True
    return face, finished


@functools.lru_cache(maxsize=None)
def _run(name):
    """One step of the case -> (distinct faces handed to wave_face_sums per (pass, wavefront), the
    lens surfaces' face counts, and what the gradient check needs)."""
    import tfrt.mesh_tools as mt
    n_rays, k, aperture, two_wl, f32, _ = CASES[name]
    with pytest.MonkeyPatch.context() as mp:
        plain = mt.hexagonal_mesh
        mp.setattr(mt, "hexagonal_mesh", lambda radius, _k, *a, **kw: plain(radius, k, *a, **kw))
        c = _case(n_rays, DEPTH, aperture=aperture, two_wavelengths=two_wl)
        mp.setattr(mt, "hexagonal_mesh", plain)
        force_in_place(mp, c["eng"])
        if f32:
            c["eng"].ray_dtype = torch.float32
        err, terms, _, used, grads = _step(c)
        fs = c["opt"]._fused_step
        assert fs is not None and fs.graph_replays == 0
        assert fs.in_place and fs.folded_backward      # in place, the goal folded into the sweep
        assert fs._state.N == n_rays and fs._state.P == DEPTH
        face, finished = _tape_faces(fs)
    n_faces = [s.face_verts.shape[0] for s in c["lens"].surfaces]
    wanted = (face >= 0) & (face < sum(n_faces)) & finished[None, :]     # (the target is frozen)
    per = np.zeros((DEPTH, (n_rays + 63) // 64), dtype=np.int64)
    surfaces = set()
    for p in range(DEPTH):
        for w in range(per.shape[1]):
            lanes = slice(64 * w, 64 * w + 64)
            seen = set(face[p, lanes][wanted[p, lanes]].tolist())
            per[p, w] = len(seen)
            surfaces |= {0 if f < n_faces[0] else 1 for f in seen}
    return dict(c=c, per=per, surfaces=surfaces, err=err, terms=terms, used=used, grads=grads)


@pytest.mark.parametrize("name", list(CASES))
def test_face_sums_of_every_tier_against_oracle_autograd(name):
    n_rays, k, aperture, two_wl, f32, aimed = CASES[name]
    r = _run(name)
    per = r["per"]
    hist = {t: int(sum(_tier(n) == t for n in per.ravel() if n > 0)) for t in TIERS}
    print(f"{name}: distinct faces per (pass, wavefront) handed to wave_face_sums: tiers {hist}, "
          f"max per pass {per.max(1).tolist()}, counts {np.bincount(per.ravel()).tolist()}")
    assert hist[aimed] > 0, f"no wavefront in tier {aimed}: {hist}"
    assert r["surfaces"] == {0, 1}                     # the front surface's pass and the back one's
    if n_rays % 64:
        assert n_rays % 64 == 1 and per.shape[1] == n_rays // 64 + 1     # a last wavefront of one ray

    tol = 1e-5 if f32 else 1e-8
    c, used = r["c"], r["used"]
    if f32:     # (the oracle's trace starts from the float32 block, like the step's)
        err_o, terms_o, g_o = _oracle_of(c, (n_rays, DEPTH, aperture, 2, False), used, float32_source=True)
    else:
        err_o, terms_o, g_o = _oracle(c, used, DEPTH, False)
    assert r["terms"] == terms_o and terms_o > 0
    assert abs(r["err"] - err_o / terms_o) <= tol * (err_o / terms_o)
    for i, (g, w) in enumerate(zip(r["grads"], g_o)):
        diff, ref = float((g - w).abs().max()), float(w.abs().max())
        print(f"  parameter {i}: max |d| {diff:.3e}, max |ref| {ref:.3e}")
        assert ref > 0.0
        assert diff <= tol * ref, f"parameter {i}: {diff:.3e} against {ref:.3e}"
        assert bool((g[w == 0.0] == 0.0).all())


def test_every_tier_and_the_edge_between_the_first_two_are_met():
    """Over the cases (each run once per session, here or above): every tier holds a (pass,
    wavefront), and a count of exactly 8 or 9 distinct faces occurs."""
    counts = np.concatenate([_run(name)["per"].ravel() for name in CASES])
    counts = counts[counts > 0]
    for t in TIERS:
        assert any(_tier(n) == t for n in counts), f"no wavefront in tier {t}"
    assert ((counts == 8) | (counts == 9)).any()
