"""
The yardstick of tests/test_gpu_trace3d_sweep.py checked on its own, without a GPU:

* the constants that module restates are the ones in csrc/, and the plan of the reverse sweep
  still reads them the way _route_of says;
* for every scene and pass count of its cases the reference alone has what the cases assume:
  the class counts, finite gradients throughout, a gradient for every source ray;
* the oracle's gradients of the all-class error with respect to the source rays and the face
  vertices (and with them the dead_ray_length scaling of the dead class, the stopped class and
  the start rows of the active history) agree with central differences, over the rays whose path
  -- the face met in every pass and the branch taken there -- is the same at both ends of the step.
"""
import os

import numpy as np
import pytest
import torch

from oracle import tracer
import test_gpu_inplace_oracle as _io
import test_gpu_trace3d_sweep as S
from test_gpu_trace3d_sweep import CLASSES, GUIDE, GUIDE_DEEP, GUIDE_STASH, NAMES

H = 1e-6            # test_trace2d_sweep_oracle_host's step ...
BAR = 1e-5          # ... and its bar (what it is relative to: see the test)


def test_the_constants_the_gpu_cases_state_are_the_sources():
    assert S.constants_in_the_sources() == dict(
        BLOCK=S.BLOCK, FACE_WINDOW=S.FACE_WINDOW, CHAIN_MAXP=S.CHAIN_MAXP,
        STASH_MIN_RAYS=S.STASH_MIN_RAYS, COHERENT_MIN_RAYS=S.COHERENT_MIN_RAYS)
    root = os.path.dirname(os.path.dirname(S.CSRC))
    with open(os.path.join(root, "include", "tfrt_hip.h")) as f:
        header = f.read()
    assert f"#define TFRT_PROF_BACKWARD {S.PROF_BACKWARD}\n" in header
    assert f"#define TFRT_PROF_ACCUMULATE {S.PROF_ACCUMULATE}\n" in header


def test_the_routes_the_gpu_cases_name_are_the_plans():
    M = S._scene_for(GUIDE)[0].shape[0]
    assert M == 100 and M >= 64 and M <= S.FACE_WINDOW             # a hierarchy, one face window
    for route, key, n, p in S.ROUTE_CASES:
        assert S._route_of(n, M, p, route == "C", route in "DE") == route
    assert S._route_of(S.STASH_MIN_RAYS - 1, M, 3, False, False) == "A"
    assert S._route_of(S.STASH_MIN_RAYS, M, 3, False, False) == "B"
    assert S._route_of(S.STASH_MIN_RAYS, 32 * S.FACE_WINDOW + 1, 3, False, False) == "A"
    assert S._route_of(700, M, S.CHAIN_MAXP, False, True) == "E"
    assert S._route_of(700, M, S.CHAIN_MAXP + 1, False, True) == "D"
    assert S._route_of(700, M, 0, False, True) == "D"              # (no pass: nothing to chain)
    assert S._route_of(S.STASH_MIN_RAYS, M, 3, True, True) == "C"
    for seed in S.SOUP_SEEDS:
        P0, _, _, _, rays, _, passes, dead = S._scene_for(("soup", seed))
        assert P0.shape[0] >= 64 and rays.shape[1] < S.STASH_MIN_RAYS
        assert 1 <= passes <= S.CHAIN_MAXP and dead > 0


def test_the_error_is_the_in_place_modules_and_its_modes_add_up():
    r = S._reference(GUIDE, 700, False, 4, 0.25, "all")
    blocks = {c: torch.stack([r.sets[c][n] for n in NAMES]) for c in CLASSES}
    whole = _io._error(blocks)
    assert float(S._error(blocks)) == float(whole)
    parts = sum(S._error(blocks, c) for c in CLASSES)
    assert abs(float(parts) - float(whole)) <= 1e-14 * abs(float(whole))
    cols = sum(S._error_columns(blocks[c], k).sum() for k, c in enumerate(CLASSES))
    assert abs(float(cols) - float(whole)) <= 1e-14 * abs(float(whole))
    # the start rows alone: a part of the active class's error, and a different one
    start = float(S._error(blocks, "active_start"))
    assert 0.0 < abs(start) < abs(float(S._error(blocks, "active")))


# ------------------------------------------------------------ what the GPU cases assume

COUNTS = {      # finished / active / stopped / dead
    (GUIDE, 700, 1): (2, 698, 0, 0), (GUIDE, 700, 2): (8, 1250, 74, 66),
    (GUIDE, 700, 3): (18, 1771, 83, 78), (GUIDE, 700, 4): (35, 2275, 83, 78),
    (GUIDE_DEEP, 3000, 8): (780, 16531, 378, 366), (GUIDE_DEEP, 3000, 9): (965, 17822, 378, 366),
    (GUIDE_STASH, 16384, 3): (502, 40609, 2048, 2124),
    (GUIDE_STASH, 16383, 3): (502, 40608, 2047, 2124),
    (("soup", 2), 700, None): (63, 213, 33, 590), (("soup", 16), 2500, None): (73, 843, 122, 2255),
    (("soup", 25), 2500, None): (177, 773, 249, 2010),
}


@pytest.mark.parametrize("case", list(COUNTS), ids=lambda c: f"{c[0][0]}{c[0][1]}-{c[1]}x{c[2]}")
def test_the_reference_has_what_the_gpu_cases_assume(case):
    key, n_rays, passes = case
    *_, fixture_passes, fixture_dead = S._scene_for(key)
    passes = fixture_passes if passes is None else passes
    big = n_rays > 10000        # (the largest scenes: float64 state and one dead_ray_length here)
    for dead_len in ([fixture_dead] if key[0] == "soup" else [0.25] if big else [None, 0.25]):
        for f32 in ([False] if (big or key[0] == "soup") else [False, True]):
            r = S._reference(key, n_rays, f32, passes, dead_len, "all")
            assert tuple(r.counts[c] for c in CLASSES) == COUNTS[case], (case, r.counts)
            assert bool(torch.isfinite(r.g_fv).all()) and bool(torch.isfinite(r.g_src).all())
            assert r.g_fv.shape == (S._scene_for(key)[0].shape[0], 9)
            assert r.g_src.shape == (6, n_rays)
            assert bool((r.g_src != 0).any(0).all()), "a source ray without a gradient"
            assert float(r.g_fv.abs().max()) > 0.0


@pytest.mark.parametrize("mode", ["finished", "stopped", "dead", "active", "active_start"])
def test_the_reference_of_a_single_seeded_class(mode):
    """A seed of one class reaches exactly the source rays that have a row in that class (the
    698 of the 700 that meet an optical face first, for the active history); every mode moves
    the faces."""
    r = S._reference(GUIDE, 700, False, 4, 0.25, mode)
    assert bool(torch.isfinite(r.g_fv).all()) and bool(torch.isfinite(r.g_src).all())
    assert float(r.g_fv.abs().max()) > 0.0
    cols = int((r.g_src != 0).any(0).sum())
    cls = "active" if mode == "active_start" else mode
    assert cols == len(set(r.sets[cls]["ray_id"].tolist())), (mode, cols)
    assert cols == (698 if cls == "active" else r.counts[cls])


@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 129, S.BLOCK - 1, S.BLOCK, S.BLOCK + 1])
def test_the_reference_of_the_first_rays(n_rays):
    """The ray-count edges: the first n rays, 4 and 9 passes; every gradient finite."""
    for passes in (4, 9):
        r = S._reference(GUIDE, n_rays, False, passes, 0.25, "all")
        assert sum(r.counts.values()) >= n_rays and r.counts["active"] >= n_rays
        assert bool(torch.isfinite(r.g_fv).all()) and bool(torch.isfinite(r.g_src).all())
        assert bool((r.g_src != 0).any(0).all())


# ---------------------------------------------------------------------- central differences

PASSES = 4


def _system(P, cat, n_in, n_out):
    def sub(mask):
        verts = P[mask].reshape(-1, 3)
        d = tracer.faces_from_vertices(verts, torch.arange(verts.shape[0]).reshape(-1, 3))
        d["n_in"], d["n_out"] = n_in[mask], n_out[mask]
        return d
    return tracer.System(3, optical=sub(cat == 0), stop=sub(cat == 1), target=sub(cat == 2))


def _trace(P, rays, dead_len):
    """test_gpu_inplace_oracle._oracle_soup's trace of the light guide, pass by pass.  Returns
    the error ray by ray (a source ray's own links: the error is a sum over source rays) and the
    rays' paths: path[ray, pass] = (merged face met, or -1 for none, -2 once the ray has ended;
    1 refracted, 0 reflected, -1 where it did not react)."""
    _, cat, n_in, n_out, _, L, _, _ = S._scene_for(GUIDE)
    system = _system(P, cat, n_in, n_out)
    n = rays.shape[1]
    src = {name: rays[i] for i, name in enumerate(NAMES)}
    src["ray_id"] = torch.arange(n, dtype=torch.float64)
    history = {c: [] for c in CLASSES}
    path = torch.full((n, PASSES, 2), -2, dtype=torch.int64)
    cur = src
    for p in range(PASSES):
        ids = cur["ray_id"].long()
        new, proj = tracer.single_pass(
            system, cur, history, inherit=("ray_id",), index_type="value", new_ray_length=L,
            flags=dict(compile_dead_rays=True, compile_stopped_rays=True, dead_ray_length=dead_len))
        path[ids, p, 0] = torch.where(proj["valid"], proj["gather_trig"], -1)
        path[ids, p, 1] = -1
        if not new:
            break
        act = proj["rays"]["active"]
        norm = proj["optical"]["norm"].detach()
        d_in = torch.stack([act[a + "_end"] - act[a + "_start"] for a in "xyz"], 1).detach()
        d_out = torch.stack([new[a + "_end"] - new[a + "_start"] for a in "xyz"], 1).detach()
        same_side = ((d_in * norm).sum(1) > 0) == ((d_out * norm).sum(1) > 0)
        path[act["ray_id"].long(), p, 1] = same_side.long()
        cur = new
    per_ray = torch.zeros(n, dtype=torch.float64)
    counts = {}
    for k, c in enumerate(CLASSES):
        h = tracer.amalgamate(history[c])
        counts[c] = h["ray_id"].shape[0] if h else 0
        if h:
            per_ray = per_ray.index_add(0, h["ray_id"].long(),
                                        S._error_columns(torch.stack([h[f] for f in NAMES]), k))
    return per_ray, path, counts


@pytest.mark.parametrize("dead_len", [0.25, None])
def test_oracle_gradients_against_central_differences(dead_len):
    """Source rays: each of the six rows of all 700 rays stepped by +-H at once (a ray's error
    reads its own source ray only), every entry of the oracle's 6 x 700 gradient of the rays
    whose path is the same at all thirteen traces -- at least 97 % of them, asserted -- to BAR of
    the ray's largest gradient entry.  Face vertices: the M x 9 block stepped by +-H along six
    directions (three over all faces, one each over the mirrors, the glass walls, and the stop
    and target), the directional derivative of the error of the rays that keep their path (at
    least 95 %, asserted), under three weightings of the rays, to BAR of sum |gradient x
    direction|."""
    P0, cat, n_in, n_out, rays0, L, _, _ = S._scene_for(GUIDE)
    n, M = rays0.shape[1], P0.shape[0]
    P = P0.clone().requires_grad_(True)
    rays = rays0.clone().requires_grad_(True)
    per_ray, base, counts = _trace(P, rays, dead_len)
    assert tuple(counts[c] for c in CLASSES) == COUNTS[GUIDE, 700, PASSES]
    ref = S._reference(GUIDE, n, False, PASSES, dead_len, "all")
    assert abs(float(per_ray.sum().detach()) - ref.loss) <= 1e-13 * abs(ref.loss)
    g_src, g_fv = torch.autograd.grad(per_ray.sum(), [rays, P], retain_graph=True)
    assert float((g_src - ref.g_src).abs().max()) <= 1e-12 * float(ref.g_src.abs().max())
    assert float((g_fv - ref.g_fv).abs().max()) <= 1e-12 * float(ref.g_fv.abs().max())

    # ---- source rays
    with torch.no_grad():       # (a step a bounce can feel does change paths: the watch works)
        far = rays0.clone()
        far[1] += 0.05
        moved = float((_trace(P0, far, dead_len)[1] != base).any(2).any(1).float().mean())
    assert 0.02 < moved < 1.0, moved
    steady = torch.ones(n, dtype=torch.bool)
    fd = torch.zeros_like(g_src)
    with torch.no_grad():
        for row in range(6):
            vals = []
            for sgn in (1.0, -1.0):
                shifted = rays0.clone()
                shifted[row] += sgn * H
                v, path, _ = _trace(P0, shifted, dead_len)
                steady &= (path == base).all(2).all(1)
                vals.append(v)
            fd[row] = (vals[0] - vals[1]) / (2 * H)
    share = float(steady.float().mean())
    scale = g_src.abs().max(0).values
    err = ((fd - g_src).abs() / scale)[:, steady]
    print(f"dead_ray_length {dead_len}: source rays, {share:.3f} of the rays keep their path, "
          f"central difference rel err {float(err.max()):.2e}")
    assert share >= 0.97, share
    for k, c in enumerate(CLASSES):         # rays that end in every class are among them
        ended = torch.zeros(n, dtype=torch.bool)
        ended[ref.sets[c]["ray_id"].long()] = True
        assert int((ended & steady).sum()) >= 0.9 * int(ended.sum()), c
    assert float(err.max()) <= BAR, float(err.max())

    # ---- face vertices
    rng = np.random.default_rng(11)
    kinds = {"all 1": cat >= 0, "all 2": cat >= 0, "all 3": cat >= 0, "mirrors": n_in == 0.0,
             "glass": n_in == 1.5, "stop and target": cat > 0}
    weights = [torch.ones(n, dtype=torch.float64)] + \
        [torch.tensor(rng.uniform(0.5, 1.5, n)) for _ in range(2)]
    for name, faces in kinds.items():
        assert int(faces.sum()) > 0, name
        V = torch.tensor(rng.uniform(-1.0, 1.0, (M, 9))) * faces[:, None]
        with torch.no_grad():
            plus, path_p, _ = _trace(P0 + H * V, rays0, dead_len)
            minus, path_m, _ = _trace(P0 - H * V, rays0, dead_len)
        keep = (path_p == base).all(2).all(1) & (path_m == base).all(2).all(1)
        share = float(keep.float().mean())
        assert share >= 0.95, (name, share)
        for w in weights:
            wk = w * keep
            (g,) = torch.autograd.grad((wk * per_ray).sum(), [P], retain_graph=True)
            want = float((g * V).sum())
            got = float((wk * (plus - minus)).sum() / (2 * H))
            rel = abs(got - want) / float((g * V).abs().sum())
            print(f"dead_ray_length {dead_len}: faces, {name}: {share:.3f} of the rays keep "
                  f"their path, directional derivative {want:.6e}, central difference rel err "
                  f"{rel:.2e}")
            assert float((g * V).abs().sum()) > 0.0
            assert rel <= BAR, (name, rel)
