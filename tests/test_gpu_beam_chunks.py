"""
The chunks of the beam walk (beam_pass, tfrt_trace3d.hip): the candidate faces of a bundle are met in
chunks of CHUNK entries of its face list -- 32 in k_trace_inplace<float>, whose shorter record table
leaves room for a sixth wavefront per SIMD, 64 in every other kernel that shares the walk
(k_intersect_beam, k_trace_inplace_rows, float64 state).  A chunk boundary only decides the order in
which the faces are met, so every trace must equal the all-pairs trace of the same scene -- the
independent path with plain division and no hierarchy: counts, decided pairs, and every class's
rays (ids, faces, rows: start and hit point of every pass) bit for bit.  (The tape's hit parameter
is not handed out by the public API; it is compared through the rows made of it.)

Scenes: K small triangles stacked along the x axis, perpendicular to it, all inside the radius of
ONE wavefront's bundle of parallel rays, so that the bundle's face list holds exactly K entries
(64 filler faces far off the axis give the scene its hierarchy and are nobody's candidates).

  K        31, 32, 33, 63, 64, 65, 97: around one and two boundaries of either chunk size; 200:
           more than BEAM_FLIST = 192 candidates, the bundle is cut down to single rays and each
           goes through the brute-force arm
  order    face index ascending with depth, descending, shuffled (the face list follows the
           cluster order; ties go to the lower INDEX whatever the list's order)
  starts   ray i starts just in front of stack position (5 i) mod K, so the nearest face of
           some ray lies in every chunk, the first, the second and the last among them; towards
           +x and towards -x
  ties     every stack position holds TWO coplanar, congruent faces (the twin's index is higher by
           the number of positions), with one single face in front of the stack or without it
           (K or K - 1 faces): in a list that follows depth the pairs sit at places
           (2j, 2j + 1) or (2j + 1, 2j + 2), so one of the two variants has a pair on either side
           of every boundary -- equal hit parameters to the last bit, the lower index must win
  rays     1, 63 (fewer than 64: not an in-place trace -- the per-pass path), 64, 65, 129
  passes   1 and 3: the faces refract with equal indices on both sides (the child goes straight
           on to the next face that holds it: passes 2 and 3 meet the boundaries too), every fifth
           is a mirror (the child goes back through the stack), targets close both ends

Each scene goes through the in-place trace with float32 state (32-face chunks), with float64 state
and through the per-pass beam path (64-face chunks).  The triangles differ in size and centre, so
rays of one wavefront hit different faces; _margin() asserts on the host that no ray passes the
line of a face's edge nearer than 1e-8: a hundred times eps_size (1e-10), and 1e8 times what the
float64 decisions of two paths can differ by on coordinates of 0.1 (some forty thousand ray-edge
pairs over a disc of 0.04 leave no more than a few 1e-8 in the worst scene).
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_inplace import assert_in_place, _flags, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

X0, DX = 1.0, 0.05           # the stack: position p at x = X0 + p DX
R_BUNDLE = 0.04              # the rays' disc
N_FILL = 64


def _triangle(rng, x):
    """A triangle in the plane x = const around the axis: circumradius 0.03 .. 0.12 (some hold the
    whole disc of rays, some a part of it), centre off the axis by up to 0.01."""
    r = rng.uniform(0.03, 0.12)
    c = rng.uniform(-0.01, 0.01, 2)
    a0 = rng.uniform(0, 2 * np.pi)
    ang = a0 + np.array([0.0, 2.1, 4.2])
    return np.stack([np.full(3, x), c[0] + r * np.cos(ang), c[1] + r * np.sin(ang)], axis=1)   # (3, 3)


@functools.lru_cache(maxsize=None)
def _stack(K, order, ties, lead):
    """-> face vertices (M, 9) float64, category (M,), n_in, n_out (M,), x of every stack position.
    ties: two congruent faces per position, K apart in index; lead: one single face in front."""
    rng = np.random.default_rng(1000 * K + 10 * ("ascending", "descending", "shuffled").index(order)
                                + 2 * ties + lead)
    n_lead = 1 if ties and lead else 0
    n_pos = (K - n_lead) // 2 if ties else K
    pos_x = X0 + DX * np.arange(n_lead + n_pos)
    leads = [_triangle(rng, pos_x[p]) for p in range(n_lead)]
    first = [_triangle(rng, pos_x[n_lead + j]) for j in range(n_pos)]
    second = [t.copy() for t in first] if ties else []
    stack = leads + first + second          # index: the single face, the positions, then their twins
    depth = list(range(n_lead)) + list(range(n_lead, n_lead + n_pos)) * (2 if ties else 1)
    if not ties:
        perm = {"ascending": np.arange(len(stack)), "descending": np.arange(len(stack))[::-1],
                "shuffled": rng.permutation(len(stack))}[order]
        stack = [stack[j] for j in perm]
        depth = [depth[j] for j in perm]
    n_stack = len(stack)
    cat = np.zeros(n_stack, dtype=np.int64)                       # optical
    n_in = np.ones(n_stack)
    n_out = np.ones(n_stack)
    for j in range(n_stack):
        if depth[j] % 5 == 4:
            n_in[j] = 0.0                                         # a mirror (both twins of a pair)
    # targets behind both ends, filler (stops) far off the axis
    far = []
    for x in (X0 - 2.0, X0 + DX * len(pos_x) + 2.0):
        far.append(np.array([[x, -3.0, -3.0], [x, 3.0, -3.0], [x, 0.0, 4.0]]))
    fill = []
    for j in range(N_FILL):
        y, z = 50.0 + 2.0 * (j % 8), 50.0 + 2.0 * (j // 8)
        fill.append(np.array([[3.0, y, z], [3.0, y + 1.0, z], [3.0, y, z + 1.0]]))
    P = np.stack(stack + far + fill).reshape(-1, 9)
    cat = np.concatenate([cat, np.full(2, 2), np.full(N_FILL, 1)])
    n_in = np.concatenate([n_in, np.ones(2 + N_FILL)])
    n_out = np.concatenate([n_out, np.ones(2 + N_FILL)])
    return P, cat, n_in, n_out, pos_x, np.array(depth)


def _rays(N, pos_x, sign):
    """(6, N) float64, float32-representable: parallel to x on a sunflower disc, ray i starting
    DX / 2 in front of stack position (5 i) mod len(pos_x), seen along its direction."""
    i = np.arange(N)
    r = R_BUNDLE * np.sqrt((i + 0.5) / N)
    a = i * 2.399963229728653
    y, z = (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32)
    xs = (pos_x[(5 * i) % len(pos_x)] - sign * DX / 2).astype(np.float32)
    xe = (xs + np.float32(sign)).astype(np.float32)
    return np.stack([xs, y, z, xe, y, z]).astype(np.float64)


def _margin(P, n_stack, rays):
    """Smallest distance of a ray's (y, z) from the line through an edge of a stack face."""
    y, z = rays[1], rays[2]
    m = np.inf
    for f in range(n_stack):
        v = P[f].reshape(3, 3)[:, 1:]
        for k in range(3):
            a, b = v[k], v[(k + 1) % 3]
            e = b - a
            d = np.abs(e[0] * (z - a[1]) - e[1] * (y - a[0])) / np.hypot(e[0], e[1])
            m = min(m, float(d.min()))
    return m


def _trace(P, cat, n_in, n_out, rays, dtype, passes, mode):
    from tensorflowraytrace_amd import ops
    fv = torch.tensor(P, dtype=torch.float64, device=DEV)
    base = dict(n_in=torch.tensor(n_in, device=DEV), n_out=torch.tensor(n_out, device=DEV))
    r = torch.tensor(rays, device=DEV).to(dtype)
    c = torch.tensor(cat, device=DEV).int()
    if mode == "all_pairs":
        args = ops.Scene3DArgs(fv, c, **base)
    else:
        args = ops.Scene3DArgs(fv, c, cluster_order=ops.cluster_order(fv), coherent_rays=True, **base)
        args.coherent_only = True
        args.in_place = mode == "in_place"
        if args.in_place and r.shape[1] >= 64:
            assert_in_place(args, fv, r.shape[1], passes)
    return ops.trace3d(r, fv, args, max_passes=passes, flags=_flags())


def _check(K, order, ties, lead, N, passes, sign):
    P, cat, n_in, n_out, pos_x, depth = _stack(K, order, ties, lead)
    n_stack = P.shape[0] - 2 - N_FILL
    rays = _rays(N, pos_x, sign)
    assert _margin(P, n_stack, rays) > 1e-8
    for dtype in (torch.float32, torch.float64):
        ref = _trace(P, cat, n_in, n_out, rays, dtype, passes, "all_pairs")
        assert int(ref["counts"][0, 0]) + int(ref["counts"][0, 1]) == N     # every ray hits in pass 1
        for mode in ("in_place", "per_pass"):
            out = _trace(P, cat, n_in, n_out, rays, dtype, passes, mode)
            _same(out, ref, (K, order, ties, lead, N, passes, sign, dtype, mode))


KS = (31, 32, 33, 63, 64, 65, 97)
NS = (1, 63, 64, 65, 129)


@pytest.mark.parametrize("sign", [1, -1], ids=["towards+x", "towards-x"])
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("K", KS)
def test_stack_around_the_chunk_boundaries(K, order, sign):
    # (every K meets every ray count and both depths over the orders and directions)
    j = KS.index(K) + ("ascending", "descending", "shuffled").index(order) + (sign < 0)
    for N, passes in ((NS[j % 5], 3), (NS[(j + 2) % 5], 1), (64, 3 if j % 2 else 1)):
        _check(K, order, False, False, N, passes, sign)


@pytest.mark.parametrize("lead", [False, True], ids=["pairs_from_place_0", "pairs_from_place_1"])
@pytest.mark.parametrize("K", (64, 65, 97))
def test_equal_hit_parameters_on_either_side_of_a_boundary(K, lead):
    """Twins at equal depth: every hit is a tie between two faces, adjacent in any list that follows
    depth; with and without a single face in front one of the variants has a pair on either side of
    the boundaries at 32 and 64.  The all-pairs trace gives the lower index; so must the walk."""
    P, cat, n_in, n_out, pos_x, depth = _stack(K, "ascending", True, lead)
    n_lead = 1 if lead else 0
    n_pos = (K - n_lead) // 2
    n_stack = n_lead + 2 * n_pos
    assert P.shape[0] == n_stack + 2 + N_FILL
    for N, passes, sign in ((64, 1, 1), (129, 3, 1), (65, 3, -1)):
        _check(K, "ascending", True, lead, N, passes, sign)
        out = _trace(P, cat, n_in, n_out, _rays(N, pos_x, sign), torch.float32, 1, "in_place")
        hit = torch.cat([out["active_face"], out["finished_face"]]).cpu().numpy()
        paired = hit[(hit >= n_lead) & (hit < n_stack)]
        # a face that has a twin is hit through the lower of the two indices
        assert paired.size > 0 and int(paired.max()) < n_lead + n_pos


@pytest.mark.parametrize("N", [1, 64])
def test_more_candidates_than_the_face_list_holds(N):
    """200 faces on the axis: more than BEAM_FLIST, the bundle is cut down to single rays and every
    ray goes against every member slot of the scene, a chunk at a time (one ray: the per-pass path)."""
    _check(200, "shuffled", False, False, N, 3, 1)
