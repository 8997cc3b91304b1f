"""BASELINE.json's full-size workload (configs[3]: 1,000,000 rays x 10,574 faces, 3 passes) through
size-independent properties: the dense oracle cannot run at this size, so the checks are

* conservation: every ray entering a pass leaves it in exactly one class; the test counter is
  sum(N_active) x M; source-ray ids inside a class are strictly increasing (the reference's
  boolean_mask keeps the order);
* trace-mode independence: the sphere hierarchy and the all-pairs filter give bit-identical rays,
  ids and faces;
* a random sample of the 1M rays traced by the oracle (256 rays x 10,574 faces is seconds of CPU)
  agrees ray by ray with the full-size run (float32 state: 1e-5 relative);
* shard additivity: the two halves of the ray set traced separately give the same rays, and their
  parameter gradients sum to the gradient of the whole (the multi-GPU ray sharding relies on it);
* permutation invariance: the same rays in another order give the same per-ray result.
"""
import numpy as np
import pytest
import torch

import oracle_util
import scene_util
from oracle import tracer
from test_gpu_trace3d import _gpu_scene
from scene_configs import _build_5a, _oracle_5a, _scene_5b, N_5A, PASSES_5A

pytestmark = pytest.mark.gpu

N_FULL, K_FRONT, K_BACK, PASSES = 1_000_000, 41, 9, 3


@pytest.fixture(scope="module")
def full():
    from tensorflowraytrace_amd import ops, _lib
    scene = scene_util.lens_scene(N_FULL, k_front=K_FRONT, k_back=K_BACK)
    flags = _lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_DEAD | _lib.COMPILE_STOPPED
    src, fv, sc, params = _gpu_scene(scene, torch.float32, cluster="group")
    out = ops.trace3d(src, fv, sc, max_passes=PASSES, flags=flags)
    return dict(scene=scene, src=src, fv=fv, sc=sc, params=params, out=out, flags=flags)


def test_full_size_conservation_and_order(full):
    out, M = full["out"], full["fv"].shape[0]
    assert M == 10_574
    counts = out["counts"]                                    # (P, 8): per-pass class counts + bases
    n_in = N_FULL
    for p in range(PASSES):
        assert int(counts[p, :4].sum()) == n_in               # nothing lost, nothing duplicated
        n_in = int(counts[p, 0])                              # the active rays go on
    assert out["n_tests"] == int(counts[:, :4].sum()) * M
    assert out["finished"].shape[1] > 800_000                 # the lens images most of the beam
    assert out["finished"].shape[1] == int(counts[:, 1].sum())
    assert out["dead"].shape[1] == int(counts[:, 3].sum())
    # inside a class the rays of one pass keep the source order (boolean_mask semantics)
    for col, cls in ((1, "finished"), (2, "stopped"), (3, "dead")):
        ids = out[cls + "_id"].long()
        assert torch.unique(ids).numel() == ids.numel()       # one entry per ray at most
        base = 0
        for p in range(PASSES):
            seg = ids[base:base + int(counts[p, col])]
            assert bool((seg[1:] > seg[:-1]).all()), (cls, p)
            base += int(counts[p, col])
        assert base == ids.numel()
    # per pass the active history keeps the source order
    act = out["active_id"].long()
    base = 0
    for p in range(PASSES):
        n = int(counts[p, 0])
        seg = act[base:base + n]
        assert bool((seg[1:] > seg[:-1]).all())
        base += n
    fin = out["finished"].detach()
    assert bool(torch.isfinite(fin).all())
    assert float((fin[3] - 10.0).abs().max()) < 1e-5          # finished rays end on the target plane


def test_full_size_hierarchy_equals_all_pairs(full):
    from tensorflowraytrace_amd import ops
    src, fv, sc_all, _ = _gpu_scene(full["scene"], torch.float32, cluster=False)
    ref = ops.trace3d(src, fv, sc_all, max_passes=PASSES, flags=full["flags"])
    out = full["out"]
    assert np.array_equal(out["counts"], ref["counts"]) and out["n_tests"] == ref["n_tests"]
    for cls in ("finished", "active", "stopped", "dead"):
        assert torch.equal(out[cls + "_id"], ref[cls + "_id"]), cls
        assert torch.equal(out[cls + "_face"], ref[cls + "_face"]), cls
        assert torch.equal(out[cls], ref[cls]), cls


def test_full_size_coherent_order_changes_nothing(full):
    """cfg4 at full size traced in the coherent order (tfrt_scene3d.coherent_rays: the source
    sorted along a Hilbert curve, k_intersect_beam): every wavefront is a narrow bundle (nothing is
    left to the grouped kernel) and ops.restore_order gives the natural-order trace back bit for
    bit -- with and without the grouped-kernel launch behind the beam kernel (coherent_only)."""
    from tensorflowraytrace_amd import ops
    sc, out, src = full["sc"], full["out"], full["src"]
    order = ops.ray_order(src)
    p64 = order.long()
    sc2 = ops.Scene3DArgs(full["fv"], sc.catagory, mat_in=sc.mat_in, mat_out=sc.mat_out,
                          n_table=sc.n_table[:, p64].contiguous(), face_grad_mask=sc.face_grad_mask,
                          cluster_order=sc.cluster_order, coherent_rays=True)
    src_p = src[:, p64].contiguous()
    for only in (False, True):
        sc2.coherent_only = only
        raw = ops.trace3d(src_p, full["fv"], sc2, max_passes=PASSES, flags=full["flags"])
        assert raw["left_over"] == 0
        got = ops.restore_order(raw, order)
        assert np.array_equal(got["counts"], out["counts"]) and got["n_tests"] == out["n_tests"]
        for cls in ("finished", "active", "stopped", "dead", "unfinished"):
            assert torch.equal(got[cls + "_id"], out[cls + "_id"]), cls
            if cls != "unfinished":
                assert torch.equal(got[cls + "_face"], out[cls + "_face"]), cls
            assert torch.equal(got[cls].detach(), out[cls].detach()), cls


def test_full_size_sample_against_the_oracle(full):
    scene, out = full["scene"], full["out"]
    rng = np.random.default_rng(17)
    pick = np.sort(rng.choice(N_FULL, 256, replace=False))
    system, _, _ = oracle_util.lens_oracle(scene)
    ref = tracer.ray_trace(
        system, oracle_util.source_dict(scene["rays"][:, pick], scene["wavelength"][pick], np.float32),
        max_iterations=PASSES, inherit=("wavelength", "ray_id"),
        flags=dict(compile_dead_rays=True, compile_stopped_rays=True))
    checked = 0
    for cls in ("finished", "dead"):
        if not ref[cls] or ref[cls]["ray_id"].shape[0] == 0:
            continue
        want_ids = pick[ref[cls]["ray_id"].numpy().astype(np.int64)]
        ids = out[cls + "_id"].long().cpu().numpy()
        where = np.full(N_FULL, -1, dtype=np.int64)          # row of every source ray in the class
        where[ids] = np.arange(ids.shape[0])
        pos = where[want_ids]
        assert (pos >= 0).all(), f"{cls}: a sampled ray is in this class for the oracle only"
        assert np.array_equal(ids[pos], want_ids), f"{cls}: sampled rays classified differently"
        got = out[cls].detach()[:, torch.as_tensor(pos, device=out[cls].device)].cpu().double().numpy()
        want = oracle_util.block(ref[cls])
        rel = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        assert rel <= 1e-5, f"{cls}: {rel:.2e}"
        checked += want_ids.shape[0]
    assert checked >= 250


def _loss_and_grads(out, scene, params):
    fin = out["finished"]
    goal = torch.tensor(scene["goal"], dtype=torch.float64, device=fin.device)[out["finished_id"].long()]
    loss = ((fin[4].double() - goal[:, 0]) ** 2 + (fin[5].double() - goal[:, 1]) ** 2).sum()
    return loss, torch.autograd.grad(loss, params)


def test_full_size_shards_add_up(full):
    """Two contiguous halves of the ray set (what two ranks would trace) against the whole."""
    from tensorflowraytrace_amd import ops
    scene, out = full["scene"], full["out"]
    loss, (g_f, g_b) = _loss_and_grads(out, scene, full["params"])
    half = N_FULL // 2
    parts, fin_rows, fin_ids = [], [], []
    for lo, hi in ((0, half), (half, N_FULL)):
        sub = dict(scene)
        sub["rays"] = scene["rays"][:, lo:hi]
        sub["wavelength"] = scene["wavelength"][lo:hi]
        sub["goal"] = scene["goal"][lo:hi]
        src, fv, sc, params = _gpu_scene(sub, torch.float32, cluster="group")
        o = ops.trace3d(src, fv, sc, max_passes=PASSES, flags=full["flags"])
        parts.append(_loss_and_grads(o, sub, params))
        fin_rows.append(o["finished"])
        fin_ids.append(o["finished_id"].long() + lo)
    ids, rows = torch.cat(fin_ids), torch.cat(fin_rows, dim=1)
    a, b = torch.argsort(ids), torch.argsort(out["finished_id"].long())    # (classes are per-pass blocks)
    assert torch.equal(ids[a], out["finished_id"].long()[b])
    assert torch.equal(rows[:, a], out["finished"][:, b])                   # same rays, bit for bit
    total = parts[0][0] + parts[1][0]
    assert abs(float((total - loss).detach())) <= 1e-12 * abs(float(loss.detach()))
    for k, g in enumerate((g_f, g_b)):
        s = parts[0][1][k] + parts[1][1][k]
        assert float((s - g).abs().max()) <= 1e-11 * float(g.abs().max())


def test_full_size_permutation_invariance(full):
    from tensorflowraytrace_amd import ops
    scene, out = full["scene"], full["out"]
    perm = torch.randperm(N_FULL, generator=torch.Generator().manual_seed(3)).numpy()
    sub = dict(scene)
    sub["rays"] = scene["rays"][:, perm]
    sub["wavelength"] = scene["wavelength"][perm]
    src, fv, sc, _ = _gpu_scene(sub, torch.float32, cluster="group")
    o = ops.trace3d(src, fv, sc, max_passes=PASSES, flags=full["flags"])
    assert np.array_equal(o["counts"][:, :4], out["counts"][:, :4])
    perm_t = torch.as_tensor(perm, device=o["finished_id"].device)
    orig_ids = perm_t[o["finished_id"].long()]                  # source ids of the permuted run's rows
    order = torch.argsort(orig_ids)
    ref_order = torch.argsort(out["finished_id"].long())        # (classes are per-pass blocks)
    assert torch.equal(orig_ids[order], out["finished_id"].long()[ref_order])
    assert torch.equal(o["finished"].detach()[:, order], out["finished"].detach()[:, ref_order])
    assert torch.equal(o["finished_face"][order], out["finished_face"][ref_order])


# ------------------------------------------------------------------------------------------
# 2-D at cfg5b's size: 4,000,000 rays x (256 segments + 64 arcs), 4 passes

def test_full_size_2d_conservation_sample_and_shards():
    from tensorflowraytrace_amd import ops, _lib
    import test_gpu_trace2d as t2
    N, P = 4_000_000, 4
    sets, rays, wl = _scene_5b(N)
    scene, _, _ = t2._gpu_scene(sets, wl)
    flags = _lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_DEAD | _lib.COMPILE_STOPPED
    src = torch.tensor(rays, dtype=torch.float32, device="cuda:0")
    out = ops.trace2d(src, scene, max_passes=P, flags=flags)
    counts = out["counts"]
    n_in = N
    for p in range(P):
        assert int(counts[p, :4].sum()) == n_in
        n_in = int(counts[p, 0])
    assert out["n_tests"] == int(counts[:, :4].sum()) * 320
    assert out["unfinished"].shape[1] == n_in
    assert out["dead"].shape[1] == int(counts[:, 3].sum()) > 3_000_000     # most rays leave the scene

    # 256 sampled rays through the oracle: same class, same geometry (float32 state: 1e-5)
    pick = np.sort(np.random.default_rng(5).choice(N, 256, replace=False))
    ref = tracer.ray_trace(t2._oracle_system(sets), t2._src2(rays[:, pick], wl[pick], True),
                           max_iterations=P, inherit=("wavelength", "ray_id"),
                           flags=dict(compile_dead_rays=True, compile_stopped_rays=True))
    checked = 0
    for cls in ("finished", "dead"):
        r = ref[cls]
        if not r or r["ray_id"].shape[0] == 0:
            continue
        want_ids = pick[r["ray_id"].numpy().astype(np.int64)]
        ids = out[cls + "_id"].long().cpu().numpy()
        where = np.full(N, -1, dtype=np.int64)
        where[ids] = np.arange(ids.shape[0])
        pos = where[want_ids]
        assert (pos >= 0).all(), cls
        got = out[cls].detach()[:, torch.as_tensor(pos, device="cuda:0")].cpu().double().numpy()
        want = oracle_util.block(r, dim=2)
        assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) <= 1e-5, cls
        checked += want_ids.shape[0]
    assert checked >= 200

    # halves of the ray set reproduce the whole, ray for ray
    half = N // 2
    ids_parts, rows_parts = [], []
    for lo, hi in ((0, half), (half, N)):
        sc_h, _, _ = t2._gpu_scene(sets, wl[lo:hi])
        o = ops.trace2d(src[:, lo:hi].contiguous(), sc_h, max_passes=P, flags=flags)
        ids_parts.append(o["dead_id"].long() + lo)
        rows_parts.append(o["dead"].detach())
    ids, rows = torch.cat(ids_parts), torch.cat(rows_parts, dim=1)
    a, b = torch.argsort(ids), torch.argsort(out["dead_id"].long())
    assert torch.equal(ids[a], out["dead_id"].long()[b])
    assert torch.equal(rows[:, a], out["dead"].detach()[:, b])


def test_3d_trace_beyond_8192_ray_blocks_matches_its_halves():
    """From 8192 ray blocks (2.1M rays) on the per-pass offsets come from the grid scan
    (k_scan3d, a ticket across workgroups) instead of the single-block one: 2.3M rays in one trace
    against the same rays traced as two halves, which take the single-block path."""
    from tensorflowraytrace_amd import ops, _lib
    N = 2_300_000
    scene = scene_util.lens_scene(N, k_front=6, k_back=5)
    flags = _lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_DEAD | _lib.COMPILE_STOPPED
    src, fv, sc, _ = _gpu_scene(scene, torch.float32, cluster="group")
    out = ops.trace3d(src, fv, sc, max_passes=4, flags=flags)
    counts = out["counts"]
    n_in = N
    for p in range(4):
        assert int(counts[p, :4].sum()) == n_in
        n_in = int(counts[p, 0])
    half = N // 2
    parts = {c: ([], []) for c in ("finished", "dead", "active")}
    for lo, hi in ((0, half), (half, N)):
        sub = dict(scene)
        sub["rays"] = scene["rays"][:, lo:hi]
        sub["wavelength"] = scene["wavelength"][lo:hi]
        s2, f2, c2, _ = _gpu_scene(sub, torch.float32, cluster="group")
        o = ops.trace3d(s2, f2, c2, max_passes=4, flags=flags)
        for c in parts:
            parts[c][0].append(o[c + "_id"].long() + lo)
            parts[c][1].append(o[c].detach())
    for c in ("finished", "dead"):
        ids, rows = torch.cat(parts[c][0]), torch.cat(parts[c][1], dim=1)
        a, b = torch.argsort(ids), torch.argsort(out[c + "_id"].long())
        assert torch.equal(ids[a], out[c + "_id"].long()[b]), c
        assert torch.equal(rows[:, a], out[c].detach()[:, b]), c
    assert out["active"].shape[1] == sum(x.shape[1] for x in parts["active"][1])


# ------------------------------------------------------------------------------------------
# cfg2 / cfg3 at their stated size: 100,000 rays x 974 faces (two H(9) surfaces + target), 5 passes

def test_cfg2_cfg3_stated_size_sample_and_gradients():
    """BASELINE configs[1] and [2] at full size: conservation, 512 sampled rays against the oracle
    (float32 state, 1e-5), and the parameter gradients of the sampled rays alone against oracle
    autograd (the gradient is a sum over rays, so the sample's gradient is checked exactly and
    the full gradient through shard additivity)."""
    from tensorflowraytrace_amd import ops, _lib
    N, P = 100_000, 5
    scene = scene_util.lens_scene(N, k_front=9, k_back=9)
    flags = _lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_DEAD | _lib.COMPILE_STOPPED
    src, fv, sc, params = _gpu_scene(scene, torch.float32, cluster="group")
    assert fv.shape[0] == 974
    out = ops.trace3d(src, fv, sc, max_passes=P, flags=flags)
    counts = out["counts"]
    n_in = N
    for p in range(P):
        assert int(counts[p, :4].sum()) == n_in
        n_in = int(counts[p, 0])
    assert out["n_tests"] == int(counts[:, :4].sum()) * 974
    assert out["finished"].shape[1] > 90_000
    loss, g_full = _loss_and_grads(out, scene, params)

    pick = np.sort(np.random.default_rng(23).choice(N, 512, replace=False))
    sub = dict(scene)
    sub["rays"], sub["wavelength"], sub["goal"] = (scene["rays"][:, pick], scene["wavelength"][pick],
                                                   scene["goal"][pick])
    system, (q_f, q_b), _ = oracle_util.lens_oracle(sub)
    ref = tracer.ray_trace(system, oracle_util.source_dict(sub["rays"], sub["wavelength"], np.float32),
                           max_iterations=P, inherit=("wavelength", "ray_id"),
                           flags=dict(compile_dead_rays=True, compile_stopped_rays=True))
    rf = ref["finished"]
    want_ids = pick[rf["ray_id"].numpy().astype(np.int64)]
    ids = out["finished_id"].long().cpu().numpy()
    where = np.full(N, -1, dtype=np.int64)
    where[ids] = np.arange(ids.shape[0])
    pos = where[want_ids]
    assert (pos >= 0).all() and want_ids.shape[0] > 450
    got = out["finished"].detach()[:, torch.as_tensor(pos, device="cuda:0")].cpu().double().numpy()
    want = oracle_util.block(rf)
    assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) <= 1e-5

    # cfg3: gradients of the sampled rays alone, GPU vs oracle autograd (float32 state: 1e-5)
    s_src, s_fv, s_sc, s_params = _gpu_scene(sub, torch.float32, cluster="group")
    s_out = ops.trace3d(s_src, s_fv, s_sc, max_passes=P, flags=flags)
    _, g_sample = _loss_and_grads(s_out, sub, s_params)
    goal = torch.tensor(sub["goal"], dtype=torch.float64)[rf["ray_id"].long()]
    r_loss = ((rf["y_end"] - goal[:, 0]) ** 2 + (rf["z_end"] - goal[:, 1]) ** 2).sum()
    r_g = torch.autograd.grad(r_loss, [q_f, q_b])
    for g, r in zip(g_sample, r_g):
        rel = float((g.cpu() - r).abs().max() / r.abs().max())
        assert rel <= 1e-5, f"sample gradient rel err {rel:.2e}"

    # the full gradient is the sum over two shards (what ray sharding over GPUs relies on)
    half = N // 2
    g_sum = [torch.zeros_like(g) for g in g_full]
    for lo, hi in ((0, half), (half, N)):
        part = dict(scene)
        part["rays"], part["wavelength"], part["goal"] = (scene["rays"][:, lo:hi],
                                                          scene["wavelength"][lo:hi], scene["goal"][lo:hi])
        p_src, p_fv, p_sc, p_params = _gpu_scene(part, torch.float32, cluster="group")
        p_out = ops.trace3d(p_src, p_fv, p_sc, max_passes=P, flags=flags)
        _, g_part = _loss_and_grads(p_out, part, p_params)
        for acc, g in zip(g_sum, g_part):
            acc += g
    for s, g in zip(g_sum, g_full):
        assert float((s - g).abs().max()) <= 1e-11 * float(g.abs().max())


# ------------------------------------------------------------------------------------------
# cfg5a: hex lens H(24) x 2 + ParametricCylindricalGuide(64, 64) + target,
# 4,000,000 rays, 8 passes, through the public API; float32 vs float16 vs float64 ray state



@pytest.fixture(scope="module")
def cfg5a():
    eng, system, parts = _build_5a(torch.float32)
    eng.ray_trace(PASSES_5A)
    return dict(eng=eng, system=system, parts=parts, out=eng.last_trace)


def test_cfg5a_conservation_and_order(cfg5a):
    out, M = cfg5a["out"], int(cfg5a["system"]._merged_face_verts.shape[0])
    assert M == 2 * 3456 + 64 * 64 * 2 + 2           # two H(24) surfaces, the guide's wall + caps, target
    counts = out["counts"]
    n_in = N_5A
    for p in range(PASSES_5A):
        assert int(counts[p, :4].sum()) == n_in
        n_in = int(counts[p, 0])
    assert out["n_tests"] == int(counts[:, :4].sum()) * M
    assert out["finished"].shape[1] > 3_000_000      # the guide pipes most of the light to the target
    assert np.count_nonzero(counts[:, 1]) >= 3       # after different numbers of bounces
    for col, cls in ((1, "finished"), (3, "dead")):
        ids = out[cls + "_id"].long()
        base = 0
        for p in range(PASSES_5A):
            seg = ids[base:base + int(counts[p, col])]
            assert bool((seg[1:] > seg[:-1]).all()), (cls, p)
            base += int(counts[p, col])
        assert base == ids.numel()
    fin = out["finished"].detach()
    assert bool(torch.isfinite(fin).all())
    assert float((fin[5] - 6.9).abs().max()) < 1e-5  # finished rays end on the target plane z = 6.9


def test_cfg5a_hierarchy_equals_all_pairs(cfg5a):
    eng2, _, _ = _build_5a(torch.float32, accelerate="all-pairs")
    eng2.ray_trace(PASSES_5A)
    ref, out = eng2.last_trace, cfg5a["out"]
    assert np.array_equal(out["counts"], ref["counts"]) and out["n_tests"] == ref["n_tests"]
    for cls in ("finished", "active", "stopped", "dead"):
        assert torch.equal(out[cls + "_id"], ref[cls + "_id"]), cls
        assert torch.equal(out[cls + "_face"], ref[cls + "_face"]), cls
        assert torch.equal(out[cls].detach(), ref[cls].detach()), cls


def test_cfg5a_coherent_order_changes_nothing(cfg5a):
    """4M rays, 8 passes, lens + light guide through the public API with coherent=True: bundles
    widen with every bounce off the faceted wall (wavefronts are cut, some are left to the grouped
    kernel) -- the ray sets stay identical."""
    eng2, _, _ = _build_5a(torch.float32)
    eng2.coherent = True
    eng2.ray_trace(PASSES_5A)
    got, out = eng2.last_trace, cfg5a["out"]
    assert getattr(eng2, "_order_cache", None) is not None
    assert np.array_equal(got["counts"], out["counts"]) and got["n_tests"] == out["n_tests"]
    for cls in ("finished", "active", "stopped", "dead"):
        assert torch.equal(got[cls + "_id"], out[cls + "_id"]), cls
        assert torch.equal(got[cls + "_face"], out[cls + "_face"]), cls
        assert torch.equal(got[cls].detach(), out[cls].detach()), cls
    print(f"cfg5a coherent order: {got['left_over']} wavefront-passes left to the grouped kernel "
          f"of {PASSES_5A * N_5A // 64}")


def test_cfg5a_sample_against_the_oracle(cfg5a):
    out, system = cfg5a["out"], cfg5a["system"]
    pick = np.sort(np.random.default_rng(41).choice(N_5A, 256, replace=False))
    src = system._amalgamated_sources
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
    pick_t = torch.as_tensor(pick, device=src["x_start"].device)
    rays = np.stack([src[n][pick_t].cpu().numpy() for n in names])
    wl = src["wavelength"][pick_t].cpu().numpy()
    ref = tracer.ray_trace(_oracle_5a(cfg5a["parts"]), oracle_util.source_dict(rays, wl, np.float32),
                           max_iterations=PASSES_5A, inherit=("wavelength", "ray_id"),
                           flags=dict(compile_dead_rays=True, compile_stopped_rays=True))
    # Which sampled rays end differently on the device (float32 ray state: a child ray's start and
    # end are rounded to 2^-24 relative between passes) than in the float64 oracle?  Each one is
    # NAMED and must be explained: its oracle path has a hit within EDGE_MARGIN (barycentric
    # units) of a facet edge, where a 1e-7 shift of the ray selects the neighbouring facet --
    # another normal, an O(1) change of every later bounce.  A random ray has such a hit with
    # probability ~ 8 bounces x 3 edges x EDGE_MARGIN = 1 %; any other difference fails.
    EDGE_MARGIN = 5e-4
    differing = []
    checked = 0
    for cls in ("finished", "dead"):
        if not ref[cls] or ref[cls]["ray_id"].shape[0] == 0:
            continue
        local = ref[cls]["ray_id"].numpy().astype(np.int64)
        want_ids = pick[local]
        ids = out[cls + "_id"].long().cpu().numpy()
        where = np.full(N_5A, -1, dtype=np.int64)
        where[ids] = np.arange(ids.shape[0])
        pos = where[want_ids]
        same = pos >= 0
        differing += [(int(k), cls, "class") for k in local[~same]]
        got = out[cls].detach()[:, torch.as_tensor(pos[same], device="cuda:0")].cpu().double().numpy()
        want = oracle_util.block(ref[cls])[:, same]
        err = np.abs(got - want).max(axis=0) / max(1.0, np.abs(want).max())
        differing += [(int(k), cls, f"end point off by {e:.1e}")
                      for k, e in zip(local[same][err > 1e-5], err[err > 1e-5])]
        checked += int(same.sum() - (err > 1e-5).sum())
    # <= 1e-4 of the rays may be reclassified; of 256 sampled rays that is none
    # in expectation, and every one that is must be a grazing ray (below)
    assert len(differing) <= 2 and checked >= 254 - len(differing), differing
    if differing:
        system_o = _oracle_5a(cfg5a["parts"])
        m = system_o.merged
        ie, se, rse = system_o.eps
        for k, cls, what in differing:
            rays_k = oracle_util.source_dict(rays[:, k:k + 1], wl[k:k + 1], np.float32)
            history = {"active": [], "finished": [], "stopped": [], "dead": []}
            margin = np.inf
            for _ in range(PASSES_5A):
                hit = tracer.intersection_3d(
                    rays_k["x_start"], rays_k["y_start"], rays_k["z_start"], rays_k["x_end"],
                    rays_k["y_end"], rays_k["z_end"], m["xp"], m["yp"], m["zp"], m["x1"], m["y1"],
                    m["z1"], m["x2"], m["y2"], m["z2"], ie, se, rse)
                if bool(hit[3][0]):
                    u, v = float(hit[5][0]), float(hit[6][0])
                    margin = min(margin, u, v, 1.0 - u - v)
                rays_k, _ = tracer.single_pass(system_o, rays_k, history,
                                               inherit=("wavelength", "ray_id"))
                if not rays_k:
                    break
            print(f"cfg5a sample ray {pick[k]} ({cls}: {what}): nearest facet edge along the "
                  f"oracle path at {margin:.2e} barycentric units")
            assert margin < EDGE_MARGIN, \
                f"sampled ray {pick[k]} differs ({cls}: {what}) without a grazing hit: {margin:.2e}"


def test_cfg5a_shards_add_up(cfg5a):
    """Two ranks' worth of rays (ray_shard=(r, 2)) against the whole: same rays bit for bit, and
    the gradients w.r.t. the lens and the guide parameters add up."""
    def loss_and_grads(eng, parts):
        fin = eng.finished_rays
        loss = (fin["x_end"].double() ** 2 + fin["y_end"].double() ** 2).sum()
        params = [parts[0].parameters, parts[1].parameters, parts[2].parameters]
        return loss, torch.autograd.grad(loss, params)

    eng, parts, out = cfg5a["eng"], cfg5a["parts"], cfg5a["out"]
    loss, grads = loss_and_grads(eng, parts)
    total, g_sum, ids_parts, rows_parts = 0.0, None, [], []
    half = N_5A // 2
    for r in (0, 1):
        e, _, p = _build_5a(torch.float32, ray_shard=(r, 2))
        e.ray_trace(PASSES_5A)
        l, g = loss_and_grads(e, p)
        total = total + float(l.detach())
        g_sum = [x.clone() for x in g] if g_sum is None else [a + b for a, b in zip(g_sum, g)]
        ids_parts.append(e.last_trace["finished_id"].long() + r * half)
        rows_parts.append(e.last_trace["finished"].detach())
    ids, rows = torch.cat(ids_parts), torch.cat(rows_parts, dim=1)
    a, b = torch.argsort(ids), torch.argsort(out["finished_id"].long())
    assert torch.equal(ids[a], out["finished_id"].long()[b])
    assert torch.equal(rows[:, a], out["finished"].detach()[:, b])
    assert abs(total - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    for s, g in zip(g_sum, grads):
        assert float(g.abs().max()) > 0
        assert float((s - g).abs().max()) <= 1e-10 * float(g.abs().max())


def test_cfg5a_reduced_precision_ray_state_against_float64(cfg5a):
    """The fp32-vs-fp16 experiment of BASELINE configs[4]: accuracy of the reduced ray states against
    float64 state on the finished rays they share (fp16 is an accuracy experiment,
    not held to 1e-5)."""
    def ends(eng):
        ids = eng.last_trace["finished_id"].long()
        fin = eng.last_trace["finished"].detach()
        return ids, fin[3:5].double()

    e64, _, _ = _build_5a(torch.float64, compile_all=False)
    e64.ray_trace(PASSES_5A)
    ids64, xy64 = ends(e64)
    where = torch.full((N_5A,), -1, dtype=torch.int64, device=ids64.device)
    where[ids64] = torch.arange(ids64.shape[0], device=ids64.device)
    del e64

    def compare(ids, xy):
        pos = where[ids]
        common = pos >= 0
        err = (xy[:, common] - xy64[:, pos[common]]).abs().max(dim=0).values
        return int(common.sum()), err

    ids32, xy32 = ends(cfg5a["eng"])
    n32, err32 = compare(ids32, xy32)
    assert n32 >= ids64.shape[0] - 40 and ids32.shape[0] <= ids64.shape[0] + 40
    assert float(err32.median()) < 2e-7
    assert float((err32 > 2e-6).double().mean()) < 1e-3      # 99.9 % of the rays within 2e-6
    e16, _, _ = _build_5a(torch.float16, compile_all=False)
    e16.ray_trace(PASSES_5A)
    ids16, xy16 = ends(e16)
    n16, err16 = compare(ids16, xy16)
    assert n16 > 0.99 * ids64.shape[0]
    assert 1e-5 < float(err16.median()) < 2e-3               # ~3e-4: storage rounding of half floats
    assert float((err16 > 0.05).double().mean()) < 0.03      # ~1.3 % of the rays end elsewhere


# ------------------------------------------------------------------------------------------
# a scene beyond 100,000 faces: several L2s' worth of geometry, level 0 of the hierarchy 960 wide

def test_scene_with_122882_faces_hierarchy_equals_all_pairs_and_the_oracle():
    """200,000 rays x 122,882 faces (hex lens surfaces H(128) + H(64) + target), 3 passes: the
    hierarchy and the all-pairs filter give bit-identical rays, ids and faces; 128 sampled rays
    agree with the oracle (float32 state, 1e-5); the reverse sweep (scattered-atomics path:
    more than 32 face windows) gives finite, non-zero parameter gradients that two ray shards add
    up to."""
    from tensorflowraytrace_amd import ops, _lib
    N, P = 200_000, 3
    scene = scene_util.lens_scene(N, k_front=128, k_back=64)
    flags = _lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED | _lib.COMPILE_DEAD | _lib.COMPILE_STOPPED
    src, fv, sc, params = _gpu_scene(scene, torch.float32, cluster="group")
    assert fv.shape[0] == 6 * 128 ** 2 + 6 * 64 ** 2 + 2 == 122_882
    out = ops.trace3d(src, fv, sc, max_passes=P, flags=flags)
    src2, fv2, sc2, _ = _gpu_scene(scene, torch.float32, cluster=False)
    ref = ops.trace3d(src2, fv2, sc2, max_passes=P, flags=flags)
    assert np.array_equal(out["counts"], ref["counts"]) and out["n_tests"] == ref["n_tests"]
    for cls in ("finished", "active", "stopped", "dead"):
        assert torch.equal(out[cls + "_id"], ref[cls + "_id"]), cls
        assert torch.equal(out[cls + "_face"], ref[cls + "_face"]), cls
        assert torch.equal(out[cls].detach(), ref[cls].detach()), cls
    assert out["finished"].shape[1] > 150_000

    pick = np.sort(np.random.default_rng(9).choice(N, 128, replace=False))
    system, _, _ = oracle_util.lens_oracle(scene)
    oref = tracer.ray_trace(
        system, oracle_util.source_dict(scene["rays"][:, pick], scene["wavelength"][pick], np.float32),
        max_iterations=P, inherit=("wavelength", "ray_id"), chunk=32)
    rf = oref["finished"]
    want_ids = pick[rf["ray_id"].numpy().astype(np.int64)]
    ids = out["finished_id"].long().cpu().numpy()
    where = np.full(N, -1, dtype=np.int64)
    where[ids] = np.arange(ids.shape[0])
    pos = where[want_ids]
    assert (pos >= 0).all() and want_ids.shape[0] > 100
    got = out["finished"].detach()[:, torch.as_tensor(pos, device="cuda:0")].cpu().double().numpy()
    want = oracle_util.block(rf)
    assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) <= 1e-5

    loss, grads = _loss_and_grads(out, scene, params)
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    half = N // 2
    g_sum = [torch.zeros_like(g) for g in grads]
    for lo, hi in ((0, half), (half, N)):
        part = dict(scene)
        part["rays"], part["wavelength"], part["goal"] = (scene["rays"][:, lo:hi],
                                                          scene["wavelength"][lo:hi], scene["goal"][lo:hi])
        p_src, p_fv, p_sc, p_params = _gpu_scene(part, torch.float32, cluster="group")
        p_out = ops.trace3d(p_src, p_fv, p_sc, max_passes=P, flags=flags)
        for acc, g in zip(g_sum, _loss_and_grads(p_out, part, p_params)[1]):
            acc += g
    for s_, g in zip(g_sum, grads):
        assert float((s_ - g).abs().max()) <= 1e-10 * float(g.abs().max())


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float64, 1e-8)])
def test_full_size_coherent_gradients_against_oracle_autograd(full, dtype, tol):
    """optimizer.py:216-220 at cfg4's size on the COHERENT path (k_intersect_beam + the reverse
    sweep's per-wavefront face sums in LDS, several copies per sum folded by DPP): contiguous
    512-ray slices of the SORTED 1M-ray source against the whole 10,574-face scene.
    (i) three slices: parameter gradients against torch.autograd through the oracle;
    (ii) the 64 slices traced as one coherent run give the sum of the 64 slice gradients;
    (iii) the whole source in coherent order gives the natural-order run's gradients."""
    from tensorflowraytrace_amd import ops
    scene = full["scene"]
    src, fv, sc, (p_f, p_b) = _gpu_scene(scene, dtype, cluster="group")
    perm = ops.ray_order(src, fv)
    goal_all = torch.tensor(scene["goal"], dtype=torch.float64, device=src.device)
    slices = [perm[k * (N_FULL // 64):k * (N_FULL // 64) + 512] for k in range(64)]

    def run(index):
        """coherent trace of the rays `index` (already in sorted order) -> parameter gradients"""
        i64 = index.long()
        sc2 = ops.Scene3DArgs(fv, sc.catagory, mat_in=sc.mat_in, mat_out=sc.mat_out,
                              n_table=sc.n_table[:, i64].contiguous(), face_grad_mask=sc.face_grad_mask,
                              cluster_order=sc.cluster_order, coherent_rays=True)
        out = ops.trace3d(src[:, i64].contiguous(), fv, sc2, max_passes=PASSES)
        fin = out["finished"]
        goal = goal_all[i64][out["finished_id"].long()]
        loss = ((fin[4].double() - goal[:, 0]) ** 2 + (fin[5].double() - goal[:, 1]) ** 2).sum()
        return [g.clone() for g in torch.autograd.grad(loss, [p_f, p_b], retain_graph=True)], out

    # (i) against oracle autograd
    for k in (0, 29, 63):
        (g_f, g_b), out = run(slices[k])
        pick = slices[k].long().cpu().numpy()
        system, (q_f, q_b), _ = oracle_util.lens_oracle(scene)
        rays = scene["rays"][:, pick]
        ref = tracer.ray_trace(
            system, oracle_util.source_dict(rays, scene["wavelength"][pick],
                                            np.float32 if dtype == torch.float32 else np.float64),
            max_iterations=PASSES, inherit=("wavelength", "ray_id"), chunk=256)
        rf = ref["finished"]
        assert np.array_equal(out["finished_id"].cpu().numpy(), rf["ray_id"].numpy().astype(np.int32))
        rgoal = torch.tensor(scene["goal"][pick], dtype=torch.float64)[rf["ray_id"].long()]
        rerr = ((rf["y_end"] - rgoal[:, 0]) ** 2 + (rf["z_end"] - rgoal[:, 1]) ** 2).sum()
        r_f, r_b = torch.autograd.grad(rerr, [q_f, q_b])
        for g, r in ((g_f, r_f), (g_b, r_b)):
            rel = float((g.cpu() - r).abs().max() / r.abs().max())
            assert rel < tol, f"slice {k}: gradient rel err {rel:.2e}"
    # (ii) the slices as one coherent run (32,768 rays: full wavefronts, 64-ray bundles)
    total = [torch.zeros_like(p_f), torch.zeros_like(p_b)]
    for sl in slices:
        g, _ = run(sl)
        total[0] += g[0]
        total[1] += g[1]
    union, _ = run(torch.cat(slices))
    add_tol = 1e-11 if dtype == torch.float64 else 1e-6
    for a, b in zip(union, total):
        assert float((a - b).abs().max()) <= add_tol * float(b.abs().max())
    # (iii) the whole source, coherent against natural order
    whole, out = run(perm)
    assert out["left_over"] == 0
    nat_src, nat_fv, nat_sc, nat_p = _gpu_scene(scene, dtype, cluster="group")
    nat = ops.trace3d(nat_src, nat_fv, nat_sc, max_passes=PASSES)
    _, nat_g = _loss_and_grads(nat, scene, list(nat_p))
    for a, b in zip(whole, nat_g):
        assert float((a - b).abs().max()) <= (1e-10 if dtype == torch.float64 else 2e-6) * float(b.abs().max())


@pytest.fixture(scope="module")
def full_inplace(full):
    """cfg4's 1M-ray source sorted (ops.ray_order) and traced in place over the 3 passes
    (tfrt_scene3d.in_place: one launch, 64-ray wavefronts at this size), the sets restored to the
    reference's order by ops.restore_order."""
    from tensorflowraytrace_amd import ops
    from test_gpu_inplace import assert_in_place
    sc, src, fv = full["sc"], full["src"], full["fv"].detach()
    order = ops.ray_order(src)
    p64 = order.long()
    args = ops.Scene3DArgs(fv, sc.catagory, mat_in=sc.mat_in, mat_out=sc.mat_out,
                           n_table=sc.n_table[:, p64].contiguous(), face_grad_mask=sc.face_grad_mask,
                           cluster_order=sc.cluster_order, coherent_rays=True)
    args.coherent_only = args.in_place = True
    assert_in_place(args, fv, N_FULL, PASSES)
    raw = ops.trace3d(src[:, p64].contiguous(), fv, args, max_passes=PASSES, flags=full["flags"])
    assert raw["left_over"] == 0
    return ops.restore_order(raw, order)


def test_full_size_in_place_trace_equals_the_natural_order_trace(full, full_inplace):
    out, got = full["out"], full_inplace
    assert np.array_equal(got["counts"], out["counts"]) and got["n_tests"] == out["n_tests"]
    for cls in ("finished", "active", "stopped", "dead", "unfinished"):
        assert torch.equal(got[cls + "_id"], out[cls + "_id"]), cls
        if cls != "unfinished":
            assert torch.equal(got[cls + "_face"], out[cls + "_face"]), cls
        assert torch.equal(got[cls].detach(), out[cls].detach()), cls


def test_full_size_in_place_sample_against_the_oracle(full, full_inplace):
    """test_full_size_sample_against_the_oracle's 256 rays, read from the in-place trace."""
    test_full_size_sample_against_the_oracle(dict(full, out=full_inplace))


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.float64, 1e-10)])
def test_cfg4_in_place_fused_step_against_the_generic_step(dtype, tol):
    """The step bench.py times, on its own cfg4 scene (bench.build_scene: 1M rays, 10,574 faces,
    3 passes) and with its optimiser: once the engine traces the sorted source in place, the fused
    step runs the in-place goal chain with 64-ray wavefronts (k_backward_chain recomputing the
    finished rows from the tape).  Its gradient, read from the parameter change, against the
    generic natural-order step (ops.trace3d + torch.autograd, the path the 512-ray oracle slices
    of test_full_size_coherent_gradients_against_oracle_autograd pin) at the same parameters.
    (The clip is opened so that the parameter change is the gradient; the warm-up steps take
    lr_scale = 0 so the lens stays where the second system is built, the measured one a larger
    scale so that the change stands well above the parameters' rounding.)"""
    import bench
    import tfrt.optimizer as optimizer
    eng, system, params = bench.build_scene(N_FULL, K_FRONT, K_BACK, dtype)
    opt = optimizer.SGD_Optimizer(eng, params, bench.make_error_function(), trace_depth=3,
                                  learning_rate=1e-6, grad_clip=1e9, fused="auto", graph="auto",
                                  speculative=False)
    opt.suppress_warnings = True
    for _ in range(10):
        opt.single_step(None, lr_scale=0.0)
        fs = opt._fused_step
        if fs is not None and fs.in_place and fs.folded_backward:
            break
    assert fs.in_place and fs.folded_backward
    used = [p.detach().clone() for p in params]
    lr_scale = 100.0
    opt.single_step(None, lr_scale=lr_scale)
    assert fs.in_place and fs.folded_backward
    assert fs.capture_error is None, fs.capture_error
    scale = opt.sgd_learning_rate * opt.learning_rate * lr_scale
    got = [(u - p.detach()) / scale for u, p in zip(used, params)]

    eng2, system2, params2 = bench.build_scene(N_FULL, K_FRONT, K_BACK, dtype, coherent=False)
    with torch.no_grad():
        for p2, u in zip(params2, used):
            p2.copy_(u)
    opt2 = optimizer.SGD_Optimizer(eng2, params2, bench.make_error_function(), trace_depth=3,
                                   learning_rate=1e-6, grad_clip=1e9, fused=False, speculative=False)
    opt2.suppress_warnings = True
    want, _, n_terms = opt2.raw_gradient()
    assert getattr(eng2, "_order_cache", None) is None          # (natural order)
    assert int(float(opt.last_error_terms)) == int(n_terms) > 1_500_000
    for g, w in zip(got, want):
        assert float(w.abs().max()) > 0
        rel = float((g - w).abs().max() / w.abs().max())
        assert rel <= tol, f"gradient rel err {rel:.2e}"
