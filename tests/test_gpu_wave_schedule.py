"""
The wavefront schedule of the in-place goal step (tfrt_scene3d.wave_schedule: k_trace_inplace and
k_backward_chain_goal_inplace take the groups of 64 rays in the order a permutation lists, the
expensive ones first; csrc/wave_schedule.h, k_wave_schedule).

The schedule is a hint about time, so the tests are about everything else staying put: one eager
fused step under any permutation gives the error bit for bit, the term count, the ray counts and
every ray-set field of the step without one, and its gradients within the reverse sweep's
tolerance of that step and of torch.autograd through the oracle; the schedule the step builds
itself is the header's rule applied to the count rows the trace left; a captured graph reads the
buffer by address; what is no permutation is refused.

Lens, steps, oracle and measure are tests/test_gpu_chain_goal_inplace.py's (hex mesh k = 3, eager
fused steps, float64 state at 1e-8); the float32-state case is held to 1e-5, the tolerance
tests/test_gpu_fullsize.py uses for float32 state.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_gpu_chain_goal_inplace import _case, _close, _oracle, _step

pytestmark = pytest.mark.gpu

DEPTH = 3
TOL32 = 1e-5
# rays, source aperture, ray state
SHAPES = {
    "8192_rays_128_groups": (8192, 0.8, torch.float64),
    "4161_rays_last_group_of_one_ray": (4161, 0.8, torch.float64),
    "aperture_wider_than_the_lens": (8192, 1.6, torch.float64),
    "float32_state": (8192, 0.8, torch.float32),
}
SCHEDULES = ("identity", "reversed", "random", "auto")
CLASSES = ("finished", "active", "stopped", "dead")


def _groups(n_rays):
    return (n_rays + 63) // 64


def _permutation(kind, n_rays):
    G = _groups(n_rays)
    if kind == "identity":
        p = torch.arange(G)
    elif kind == "reversed":
        p = torch.arange(G - 1, -1, -1)
    else:
        p = torch.randperm(G, generator=torch.Generator().manual_seed(11))
    return p.to(torch.int32).cuda()


def _sets(eng):
    out = {}
    for cls in CLASSES:
        rays = getattr(eng, cls + "_rays")
        out[cls] = {k: rays[k].detach().cpu().clone() for k in rays.keys()}
    return out


def _run(shape, schedule):
    """One eager fused step of `shape` under `schedule` (False, "auto" or a kind of permutation)."""
    n_rays, aperture, dtype = SHAPES[shape]
    c = _case(n_rays, DEPTH, aperture=aperture)
    c["eng"].ray_dtype = dtype
    c["eng"].wave_schedule = (schedule if schedule in (False, "auto")
                              else _permutation(schedule, n_rays))
    err, terms, counts, used, grads = _step(c)
    fs = c["opt"]._fused_step
    assert fs is not None and fs.graph_replays == 0
    assert fs.in_place and fs.folded_backward     # the kernels under test are the ones that ran
    return dict(c=c, fs=fs, err=err, terms=terms, counts=counts, used=used, grads=grads,
                sets=_sets(c["eng"]))


_BASE = {}


def _baseline(shape):
    """The step without a schedule and the oracle's gradients, once per shape, never changed."""
    if shape not in _BASE:
        r = _run(shape, False)
        assert r["fs"]._state.sched is None
        err_o, terms_o, g_o = _oracle(r["c"], r["used"], DEPTH, False)
        _BASE[shape] = (r, (err_o, terms_o, g_o))
    return _BASE[shape]


def _within(got, want, tol, what):
    for k, (g, w) in enumerate(zip(got, want)):
        diff, ref = float((g - w).abs().max()), float(w.abs().max())
        print(f"{what}, parameter {k}: max |d| {diff:.3e}, max |ref| {ref:.3e}")
        assert diff <= tol * ref, f"{what}, parameter {k}: {diff:.3e} against {ref:.3e}"


def _same_results(r, base, what):
    print(f"{what}: error {r['err']!r} / {base['err']!r}, terms {r['terms']} / {base['terms']}")
    for u, v in zip(r["used"], base["used"]):
        assert torch.equal(u, v)                   # the two steps started from the same parameters
    assert np.array_equal(np.float64(r["err"]), np.float64(base["err"]), equal_nan=True)
    assert r["terms"] == base["terms"]
    assert np.array_equal(r["counts"], base["counts"])
    for cls in CLASSES:
        assert r["sets"][cls].keys() == base["sets"][cls].keys(), cls
        for k, v in base["sets"][cls].items():
            assert torch.equal(r["sets"][cls][k], v), f"{what}: {cls}[{k}]"
    assert base["terms"] > 0 and len(base["sets"]["finished"]) > 0


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_same_results_under_any_schedule(shape, schedule, monkeypatch):
    """Error (bitwise), term count, ray counts and every ray-set field equal the step's without a
    schedule; gradients within the tolerance of that step and of the oracle's autograd."""
    from tensorflowraytrace_amd.fused_step import FusedStep
    # ("auto" leaves launches alone that are resident all at once: these are, so ask for every size)
    monkeypatch.setattr(FusedStep, "schedule_min_waves", 0)
    base, (err_o, terms_o, g_o) = _baseline(shape)
    r = _run(shape, schedule)
    st = r["fs"]._state
    if schedule == "auto":
        assert st.sched is not None and st.sched_key is not None   # the step made one and ran with it
        assert st.sched.numel() == _groups(SHAPES[shape][0])
    _same_results(r, base, f"{shape}, {schedule}")
    assert base["terms"] == terms_o
    if SHAPES[shape][2] == torch.float64:
        assert abs(base["err"] - err_o / terms_o) <= 1e-8 * (err_o / terms_o)
        _close(r["grads"], base["grads"], f"{schedule} against no schedule")
        _close(r["grads"], g_o, f"{schedule} against oracle autograd")
    else:
        _within(r["grads"], base["grads"], TOL32, f"{schedule} against no schedule")
        _within(r["grads"], g_o, TOL32, f"{schedule} against oracle autograd")


def _header_constants():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "tensorflowraytrace_amd", "csrc", "wave_schedule.h")
    text = open(path).read()

    def value(name):
        m = re.search(r"(?:constexpr \w+ |#define TFRT_)" + name + r" =? ?(\d+)u?(?: << (\d+))?;?\n",
                      text)                                                      # ("1u << 24")
        return int(m.group(1)) << int(m.group(2) or 0)
    return {n: value(n) for n in ("WAVE_SCHED_CLASSES", "WAVE_COST_PASS", "WAVE_COST_FACE",
                                  "WAVE_COST_MAX_PASSES", "WAVE_COST_MAX_FACES")}


def test_the_built_schedule_is_the_headers_rule_on_the_count_rows(monkeypatch):
    """After an "auto" step of the wide-aperture case: a permutation of the groups, classes never
    rising along it, indices ascending inside a class, equal to a numpy restatement of
    wave_schedule.h applied to the count rows read back (the warm-up steps move nothing: the rows
    of the last trace are those the schedule was made from)."""
    from tensorflowraytrace_amd import ops
    from tensorflowraytrace_amd.fused_step import FusedStep
    monkeypatch.setattr(FusedStep, "schedule_min_waves", 0)
    r = _run("aperture_wider_than_the_lens", "auto")
    st = r["fs"]._state
    G, P = _groups(st.N), st.P
    sched = st.sched.cpu().numpy()
    rows = ops.wave_rows(st.N, st.M, P, st.block.dtype, st.ws).cpu().numpy().view(np.uint32)
    assert rows.shape[0] == P + 2
    W = rows.shape[1]
    per = -(-W // G)
    assert per in (1, 2) and -(-W // per) == G
    k = _header_constants()
    pad = np.zeros((P + 2, G * per), dtype=np.uint64)
    pad[:, :W] = rows
    passes = (pad[:P] != 0).sum(0).reshape(G, per).max(1)
    faces = np.minimum(pad[P + 1].reshape(G, per), k["WAVE_COST_MAX_FACES"]).sum(1)
    faces = np.minimum(faces, k["WAVE_COST_MAX_FACES"])
    cost = (k["WAVE_COST_PASS"] * np.minimum(passes, k["WAVE_COST_MAX_PASSES"])
            + k["WAVE_COST_FACE"] * faces).astype(np.uint64)
    span = int(cost.max() - cost.min()) + 1
    cls = ((cost - cost.min()) * np.uint64(k["WAVE_SCHED_CLASSES"]) // np.uint64(span)).astype(int)
    print(f"{G} groups, {W} wavefronts, passes {np.bincount(passes.astype(int))}, "
          f"classes {np.bincount(cls, minlength=k['WAVE_SCHED_CLASSES'])}")
    assert len(set(cls.tolist())) > 1 and passes.min() == 1 and passes.max() == P   # the case separates
    assert np.array_equal(np.sort(sched), np.arange(G))
    along = cls[sched]
    assert np.all(along[:-1] >= along[1:])
    assert np.all((along[:-1] != along[1:]) | (sched[:-1] < sched[1:]))
    assert np.array_equal(sched, np.argsort(-cls, kind="stable"))


def test_a_captured_step_reads_the_schedule_by_address():
    """graph="auto": once the step replays, another valid permutation written into the same buffer
    gives the same error, counts and ray sets on the next replay."""
    n_rays = 8192
    c = _case(n_rays, DEPTH)
    opt, eng = c["opt"], c["eng"]
    opt.graph = "auto"
    buf = _permutation("identity", n_rays)
    eng.wave_schedule = buf

    def replay():
        before = opt._fused_step.graph_replays
        err = float(opt.single_step(None, lr_scale=0.0))
        assert opt._fused_step.graph_replays == before + 1
        counts = np.stack([np.asarray(x) for x in eng.last_trace["counts"]])
        return err, int(float(opt.last_error_terms)), counts, _sets(eng)

    for _ in range(16):
        opt.single_step(None, lr_scale=0.0)
        if opt._fused_step.graph_replays > 0:
            break
    fs = opt._fused_step
    assert fs.graph_replays > 0 and fs.capture_error is None
    assert fs.in_place and fs.folded_backward
    err_a, terms_a, counts_a, sets_a = replay()
    buf.copy_(_permutation("random", n_rays))
    torch.cuda.synchronize()
    err_b, terms_b, counts_b, sets_b = replay()
    assert terms_a > 0
    assert np.array_equal(np.float64(err_a), np.float64(err_b)) and terms_a == terms_b
    assert np.array_equal(counts_a, counts_b)
    for cls in CLASSES:
        assert sets_a[cls].keys() == sets_b[cls].keys()
        for k, v in sets_a[cls].items():
            assert torch.equal(sets_b[cls][k], v), f"{cls}[{k}]"


def test_what_is_no_permutation_is_refused():
    """A tensor of the wrong length or dtype, with a duplicate or with an entry out of range raises
    before the trace is launched; tfrt_trace3d_wave_schedule without an output or with a short
    workspace returns its error code."""
    from tensorflowraytrace_amd import _lib
    n_rays = 8192
    G = _groups(n_rays)
    c = _case(n_rays, DEPTH)
    opt, eng = c["opt"], c["eng"]
    eng.wave_schedule = False
    for _ in range(8):
        opt.single_step(None, lr_scale=0.0)
    fs = opt._fused_step
    assert fs.in_place and fs.folded_backward
    good = _permutation("identity", n_rays)
    duplicate, out_of_range, negative = good.clone(), good.clone(), good.clone()
    duplicate[5] = 6
    out_of_range[G - 1] = G
    negative[0] = -1
    bad = {"short": good[:-1].contiguous(), "long": torch.cat([good, good[:1]]),
           "int64": good.long(), "duplicate": duplicate, "out of range": out_of_range,
           "negative": negative, "on the host": good.cpu()}
    steps = fs.steps
    for what, t in bad.items():
        eng.wave_schedule = t
        with pytest.raises((_lib.TfrtError, RuntimeError)):
            opt.single_step(None, lr_scale=0.0)
        print(f"{what}: refused")
    eng.wave_schedule = "no"
    with pytest.raises(ValueError):
        opt.single_step(None, lr_scale=0.0)
    eng.wave_schedule = good                        # (and the step goes on with a valid one)
    opt.single_step(None, lr_scale=0.0)
    assert fs.steps > steps and fs.in_place

    st = fs._state
    L = _lib.lib()
    out = torch.empty(G, dtype=torch.int32, device="cuda")
    ws, dt = ctypes.c_void_p(st.ws.data_ptr()), st.dt
    o = ctypes.c_void_p(out.data_ptr())
    assert L.tfrt_trace3d_wave_schedule(st.N, st.M, st.P, dt, ws, st.wsb, None, None) == -1
    assert L.tfrt_trace3d_wave_schedule(st.N, st.M, st.P, dt, None, st.wsb, o, None) == -1
    assert L.tfrt_trace3d_wave_schedule(32, st.M, st.P, dt, ws, st.wsb, o, None) == -1
    assert L.tfrt_trace3d_wave_schedule(st.N, st.M, 0, dt, ws, st.wsb, o, None) == -1
    assert L.tfrt_trace3d_wave_schedule(st.N, st.M, st.P, dt, ws, st.wsb - 1, o, None) == -2
    assert L.tfrt_trace3d_wave_rows(st.N, st.M, st.P, dt, ws, st.wsb - 1, None, None) == -2
    assert L.tfrt_trace3d_wave_rows(st.N, st.M, st.P, dt, None, st.wsb, None, None) == -1
