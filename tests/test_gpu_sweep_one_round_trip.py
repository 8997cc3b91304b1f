"""
k_backward_chain_goal_inplace with all of a pass's loads asked for together (ray, hit parameter,
goal columns, face, indices, mask byte -- each under the condition the lane reads it on) and
adjoint3d's single pair of cross products: eager fused steps on the k = 3 lens of
tests/test_gpu_chain_goal_inplace.py, over what decides which loads a lane issues and how the
goal is addressed --

  rays      4,161 (a last wavefront of one ray) and 8,192
  depth     1, 2, 3 (only the third pass reaches the target through the lens)
  aperture  0.8, and 1.6: rays that miss the lens and finish on the target in the FIRST pass
            (finished lanes below the wavefront's top pass, faces whose mask byte is zero)
  columns   one, two and three goal columns, the third one a START coordinate (its seed enters
            the adjoint through g_s)
  goal      (fields, N) table, and (N, fields) rows -- the layout a row-wise goal of a
            device-made source arrives in; the static source of this lens always takes the table,
            so the rows are handed to the step's launches by transposing what _goal_rows returns

float64 ray state: error, term count and ray counts equal those of the per-pass step
(``eng.in_place = False``) exactly; parameter gradients within 1e-8 (the reverse sweep's stated
tolerance, csrc/trace_math.h) of the per-pass step and of torch.autograd through the oracle.
float32 ray state: error and gradients against the oracle at 1e-5 (DESIGN section 6,
tests/test_gpu_fused_step.py).  Every case asserts that the step ran in place with the goal folded
into the sweep, i.e. that the kernel under test is the one that ran.  The oracle's result is
computed once per (rays, depth, aperture, columns, rounding) and shared.
"""
import numpy as np
import pytest
import torch

from oracle import tracer
from test_gpu_chain_goal_inplace import SLICE, _case, _oracle, _step
from test_gpu_engine import _oracle_for

pytestmark = pytest.mark.gpu

_GEO = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")

# goal columns: fields and the goal row of a ray from its object point
COLUMNS = {
    1: (("z_end",), lambda src: -src["object_coords"][:, 2]),
    2: (("y_end", "z_end"), lambda src: -src["object_coords"][:, 1:]),
    3: (("y_end", "z_end", "y_start"),
        lambda src: torch.stack([-src["object_coords"][:, 1], -src["object_coords"][:, 2],
                                 0.5 * src["object_coords"][:, 1]], dim=1)),
}

# rays, depth, aperture, goal columns, goal as (N, fields) rows
CASES_F64 = [
    (8192, 3, 0.8, 2, False),
    (4161, 3, 1.6, 2, True),
    (4161, 3, 0.8, 1, True),
    (8192, 3, 1.6, 3, False),
    (8192, 2, 1.6, 3, True),
    (4161, 2, 0.8, 1, False),
    (8192, 1, 0.8, 2, True),
    (4161, 1, 1.6, 3, False),
]
CASES_F32 = [
    (8192, 3, 0.8, 2, False),
    (4161, 3, 1.6, 3, True),
    (8192, 2, 1.6, 1, True),
]


def _id(case):
    n, depth, aperture, cols, rows = case
    return f"{n}_rays-depth_{depth}-aperture_{aperture}-{cols}_col-{'rows' if rows else 'table'}"


@pytest.fixture
def goal_as_rows(monkeypatch):
    """Hands every fused step's goal to its launches as (N, fields) rows."""
    import tensorflowraytrace_amd.fused_step as fs
    plain = fs.FusedStep._goal_rows

    def rows(self, erf, src, perm):
        table, by_ray = plain(self, erf, src, perm)
        if by_ray:
            return table, True
        kept = self.__dict__.get("_rows_of_table")
        if kept is None or kept[0] is not table:
            kept = self._rows_of_table = (table, table.t().contiguous())
        return kept[1], True
    monkeypatch.setattr(fs.FusedStep, "_goal_rows", rows)


def _make(case, in_place=True, ray_dtype=None):
    import tfrt.optimizer as optimizer
    n, depth, aperture, cols, _ = case
    c = _case(n, depth, aperture=aperture)
    fields, goal = COLUMNS[cols]
    c["opt"].error_function = optimizer.GoalError(fields, goal)
    if not in_place:
        c["eng"].in_place = False
    if ray_dtype is not None:
        c["eng"].ray_dtype = ray_dtype
    return c


_oracle_results = {}


def _oracle_of(c, case, used, float32_source=False):
    """(error sum, terms, gradients) by autograd through the oracle; the gradients are handed out
    as they were computed and never written to."""
    n, depth, aperture, cols, _ = case
    key = (n, depth, aperture, cols, float32_source)
    hit = _oracle_results.get(key)
    if hit is not None and all(torch.equal(u, v) for u, v in zip(hit[0], used)):
        return hit[1]
    if cols == 2 and not float32_source:
        res = _oracle(c, used, depth, False)
    else:
        fields, goal = COLUMNS[cols]
        q = [u.clone().requires_grad_(True) for u in used]
        osys, src = _oracle_for(c["system"], c["lens"], c["target"], c["source"], q)
        if float32_source:                      # (the trace starts from the float32 block)
            for k in _GEO:
                src[k] = src[k].float().double()
        total = [torch.zeros_like(u) for u in used]
        err_sum, terms = 0.0, 0
        for a in range(0, src["x_start"].shape[0], SLICE):
            part = {k: v[a:a + SLICE] for k, v in src.items()}
            ref = tracer.ray_trace(osys, part, max_iterations=depth,
                                   inherit=("wavelength", "object_coords"))
            rf = ref.get("finished")
            if not rf or rf["y_end"].shape[0] == 0:
                continue
            out = torch.stack([rf[f] for f in fields], 1)
            rerr = (out - goal(rf).reshape(out.shape)) ** 2
            if rerr.requires_grad:
                for t, g in zip(total, torch.autograd.grad(rerr.sum(), q, retain_graph=True,
                                                           allow_unused=True)):
                    if g is not None:
                        t += g
            err_sum += float(rerr.sum().detach())
            terms += rerr.numel()
        res = (err_sum, terms, total)
    _oracle_results[key] = ([u.clone() for u in used], res)
    return res


def _close(got, want, tol, what):
    """max |got - want| <= tol max |want| (a gradient that is zero must be met exactly)."""
    for k, (g, w) in enumerate(zip(got, want)):
        diff, ref = float((g - w).abs().max()), float(w.abs().max())
        print(f"{what}, parameter {k}: max |d| {diff:.3e}, max |ref| {ref:.3e}")
        assert diff <= tol * ref, f"{what}, parameter {k}: {diff:.3e} against {ref:.3e}"


def _ran_the_kernel(c):
    fs = c["opt"]._fused_step
    assert fs is not None and fs.graph_replays == 0
    assert fs.in_place and fs.folded_backward
    return fs


def _check_f64(case):
    tol = 1e-8
    a, b = _make(case), _make(case, in_place=False)
    err_a, terms_a, counts_a, used_a, g_a = _step(a)
    err_b, terms_b, counts_b, used_b, g_b = _step(b)
    _ran_the_kernel(a)
    assert not b["opt"]._fused_step.in_place
    for u, v in zip(used_a, used_b):
        assert torch.equal(u, v)                   # the two steps started from the same parameters
    print(f"{_id(case)}: error {err_a!r} / {err_b!r}, terms {terms_a} / {terms_b}")
    assert np.array_equal(np.float64(err_a), np.float64(err_b), equal_nan=True)
    assert terms_a == terms_b
    assert np.array_equal(counts_a, counts_b)
    _close(g_a, g_b, tol, "in place against per pass")
    err_o, terms_o, g_o = _oracle_of(a, case, used_a)
    assert terms_a == terms_o
    if terms_o:
        assert abs(err_a - err_o / terms_o) <= tol * (err_o / terms_o)
    _close(g_a, g_o, tol, "in place against oracle autograd")


def _check_f32(case):
    tol = 1e-5
    a = _make(case, ray_dtype=torch.float32)
    err_a, terms_a, _, used_a, g_a = _step(a)
    _ran_the_kernel(a)
    err_o, terms_o, g_o = _oracle_of(a, case, used_a, float32_source=True)
    print(f"{_id(case)}: error {err_a!r} / {err_o / max(terms_o, 1)!r}, terms {terms_a} / {terms_o}")
    assert terms_a == terms_o
    if terms_o:
        assert abs(err_a - err_o / terms_o) <= tol * (err_o / terms_o)
    _close(g_a, g_o, tol, "in place, float32 state, against oracle autograd")


@pytest.mark.parametrize("case", [c for c in CASES_F64 if not c[4]], ids=_id)
def test_float64_goal_table(case):
    _check_f64(case)


@pytest.mark.parametrize("case", [c for c in CASES_F64 if c[4]], ids=_id)
def test_float64_goal_rows(case, goal_as_rows):
    _check_f64(case)


@pytest.mark.parametrize("case", [c for c in CASES_F32 if not c[4]], ids=_id)
def test_float32_goal_table(case):
    _check_f32(case)


@pytest.mark.parametrize("case", [c for c in CASES_F32 if c[4]], ids=_id)
def test_float32_goal_rows(case, goal_as_rows):
    _check_f32(case)
