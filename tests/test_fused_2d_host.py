"""Host side of the fused 2-D optimiser step: the C ABI of tfrt_trace2d_backward_goal refuses bad
arguments before any launch, GoalError resolves its rows for a 2-D engine, and manual 2-D boundary
fields reach the merged geometry through boundaries.tap.  No GPU needed."""
import ctypes

import pytest
import torch

from tensorflowraytrace_amd import _lib
from tensorflowraytrace_amd.fused_step import GoalError


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_backward_goal_2d_rejects_bad_arguments_before_any_launch(lib):
    sc = _lib.Scene2D()
    sc.n_segments, sc.n_arcs = 0, 0
    fin, pend = _lib.RayOut(), _lib.GoalPending()
    dummy = ctypes.create_string_buffer(1 << 16)
    ptr = ctypes.cast(dummy, ctypes.c_void_p)
    fin.rays, fin.capacity = ptr, 10

    def call(n_rays=10, scene=ctypes.byref(sc), P=3, dtype=_lib.F64, finished=ctypes.byref(fin),
             fields=(3,), n_fields=None, goal=ptr, goal_stride=10, goal_ray_stride=1,
             error_out=ptr, goal_ws_bytes=1 << 16, pending=ctypes.byref(pend), counts=ptr,
             workspace=ptr, ws_bytes=1 << 16, src=ptr, src_stride=10):
        f = (ctypes.c_int32 * 4)(*(list(fields) + [0] * 4)[:4]) if fields is not None else None
        return lib.tfrt_trace2d_backward_goal(
            src, src_stride, n_rays, scene, 1.0, P, dtype, finished, f,
            len(fields or (3,)) if n_fields is None else n_fields, goal, goal_stride, goal_ray_stride,
            error_out, None, ptr, goal_ws_bytes, pending, None, None, counts, workspace, ws_bytes,
            None)

    bad = _lib.Scene2D()
    bad.n_segments = -1
    assert call(scene=ctypes.byref(bad)) == -1
    assert call(scene=None) == -1
    assert call(n_rays=-1) == -1 and call(P=-1) == -1
    assert call(n_fields=0) == -1 and call(fields=(0, 1, 2, 3, 3)) == -1     # n_fields 1..4
    assert call(fields=(4,)) == -1 and call(fields=(-1,)) == -1              # rows 0..3
    assert call(fields=None) == -1
    assert call(goal_stride=-1) == -1 and call(goal_ray_stride=-1) == -1
    assert call(goal_ws_bytes=0) == -1
    assert call(pending=None) == -1 and call(error_out=None) == -1
    assert call(counts=None) == -1 and call(workspace=None) == -1
    assert call(finished=None) == -1
    assert call(goal=None) == -1 and call(src=None) == -1 and call(src_stride=5) == -1
    # a forward compiled without finished rays: no block to compare with the goal
    none = _lib.RayOut()
    assert call(finished=ctypes.byref(none)) == -1
    empty = _lib.RayOut()
    empty.rays, empty.capacity = ptr, 0
    assert call(finished=ctypes.byref(empty)) == -1
    assert call(dtype=7) == -4
    # the forward's tape does not fit: refused before the launch
    assert call(ws_bytes=16) == -2


def test_backward_goal_2d_workspace_bytes(lib):
    assert lib.tfrt_trace2d_backward_goal_workspace_bytes(-1) == 0
    assert lib.tfrt_trace2d_backward_goal_workspace_bytes(0) >= 8
    assert lib.tfrt_trace2d_backward_goal_workspace_bytes(64) >= 8
    assert lib.tfrt_trace2d_backward_goal_workspace_bytes(65) >= 16
    assert lib.tfrt_trace2d_backward_goal_workspace_bytes(1_000_000) >= 15_625 * 8


def test_goal_error_rows_for_a_2d_engine():
    assert GoalError(("y_end",), torch.zeros(3)).rows_for(2) == [3]
    assert GoalError(("y_end",), torch.zeros(3)).rows_for(3) == [4]
    e = GoalError(("x_start", "y_start", "x_end", "y_end"), torch.zeros(3, 4))
    assert e.rows_for(2) == [0, 1, 2, 3]
    assert e.rows == [0, 1, 3, 4]                       # (the 3-D rows are unchanged)


@pytest.mark.parametrize("fields", [("z_end",), ("y_end", "z_start")])
def test_goal_error_rejects_z_fields_on_a_2d_engine(fields):
    e = GoalError(fields, torch.zeros(3, len(fields)))
    e.rows_for(3)
    z = [f for f in fields if f.startswith("z")][0]
    with pytest.raises(ValueError, match=z):
        e.rows_for(2)

    class Engine2D:
        dimension = 2
    with pytest.raises(ValueError, match=z):
        e(Engine2D())


def test_manual_2d_fields_are_read_through_taps_inside_collect_taps():
    from tensorflowraytrace_amd import boundaries
    p = torch.tensor([5.0], dtype=torch.float64, requires_grad=True)
    arc = boundaries.ManualArcBoundary()
    arc["x_center"] = p
    arc["radius"] = p
    arc["y_center"] = torch.zeros(1, dtype=torch.float64)
    assert arc["x_center"] is p                         # outside a block: the field itself
    with boundaries.collect_taps() as log:
        a, b, c = arc["x_center"], arc["radius"], arc["y_center"]
    assert a is not p and b is not p and c is arc._fields["y_center"]
    assert [t is a or t is b for t in log[id(p)]] == [True, True]
    (a * 2 + b * 3).backward()
    assert float(p.grad) == 5.0                         # one parameter feeding two fields
    sig = arc.field_signature()
    assert ("x_center", id(p), (1,)) in sig
    arc["radius"] = torch.tensor([4.0], dtype=torch.float64)
    assert arc.field_signature() != sig
