"""Host side of the 2-D RowwiseError route: tfrt_trace2d_rows and tfrt_trace2d_backward_rows refuse
bad arguments before any launch (every call here would fault on the device if it got that far:
the pointers are host memory).  No GPU needed."""
import ctypes

import pytest

from tensorflowraytrace_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(1 << 16)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _finished(ptr, capacity=10):
    fin = _lib.RayOut()
    fin.rays, fin.capacity = ptr, capacity
    return fin


def test_rows_2d_rejects_bad_arguments_before_any_launch(lib, mem):
    _, ptr = mem
    fin = _finished(ptr)

    def call(n_rays=10, P=3, dtype=_lib.F64, finished=ctypes.byref(fin), rows=ptr,
             rows_stride=10, row_face=ptr, counts=ptr, workspace=ptr, ws_bytes=1 << 16, src=ptr,
             src_stride=10):
        return lib.tfrt_trace2d_rows(src, src_stride, n_rays, P, dtype, finished, rows,
                                     rows_stride, row_face, counts, workspace, ws_bytes, None)

    assert call(n_rays=-1) == -1 and call(P=-1) == -1
    assert call(counts=None) == -1 and call(workspace=None) == -1
    assert call(finished=None) == -1
    assert call(src=None) == -1 and call(src_stride=9) == -1
    assert call(rows=None) == -1 and call(row_face=None) == -1
    assert call(rows_stride=9) == -1 and call(rows_stride=-1) == -1
    none = _lib.RayOut()
    assert call(finished=ctypes.byref(none)) == -1
    empty = _finished(ptr, capacity=0)
    assert call(finished=ctypes.byref(empty)) == -1
    assert call(dtype=7) == -4
    for dtype in (_lib.F32, _lib.F64, _lib.F16):
        # the forward's tape does not fit: refused before the launch
        assert call(dtype=dtype, ws_bytes=16) == -2


def test_backward_rows_2d_rejects_bad_arguments_before_any_launch(lib, mem):
    _, ptr = mem
    fin = _finished(ptr)
    sc = _lib.Scene2D()
    sc.n_segments, sc.n_arcs = 0, 0
    pend = _lib.GoalPending()

    def call(n_rays=10, scene=ctypes.byref(sc), P=3, dtype=_lib.F64, finished=ctypes.byref(fin),
             terms=ptr, n_terms=2, err_stride=1, err_ray_stride=2, grad_rows=ptr, grad_stride=10,
             error_out=ptr, goal_ws_bytes=1 << 16, pending=ctypes.byref(pend), counts=ptr,
             workspace=ptr, ws_bytes=1 << 16, src=ptr, src_stride=10):
        return lib.tfrt_trace2d_backward_rows(
            src, src_stride, n_rays, scene, 1.0, P, dtype, finished, terms, n_terms, err_stride,
            err_ray_stride, grad_rows, grad_stride, error_out, None, ptr, goal_ws_bytes, pending,
            None, None, counts, workspace, ws_bytes, None)

    bad = _lib.Scene2D()
    bad.n_segments = -1
    assert call(scene=ctypes.byref(bad)) == -1 and call(scene=None) == -1
    assert call(n_rays=-1) == -1 and call(P=-1) == -1
    assert call(counts=None) == -1 and call(workspace=None) == -1
    assert call(finished=None) == -1
    assert call(src=None) == -1 and call(src_stride=9) == -1
    assert call(grad_stride=9) == -1 and call(grad_stride=-1) == -1
    assert call(terms=None) == -1 and call(n_terms=0) == -1
    assert call(err_stride=-1) == -1 and call(err_ray_stride=-1) == -1
    assert call(error_out=None) == -1 and call(pending=None) == -1
    assert call(goal_ws_bytes=0) == -1
    none = _lib.RayOut()
    assert call(finished=ctypes.byref(none)) == -1
    empty = _finished(ptr, capacity=0)
    assert call(finished=ctypes.byref(empty)) == -1
    assert call(dtype=7) == -4
    for dtype in (_lib.F32, _lib.F64, _lib.F16):
        assert call(dtype=dtype, ws_bytes=16) == -2


def test_rows_2d_with_no_rays_needs_no_buffers_but_the_tape(lib, mem):
    """n_rays = 0: nothing to write, so rows, row_face and the source may be NULL -- but the call
    still refuses a workspace the forward's tape does not fit."""
    _, ptr = mem
    fin = _lib.RayOut()
    assert lib.tfrt_trace2d_rows(None, 0, 0, 3, _lib.F64, ctypes.byref(fin), None, 0, None, ptr,
                                 ptr, 16, None) == -2
