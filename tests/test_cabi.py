"""
The C-ABI library loads without a GPU and exports every symbol include/tfrt_hip.h declares;
host-only entry points (version, strerror, workspace sizing, argument validation) behave.
No kernel is launched here.
"""
import ctypes
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tfrt_hip.h")


@pytest.fixture(scope="module")
def lib():
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    return _lib.lib()


def _declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tfrt_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from tensorflowraytrace_amd import _lib
    declared = _declared_symbols()
    assert len(declared) >= 18
    assert sorted(_lib.SIGNATURES) == declared, "ctypes binding and header disagree"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (tfrt_[a-z0-9_]+)", out))
    assert set(declared) <= exported, set(declared) - exported


def test_header_compiles_as_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "tfrt_hip.h"\nint main(void){return TFRT_COUNTS_LEN(3) == 32 ? 0 : 1;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                    "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_version_and_strerror(lib):
    from tensorflowraytrace_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tfrt_hip.h")).read()
    declared = int(re.search(r"#define TFRT_VERSION (\d+)", header).group(1))
    assert lib.tfrt_version() == declared == _lib.ABI_VERSION == 107
    assert lib.tfrt_strerror(0) == b"ok"
    for code in (-1, -2, -3, -4, -99):
        assert len(lib.tfrt_strerror(code)) > 0


def test_workspace_sizes(lib):
    a = lib.tfrt_trace3d_workspace_bytes(1000, 100, 3, 0)
    b = lib.tfrt_trace3d_workspace_bytes(2000, 100, 3, 0)
    c = lib.tfrt_trace3d_workspace_bytes(1000, 100, 6, 0)
    d = lib.tfrt_trace3d_workspace_bytes(1000, 100, 3, 1)
    assert 0 < a < b and a < c and a < d
    assert lib.tfrt_trace3d_workspace_bytes(-1, 100, 3, 0) == 0
    assert lib.tfrt_trace2d_workspace_bytes(1000, 10, 10, 3, 0) > 0
    assert lib.tfrt_intersect3d_workspace_bytes(1000, 100) > 0
    # 1M rays x 10k faces x 5 passes stays far below HBM capacity
    assert lib.tfrt_trace3d_workspace_bytes(1_000_000, 10_574, 5, 0) < 2 * 1024 ** 3


def test_bad_arguments_are_rejected_before_any_launch(lib):
    from tensorflowraytrace_amd import _lib
    sc = _lib.Scene3D()
    sc.n_faces = -1
    code = lib.tfrt_trace3d_forward(None, 0, 10, ctypes.byref(sc), 1.0, 0.0, 3, 0, 3, None, None,
                                    None, None, None, None, None, None, 0, None)
    assert code == -1
    assert lib.tfrt_build_faces_forward(None, -1, None, 5, None, None, None) == -1
    assert lib.tfrt_snell3d(-5, *([None] * 9), 1.0, None, None) == -1
    assert lib.tfrt_segment_intersection(None, 0, -1, 0, None, 0, 0.0, 0.0, 0.0, None, None, None,
                                         None, None, None, None) == -1
    # round 4 entry points: the folded reverse sweep, the orders, the source programs
    ok = _lib.Scene3D()
    ok.n_faces = 0
    fin, pend = _lib.RayOut(), _lib.GoalPending()
    fields = (ctypes.c_int32 * 6)(4, 5, 0, 0, 0, 0)
    dummy = ctypes.create_string_buffer(1 << 16)
    ptr = ctypes.cast(dummy, ctypes.c_void_p)

    def backward_goal(n_fields=2, goal_ws_bytes=1 << 16, pending=ctypes.byref(pend), stride=10):
        return lib.tfrt_trace3d_backward_goal(
            None, 0, 10, ctypes.byref(ok), 1.0, 0.0, 3, 0, ctypes.byref(fin), fields, n_fields, ptr,
            stride, 1, ptr, None, ptr, goal_ws_bytes, pending, None, 0, None, 0, None, 0, ptr, None,
            ptr, ptr, 1 << 16, None)
    assert backward_goal(n_fields=0) == -1 and backward_goal(n_fields=7) == -1
    assert backward_goal(goal_ws_bytes=0) == -1 and backward_goal(pending=None) == -1
    assert backward_goal(stride=-1) == -1
    assert backward_goal() == -1                     # (no finished-ray block: rays is NULL)
    assert lib.tfrt_trace3d_backward_goal_workspace_bytes(1_000_000) >= 15_625 * 8
    assert lib.tfrt_trace3d_backward_goal_workspace_bytes(-1) == 0
    assert lib.tfrt_ray_order(None, 0, -1, 0, None, 0, None, None, None, None, 0, None) == -1
    assert lib.tfrt_ray_order_workspace_bytes(1_000_000) > 0
    assert lib.tfrt_source3d_order(None, 0, 10, None, 0, None, None, None, None, 0, None) == -1
    # a program tfrt_source3d_generate refuses is refused by tfrt_source3d_order too (same check):
    # unknown kind, a random distribution without an epoch counter, a table without storage, an
    # input that has neither one sample nor one per ray
    def program(kind=_lib.SRC_APERTURE, a_kind=_lib.PTS_CIRCLE, a_count=10, epoch=ptr, table=None):
        sp = _lib.Source3DProgram()
        sp.kind, sp.n_rays = kind, 10
        for pg, knd, cnt in ((sp.a, a_kind, a_count), (sp.b, _lib.PTS_CIRCLE, 10)):
            pg.kind, pg.count, pg.epoch, pg.table = knd, cnt, epoch, table
        return sp

    for bad in (program(kind=7), program(epoch=None), program(a_kind=_lib.PTS_TABLE),
                program(a_kind=9), program(a_count=3)):
        args = (ctypes.byref(bad), 0, 10, None, 0, None, ptr, None, ptr, 1 << 16, None)
        assert lib.tfrt_source3d_order(*args) == -1
        assert lib.tfrt_source3d_generate(ctypes.byref(bad), None, 0, 10, 0, ptr, 10, None, 0,
                                          None) == -1
    assert lib.tfrt_epoch_advance(None, 9, None) == -1


def test_face_entry_points_reject_bad_arguments_before_any_launch(lib):
    """tfrt_build_faces_backward, tfrt_param_faces_backward, tfrt_param_faces_backward_multi,
    tfrt_param_faces_forward and tfrt_param_faces_forward_multi: every refusal, and the empty
    calls that return 0 without a launch."""
    from tensorflowraytrace_amd import _lib
    dummy = ctypes.create_string_buffer(1 << 12)
    ptr = ctypes.cast(dummy, ctypes.c_void_p)

    def build(g_fv=ptr, g_n=ptr, fv=ptr, faces=ptr, F=4, V=4, start=ptr, lst=ptr, out=ptr):
        return lib.tfrt_build_faces_backward(g_fv, g_n, fv, faces, None, F, V, start, lst, out, None)

    def param(g_fv=ptr, g_n=ptr, fv=ptr, faces=ptr, vec=ptr, F=4, V=4, start=ptr, lst=ptr, out=ptr):
        return lib.tfrt_param_faces_backward(g_fv, g_n, fv, faces, None, vec, F, V, start, lst, out,
                                             None)

    for call in (build, param):
        assert call(F=-1) == -1 and call(V=-1) == -1
        assert call(g_fv=None, g_n=None) == -1               # no upstream at all
        assert call(fv=None) == -1                           # grad_norm needs the face block
        assert call(start=None) == -1 and call(lst=None) == -1
        assert call(faces=None) == -1 and call(out=None) == -1
        assert call(F=0) == 0 and call(F=0, g_fv=None, g_n=None, out=None) == 0
    assert param(vec=None) == -1
    assert lib.tfrt_param_faces_forward(None, ptr, ptr, 4, ptr, 4, ptr, None, None) == -1
    assert lib.tfrt_param_faces_forward(ptr, ptr, ptr, 0, ptr, 4, ptr, None, None) == -1
    assert lib.tfrt_param_faces_forward(None, None, None, 0, None, 0, None, None, None) == 0

    def grad_surface(**kw):
        d = _lib.FaceSurfaceGrad()
        for k in ("grad_face_verts", "grad_norm", "face_verts", "vectors", "corner_start",
                  "corner_list", "grad_parameters"):
            setattr(d, k, ptr)
        d.n_vertices = 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def backward_multi(*surfaces, n=None):
        arr = (_lib.FaceSurfaceGrad * max(len(surfaces), 1))(*surfaces)
        return lib.tfrt_param_faces_backward_multi(arr, len(surfaces) if n is None else n, None)

    assert backward_multi(n=-1) == -1 and backward_multi(n=_lib.MAX_SURFACES + 1) == -1
    assert lib.tfrt_param_faces_backward_multi(None, 1, None) == -1
    assert lib.tfrt_param_faces_backward_multi(None, 0, None) == 0
    for bad in (dict(n_vertices=-1), dict(grad_face_verts=None, grad_norm=None),
                dict(face_verts=None), dict(corner_start=None), dict(corner_list=None),
                dict(vectors=None), dict(grad_parameters=None)):
        assert backward_multi(grad_surface(n_vertices=0), grad_surface(**bad)) == -1, bad
    assert backward_multi(grad_surface(n_vertices=0), grad_surface(n_vertices=0)) == 0

    def surface(**kw):
        d = _lib.FaceSurface()
        for k in ("zero_points", "vectors", "parameters", "faces", "face_verts"):
            setattr(d, k, ptr)
        d.n_vertices, d.n_faces = 4, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def forward_multi(*surfaces, n=None):
        arr = (_lib.FaceSurface * max(len(surfaces), 1))(*surfaces)
        return lib.tfrt_param_faces_forward_multi(arr, len(surfaces) if n is None else n, None)

    assert forward_multi(n=-1) == -1 and forward_multi(n=_lib.MAX_SURFACES + 1) == -1
    assert lib.tfrt_param_faces_forward_multi(None, 1, None) == -1
    for bad in (dict(n_faces=-1), dict(n_vertices=-1), dict(face_verts=None), dict(faces=None),
                dict(parameters=None), dict(n_vertices=0)):
        assert forward_multi(surface(n_faces=0), surface(**bad)) == -1, bad
    assert forward_multi(surface(n_faces=0), surface(n_faces=0, face_verts=None)) == 0


def test_ops_refuse_cpu_tensors():
    import torch
    from tensorflowraytrace_amd import ops, _lib
    with pytest.raises(_lib.TfrtError):
        ops.build_faces(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(_lib.TfrtError):
        ops.intersect3d(torch.zeros(6, 4), torch.zeros(2, 9, dtype=torch.float64))


_BAD_DTYPE = 7      # no TFRT_F32 / TFRT_F64 / TFRT_F16


def _unknown_dtype_calls(lib):
    """(entry, code, call): every entry that dispatches on the state dtype and gets to that
    dispatch without a HIP call, with arguments that pass its validation and a dtype code outside
    the three.  tfrt_intersect3d is not here: it launches its set-up kernels first."""
    from tensorflowraytrace_amd import _lib
    dummy = ctypes.create_string_buffer(1 << 16)
    ptr = ctypes.cast(dummy, ctypes.c_void_p)
    big = 1 << 40
    sc3 = _lib.Scene3D()
    sc3.n_faces = 0
    sc2 = _lib.Scene2D()
    fin = _lib.RayOut()
    fin.rays, fin.capacity = ptr, 10
    pend = _lib.GoalPending()
    fields = (ctypes.c_int32 * 6)(0, 1, 0, 0, 0, 0)
    sp3 = _lib.Source3DProgram()
    sp3.kind, sp3.n_rays = _lib.SRC_APERTURE, 10
    for pg in (sp3.a, sp3.b):
        pg.kind, pg.count, pg.epoch = _lib.PTS_CIRCLE, 10, ptr
    sp2 = _lib.Source2DProgram()
    sp2.kind, sp2.n_rays = _lib.SRC_POINT, 10
    sp2.b.kind, sp2.b.count, sp2.b.epoch, sp2.b.lo, sp2.b.hi = _lib.SMP_UNIFORM_ANGLE, 10, ptr, 0.0, 1.0
    # (the generators return 0 for no rays once the program is accepted: the refusals below are
    # the dtype's)
    assert lib.tfrt_source3d_generate(ctypes.byref(sp3), None, 0, 0, 0, ptr, 10, None, 0, None) == 0
    assert lib.tfrt_source2d_generate(ctypes.byref(sp2), None, 0, 0, 0, ptr, 10, None, 0, None) == 0
    d = _BAD_DTYPE
    return [
        ("tfrt_trace3d_forward", -4, lambda: lib.tfrt_trace3d_forward(
            ptr, 10, 10, ctypes.byref(sc3), 1.0, 0.0, 3, d, 0, None, None, None, None, None, None,
            ptr, ptr, big, None)),
        ("tfrt_trace3d_compact", -4, lambda: lib.tfrt_trace3d_compact(
            ptr, 64, 64, 0.0, 1, d, 0, None, None, None, None, None, None, ptr, 0, None, ptr, big,
            None)),
        ("tfrt_trace3d_backward", -4, lambda: lib.tfrt_trace3d_backward(
            ptr, 10, 10, ctypes.byref(sc3), 1.0, 0.0, 3, d, None, 0, None, 0, None, 0, None, 0, ptr,
            None, ptr, ptr, big, None)),
        ("tfrt_trace3d_backward_goal", -4, lambda: lib.tfrt_trace3d_backward_goal(
            ptr, 10, 10, ctypes.byref(sc3), 1.0, 0.0, 3, d, ctypes.byref(fin), fields, 2, ptr, 10,
            1, ptr, None, ptr, 1 << 16, ctypes.byref(pend), None, 0, None, 0, None, 0, ptr, None,
            ptr, ptr, big, None)),
        ("tfrt_segment_intersection", -4, lambda: lib.tfrt_segment_intersection(
            ptr, 10, 10, d, ptr, 1, 0.0, 0.0, 0.0, ptr, ptr, ptr, ptr, ptr, ptr, None)),
        ("tfrt_arc_intersection", -4, lambda: lib.tfrt_arc_intersection(
            ptr, 10, 10, d, ptr, 1, 0.0, 0.0, 0.0, ptr, ptr, ptr, ptr, ptr, ptr, None)),
        ("tfrt_trace2d_forward", -4, lambda: lib.tfrt_trace2d_forward(
            ptr, 10, 10, ctypes.byref(sc2), 1.0, 0.0, 3, d, 0, None, None, None, None, None, None,
            ptr, ptr, big, None)),
        ("tfrt_trace2d_backward", -4, lambda: lib.tfrt_trace2d_backward(
            ptr, 10, 10, ctypes.byref(sc2), 1.0, 0.0, 3, d, None, 0, None, 0, None, 0, None, 0,
            None, None, None, ptr, ptr, big, None)),
        ("tfrt_trace2d_backward_goal", -4, lambda: lib.tfrt_trace2d_backward_goal(
            ptr, 10, 10, ctypes.byref(sc2), 1.0, 3, d, ctypes.byref(fin), fields, 2, ptr, 10, 1,
            ptr, None, ptr, 1 << 16, ctypes.byref(pend), None, None, ptr, ptr, big, None)),
        ("tfrt_trace2d_rows", -4, lambda: lib.tfrt_trace2d_rows(
            ptr, 10, 10, 3, d, ctypes.byref(fin), ptr, 10, ptr, ptr, ptr, big, None)),
        ("tfrt_trace2d_backward_rows", -4, lambda: lib.tfrt_trace2d_backward_rows(
            ptr, 10, 10, ctypes.byref(sc2), 1.0, 3, d, ctypes.byref(fin), ptr, 1, 10, 1, None, 0,
            ptr, None, ptr, 1 << 16, ctypes.byref(pend), None, None, ptr, ptr, big, None)),
        ("tfrt_ray_order", -1, lambda: lib.tfrt_ray_order(
            ptr, 10, 10, d, None, 0, None, ptr, None, ptr, big, None)),
        ("tfrt_permute_rays", -1, lambda: lib.tfrt_permute_rays(
            ptr, 10, 10, d, ptr, ptr, 10, ptr, big, None)),
        ("tfrt_source3d_generate", -1, lambda: lib.tfrt_source3d_generate(
            ctypes.byref(sp3), None, 0, 10, d, ptr, 10, None, 0, None)),
        ("tfrt_source2d_generate", -1, lambda: lib.tfrt_source2d_generate(
            ctypes.byref(sp2), None, 0, 10, d, ptr, 10, None, 0, None)),
        ("tfrt_goal_error3d", -1, lambda: lib.tfrt_goal_error3d(
            ptr, 10, ptr, d, ptr, 3, fields, 2, ptr, 10, 1, ptr, ptr, None, 0, None, ptr, big,
            None)),
        ("tfrt_goal_error3d_deferred", -1, lambda: lib.tfrt_goal_error3d_deferred(
            ptr, 10, ptr, d, ptr, 3, fields, 2, ptr, 10, 1, ptr, ptr, None, 0, None, ptr, big,
            ctypes.byref(pend), None)),
        ("tfrt_density_error", -1, lambda: lib.tfrt_density_error(
            ptr, 10, 10, d, None, 0, 1, ptr, 4, 4, 0.0, 1.0, 0.1, 0.0, 1.0, 0.1, 1.0, ptr, 10, ptr,
            ptr, 0, ptr, big, None)),
    ]


def test_unknown_state_dtype_is_refused_with_each_entry_s_own_code(lib):
    calls = _unknown_dtype_calls(lib)
    assert {name: call() for name, _, call in calls} == {name: code for name, code, _ in calls}


_WS_RAYS = (0, 1, 63, 64, 65, 4095, 4096, 32768, 1_048_832)
_WS_FACES = (0, 63, 64, 10_574)        # 2-D: split over segments and arcs, M // 2 and the rest
_WS_PASSES = (0, 1, 5)
_WS_DTYPES = (0, 1, 2)
# itertools.product order of the axes above, recorded from the build before the workspace views
_TRACE3D_BYTES = (
    9728, 9728, 9728, 11520, 11520, 11520, 17920, 17920, 17920, 21504, 21504, 21504, 23296,
    23296, 23296, 29696, 29696, 29696, 21504, 21504, 21504, 23296, 23296, 23296, 29696, 29696,
    29696, 2356736, 2356736, 2356736, 2358528, 2358528, 2358528, 2364928, 2364928, 2364928,
    9728, 9728, 9728, 11520, 11520, 11520, 17920, 17920, 17920, 21504, 21504, 21504, 23296,
    23296, 23296, 29696, 29696, 29696, 21504, 21504, 21504, 23296, 23296, 23296, 29696, 29696,
    29696, 2356736, 2356736, 2356736, 2358528, 2358528, 2358528, 2364928, 2364928, 2364928,
    22016, 22016, 22016, 25344, 26880, 24576, 63232, 70912, 59392, 33792, 33792, 33792, 37120,
    38656, 36352, 75008, 82688, 71168, 33792, 33792, 33792, 37120, 38656, 36352, 75008, 82688,
    71168, 2400000, 2400000, 2400000, 2403328, 2404864, 2402560, 2441216, 2448896, 2437376,
    22016, 22016, 22016, 25344, 26880, 24576, 63488, 71168, 59648, 33792, 33792, 33792, 37120,
    38656, 36352, 75264, 82944, 71424, 33792, 33792, 33792, 37120, 38656, 36352, 75264, 82944,
    71424, 2400256, 2400256, 2400256, 2403584, 2405120, 2402816, 2441728, 2449408, 2437888,
    23552, 23552, 23552, 28416, 29952, 27648, 66816, 74496, 62976, 35328, 35328, 35328, 40192,
    41728, 39424, 78592, 86272, 74752, 35328, 35328, 35328, 40192, 41728, 39424, 78592, 86272,
    74752, 2402048, 2402048, 2402048, 2406912, 2408448, 2406144, 2445312, 2452992, 2441472,
    895488, 895488, 895488, 1096192, 1194496, 1047040, 3156224, 3647744, 2910464, 907264,
    907264, 907264, 1107968, 1206272, 1058816, 3168000, 3659520, 2922240, 907264, 907264,
    907264, 1107968, 1206272, 1058816, 3168000, 3659520, 2922240, 5257216, 5257216, 5257216,
    5457920, 5556224, 5408768, 7517952, 8009472, 7272192, 895488, 895488, 895488, 1096192,
    1194496, 1047040, 3156480, 3648000, 2910720, 907264, 907264, 907264, 1107968, 1206272,
    1058816, 3168256, 3659776, 2922496, 907264, 907264, 907264, 1107968, 1206272, 1058816,
    3168256, 3659776, 2922496, 5257472, 5257472, 5257472, 5458176, 5556480, 5409024, 7518464,
    8009984, 7272704, 7126272, 7126272, 7126272, 8731904, 9518336, 8338688, 25214208, 29146368,
    23248128, 7138048, 7138048, 7138048, 8743680, 9530112, 8350464, 25225984, 29158144,
    23259904, 7138048, 7138048, 7138048, 8743680, 9530112, 8350464, 25225984, 29158144,
    23259904, 25594880, 25594880, 25594880, 27200512, 27986944, 26807296, 43682816, 47614976,
    41716736, 227932160, 227932160, 227932160, 279324928, 304496896, 266738944, 806892800,
    932752640, 743962880, 227943936, 227943936, 227943936, 279336704, 304508672, 266750720,
    806904576, 932764416, 743974656, 227943936, 227943936, 227943936, 279336704, 304508672,
    266750720, 806904576, 932764416, 743974656, 268036864, 268036864, 268036864, 319429632,
    344601600, 306843648, 846997504, 972857344, 784067584,
)

_TRACE2D_BYTES = (
    2048, 2048, 2048, 4096, 4096, 4096, 4096, 4096, 4096, 9216, 9216, 9216, 11264, 11264, 11264,
    11264, 11264, 11264, 9216, 9216, 9216, 11264, 11264, 11264, 11264, 11264, 11264, 1170688,
    1170688, 1170688, 1172736, 1172736, 1172736, 1172736, 1172736, 1172736, 2048, 2048, 2048,
    4096, 4096, 4096, 4096, 4096, 4096, 9216, 9216, 9216, 11264, 11264, 11264, 11264, 11264,
    11264, 9216, 9216, 9216, 11264, 11264, 11264, 11264, 11264, 11264, 1170688, 1170688,
    1170688, 1172736, 1172736, 1172736, 1172736, 1172736, 1172736, 5888, 5888, 5888, 9216,
    10240, 8704, 21760, 26880, 19200, 13056, 13056, 13056, 16384, 17408, 15872, 28928, 34048,
    26368, 13056, 13056, 13056, 16384, 17408, 15872, 28928, 34048, 26368, 1174528, 1174528,
    1174528, 1177856, 1178880, 1177344, 1190400, 1195520, 1187840, 5888, 5888, 5888, 9216,
    10240, 8704, 21760, 26880, 19200, 13056, 13056, 13056, 16384, 17408, 15872, 28928, 34048,
    26368, 13056, 13056, 13056, 16384, 17408, 15872, 28928, 34048, 26368, 1174528, 1174528,
    1174528, 1177856, 1178880, 1177344, 1190400, 1195520, 1187840, 6144, 6144, 6144, 11264,
    12288, 10752, 23808, 28928, 21248, 13312, 13312, 13312, 18432, 19456, 17920, 30976, 36096,
    28416, 13312, 13312, 13312, 18432, 19456, 17920, 30976, 36096, 28416, 1174784, 1174784,
    1174784, 1179904, 1180928, 1179392, 1192448, 1197568, 1189888, 264448, 264448, 264448,
    465152, 530688, 432384, 1267968, 1595648, 1104128, 271616, 271616, 271616, 472320, 537856,
    439552, 1275136, 1602816, 1111296, 271616, 271616, 271616, 472320, 537856, 439552, 1275136,
    1602816, 1111296, 1433088, 1433088, 1433088, 1633792, 1699328, 1601024, 2436608, 2764288,
    2272768, 264448, 264448, 264448, 465152, 530688, 432384, 1267968, 1595648, 1104128, 271616,
    271616, 271616, 472320, 537856, 439552, 1275136, 1602816, 1111296, 271616, 271616, 271616,
    472320, 537856, 439552, 1275136, 1602816, 1111296, 1433088, 1433088, 1433088, 1633792,
    1699328, 1601024, 2436608, 2764288, 2272768, 2106624, 2106624, 2106624, 3712256, 4236544,
    3450112, 10134784, 12756224, 8824064, 2113792, 2113792, 2113792, 3719424, 4243712, 3457280,
    10141952, 12763392, 8831232, 2113792, 2113792, 2113792, 3719424, 4243712, 3457280, 10141952,
    12763392, 8831232, 3275264, 3275264, 3275264, 4880896, 5405184, 4618752, 11303424, 13924864,
    9992704, 67389184, 67389184, 67389184, 118781952, 135563264, 110391296, 324353024,
    408259584, 282399744, 67396352, 67396352, 67396352, 118789120, 135570432, 110398464,
    324360192, 408266752, 282406912, 67396352, 67396352, 67396352, 118789120, 135570432,
    110398464, 324360192, 408266752, 282406912, 68557824, 68557824, 68557824, 119950592,
    136731904, 111559936, 325521664, 409428224, 283568384,
)

_INTERSECT3D_BYTES = (
    1536, 2304, 2304, 170752, 1536, 2304, 2304, 170752, 3584, 4352, 4352, 203776, 3584, 4352,
    4352, 204032, 4352, 5120, 5120, 205056, 180992, 181760, 181760, 2364928, 180992, 181760,
    181760, 2365184, 1442560, 1443328, 1443328, 17733376, 46149376, 46150144, 46150144, 84076288,
)

_PERMUTE_BYTES = (
    256, 256, 256, 256, 256, 256, 2048, 4096, 1024, 2048, 4096, 1024, 2304, 4352, 1280, 131072,
    262144, 65536, 131072, 262144, 65536, 1048576, 2097152, 524288, 33562624, 67125248, 16781312,
)


def test_workspace_byte_counts_are_the_recorded_ones(lib):
    shapes = list(itertools.product(_WS_RAYS, _WS_FACES, _WS_PASSES, _WS_DTYPES))
    assert len(shapes) == len(_TRACE3D_BYTES) == len(_TRACE2D_BYTES) == 324
    assert tuple(lib.tfrt_trace3d_workspace_bytes(n, m, p, d) for n, m, p, d in shapes) == _TRACE3D_BYTES
    assert tuple(lib.tfrt_trace2d_workspace_bytes(n, m // 2, m - m // 2, p, d)
                 for n, m, p, d in shapes) == _TRACE2D_BYTES
    assert tuple(lib.tfrt_intersect3d_workspace_bytes(n, m)
                 for n, m in itertools.product(_WS_RAYS, _WS_FACES)) == _INTERSECT3D_BYTES
    assert tuple(lib.tfrt_permute_rays_workspace_bytes(n, d)
                 for n, d in itertools.product(_WS_RAYS, _WS_DTYPES)) == _PERMUTE_BYTES
