"""tfrt_scene2d.deterministic on the host: the ctypes struct agrees with the header, the Python
layers set the field, the ordered sum's scale rule cannot overflow at the largest supported sizes,
and the workspace and argument checks of the 2-D reverse sweeps refuse what they refused before
(no kernel is launched here)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tfrt_hip.h")
E_BADARG, E_WORKSPACE = -1, -2
F64 = 1


@pytest.fixture(scope="module")
def lib():
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    return _lib.lib()


def test_scene2d_struct_matches_the_header(tmp_path):
    from tensorflowraytrace_amd._lib import Scene2D
    names = [f[0] for f in Scene2D._fields_]
    assert names[-1] == "deterministic" and names[-2] == "grad_arc_n_out"
    src = tmp_path / "t.c"
    body = "".join(f'printf("%s %zu\\n", "{n}", offsetof(tfrt_scene2d, {n}));' for n in names)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tfrt_hip.h"\n'
                   'int main(void){' + body +
                   'printf("sizeof %zu\\n", sizeof(tfrt_scene2d)); return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                    "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    for n in names:
        assert int(out[n]) == getattr(Scene2D, n).offset, n
    assert int(out["sizeof"]) == ctypes.sizeof(Scene2D)


def test_scene2d_args_sets_the_field():
    from tensorflowraytrace_amd import ops
    for det, want in ((False, 0), (True, 1)):
        sc = ops.Scene2DArgs(None, None, None, True, False, deterministic=det).struct(None, None)
        assert sc.deterministic == want
    assert ops.Scene2DArgs(None, None, None, True, False).struct(None, None).deterministic == 0


def test_engine_hands_the_flag_to_the_2d_scene():
    import inspect
    from tensorflowraytrace_amd import engine
    assert "deterministic" in inspect.signature(engine.OpticalSystem2D.scene_args).parameters
    system = engine.OpticalSystem2D.__new__(engine.OpticalSystem2D)
    system._merged_segments = system._merged_arcs = None
    system.intersect_epsilion = system.size_epsilion = system.ray_start_epsilion = 1e-10
    assert system.scene_args(None, True, deterministic=True).deterministic is True
    assert system.scene_args(None, True).deterministic is False


# ---- the scale rule (tfrt_trace2d.hip: fixed_bits2, fixed_scale2), restated with exact integers
def _bits(terms):
    lg = 0
    while lg < 62 and (1 << lg) < terms:
        lg += 1
    return min(40, 62 - lg)


def _rounded(x, maxabs, bits):
    """round(x * 2^(bits - e)) with maxabs = f 2^e, f in [0.5, 1) (llrint: ties to even)."""
    _, e = np.frexp(maxabs)
    return int(np.rint(np.ldexp(x, bits - int(e))))


def test_scale_rule_has_40_bits_up_to_2_22_terms_and_loses_one_per_doubling():
    assert _bits(1) == 40 and _bits(2 ** 22) == 40
    assert _bits(2 ** 22 + 1) == 39 and _bits(4_200_000 * 2) == 38
    for k in range(23, 62):
        assert _bits(2 ** k) == 62 - k


@pytest.mark.parametrize("n_rays,passes", [(2 ** 22, 1), (4_200_000, 2), (4_200_000, 5),
                                           (2 ** 31 - 4097, 1), (2 ** 31 - 4097, 64)])
def test_no_overflow_at_the_largest_supported_sizes(n_rays, passes):
    """The worst case: every term of an entry equals its largest one (rounded up to 2^bits), all
    of one sign, as many as rays x passes (the largest ray count a trace takes, and more passes than
    its tape could hold at that count).  The int64 sum stays below 2^63."""
    terms = n_rays * passes
    bits = _bits(terms)
    rng = np.random.default_rng(terms % 1000)
    for maxabs in (1.0, 0.75, np.nextafter(1.0, 0.0), 3e-300, 1.7e308, float(rng.random())):
        q = _rounded(maxabs, maxabs, bits)
        assert 0 < q <= 2 ** bits
        assert abs(_rounded(-maxabs, maxabs, bits)) <= 2 ** bits
        assert terms * q < 2 ** 63
    # and a random mix sums to what the float64 sum says, to the scale's resolution
    x = rng.normal(size=4096)
    m = float(np.abs(x).max())
    s = sum(_rounded(v, m, bits) for v in x)
    _, e = np.frexp(m)
    assert abs(s / 2.0 ** (bits - int(e)) - float(np.sum(x))) <= 4096 * 2.0 ** (int(e) - bits)


# ---- workspace and refusals
def test_workspace_covers_the_ordered_accumulators(lib):
    base = lib.tfrt_trace2d_workspace_bytes(1000, 0, 0, 4, F64)
    assert base > 0
    with_prims = lib.tfrt_trace2d_workspace_bytes(1000, 100, 50, 4, F64)
    # per entry: maximum, sum (8 B each) and a flag; 6 Ms + 7 Ma entries, each region aligned
    assert with_prims - base >= 17 * (6 * 100 + 7 * 50)
    assert with_prims - base <= 17 * (6 * 100 + 7 * 50) + 3 * 256
    assert lib.tfrt_trace2d_workspace_bytes(1000, -1, 0, 4, F64) == 0
    assert lib.tfrt_trace2d_workspace_bytes(1000, 0, -1, 4, F64) == 0


def _scene(det, Ms=2, Ma=0):
    from tensorflowraytrace_amd._lib import Scene2D
    sc = Scene2D()
    geo = (ctypes.c_double * (4 * max(Ms, 1)))()
    cat = (ctypes.c_int32 * max(Ms, 1))()
    n = (ctypes.c_double * max(Ms, 1))()
    sc.seg, sc.seg_cat, sc.seg_n_in, sc.seg_n_out = (ctypes.addressof(geo), ctypes.addressof(cat),
                                                     ctypes.addressof(n), ctypes.addressof(n))
    sc.n_segments, sc.n_arcs = Ms, Ma
    sc.deterministic = det
    return sc, (geo, cat, n)


def _backward(lib, sc, n_rays, ws_bytes, g_seg, counts=True):
    ws = (ctypes.c_uint8 * 64)()
    cnt = (ctypes.c_int32 * 64)()
    return lib.tfrt_trace2d_backward(
        None, n_rays, n_rays, ctypes.byref(sc) if sc is not None else None, 1.0, 0.0, 4, F64,
        None, 0, None, 0, None, 0, None, 0, g_seg, None, None, cnt if counts else None, ws,
        ws_bytes, None)


@pytest.mark.parametrize("det", [0, 1])
def test_bad_arguments_are_refused_in_both_modes(lib, det):
    sc, keep = _scene(det)
    g = (ctypes.c_double * 8)()
    assert _backward(lib, None, 10, 1 << 20, g) == E_BADARG
    assert _backward(lib, sc, -1, 1 << 20, g) == E_BADARG
    assert _backward(lib, sc, 10, 1 << 20, g, counts=False) == E_BADARG
    bad, keep2 = _scene(det)
    bad.seg = None
    assert _backward(lib, bad, 10, 1 << 20, g) == E_BADARG
    small = lib.tfrt_trace2d_workspace_bytes(10, 0, 0, 4, F64) - 1
    assert _backward(lib, sc, 10, small, g) == E_WORKSPACE


def test_ordered_sweep_refuses_a_workspace_without_its_accumulators(lib):
    """A workspace sized for no primitives is enough for the atomic sweep (as before), not for the
    ordered one, which says so before it launches anything."""
    sc, keep = _scene(1, Ms=2)
    g = (ctypes.c_double * 8)()
    plain = lib.tfrt_trace2d_workspace_bytes(10, 0, 0, 4, F64)
    assert _backward(lib, sc, 10, plain, g) == E_WORKSPACE
