"""Host side of the 2-D pool program (tfrt_source2d_program.kind = TFRT_SRC_POOL, a 2-D
PrecompiledSource made on the device): the ctypes mirror of the struct against a host compile of the
header, the refusal of malformed pool programs before any launch, and the host path of a 2-D
PrecompiledSource, which the CPU device keeps.  No kernel is launched here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tfrt_hip.h")
GEO2 = ("x_start", "y_start", "x_end", "y_end")
POOL_FIELDS = ["pool", "pool_count", "sigma_start", "sigma_end", "pool_downsample", "pool_stream",
               "pool_seed", "pool_epoch"]
E_BADARG = -1


@pytest.fixture(scope="module")
def lib():
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    return _lib.lib()


def test_source2d_program_struct_matches_the_header(tmp_path):
    from tensorflowraytrace_amd import _lib
    from tensorflowraytrace_amd._lib import SamplesProgram, Source2DProgram, Source3DProgram
    for name, struct in (("tfrt_samples_program", SamplesProgram),
                         ("tfrt_source2d_program", Source2DProgram)):
        names = [f[0] for f in struct._fields_]
        if struct is Source2DProgram:        # the pool fields come last: every earlier offset stays
            assert names[-8:] == POOL_FIELDS
            assert names[:names.index("pool")][-1] == "n_rays"
        src = tmp_path / (name + ".c")
        body = "".join(f'printf("%s %zu\\n", "{n}", offsetof({name}, {n}));' for n in names)
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tfrt_hip.h"\n'
                       'int main(void){' + body +
                       f'printf("sizeof %zu\\n", sizeof({name}));'
                       'printf("pool_kind %d\\n", TFRT_SRC_POOL); return 0;}\n')
        exe = tmp_path / name
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                        "-o", str(exe)], check=True)
        out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                            check=True).stdout.splitlines())
        for n in names:
            assert int(out[n]) == getattr(struct, n).offset, (name, n)
        assert int(out["sizeof"]) == ctypes.sizeof(struct)
        assert int(out["pool_kind"]) == 3 == _lib.SRC_POOL
    # the fields before the pool's sit where they sat before it was added
    assert Source2DProgram.n_rays.offset + 8 == Source2DProgram.pool.offset
    # the same names as in the 3-D struct, two axes
    assert [f[0] for f in Source3DProgram._fields_][-8:] == POOL_FIELDS
    assert Source2DProgram.sigma_start.size == Source2DProgram.sigma_end.size == 16
    assert "tfrt_source2d_pool_rows" in _lib.SIGNATURES
    assert _lib.SIGNATURES["tfrt_source2d_pool_rows"][1][0]._type_ is Source2DProgram
    with open(HEADER) as f:
        text = f.read()
    assert "tfrt_source2d_pool_rows(" in text and "has no 2-D form" not in text


def test_bad_2d_pool_programs_are_refused_before_any_launch(lib):
    """Every pointer here is host memory: a launch on one of these programs would not return -1."""
    from tensorflowraytrace_amd import _lib
    dummy = ctypes.create_string_buffer(1 << 12)
    ptr = ctypes.cast(dummy, ctypes.c_void_p).value
    n_pool, n = 37, 100

    def program(**changes):
        sp = _lib.Source2DProgram()
        sp.kind, sp.n_rays = _lib.SRC_POOL, n
        sp.pool, sp.pool_count, sp.pool_downsample = ptr, n_pool, 1
        sp.pool_stream, sp.pool_seed, sp.pool_epoch = 5, 1234, ptr
        sp.sigma_end[1] = 1e-3
        for k, v in changes.items():
            if isinstance(v, tuple):
                for q, x in enumerate(v):
                    getattr(sp, k)[q] = x
            else:
                setattr(sp, k, v)
        return sp

    def calls(sp, count):
        return (lib.tfrt_source2d_generate(ctypes.byref(sp), None, 0, count, _lib.F64, ptr, max(count, 1),
                                           None, 0, None),
                lib.tfrt_source2d_generate(ctypes.byref(sp), None, 0, count, _lib.F32, None, 0,
                                           ptr, max(count, 1), None),
                lib.tfrt_source2d_pool_rows(ctypes.byref(sp), None, 0, count, ptr, None))

    bad = [program(pool=None), program(pool_count=0), program(pool_count=-5),
           program(pool_count=(1 << 31)),                                    # INT32_MAX + 1
           program(sigma_end=(0.0, -1e-3)), program(sigma_start=(float("nan"), 0.0)),
           program(sigma_end=(float("inf"), 0.0)), program(sigma_start=(0.0, -0.0 - 1e-300)),
           program(pool_epoch=None),                                         # samples and perturbs
           program(pool_epoch=None, sigma_end=(0.0, 0.0)),                   # samples
           program(pool_epoch=None, pool_downsample=0, n_rays=n_pool),       # perturbs
           program(pool_downsample=0),                                       # n_rays != pool_count
           program(n_rays=-1)]
    for k, sp in enumerate(bad):
        assert calls(sp, n) == (E_BADARG,) * 3, k
        assert calls(sp, 0) == (E_BADARG,) * 3, k                            # before the n = 0 way out
    # well-formed programs with nothing to do: no launch, no error
    assert calls(program(), 0) == (0, 0, 0)
    assert calls(program(pool_count=(1 << 31) - 1), 0) == (0, 0, 0)
    plain = program(pool_epoch=None, pool_downsample=0, n_rays=n_pool, sigma_end=(0.0, 0.0))
    assert calls(plain, 0) == (0, 0, 0)                # nothing sampled, nothing perturbed: no counter
    assert calls(program(), n + 1) == (E_BADARG,) * 3                        # past the last ray
    assert lib.tfrt_source2d_pool_rows(ctypes.byref(program()), None, -1, 0, ptr, None) == E_BADARG
    assert lib.tfrt_source2d_pool_rows(ctypes.byref(program()), None, 0, -1, ptr, None) == E_BADARG
    assert lib.tfrt_source2d_pool_rows(None, None, 0, 0, ptr, None) == E_BADARG
    assert lib.tfrt_source2d_pool_rows(ctypes.byref(program()), None, 0, n, None, None) == E_BADARG
    # the rows of another kind of program do not exist
    other = _lib.Source2DProgram()
    other.kind, other.n_rays = _lib.SRC_POINT, 1
    other.b.kind, other.b.count, other.b.table, other.b.columns = _lib.SMP_TABLE, 1, ptr, 1
    assert lib.tfrt_source2d_generate(ctypes.byref(other), None, 0, 0, _lib.F64, ptr, 1, None, 0,
                                      None) == 0
    assert lib.tfrt_source2d_pool_rows(ctypes.byref(other), None, 0, 0, ptr, None) == E_BADARG


def _sample(n, offset):
    out = {g: np.arange(n, dtype=np.float64) + offset + 1000.0 * k for k, g in enumerate(GEO2)}
    out["wavelength"] = np.linspace(450.0, 650.0, n)
    out["tag"] = np.stack([np.arange(n, dtype=np.float64), -np.arange(n, dtype=np.float64)], axis=1)
    return out


def test_on_the_cpu_a_2d_pool_is_drawn_on_the_host_as_before():
    import tensorflowraytrace_amd.config as config
    import tfrt.distributions as d
    import tfrt.sources as sources
    assert config.get_device().type == "cpu"
    d.seed(7)
    s = _sample(11, 0.5)
    src = sources.PrecompiledSource(2, sample_count=40)
    assert not src._device_mode()
    src.from_samples([s])
    assert not src.device_mode and isinstance(src._fields, dict)
    assert set(src.keys()) == set(s.keys())
    for _ in range(2):
        src.update()
        assert not src.device_mode
        rows = (src["x_start"].numpy() - 0.5).astype(np.int64)
        assert rows.shape == (40,) and rows.min() >= 0 and rows.max() < 11
        for f, v in s.items():                              # one draw of rows for every field
            assert src[f].shape == (40,) + v.shape[1:], f
            assert np.array_equal(src[f].numpy(), v[rows]), f
    # without down-sampling: the pool in order
    src.do_downsample = False
    src.update()
    for f, v in s.items():
        assert np.array_equal(src[f].numpy(), v), f
    # a perturbation moves the axis it names and nothing else
    big = _sample(2000, 0.0)
    for which, field in (("start_perturbation", "x_start"), ("end_perturbation", "y_end")):
        sigma = (0.5, 0.0) if field[0] == "x" else (0.0, 0.5)
        src = sources.PrecompiledSource(2, do_downsample=False, **{which: sigma})
        src.from_samples([big])
        assert not src.device_mode
        for f in GEO2:
            moved = src[f].numpy() - big[f]
            if f == field:
                assert 0.4 < moved.std() < 0.6, f
            else:
                assert not moved.any(), (field, f)
        assert np.array_equal(src["tag"].numpy(), big["tag"])
    # a pool that lacks a geometry field has no device form anywhere
    part = {f: v for f, v in s.items() if f != "y_end"}
    src = sources.PrecompiledSource(2, do_downsample=False)
    src.from_samples([part])
    assert not src._device_mode() and set(src.keys()) == set(part.keys())
