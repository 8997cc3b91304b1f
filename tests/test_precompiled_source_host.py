"""PrecompiledSource on the host (tfrt/sources.py:1099-1358): from_samples / clear, the pickle
layout, the rows handed out without down-sampling, the setters' checks -- and the ctypes mirror of
tfrt_source3d_program, whose pool fields (TFRT_SRC_POOL) were appended to the struct, against a
host compile of the header.  No kernel is launched here."""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tfrt_hip.h")
GEO = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")


def _sources():
    import tfrt.sources as sources
    return sources


def _sample(n, offset, as_numpy=False, extra=True):
    out = {g: torch.arange(n, dtype=torch.float64) + offset + 1000.0 * k for k, g in enumerate(GEO)}
    out["wavelength"] = torch.full((n,), 500.0 + offset, dtype=torch.float64)
    if extra:
        out["object_coords"] = torch.stack([torch.arange(n, dtype=torch.float64) + offset,
                                            -torch.arange(n, dtype=torch.float64)], dim=1)
    if as_numpy:
        out = {k: v.numpy() for k, v in out.items()}
    return out


def test_from_samples_concatenates_in_list_order_and_replaces_the_pool():
    sources = _sources()
    src = sources.PrecompiledSource(3, do_downsample=False)
    assert not src and src.sampling_domain_size == 0
    a, b = _sample(4, 0.0), _sample(3, 100.0, as_numpy=True)      # a snapshot-like dict and a plain one
    src.from_samples([a, b])
    assert bool(src) and src.sampling_domain_size == 7
    assert set(src.keys()) == set(a.keys())
    for f in a:
        want = np.concatenate([a[f].numpy(), b[f]], axis=0)
        assert np.array_equal(src[f].cpu().numpy(), want), f
        assert np.array_equal(src._full_fields[f], want), f
    # a real snapshot of another source
    manual = sources.ManualSource(3)
    for f, v in _sample(5, 7.0, extra=False).items():
        manual[f] = v
    src.from_samples([manual.snapshot(do_update=False)])
    assert src.sampling_domain_size == 5 and "object_coords" not in src.keys()
    assert np.array_equal(src["y_end"].cpu().numpy(), np.arange(5.0) + 7.0 + 4000.0)


def test_clear_leaves_an_empty_falsy_source():
    sources = _sources()
    src = sources.PrecompiledSource(3, sample_count=6)
    src.from_samples([_sample(9, 0.0)])
    assert bool(src) and src["x_start"].shape == (6,)
    src.clear()
    assert not src and src.sampling_domain_size == 0 and list(src.keys()) == []
    src.update()
    assert not src
    src.from_samples([_sample(2, 1.0)])
    assert bool(src) and src.sampling_domain_size == 2


def test_save_and_load_keep_the_pickle_layout(tmp_path):
    sources = _sources()
    src = sources.PrecompiledSource(3, do_downsample=False)
    src.from_samples([_sample(6, 3.0)])
    name = str(tmp_path / "pool.dat")
    src.save(name)
    with open(name, "rb") as f:
        data = pickle.load(f)
    assert set(data.keys()) == {"dimension", "standard_domains", "fields"}
    assert data["dimension"] == 3 and isinstance(data["standard_domains"], set)
    assert all(isinstance(v, np.ndarray) for v in data["fields"].values())
    back = sources.PrecompiledSource(name, do_downsample=False)
    assert back.dimension == 3 and back.sampling_domain_size == 6
    for f in src.keys():
        assert np.array_equal(back[f].cpu().numpy(), src[f].cpu().numpy()), f


def test_without_downsampling_the_pool_rows_come_in_order():
    sources = _sources()
    src = sources.PrecompiledSource(3, sample_count=3, do_downsample=False)
    s = _sample(11, 0.5)
    src.from_samples([s])
    for _ in range(2):
        src.update()
        for f in s:
            assert np.array_equal(src[f].cpu().numpy(), s[f].numpy()), f
    # and with it: sample_count rows of the pool, drawn with replacement
    src.do_downsample = True
    src.sample_count = 40
    src.update()
    x = src["x_start"].cpu().numpy() - 0.5
    assert x.shape == (40,) and set(x.tolist()) <= set(range(11))
    assert np.array_equal(src["object_coords"].cpu().numpy()[:, 0], x + 0.5)      # one row per ray


def test_perturbation_setters_and_the_sample_count_check():
    sources = _sources()
    src = sources.PrecompiledSource(3)
    for ok in (None, 0.1, (0.1, 0.0, 0.2), [0.0, 0.0, 0.0], np.float64(2.0), torch.tensor([1.0, 2.0, 3.0])):
        src.start_perturbation = ok
        src.end_perturbation = ok
        if ok is None:
            assert src.start_perturbation is None and src.end_perturbation is None
        else:
            assert np.shape(src.end_perturbation) == (3,)
    for bad in ((0.1, 0.2), (1.0, 2.0, 3.0, 4.0), "wide", np.ones((2, 3))):
        with pytest.raises(ValueError):
            src.start_perturbation = bad
        with pytest.raises(ValueError):
            src.end_perturbation = bad
    src2 = sources.PrecompiledSource(2, end_perturbation=(0.1, 0.2))
    assert np.shape(src2.end_perturbation) == (2,)
    with pytest.raises(ValueError):
        src2.end_perturbation = (0.1, 0.2, 0.3)
    for bad in (0, -3, 2.5, "7", None):
        with pytest.raises(ValueError):
            src.sample_count = bad
        with pytest.raises(ValueError):
            sources.PrecompiledSource(3, sample_count=bad)
    src.sample_count = np.int32(12)
    assert src.sample_count == 12
    # the perturbation moves the end points it names and nothing else
    src = sources.PrecompiledSource(3, do_downsample=False, end_perturbation=(0.0, 0.5, 0.0))
    s = _sample(2000, 0.0)
    src.from_samples([s])
    for f in GEO:
        moved = src[f].cpu().numpy() - s[f].numpy()
        if f == "y_end":
            assert 0.4 < moved.std() < 0.6
        else:
            assert not moved.any(), f


def test_source3d_program_struct_matches_the_header(tmp_path):
    from tensorflowraytrace_amd._lib import PointsProgram, Source3DProgram
    for name, struct in (("tfrt_points_program", PointsProgram), ("tfrt_source3d_program", Source3DProgram)):
        names = [f[0] for f in struct._fields_]
        if struct is Source3DProgram:        # the pool fields come last: every earlier offset stays
            assert names[-8:] == ["pool", "pool_count", "sigma_start", "sigma_end", "pool_downsample",
                                  "pool_stream", "pool_seed", "pool_epoch"]
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
        assert int(out["pool_kind"]) == 3
    from tensorflowraytrace_amd import _lib
    assert _lib.SRC_POOL == 3
    # the fields before the pool's sit where they sat before it was added
    assert Source3DProgram.n_rays.offset + 8 == Source3DProgram.pool.offset
    assert "tfrt_source3d_pool_rows" in _lib.SIGNATURES
