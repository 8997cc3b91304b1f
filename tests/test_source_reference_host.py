"""Guards of tests/source_reference.py, the float64 numpy reference that
tests/test_gpu_source_programs_exact.py holds the 3-D source kernels to: the generator against the
published Philox4x32-10 vectors, the point formulas against the package's torch path (the mirror of
the reference project's code that the golden tests cover), and the conditions on the GPU tests'
inputs under which rounding alone cannot move a sample by more than their tolerance."""
import math

import numpy as np
import pytest
import torch

import source_reference as sr

PI = math.pi


# ------------------------------------------------------------------------------ generator
# counter words, key words, output words after 10 rounds (the published Philox4x32-10 vectors)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("stream", [0, 5, 0x7FFFFFFF])
@pytest.mark.parametrize("vector", range(len(KNOWN_ANSWERS)))
def test_philox_known_answers_through_the_key_and_counter_mapping(vector, stream):
    """counter = (sample lo, sample hi, epoch lo, epoch hi), key = (seed lo, seed hi ^ stream): the
    high words of seed, epoch and sample number all carry bits in the second and third vector."""
    counter, key, want = KNOWN_ANSWERS[vector]
    sample = counter[0] | (counter[1] << 32)
    epoch = counter[2] | (counter[3] << 32)
    seed = key[0] | ((key[1] ^ stream) << 32)
    words = sr.philox_words(seed, stream, epoch, 1, first=sample)
    assert tuple(int(w[0]) for w in words) == want
    u0, u1 = sr.philox_uv(seed, stream, epoch, 1, first=sample)
    assert u0[0] == (((want[0] << 32) | want[1]) >> 11) * 2.0 ** -53
    assert u1[0] == (((want[2] << 32) | want[3]) >> 11) * 2.0 ** -53
    assert 0.0 <= u0[0] < 1.0 and 0.0 <= u1[0] < 1.0
    # the vector as one sample among others: `first` only shifts the sample numbers
    if sample >= 2:
        many = sr.philox_words(seed, stream, epoch, 5, first=sample - 2)
        assert tuple(int(w[2]) for w in many) == want
    # a dropped high word gives other numbers (the mapping's high words are exercised)
    if vector:
        for other in (sr.philox_words(seed & 0xFFFFFFFF, stream, epoch, 1, first=sample),
                      sr.philox_words(seed, stream, epoch & 0xFFFFFFFF, 1, first=sample),
                      sr.philox_words(seed, stream, epoch, 1, first=sample & 0xFFFFFFFF)):
            assert tuple(int(w[0]) for w in other) != want


def test_sample_numbers_wrap_at_two_to_the_64():
    a = sr.philox_words(7, 1, 3, 4, first=2 ** 64 - 2)
    b = sr.philox_words(7, 1, 3, 2, first=0)
    assert [int(w[2]) for w in a] == [int(w[0]) for w in b]
    assert [int(w[3]) for w in a] == [int(w[1]) for w in b]


# ------------------------------------------------------------------- the torch path
def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("transformed", [False, True])
@pytest.mark.parametrize("name", sorted(sr.POINT_CASES))
def test_reference_equals_the_torch_path_fed_the_same_numbers(name, transformed, monkeypatch):
    """distributions._uniform hands out low + (high - low) u with u from ``philox_uv``: u0 on the
    first call of an update, u1 on the second, of the epoch the update makes."""
    import tfrt.distributions as d
    import tensorflowraytrace_amd.config as config
    assert config.get_device().type == "cpu"
    case = sr.POINT_CASES[name]
    n = 257
    calls = [0]

    def uniform(count, low=0.0, high=1.0):
        assert int(count) == n
        epoch, which = calls[0] // 2 + 1, calls[0] % 2
        calls[0] += 1
        u = torch.from_numpy(sr.philox_uv(sr.SEED, sr.STREAM, epoch, n)[which].copy())
        return low + (high - low) * u

    monkeypatch.setattr(d, "_uniform", uniform)
    d.set_device_random(False)
    try:
        dist = case["make"](getattr(d, case["cls"]), n)            # (the constructor updates: epoch 1)
        assert calls[0] == 2 and not dist.__dict__.get("_device_active")
        epoch = 1
        if transformed:
            t = sr.TRANSFORMATION
            d.BasePointTransformation(dist, rotation=t["quat"], translation=t["shift"], scale=t["scale"])
            dist.update()
            epoch = 2
            assert calls[0] == 4
        u0, u1 = sr.philox_uv(sr.SEED, sr.STREAM, epoch, n)
        pts, a0, a1 = sr.points(case["kind"], case["params"], u0, u1, **sr.transformation(transformed))
        want = sr.class_properties(case["kind"], case["params"], pts, a0, a1, transformed)
        checked = 0
        for prop in ("points", "ranks", "polar_ranks", "angles"):
            assert hasattr(dist, prop) == (prop in want), prop
            if prop in want:
                got = _np(getattr(dist, prop))
                assert got.shape == want[prop].shape and got.dtype == np.float64
                np.testing.assert_allclose(got, want[prop], rtol=0, atol=1e-13, err_msg=prop)
                checked += 1
        assert checked >= 2
    finally:
        d.set_device_random(True)


def test_reference_rotates_like_the_packages_quaternion_helper():
    """scale, then rotation, then translation; the rotation is the package's v + w t + u x t."""
    import tfrt.distributions as d
    t = sr.TRANSFORMATION
    u0, u1 = sr.philox_uv(3, 1, 1, 64)
    plain = sr.points(sr.SQUARE, (0.5, 0.0, 0.0, 0.25), u0, u1)[0]
    moved = sr.points(sr.SQUARE, (0.5, 0.0, 0.0, 0.25), u0, u1, **t)[0]
    want = d.rotate_vector_by_quaternion(torch.tensor(t["quat"], dtype=torch.float64),
                                         torch.from_numpy(plain * np.array(t["scale"])))
    np.testing.assert_allclose(moved, _np(want) + np.array(t["shift"]), rtol=0, atol=1e-14)
    assert abs(sum(q * q for q in t["quat"]) - 1.0) < 1e-15
    # no rotation about a coordinate axis, no uniform scale: an order or a sign slip shows
    assert float(np.abs(moved - (plain * np.array(t["scale"]) + np.array(t["shift"]))).max()) > 0.05


# ------------------------------------------------------------------------------ the pool
def test_pool_rays_is_the_headers_draw_on_a_case_small_enough_to_do_by_hand():
    pool = np.array([[0.0, 1.0, 2.0, 3.0, 4.0, 5.0],
                     [10.0, 11.0, 12.0, 13.0, 14.0, 15.0],
                     [20.0, 21.0, 22.0, 23.0, 24.0, 25.0]])
    u0 = np.array([0.0, 0.34, 0.999999, 1.0 - 2.0 ** -53])
    zeros = np.zeros(4)
    # u = 1 - exp(-1/2): r = 1; v = 0, 1/4, 1/2, 1/8: (cos, sin) = (1, 0), (0, 1), (-1, 0), (s, s)
    u = np.full(4, 1.0 - math.exp(-0.5))
    v = np.array([0.0, 0.25, 0.5, 0.125])
    numbers = [(u0, zeros), (u, v), (u, v), (u, v)]
    rows, start, end = sr.pool_rays(pool, numbers, (0.0, 0.5, 2.0), (0.25, 0.0, 4.0), True)
    assert rows.tolist() == [0, 1, 2, 2]
    s = math.sqrt(0.5)
    cos, sin = np.array([1.0, 0.0, -1.0, s]), np.array([0.0, 1.0, 0.0, s])
    assert np.array_equal(start[:, 0], pool[rows, 0])                 # sigma 0: the stored value
    assert np.array_equal(end[:, 1], pool[rows, 4])
    np.testing.assert_allclose(start[:, 1], pool[rows, 1] + 0.5 * cos, rtol=0, atol=1e-15)
    np.testing.assert_allclose(start[:, 2], pool[rows, 2] + 2.0 * cos, rtol=0, atol=1e-15)
    np.testing.assert_allclose(end[:, 0], pool[rows, 3] + 0.25 * sin, rtol=0, atol=1e-15)
    np.testing.assert_allclose(end[:, 2], pool[rows, 5] + 4.0 * sin, rtol=0, atol=1e-15)
    # without down-sampling ray i is row i; without sigmas nothing moves
    rows, start, end = sr.pool_rays(pool, [(u0[:3], zeros[:3])] + [(u[:3], v[:3])] * 3,
                                    (0.0,) * 3, (0.0,) * 3, False)
    assert rows.tolist() == [0, 1, 2]
    assert np.array_equal(start, pool[:, :3]) and np.array_equal(end, pool[:, 3:])


# ------------------------------------------------- conditions on the GPU tests' inputs
def _conditions():
    """(label, case, seed, stream, epoch, count, first) of every draw whose azimuths or polar angles the
    GPU tests compare."""
    out = []
    for name in sorted(sr.POINT_CASES):
        for epoch in sr.EPOCHS:
            out.append((f"{name} epoch {epoch}", name, sr.SEED, sr.STREAM, epoch, sr.N, 0))
        out.append((f"{name} advanced epoch", name, sr.SEED, sr.STREAM, 3, sr.N, 0))
    for name in sr.ABI_CASES:          # (the samples the test reads: first .. first + n - 1)
        out.append((f"{name} C ABI", name, sr.ABI_SEED, sr.ABI_STREAM, sr.ABI_EPOCH, sr.ABI_N,
                    sr.ABI_FIRST))
    for name, stream in sr.SOURCE_CAPS:
        for epoch in sr.SOURCE_EPOCHS:
            out.append((f"{name} source epoch {epoch}", name, sr.SOURCE_SEED, stream, epoch, sr.N, 0))
    return out


@pytest.mark.parametrize("label,name,seed,stream,epoch,count,first", _conditions(),
                         ids=[c[0].replace(" ", "_") for c in _conditions()])
def test_no_sample_of_the_gpu_tests_sits_on_a_fold_or_at_the_pole(label, name, seed, stream, epoch,
                                                                  count, first):
    """The kernel forms ((1 + sqrt 5) u) pi and the host pi (1 + sqrt 5) u: a sample on a fold of the
    wedge (or of the ranks' floormod 2 pi) could land one span apart through rounding alone, and
    acos amplifies the rounding of its argument by 1 / sin(phi).  With both kept away the GPU
    comparison leaves no sample out."""
    fold, acos_bound = sr.input_conditions(name, seed, stream, epoch, count, first)
    kind = sr.POINT_CASES[name]["kind"]
    assert (fold is None) == (kind == sr.SQUARE)
    if fold is not None:
        assert fold > 1e-9, (label, fold)
    assert (acos_bound is None) == (kind in (sr.CIRCLE, sr.SQUARE))
    if acos_bound is not None:
        assert acos_bound < 1e-13, (label, acos_bound)


def test_the_shared_references_are_computed_once_and_read_only():
    a = sr.case_reference("circle", False, 1)
    assert sr.case_reference("circle", False, 1) is a
    assert a[0].shape == (sr.N, 3) and not a[0].flags.writeable
    with pytest.raises(ValueError):
        a[0][0, 0] = 1.0


# ------------------------------------- the GPU tests' source expectations, on the torch path
@pytest.mark.parametrize("kind,flag", [("aperture", True), ("point", True), ("point", False),
                                       ("angular", True), ("angular", False)])
def test_source_expectations_of_the_gpu_tests_hold_on_the_torch_path(kind, flag, monkeypatch):
    """The sources of tests/test_gpu_source_programs_exact.py, built on the CPU with the torch
    path's generator replaced by ``philox_uv`` (each distribution on the stream and at the epoch the
    device programs would use): their fields equal what the GPU test expects of the kernels -- the
    reference points assembled by oracle/sources.py."""
    import tfrt.distributions as d
    import test_gpu_source_programs_exact as gx
    n_inputs = 1 if kind == "point" else 2
    # (stream, epoch) of every update, in the order the constructors and update() run them
    # (an AngularSource updates its angles, made second, before its base points)
    streams = list(range(1, n_inputs + 1))
    schedule = [(s, 1) for s in streams] + [(s, e) for e in (2, 3)
                                            for s in (streams[::-1] if kind == "angular" else streams)]
    calls = [0]

    def uniform(count, low=0.0, high=1.0):
        stream, epoch = schedule[calls[0] // 2]
        u = sr.philox_uv(sr.SOURCE_SEED, stream, epoch, int(count))[calls[0] % 2]
        calls[0] += 1
        return low + (high - low) * torch.from_numpy(u.copy())

    monkeypatch.setattr(d, "_uniform", uniform)
    d.set_device_random(False)
    try:
        src, inputs, want = gx.SOURCES[kind][0](d, flag)
        assert src._device_program() is None
        for epoch in sr.SOURCE_EPOCHS:
            assert calls[0] == 2 * n_inputs * epoch
            expected = want(epoch)
            for f in gx.GEO:
                np.testing.assert_allclose(_np(src[f]), expected[f], rtol=0, atol=1e-13, err_msg=f)
            np.testing.assert_array_equal(_np(src["wavelength"]), expected["wavelength"])
            if epoch != sr.SOURCE_EPOCHS[-1]:
                src.update()
    finally:
        d.set_device_random(True)
