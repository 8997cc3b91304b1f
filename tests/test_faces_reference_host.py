"""The 80-bit restatement of the face construction and of its reverse (tests/faces_reference.py)
against float64 torch autograd through the oracle, on every mesh of the GPU face test; the E_oracle
that bounds the device's error there; and the host side of ops.vertex_corners, validation of the
face indices included.  No GPU."""
import numpy as np
import pytest
import torch

import faces_oracle as fo
import faces_reference as fr

CASES = sorted(fr.cases())
EPS = fr.EPS64


def test_longdouble_is_the_80_bit_format():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("name", CASES)
def test_the_meshes_are_what_they_claim(name):
    mesh = fo.case(name)
    V, f = mesh["vertices"].shape[0], mesh["faces"]
    assert f.dtype == np.int32 and f.min() >= 0 and f.max() < V
    assert np.array_equal(mesh["vertices"],
                          fr.param_vertices(mesh["zero"], mesh["vectors"], mesh["params"]))
    again = fr.cases()[name]                                  # seeded: the same bits every time
    assert all(np.array_equal(mesh[k], again[k]) for k in mesh)
    val = fr.valence(f, V)
    if name.startswith("fan_"):
        assert val[0] == int(name[4:]) == f.shape[0]
        assert {int(np.nonzero(row == 0)[0][0]) for row in f} == set(range(min(3, f.shape[0])))
    if name.startswith("unreferenced"):
        assert (val == 0).sum() >= 13
    if name.startswith("slivers"):
        p = mesh["vertices"][f]
        a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 1]
        height = np.linalg.norm(np.cross(a, b), axis=1) / np.linalg.norm(p[:, 2] - p[:, 0], axis=1)
        assert height.max() < 2 * fr.SLIVER_HEIGHT and height.min() > 0.2 * fr.SLIVER_HEIGHT
    _, n = fr.forward(mesh["vertices"], f)
    bad = ~np.isfinite(n).all(axis=1)
    if name.startswith("zero_area"):
        _, rows = fr.zero_area(100, 40, 10)
        assert np.array_equal(np.nonzero(bad)[0], rows) and len(rows) == 5
    elif name.startswith("repeated"):
        assert np.array_equal(np.nonzero(bad)[0], np.arange(0, 50, 3))
    elif name.endswith("_V1"):
        assert bad.all()
    else:
        assert not bad.any()


@pytest.mark.parametrize("name", CASES)
def test_forward_restatement_matches_the_oracle(name):
    mesh = fo.case(name)
    fv, n = fr.forward(mesh["vertices"], mesh["faces"])
    fv_o, n_o = fo.oracle_forward(torch.tensor(mesh["vertices"]), mesh["faces"])
    assert np.array_equal(fv.astype(np.float64), fv_o.numpy())          # a gather: exact
    n_o = n_o.numpy()
    assert np.array_equal(np.isfinite(n), np.isfinite(n_o))
    # a unit normal computed in float64: C keeps |C| of products of size |A||B|
    p = mesh["vertices"][mesh["faces"]].astype(fr.LD)
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        kappa = (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
                 / np.linalg.norm(np.cross(a, b), axis=1))
    ok = np.isfinite(n).all(axis=1)
    assert np.all(np.abs(n_o[ok] - n[ok]).max(axis=1) <= 8 * EPS * kappa[ok])
    # the float64 restatement is the oracle's own arithmetic
    _, n64 = fr.forward(mesh["vertices"], mesh["faces"], dtype=np.float64)
    assert np.array_equal(n64[ok], n_o[ok])


@pytest.mark.parametrize("form", ["build", "param"])
@pytest.mark.parametrize("name", CASES)
def test_reverse_restatement_matches_oracle_autograd(name, form):
    """Every upstream combination, without mask, with a random one and with one that switches a
    whole vertex off: the 80-bit restatement and float64 autograd agree within 8 float64
    roundings of what is summed into each vertex (faces_reference.rounding_scale), are non-finite
    at the same entries, and the restatement is exactly 0.0 where nothing arrives."""
    mesh = fo.case(name)
    V = mesh["vertices"].shape[0]
    back = fo.oracle_backward_vertices if form == "build" else fo.oracle_backward_params
    for (u, m), (g_fv, g_norm, mask) in fo.combos(mesh).items():
        ref = fo.reference(mesh, form, g_fv, g_norm, mask)
        got = back(mesh, g_fv, g_norm, mask)
        assert ref.dtype == np.longdouble and ref.shape == got.shape
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got)), (u, m)
        scale = fr.rounding_scale(mesh["vertices"], mesh["faces"], g_fv, g_norm, mask,
                                  mesh["vectors"] if form == "param" else None)
        scale = scale if form == "param" else scale[:, None] * np.ones(3)
        with np.errstate(invalid="ignore"):
            err = np.abs(got.astype(fr.LD) - ref)
        assert np.all(err[fin] <= 8 * EPS * scale[fin]), (u, m, float((err[fin] / scale[fin]).max() / EPS))
        keep = np.ones_like(mesh["faces"], dtype=bool) if mask is None else mask.astype(bool)
        untouched = np.bincount(mesh["faces"][keep], minlength=V) == 0
        assert np.all(ref[untouched] == 0.0) and np.all(got[untouched] == 0.0)
        if m == "vertex_off":
            assert untouched[int(np.argmax(fr.valence(mesh["faces"], V)))]
        if name.startswith("zero_area") and u != "fv" and m == "nomask":
            _, rows = fr.zero_area(100, 40, 10)
            touched = np.zeros(V, dtype=bool)
            touched[mesh["faces"][rows].reshape(-1)] = True
            nonfinite = ~fin if form == "param" else ~fin.all(axis=1)
            assert np.array_equal(nonfinite, touched)
        # the float64 restatement: the same formulas at the device's precision
        if form == "build":
            r64 = fr.backward_vertices(mesh["vertices"], mesh["faces"], g_fv, g_norm, mask,
                                       dtype=np.float64)
        else:
            r64 = fr.backward_params(mesh["zero"], mesh["vectors"], mesh["params"], mesh["faces"],
                                     g_fv, g_norm, mask, dtype=np.float64)
        assert np.array_equal(np.isfinite(r64), fin)
        assert np.all(np.abs(r64.astype(fr.LD) - ref)[fin] <= 8 * EPS * scale[fin])


@pytest.mark.parametrize("form", ["build", "param"])
@pytest.mark.parametrize("name", CASES)
def test_e_oracle_is_finite_and_below_1e_8(name, form):
    e = fo.e_oracle(name, form)
    print(f"E_oracle {name} {form}: {e:.3e}  bound {fo.bound(name, form):.3e}")
    assert np.isfinite(e) and e < 1e-8
    assert fo.bound(name, form) >= 8 * EPS


# ------------------------------------------------------------------- ops.vertex_corners (host)

def _corners_by_hand(faces, V):
    flat = np.asarray(faces).reshape(-1)
    lists = [[q for q in range(flat.size) if flat[q] == v] for v in range(V)]
    start = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    return start, np.array([q for x in lists for q in x], dtype=np.int64)


@pytest.mark.parametrize("name", ["soup_F1_V3", "fan_9", "unreferenced_F40_V33", "repeated_F50_V20",
                                  "soup_F255_V1"])
def test_vertex_corners_lists_every_corner_once_in_corner_order(name):
    from tensorflowraytrace_amd import ops
    mesh = fo.case(name)
    faces, V = torch.tensor(mesh["faces"]), mesh["vertices"].shape[0]
    start, lst = ops.vertex_corners(faces, V)
    assert start.dtype == torch.int32 and lst.dtype == torch.int32
    assert start.shape == (V + 1,) and lst.shape == (faces.numel(),)
    want_start, want_list = _corners_by_hand(mesh["faces"], V)
    assert np.array_equal(start.numpy(), want_start) and np.array_equal(lst.numpy(), want_list)


def test_vertex_corners_validates_once_per_face_tensor(monkeypatch):
    from tensorflowraytrace_amd import ops
    from tensorflowraytrace_amd._lib import TfrtError
    monkeypatch.setattr(ops, "_corner_cache", {})
    calls = []
    check = ops._check_face_indices
    monkeypatch.setattr(ops, "_check_face_indices", lambda f, v: (calls.append(1), check(f, v)))
    mesh = fo.case("fan_9")
    faces, V = torch.tensor(mesh["faces"]), mesh["vertices"].shape[0]
    first = ops.vertex_corners(faces, V)
    assert len(ops._corner_cache) == 1 and len(calls) == 1
    entry = next(iter(ops._corner_cache.values()))
    second = ops.vertex_corners(faces, V)
    assert len(calls) == 1 and next(iter(ops._corner_cache.values())) is entry
    assert second[0] is first[0] and second[1] is first[1]
    # an index outside [0, V): V itself, -1; nothing bad is cached
    for bad in (V, -1):
        wrong = faces.clone()
        wrong[4, 1] = bad
        with pytest.raises(TfrtError, match="vertex indices"):
            ops.vertex_corners(wrong, V)
        with pytest.raises(TfrtError):
            ops.vertex_corners(wrong, V)
    assert len(ops._corner_cache) == 1
    # the same tensor against fewer vertices is another key, and is refused
    with pytest.raises(TfrtError):
        ops.vertex_corners(faces, V - 1)
    # an edit in place is seen (the key holds the tensor's version)
    faces[0, 0] = V
    with pytest.raises(TfrtError):
        ops.vertex_corners(faces, V)
