"""Face construction and its reverse (csrc/tfrt_faces.hip) against the oracle and the 80-bit
restatement of tests/faces_reference.py, in both forms of the reverse.

Forward: ``face_verts`` and ``norm`` of ops.build_faces, ops.param_faces, ops.ParamFacesBatch and
tfrt_build_faces_forward are those of ``oracle.tracer.faces_from_vertices`` bit for bit (a NaN
equals a NaN: the zero-area faces).

Reverse: the gather kernels (corner lists; through autograd and through the C ABI) and the atomic
kernels (C ABI with NULL corner lists) against the 80-bit reference.  The bound of a case, relative
to the largest reference entry, is ``8 x max(E_oracle, eps x max valence)`` (faces_oracle.bound):
E_oracle is what float64 autograd through the oracle itself misses the reference by, eps x valence
the rounding of a sum of that many terms; the 8 covers the other summation order (eight partial
sums and a butterfly, or atomics in arrival order) and the hand-derived formula.  Nothing in the
bound comes from the device.  Every test prints its largest device error before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

import faces_oracle as fo
import faces_reference as fr

pytestmark = pytest.mark.gpu

CASES = sorted(fr.cases())
FORMS = ("build", "param")
SENTINEL = -7.25e300


def _dev(a, dtype=torch.float64):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype).cuda()


class _Mesh:
    """A case on the device, with its oracle forward (CPU) and its corner lists."""

    def __init__(self, name):
        from tensorflowraytrace_amd import ops
        m = self.host = fo.case(name)
        self.V, self.F = m["vertices"].shape[0], m["faces"].shape[0]
        self.vertices, self.zero = _dev(m["vertices"]), _dev(m["zero"])
        self.vectors, self.params = _dev(m["vectors"]), _dev(m["params"])
        self.faces = _dev(m["faces"], torch.int32)
        fv, norm = fo.oracle_forward(torch.tensor(m["vertices"]), m["faces"])
        self.fv_oracle, self.norm_oracle = fv.numpy(), norm.numpy()
        self.fv = _dev(self.fv_oracle)
        self.corners = ops.vertex_corners(self.faces, self.V)


_meshes = {}


def _mesh(name):
    if name not in _meshes:
        _meshes[name] = _Mesh(name)
    return _meshes[name]


def _same_bits(got, want):
    """Bit for bit, a NaN equal to a NaN whatever its payload."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)))


def _backward_cabi(mesh, form, g_fv, g_norm, mask, out, gather):
    """tfrt_{build,param}_faces_backward into ``out`` as it is; gather form or atomic form."""
    from tensorflowraytrace_amd import _lib, ops
    start, lst = mesh.corners if gather else (None, None)
    L, p = _lib.lib(), ops._p
    if form == "build":
        code = L.tfrt_build_faces_backward(p(g_fv), p(g_norm), p(mesh.fv), p(mesh.faces), p(mask),
                                           mesh.F, mesh.V, p(start), p(lst), p(out),
                                           ops._stream(out))
    else:
        code = L.tfrt_param_faces_backward(p(g_fv), p(g_norm), p(mesh.fv), p(mesh.faces), p(mask),
                                           p(mesh.vectors), mesh.F, mesh.V, p(start), p(lst),
                                           p(out), ops._stream(out))
    assert code == 0
    return out


def _out(mesh, form, fill):
    return torch.full((mesh.V, 3) if form == "build" else (mesh.V,), fill, dtype=torch.float64,
                      device="cuda")


def _backward_autograd(mesh, form, g_fv, g_norm, mask):
    from tensorflowraytrace_amd import ops
    if form == "build":
        x = mesh.vertices.clone().requires_grad_(True)
        fv, norm = ops.build_faces(x, mesh.faces, mask)
    else:
        x = mesh.params.clone().requires_grad_(True)
        fv, norm = ops.param_faces(x, mesh.zero, mesh.vectors, mesh.faces, mask)
    outs = [t for t, g in ((fv, g_fv), (norm, g_norm)) if g is not None]
    g, = torch.autograd.grad(outs, x, [g for g in (g_fv, g_norm) if g is not None])
    return g


def _check(got, ref, bound, what):
    """Non-finite where the reference is, within ``bound`` of it elsewhere.  -> relative error."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)), what
    err = fo.relative_error(got, ref)
    assert err <= bound, (what, err, bound)
    return err


def _untouched(mesh, mask):
    f = mesh.host["faces"]
    keep = np.ones_like(f, dtype=bool) if mask is None else mask.astype(bool)
    return np.bincount(f[keep], minlength=mesh.V) == 0


# ------------------------------------------------------------------------------------ forward

@pytest.mark.parametrize("name", CASES)
def test_forward_is_the_oracle_bit_for_bit(name):
    from tensorflowraytrace_amd import _lib, ops
    mesh = _mesh(name)
    fv, norm = ops.build_faces(mesh.vertices, mesh.faces)
    assert _same_bits(fv.cpu().numpy(), mesh.fv_oracle)
    assert _same_bits(norm.cpu().numpy(), mesh.norm_oracle)
    fv, norm = ops.param_faces(mesh.params, mesh.zero, mesh.vectors, mesh.faces)
    assert _same_bits(fv.cpu().numpy(), mesh.fv_oracle)
    assert _same_bits(norm.cpu().numpy(), mesh.norm_oracle)

    class Holder:
        pass
    h, batch = Holder(), ops.ParamFacesBatch()
    batch.add(h, mesh.params, mesh.zero, mesh.vectors, mesh.faces, None)
    batch.flush([h])
    assert _same_bits(h._face_verts.cpu().numpy(), mesh.fv_oracle)
    assert _same_bits(h._norm.cpu().numpy(), mesh.norm_oracle)
    assert _same_bits(batch.merged[0].cpu().numpy(), mesh.fv_oracle)
    # norm = NULL: the same face_verts, and nothing written past them -- face_verts is the head
    # of one sentinel-filled buffer whose tail is where a norm block would follow
    both = torch.full((mesh.F * 12,), SENTINEL, dtype=torch.float64, device="cuda")
    fv = both[:mesh.F * 9].view(mesh.F, 9)
    assert _lib.lib().tfrt_build_faces_forward(ops._p(mesh.vertices), mesh.V, ops._p(mesh.faces),
                                               mesh.F, ops._p(fv), None, ops._stream(fv)) == 0
    assert _same_bits(fv.cpu().numpy(), mesh.fv_oracle)
    assert bool((both[mesh.F * 9:] == SENTINEL).all())
    both.fill_(SENTINEL)
    assert _lib.lib().tfrt_param_faces_forward(
        ops._p(mesh.zero), ops._p(mesh.vectors), ops._p(mesh.params), mesh.V, ops._p(mesh.faces),
        mesh.F, ops._p(fv), None, ops._stream(fv)) == 0
    assert _same_bits(fv.cpu().numpy(), mesh.fv_oracle)
    assert bool((both[mesh.F * 9:] == SENTINEL).all())


def test_forward_nan_normals_are_exactly_the_zero_area_faces():
    from tensorflowraytrace_amd import ops
    mesh = _mesh("zero_area_F105_V40")
    _, rows = fr.zero_area(100, 40, 10)
    for norm in (ops.build_faces(mesh.vertices, mesh.faces)[1],
                 ops.param_faces(mesh.params, mesh.zero, mesh.vectors, mesh.faces)[1]):
        norm = norm.cpu().numpy()
        assert np.array_equal(np.nonzero(np.isnan(norm).any(axis=1))[0], rows)
        assert np.isnan(norm[rows]).all()
        good = np.delete(norm, rows, axis=0)
        assert np.abs(np.linalg.norm(good, axis=1) - 1.0).max() < 4 * fr.EPS64


# ------------------------------------------------------------------------------------ reverse

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CASES)
def test_reverse_gather_form_meets_the_longdouble_reference(name, form):
    mesh, bound = _mesh(name), fo.bound(name, form)
    worst = 0.0
    for (u, m), (g_fv, g_norm, mask) in fo.combos(mesh.host).items():
        ref = fo.reference(mesh.host, form, g_fv, g_norm, mask)
        g_fv_d, g_norm_d, mask_d = _dev(g_fv), _dev(g_norm), _dev(mask, torch.uint8)
        got = _backward_autograd(mesh, form, g_fv_d, g_norm_d, mask_d)
        worst = max(worst, _check(got, ref, bound, (u, m)))
        # OVERWRITTEN: every entry of a sentinel-filled buffer is written, twice the same bits
        direct = _backward_cabi(mesh, form, g_fv_d, g_norm_d, mask_d, _out(mesh, form, SENTINEL),
                                gather=True)
        assert _same_bits(direct.cpu().numpy(), got.cpu().numpy()), (u, m)
        again = _backward_cabi(mesh, form, g_fv_d, g_norm_d, mask_d, _out(mesh, form, 3.5),
                               gather=True)
        assert _same_bits(again.cpu().numpy(), got.cpu().numpy()), (u, m)
        # nothing arrives at an unreferenced or fully masked vertex: exactly 0.0
        idle = _untouched(mesh, mask)
        assert bool((direct.cpu().numpy()[idle] == 0.0).all()), (u, m)
        if m == "vertex_off":
            assert idle[int(np.argmax(fr.valence(mesh.host["faces"], mesh.V)))]
    print(f"faces reverse gather {name} {form}: device error {worst:.3e} bound {bound:.3e}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CASES)
def test_reverse_atomic_form_meets_the_reference_and_the_gather_form(name, form):
    mesh, bound = _mesh(name), fo.bound(name, form)
    rng = np.random.default_rng(77)
    worst = 0.0
    for (u, m), (g_fv, g_norm, mask) in fo.combos(mesh.host).items():
        ref = fo.reference(mesh.host, form, g_fv, g_norm, mask)
        g_fv_d, g_norm_d, mask_d = _dev(g_fv), _dev(g_norm), _dev(mask, torch.uint8)
        got = _backward_cabi(mesh, form, g_fv_d, g_norm_d, mask_d, _out(mesh, form, 0.0),
                             gather=False)
        worst = max(worst, _check(got, ref, bound, (u, m)))
        # ACCUMULATES: into a buffer that holds something already
        fill = rng.standard_normal(ref.shape)
        acc = _backward_cabi(mesh, form, g_fv_d, g_norm_d, mask_d, _dev(fill), gather=False)
        with np.errstate(invalid="ignore"):
            _check(acc, fill.astype(fr.LD) + ref, bound, (u, m, "accumulate"))
        idle = _untouched(mesh, mask)
        assert np.array_equal(acc.cpu().numpy()[idle], fill[idle]), (u, m)
        # the two forms agree (each is within the bound of the reference; so of each other)
        gather = _backward_cabi(mesh, form, g_fv_d, g_norm_d, mask_d, _out(mesh, form, SENTINEL),
                                gather=True).cpu().numpy()
        _check(got, gather.astype(fr.LD), bound, (u, m, "atomic against gather"))
    print(f"faces reverse atomic {name} {form}: device error {worst:.3e} bound {bound:.3e}")


def test_reverse_bad_arguments_and_empty_meshes():
    from tensorflowraytrace_amd import _lib, ops
    L, p = _lib.lib(), ops._p
    mesh = _mesh("fan_9")
    g_fv = torch.ones(mesh.F, 9, dtype=torch.float64, device="cuda")
    g_n = torch.ones(mesh.F, 3, dtype=torch.float64, device="cuda")
    start, lst = mesh.corners
    gv, gp = _out(mesh, "build", SENTINEL), _out(mesh, "param", SENTINEL)

    def build(g_fv=g_fv, g_n=g_n, fv=mesh.fv, start=start, lst=lst, F=mesh.F):
        return L.tfrt_build_faces_backward(p(g_fv), p(g_n), p(fv), p(mesh.faces), None, F, mesh.V,
                                           p(start), p(lst), p(gv), None)

    def param(g_fv=g_fv, g_n=g_n, fv=mesh.fv, start=start, lst=lst, F=mesh.F):
        return L.tfrt_param_faces_backward(p(g_fv), p(g_n), p(fv), p(mesh.faces), None,
                                           p(mesh.vectors), F, mesh.V, p(start), p(lst), p(gp), None)

    for call in (build, param):
        assert call(g_fv=None, g_n=None) == -1                      # both upstreams NULL
        assert call(fv=None) == -1                                  # grad_norm without face_verts
        assert call(start=None) == -1 and call(lst=None) == -1      # one corner pointer only
        assert call(F=-1) == -1
        assert call(F=0) == 0                                       # nothing to do, nothing written
        assert call(F=0, start=None, lst=None) == 0
    torch.cuda.synchronize()
    assert bool((gv == SENTINEL).all()) and bool((gp == SENTINEL).all())


# ------------------------------------------------------------------------------ host validates

def test_face_indices_are_validated_once_per_face_tensor(monkeypatch):
    from tensorflowraytrace_amd import ops
    from tensorflowraytrace_amd._lib import TfrtError
    mesh = _mesh("soup_F257_V33")
    monkeypatch.setattr(ops, "_corner_cache", {})
    calls = []
    check = ops._check_face_indices
    monkeypatch.setattr(ops, "_check_face_indices", lambda f, v: (calls.append(1), check(f, v)))

    class Holder:
        pass
    faces = mesh.faces.clone()
    # forward only (no gradient wanted), twice, then the other entry points: one validation
    ops.build_faces(mesh.vertices, faces)
    assert len(calls) == 1 and len(ops._corner_cache) == 1
    entry = next(iter(ops._corner_cache.values()))
    assert entry[0] is faces
    ops.build_faces(mesh.vertices, faces)
    ops.param_faces(mesh.params.clone().requires_grad_(True), mesh.zero, mesh.vectors, faces)
    batch = ops.ParamFacesBatch()
    batch.add(Holder(), mesh.params, mesh.zero, mesh.vectors, faces, None)
    batch.flush()
    assert len(calls) == 1 and len(ops._corner_cache) == 1
    assert next(iter(ops._corner_cache.values())) is entry
    for bad in (mesh.V, -1):
        wrong = mesh.faces.clone()
        wrong[100, 2] = bad
        with pytest.raises(TfrtError, match="vertex indices"):
            ops.build_faces(mesh.vertices, wrong)
        with pytest.raises(TfrtError, match="vertex indices"):
            ops.build_faces(mesh.vertices.clone().requires_grad_(True), wrong)
        with pytest.raises(TfrtError, match="vertex indices"):
            ops.param_faces(mesh.params, mesh.zero, mesh.vectors, wrong)
        with pytest.raises(TfrtError, match="vertex indices"):
            ops.ParamFacesBatch().add(Holder(), mesh.params, mesh.zero, mesh.vectors, wrong, None)
    assert len(ops._corner_cache) == 1


# -------------------------------------------------------------------------------------- multi

def _multi_layout(count):
    """Entries of the merged block: ("copy", rows) or ("param", case name).  Fixed surfaces
    first, in the middle and last; an empty surface in the middle; F = 255, 256, 257 and
    V = 31, 32, 33 on neighbouring surfaces.  The forward makes a descriptor of every entry, the
    reverse of every parametric surface that has faces, and a launch takes 8: nine entries run
    the forward in two chunks (the reverse in one, of five), and thirteen entries with nine
    parametric surfaces that have faces run both in two."""
    nine = [("copy", 5), ("param", "soup_F255_V31"), ("param", "soup_F256_V32"),
            ("param", "soup_F257_V33"), ("param", "empty"), ("copy", 7), ("param", "fan_9"),
            ("param", "zero_area_F105_V40"), ("copy", 3)]
    thirteen = nine[:8] + [("param", "fan_8"), ("param", "repeated_F50_V20"),
                           ("param", "soup_F1_V3"), ("param", "unreferenced_F40_V33"), nine[8]]
    return {1: nine[3:4], 8: nine[:6] + nine[7:], 9: nine, 13: thirteen}[count]


class _Holder:
    pass


@pytest.mark.parametrize("count", [1, 8, 9, 13])
def test_multi_surface_update_matches_the_oracle_and_the_longdouble_reference(count, monkeypatch):
    from tensorflowraytrace_amd import _lib, ops
    layout = _multi_layout(count)
    rng = np.random.default_rng(100 + count)
    batch, order, entries = ops.ParamFacesBatch(), [], []
    for kind, what in layout:
        h = _Holder()
        if kind == "copy":
            rows = rng.standard_normal((what, 9))
            h._face_verts = _dev(rows)
            h.__dict__["_face_verts_value"] = h._face_verts
            entries.append(dict(kind=kind, F=what, rows=rows))
        elif what == "empty":
            p = torch.zeros(3, dtype=torch.float64, device="cuda", requires_grad=True)
            batch.add(h, p, torch.zeros(3, 3, dtype=torch.float64, device="cuda"),
                      torch.ones(3, 3, dtype=torch.float64, device="cuda"),
                      torch.zeros(0, 3, dtype=torch.int32, device="cuda"), None)
            entries.append(dict(kind=kind, F=0, name=None, p=p, mask=None))
        else:
            mesh = _mesh(what)
            mask = fr.masks(mesh.host, 5)["mask"] if what.endswith("V32") else None
            p = mesh.params.clone().requires_grad_(True)
            batch.add(h, p, mesh.zero, mesh.vectors, mesh.faces, _dev(mask, torch.uint8))
            entries.append(dict(kind=kind, F=mesh.F, name=what, p=p, mask=mask))
        order.append(h)
    calls = {"tfrt_param_faces_forward_multi": [], "tfrt_param_faces_backward_multi": []}
    for fn_name, seen in calls.items():
        fn = getattr(_lib.lib(), fn_name)
        monkeypatch.setattr(_lib.lib(), fn_name,
                            lambda arr, n, stream, fn=fn, seen=seen: (seen.append(n), fn(arr, n, stream))[1])
    batch.flush(order)
    assert calls["tfrt_param_faces_forward_multi"] == {1: [1], 8: [8], 9: [8, 1], 13: [8, 5]}[count]
    block, rows = batch.merged
    at = 0
    for e, h, (_, r0, r1) in zip(entries, order, rows):
        assert (r0, r1) == (at, at + e["F"])
        e["at"], at = at, at + e["F"]
        part = block[r0:r1].detach().cpu().numpy()
        if e["kind"] == "copy":
            assert _same_bits(part, e["rows"])
        elif e["name"] is not None:
            mesh = _mesh(e["name"])
            assert _same_bits(part, mesh.fv_oracle)
            assert _same_bits(h._face_verts.detach().cpu().numpy(), mesh.fv_oracle)
            assert _same_bits(h._norm.detach().cpu().numpy(), mesh.norm_oracle)
        else:
            assert h._face_verts.shape == (0, 9) and h._norm.shape == (0, 3)
    assert block.shape == (at, 9)
    # gradients through the block, through a boundary's own rows and through the normals
    w = rng.standard_normal((at, 9))
    loss = (block * _dev(w)).sum()
    for e, h in zip(entries, order):
        if e["kind"] == "param" and e["name"] is not None:
            e["w_own"], e["w_norm"] = rng.standard_normal((e["F"], 9)), rng.standard_normal((e["F"], 3))
            loss = loss + (h._face_verts * _dev(e["w_own"])).sum() + (h._norm * _dev(e["w_norm"])).sum()
    pars = [e for e in entries if e["kind"] == "param"]
    grads = torch.autograd.grad(loss, [e["p"] for e in pars], retain_graph=True)
    # (every parametric surface that has faces is in the loss: chunks of 8 descriptors)
    assert calls["tfrt_param_faces_backward_multi"] == {1: [1], 8: [4], 9: [5], 13: [8, 1]}[count]
    for e, g in zip(pars, grads):
        if e["name"] is None:
            assert bool((g == 0.0).all())
            continue
        host = fo.case(e["name"])
        ref = fr.backward_params(host["zero"], host["vectors"], host["params"], host["faces"],
                                 w[e["at"]:e["at"] + e["F"]] + e["w_own"], e["w_norm"], e["mask"])
        err = _check(g, ref, fo.bound(e["name"], "param"), e["name"])
        print(f"faces multi {count} {e['name']}: device error {err:.3e}")
    # a loss on one surface alone: exact zeros for every other one, whichever output it goes
    # through -- also from and to the surface with zero-area faces (NaN normals)
    for k, (e, h) in enumerate(zip(entries, order)):
        if e["kind"] != "param" or e["name"] is None:
            continue
        for one in ((h._face_verts ** 2).sum(), (h._norm[:, 0]).sum(),
                    (block[e["at"]:e["at"] + e["F"]] * _dev(w[:e["F"]])).sum()):
            gs = torch.autograd.grad(one, [x["p"] for x in pars], retain_graph=True)
            for x, g in zip(pars, gs):
                g = g.cpu().numpy()
                if x is e:
                    assert bool((g != 0.0).any())
                else:
                    assert bool((g == 0.0).all()), (e["name"], x["name"])
