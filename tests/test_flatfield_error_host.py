"""
FlatFieldError without a GPU: the numpy restatement of the definition
(tests/flatfield_error_reference.py) against torch autograd of the plain objective (the foci
differentiated through ``torch.linalg.solve``), the CPU path of ``ops.flatfield_error`` against it
-- records equal as integers; table, plane, gradient and error bit for bit --, the properties of
the definition, the class (constructor, ``graph_key``, ``seed_columns``, the generic path, a term
of a ``SumError``), the C entry's refusals, and csrc/flatfield_math.h on the host:
tests/flatfield_host/flatfield_main.cpp (its own main) compiled with g++ and the address and
undefined-behaviour sanitizers.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import flatfield_error_reference as ff
import focus_error_reference as fr
from tensorflowraytrace_amd import ops, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "flatfield_host", "flatfield_main.cpp")

COUNTS = (0, 1, 63, 64, 65, 1000, 20000)


def has_plane(n, G):
    """Which cases of the generator have a plane: with fewer rays than groups every label occurs
    once at most and no group has a focus -- the cases about having none."""
    return n > G


def _axis(dim):
    return ff.AXIS3 if dim == 3 else ff.AXIS2


@pytest.mark.parametrize("G", [3, 7, 256, 257])
def test_the_generator_keeps_its_guard(G):
    for n in COUNTS:
        for dim in (2, 3):
            for dtype in (np.float64, np.float32):
                for masked, permuted in ((False, False), (True, True)):
                    ref = ff.case(n, G, dtype, dim, permuted, masked, plane=has_plane(n, G))[4]
                    if n >= 63 and has_plane(n, G):
                        # some group is left without a focus (the parallel one), some ray without
                        # a gradient, and the plane is not degenerate
                        assert not ref["used"].all() and 0 < ref["has"].sum() < n
                        assert ref["error"] > 0.0 and np.abs(ref["grad"]).max() > 0.0


# ------------------------------------------------------------ against the plain objective
def converging(n_groups, per, dim, seed=3, noise=0.01):
    """(block, label): ``per`` noisy lines through each of ``n_groups`` points of the box
    ``DOMAIN``, float64, every column counting."""
    rng = np.random.default_rng(seed + dim)
    centre = np.array([(a + b) / 2 for a, b in ff.DOMAIN])[:dim]
    focus = centre[:, None] + rng.uniform(-0.4, 0.4, (dim, n_groups))
    label = np.repeat(np.arange(n_groups), per)
    n = label.shape[0]
    u = np.concatenate([np.ones((1, n)), rng.normal(0, .3, (dim - 1, n))])
    u /= np.sqrt((u * u).sum(axis=0))
    end = focus[:, label] + rng.uniform(-0.5, 0.5, n) * u + rng.normal(0, noise, (dim, n))
    start = end - u * rng.uniform(.5, 3, n)
    return np.ascontiguousarray(np.concatenate([start, end])), label


def torch_objective(block, label, n_groups, used, axis):
    """The plain objective in torch float64, in the scene's own coordinates: per used group
    A = sum P, b = sum P e, X = solve(A, b) -- differentiated through --, h = a . X; the plane's
    height is the mean of h weighted by the ray counts, and the error the sum over the groups of
    count * (h - mean)^2.  ``label``: the group of every column that counts, -1 otherwise."""
    d = block.shape[0] // 2
    v = block[d:] - block[:d]
    u = v / torch.sqrt((v * v).sum(dim=0))
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / torch.sqrt((a * a).sum())
    eye = torch.eye(d, dtype=torch.float64)
    hs, ns = [], []
    for k in range(n_groups):
        if not used[k]:
            continue
        at = torch.nonzero(torch.as_tensor(label == k))[:, 0]
        uk, ek = u[:, at], block[d:, at]
        P = eye[:, :, None] - uk[:, None, :] * uk[None, :, :]            # (d, d, n_k)
        X = torch.linalg.solve(P.sum(dim=2), torch.einsum("abi,bi->a", P, ek))
        hs.append((a * X).sum())
        ns.append(float(at.numel()))
    if len(hs) < 2:
        return block.sum() * 0.0
    h, n = torch.stack(hs), torch.tensor(ns, dtype=torch.float64)
    hbar = (n * h).sum() / n.sum()
    return (n * (h - hbar) ** 2).sum()


def quantisation_difference(block, label, n_groups, domain, axis, min_det):
    """(largest |reference gradient - autograd gradient| / largest |autograd gradient|, relative
    difference of the errors) between the reference (int64 records) and the plain objective on
    columns that all count."""
    ref = ff.flatfield_error(block, label.astype(np.int32), n_groups, domain, axis,
                             min_det=min_det)
    assert ref["focus"]["counts"].all() and ref["valid"]
    t = torch.tensor(block, requires_grad=True)
    e = torch_objective(t, label, n_groups, ref["used"], axis)
    g, = torch.autograd.grad(e, t)
    g = g.numpy()
    return (float(np.abs(ref["grad"] - g).max() / np.abs(g).max()),
            abs(ref["error"] - float(e.detach())) / float(e.detach()))


# measured on the CPU on ``converging(3, 50, dim)``: (gradient, error) relative differences
MEASURED = {3: (2.134e-12, 6.804e-13), 2: (1.543e-12, 7.429e-13)}


@pytest.mark.parametrize("dim", [2, 3])
def test_reference_equals_autograd_of_the_plain_objective(dim):
    """3 groups x 50 rays.  The reference works on quantised records (pbits = 40 at 150 source
    rays: entries of A and b are off by up to 2**-41 each, relative to a box of R = 1.75) and
    applies the hand-derived adjoint; torch differentiates the plain float64 objective through
    ``torch.linalg.solve``.  The difference is the quantisation of the records amplified by
    1 / det, on the foci and so on the residuals r, relative to residuals of a few 0.1.  Measured
    on the CPU on these inputs (``MEASURED``): the largest difference of a gradient entry relative
    to the largest entry was 2.134e-12 in 3-D and 1.543e-12 in 2-D, the relative difference of the
    errors 6.804e-13 and 7.429e-13; asserted is 8 x the measured value, as margin for other
    seeds."""
    block, label = converging(3, 50, dim)
    rel, rel_e = quantisation_difference(block, label, 3, ff.DOMAIN, _axis(dim), ff.MIN_DET)
    print(f"{dim}-D: gradient rel diff {rel:.3e}, error rel diff {rel_e:.3e}")
    assert rel <= 8 * MEASURED[dim][0] and rel_e <= 8 * MEASURED[dim][1]


def test_a_translated_group_sums_to_the_adjoint_of_its_focus():
    """Moving every ray of a group by one vector moves its focus by that vector: the gradient
    rows of the group's rays (start + end) sum to d error / d focus = 2 R n r a."""
    block, label = converging(4, 40, 3)
    ref = ff.flatfield_error(block, label.astype(np.int32), 4, ff.DOMAIN, ff.AXIS3)
    for k in range(4):
        total = (ref["grad"][:3] + ref["grad"][3:])[:, label == k].sum(axis=1)
        want = 2.0 * 40 * ref["residuals"][k] * ref["a"]
        assert np.abs(total - want).max() <= 1e-9 * np.abs(want).max()


# ------------------------------------------------------------ the ops CPU path
def _evaluate(block, mask, group, perm, G, dim, pad=0, axis=None, **kw):
    """ops.flatfield_error on the CPU over the block with ``pad`` spare columns."""
    n = block.shape[1]
    wide = torch.full((2 * dim, n + pad), 7.0, dtype=torch.as_tensor(block).dtype)
    wide[:, :n] = torch.as_tensor(block)
    return ops.flatfield_error(wide[:, :n], torch.as_tensor(group), G,
                               ops.focus_grid(ff.DOMAIN[:dim]), axis or _axis(dim), ff.MIN_DET,
                               mask=None if mask is None else torch.as_tensor(mask),
                               perm=None if perm is None else torch.as_tensor(perm),
                               dimension=dim, **kw)


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(
        ((got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))).all())


def check(out, ref):
    """Records as integers; table, plane, gradient and error bit for bit."""
    err, grad, acc, table, fit = (np.asarray(o) for o in out)
    assert acc.dtype == np.int64 and np.array_equal(acc, ref["acc"])
    assert same_bits(table, ref["table"]), np.nonzero(table != ref["table"])
    assert same_bits(fit, ref["fit"]), (fit, ref["fit"])
    assert same_bits(grad, ref["grad"])
    assert same_bits(err, [ref["error"], ref["terms"], ref["mean"]]), (err, ref["error"])
    if not ref["valid"]:
        assert err[0] == 0.0 and not grad.any() and not table[:, 4:].any()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("masked,permuted", [(False, False), (True, True), (True, False),
                                             (False, True)])
@pytest.mark.parametrize("n,G", [(0, 3), (1, 3), (63, 3), (64, 7), (65, 7), (1000, 7),
                                 (1000, 257), (20000, 256), (5000, 2100)])
def test_cpu_path_equals_the_reference(n, G, masked, permuted, dim):
    """(2,100 groups: the third trip of the threads over the groups.)"""
    for dtype in (np.float64, np.float32):
        block, mask, group, perm, ref = ff.case(n, G, dtype, dim, permuted, masked,
                                                plane=has_plane(n, G))
        mask, perm = (mask if masked else None), (perm if permuted else None)
        out = _evaluate(block, mask, group, perm, G, dim, pad=3)
        check([o.numpy() for o in out], ref)


def test_reused_buffers_and_another_stride_give_the_same_bits():
    n, G = 1000, 7
    block, _, group, _, ref = ff.case(n, G)
    out = _evaluate(block, None, group, None, G, 3)
    again = _evaluate(block, None, group, None, G, 3, pad=5,
                      grad=torch.full((6, n), np.nan, dtype=torch.float64),
                      acc=out[2].clone().fill_(5), table=out[3].clone().fill_(3.0),
                      fit_out=out[4].clone().fill_(2.0))
    for a, b in zip(out, again):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    terms = ops.flatfield_terms(torch.as_tensor(block), torch.as_tensor(group), G,
                                ops.focus_grid(ff.DOMAIN), out[3])
    assert same_bits(terms.numpy(), ref["term"])
    assert abs(float(terms.sum()) - ref["error"]) <= n * ff.EPS * ref["error"]


# ------------------------------------------------------------ properties
def test_the_weighted_residuals_sum_to_zero():
    """hbar minimises the sum: sum n r = 0 within the rounding of the sums, G eps sum n |r|."""
    for n, G, dim in ((1000, 7, 3), (20000, 256, 2), (5000, 2100, 3)):
        ref = ff.case(n, G, np.float64, dim)[4]
        u = ref["used"]
        cnt = ref["acc"][u, 0].astype(np.float64)
        r = ref["residuals"][u] / ref["R"]
        assert abs((cnt * r).sum()) <= 4 * G * ff.EPS * (cnt * np.abs(r)).sum()
        assert np.isnan(ref["residuals"][~u]).all()


def test_moving_a_group_along_the_axis_moves_its_height():
    block, label = converging(3, 50, 3)
    a = ff.axis_of(ff.AXIS3, 3)
    t = 0.0625
    moved = block.copy()
    moved[:, label == 1] += t * np.concatenate([a, a])[:, None]
    h0 = ff.flatfield_error(block, label.astype(np.int32), 3, ff.DOMAIN, ff.AXIS3)["heights"]
    h1 = ff.flatfield_error(moved, label.astype(np.int32), 3, ff.DOMAIN, ff.AXIS3)["heights"]
    # (the records are quantised to 2**-40 of the box: the foci move by t up to that, amplified
    # by 1 / det of a well-conditioned group)
    assert abs((h1[1] - h0[1]) - t) <= 1e-9
    assert np.abs(h1[[0, 2]] - h0[[0, 2]]).max() == 0.0


@pytest.mark.parametrize("what", ["one_ray", "two_rays", "collimated", "excluded"])
def test_a_group_without_a_focus_contributes_nothing(what):
    """Four groups; the fourth holds fewer than two rays, two rays along the same line (two lines
    that cross do have a focus), collimated rays, or is labelled -1: the result is that of the
    three other groups alone, and the fourth's rays get zeros."""
    block, label = converging(4, 40, 3)
    label = label.astype(np.int32)
    last = label == 3
    if what in ("one_ray", "two_rays"):
        keep = ~last
        keep[np.nonzero(last)[0][:1 if what == "one_ray" else 2]] = True
        block, label = block[:, keep].copy(), label[keep]
        last = label == 3
        if what == "two_rays":
            first, second = np.nonzero(last)[0]
            d = block[3:, first] - block[:3, first]
            block[:3, second] = block[:3, first] + 0.25 * d
            block[3:, second] = block[3:, first] - 0.25 * d
    elif what == "collimated":
        d = np.array([1.0, 0.2, -0.1])
        block[:3, last] = block[3:, last] - d[:, None]
    else:
        label = np.where(last, -1, label).astype(np.int32)
    ref = ff.flatfield_error(block, label, 4, ff.DOMAIN, ff.AXIS3)
    alone = ff.flatfield_error(block[:, ~last], label[~last], 4, ff.DOMAIN, ff.AXIS3)
    assert not ref["used"][3] and ref["n_used"] == 3 and ref["valid"]
    assert ref["error"] == alone["error"] and ref["terms"] == alone["terms"] == 120.0
    assert same_bits(ref["fit"], alone["fit"])
    assert same_bits(ref["grad"][:, ~last], alone["grad"]) and not ref["grad"][:, last].any()
    assert np.isnan(ref["table"][3, :3]).all() and not ref["table"][3, 3:].any()
    out = ops.flatfield_error(torch.as_tensor(block), torch.as_tensor(label), 4,
                              ops.focus_grid(ff.DOMAIN), ff.AXIS3, ff.MIN_DET)
    check([o.numpy() for o in out], ref)


def test_one_used_group_gives_no_plane():
    """Zero error, zero gradient, the terms counted, the focus still reported."""
    block, label = converging(1, 60, 3)
    ref = ff.flatfield_error(block, label.astype(np.int32), 3, ff.DOMAIN, ff.AXIS3)
    assert ref["n_used"] == 1 and not ref["valid"]
    assert ref["error"] == 0.0 and ref["terms"] == 60.0 and ref["mean"] == 0.0
    assert not ref["grad"].any() and np.isfinite(ref["table"][0, :3]).all()
    assert ref["residuals"][0] == 0.0 and np.isnan(ref["residuals"][1:]).all()
    out = ops.flatfield_error(torch.as_tensor(block), torch.as_tensor(label.astype(np.int32)), 3,
                              ops.focus_grid(ff.DOMAIN), ff.AXIS3, ff.MIN_DET)
    check([o.numpy() for o in out], ref)
    assert ops.flatfield_terms(torch.as_tensor(block), torch.as_tensor(label.astype(np.int32)), 3,
                               ops.focus_grid(ff.DOMAIN), out[3]).sum() == 0.0
    # no group at all: NaN mean, NaN height
    none = ops.flatfield_error(torch.as_tensor(block[:, :1]), torch.zeros(1, dtype=torch.int32), 3,
                               ops.focus_grid(ff.DOMAIN), ff.AXIS3, ff.MIN_DET)
    assert float(none[0][0]) == 0.0 and float(none[0][1]) == 0.0 and np.isnan(float(none[0][2]))
    assert np.isnan(float(none[4][0])) and float(none[4][4]) == 0.0


def test_masks_and_permutations_select_and_relabel():
    """A masked column is as good as absent; a permutation looks the labels up through the
    source-ray index."""
    n, G = 1000, 7
    block, mask, group, perm, ref = ff.case(n, G, masked=True)
    on = mask >= 0
    # (source ray i is column i without perm: the labels of the remaining columns)
    alone = ff.flatfield_error(block[:, on], group, G, ff.DOMAIN, ff.AXIS3,
                               perm=np.nonzero(on)[0].astype(np.int32))
    assert ref["error"] == alone["error"] and same_bits(ref["grad"][:, on], alone["grad"])
    assert not ref["grad"][:, ~on].any()
    block, mask, group, perm, ref = ff.case(n, G, permuted=True)
    ok = (perm >= 0) & (perm < group.shape[0])
    direct = ff.flatfield_error(block[:, ok], group[perm[ok]], G, ff.DOMAIN, ff.AXIS3)
    assert ref["error"] == direct["error"] and same_bits(ref["grad"][:, ok], direct["grad"])


# ------------------------------------------------------------ ops and class arguments
def test_ops_argument_errors():
    rows = torch.zeros((6, 5), dtype=torch.float64)
    g = torch.zeros(5, dtype=torch.int32)
    grid = ops.focus_grid(ff.DOMAIN)
    a = ops.flatfield_axis((3.0, 0.0, 4.0))
    assert a == (0.6, 0.0, 0.8) and ops.flatfield_axis((0.0, -2.0), 2) == (0.0, -1.0, 0.0)
    assert np.array_equal(ops.flatfield_axis(ff.AXIS3), ff.axis_of(ff.AXIS3, 3))
    for bad in ((1.0, 0.0), (0.0, 0.0, 0.0), (1.0, float("nan"), 0.0), (1.0, float("inf"), 0.0),
                "xyz", 3.0):
        with pytest.raises(ValueError, match="axis"):
            ops.flatfield_axis(bad)
    ok = dict(rows=rows, groups=g, n_groups=3, grid=grid, axis=(1.0, 0.0, 0.0), min_det=1e-6)
    for bad, match in ((dict(groups=g.long()), "groups"), (dict(n_groups=0), "n_groups"),
                       (dict(n_groups=2 ** 20 + 1), "n_groups"), (dict(rows=rows[:4]), "rows"),
                       (dict(dimension=4), "rows"), (dict(grid=grid[:6]), "grid"),
                       (dict(axis=(1.0, 0.0)), "axis"), (dict(axis=(0.0, 0.0, 0.0)), "axis"),
                       (dict(min_det=0.0), "min_det"), (dict(min_det=float("nan")), "min_det"),
                       (dict(variant=3), "variant"), (dict(n_groups=257, variant=1), "variant"),
                       (dict(mask=torch.zeros(5)), "mask"),
                       (dict(perm=torch.zeros(4, dtype=torch.int32)), "perm"),
                       (dict(grad=torch.zeros((4, 5), dtype=torch.float64)), "grad"),
                       (dict(acc=torch.zeros((3, 4), dtype=torch.int64)), "acc"),
                       (dict(table=torch.zeros((3, 4), dtype=torch.float64)), "table"),
                       (dict(fit_out=torch.zeros(4, dtype=torch.float64)), "fit_out")):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.flatfield_error(**kw)


def test_the_class_checks_its_arguments():
    import tfrt.optimizer
    from tensorflowraytrace_amd import errors, fused_step
    F = optimizer.FlatFieldError
    assert tfrt.optimizer.FlatFieldError is F and fused_step.FlatFieldError is F
    assert errors.FlatFieldError is F and F in errors._COUPLED
    assert issubclass(F, errors._CoupledError)
    lab = np.arange(12) % 4
    erf = F(lab, ff.DOMAIN)
    assert erf.axis == (1.0, 0.0, 0.0) and erf.unit_axis == (1.0, 0.0, 0.0)
    assert erf.n_groups == 4 and erf.labels.dtype == torch.int32 and erf.min_det == 1e-12
    assert erf.rows == [0, 1, 2, 3, 4, 5] and erf.seed_rows == 0x3f and erf.on_columns
    assert erf.has_direction and erf.rows_for(3) == erf.rows
    flat = F(torch.tensor(lab), ff.DOMAIN[:2], n_groups=9, min_det=1e-6)
    assert flat.axis == (1.0, 0.0) and flat.unit_axis == (1.0, 0.0, 0.0)
    assert flat.n_groups == 9 and flat.rows_for(2) == [0, 1, 2, 3]
    assert F(lab, ff.DOMAIN, axis=(0.0, 3.0, 4.0)).unit_axis == (0.0, 0.6, 0.8)
    with pytest.raises(ValueError, match="FlatFieldError.*2-D engine"):
        erf.rows_for(2)
    with pytest.raises(ValueError, match="FlatFieldError.*3-D engine"):
        flat.rows_for(3)
    for bad in (dict(domain=ff.DOMAIN[:1]), dict(domain=((1.0, 1.0),) * 3), dict(domain=None),
                dict(axis=(1.0, 0.0)), dict(axis=(0.0, 0.0, 0.0)), dict(axis=(1.0, 0.0, 0.0, 0.0)),
                dict(axis=(float("nan"), 0.0, 1.0)), dict(axis="x"), dict(axis=2.0),
                dict(domain=ff.DOMAIN[:2], axis=(1.0, 0.0, 0.0)),
                dict(min_det=0.0), dict(min_det=float("nan")), dict(min_det="small"),
                dict(groups=np.zeros((3, 2), dtype=np.int64)), dict(groups=np.zeros(3)),
                dict(groups=lambda src: lab), dict(groups=np.zeros(0, dtype=np.int64)),
                dict(n_groups=0), dict(n_groups=2 ** 20 + 1), dict(n_groups="many")):
        kw = dict(groups=lab, domain=ff.DOMAIN)
        kw.update(bad)
        with pytest.raises(ValueError, match="FlatFieldError"):
            F(**kw)
    with pytest.raises(TypeError):
        F(lab, ff.DOMAIN, weights=np.ones(12))
    for read in (erf.foci, erf.heights, erf.residuals, erf.plane):
        with pytest.raises(RuntimeError, match="FlatFieldError: no evaluation"):
            read()
    # graph_key: a FocusError's, and the axis
    k0 = erf.graph_key()
    assert k0[:-1] == errors.FocusError.graph_key(erf) and k0[-1] == (1.0, 0.0, 0.0)
    assert F(lab, ff.DOMAIN, axis=(0.0, 1.0, 0.0)).graph_key()[-1] == (0.0, 1.0, 0.0)
    other = F(lab, ff.DOMAIN, axis=(0.0, 1.0, 0.0))
    other.labels = erf.labels
    assert other.graph_key() != k0 and other.graph_key()[:-1] == k0[:-1]
    # a legal term of a SumError beside a FocusError
    focus = optimizer.FocusError(lab, ff.DOMAIN)
    both = optimizer.SumError([focus, erf], reduce="mean")
    assert both.terms == (focus, erf) and both.rows == [0, 1, 2, 3, 4, 5] * 2
    with pytest.raises(ValueError, match="FlatFieldError"):
        optimizer.SumError([erf, object()])

    class _Eng:
        dimension, ray_shard = 2, None

        @staticmethod
        def _custom_ops():
            return False

    class _Opt:
        engine, error_function = _Eng(), flat
    assert fused_step.FusedStep.eligible2d(_Opt()) is False


def test_seed_columns_equals_a_direct_call():
    """The fused step's protocol on CPU tensors: ``seed_columns`` fills the holder's seed block,
    error triple and buffers with what ``ops.flatfield_error`` gives on the same columns."""
    import types
    from tensorflowraytrace_amd import errors
    n, G = 1000, 7
    block, mask, group, perm, ref = ff.case(n, G, permuted=True, masked=True)
    erf = optimizer.FlatFieldError(group, ff.DOMAIN, axis=ff.AXIS3, n_groups=G,
                                   min_det=ff.MIN_DET)
    erf.labels = erf.labels.cpu()
    src = {"x_start": torch.zeros(group.shape[0])}
    cols = errors._Columns(torch.as_tensor(block), torch.as_tensor(mask), torch.as_tensor(perm),
                           src, n)
    hold = types.SimpleNamespace(g_fin=torch.full((6, n), np.nan, dtype=torch.float64),
                                 err=torch.zeros(3, dtype=torch.float64), buffers={})
    calls = []
    lib = types.SimpleNamespace(
        tfrt_flatfield_error_workspace_bytes=lambda n_, g_: calls.append((n_, g_)) or 256)
    orig = errors._lib.lib
    errors._lib.lib = lambda: lib
    try:
        erf.seed_columns(cols, hold)
        first = dict(hold.buffers)
        erf.seed_columns(cols, hold)
    finally:
        errors._lib.lib = orig
    assert calls == [(n, G)] and set(first) == {"workspace", "acc", "table", "fit_out"}
    assert all(hold.buffers[k] is first[k] for k in first)
    check([hold.err.numpy(), hold.g_fin.numpy(), first["acc"].numpy(), first["table"].numpy(),
           first["fit_out"].numpy()], ref)
    assert erf.last_acc is first["acc"] and erf.last_table is first["table"]
    p = erf.plane()
    assert p == dict(axis=tuple(ref["a"]), offset=ref["offset"], valid=True,
                     groups_used=ref["n_used"])
    assert same_bits(erf.residuals().numpy(), ref["residuals"])
    assert np.allclose(erf.heights().numpy(), ref["heights"], rtol=0, atol=1e-14, equal_nan=True)
    assert np.array_equal(erf.foci().numpy(), ref["foci"], equal_nan=True)


class _Engine:
    def __init__(self, block, ids, n_source, dim):
        names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end") if dim == 3 \
            else ("x_start", "y_start", "x_end", "y_end")
        self.dimension = dim
        self.leaves = [torch.tensor(r, requires_grad=True) for r in block]
        self.finished_rays = dict(zip(names, self.leaves))
        self.last_trace = {"finished_id": torch.tensor(ids)}
        self._trace_src = {"x_start": torch.zeros(n_source)}


@pytest.mark.parametrize("dim", [2, 3])
def test_the_generic_path_returns_the_terms_and_the_gradient_rows(dim):
    n, G = 300, 7
    block, _, group, perm, ref = ff.case(n, G, np.float64, dim, permuted=True)
    erf = optimizer.FlatFieldError(group, ff.DOMAIN[:dim], axis=_axis(dim), n_groups=G,
                                   min_det=ff.MIN_DET)
    erf.labels = erf.labels.cpu()
    eng = _Engine(block, perm, group.shape[0], dim)
    e = erf(eng)
    assert e.shape == (n, 1) and e.dtype == torch.float64
    (3.0 * e.sum()).backward()
    assert same_bits(e.detach().numpy()[:, 0], ref["term"])
    assert abs(float(e.detach().sum()) - ref["error"]) <= n * ff.EPS * ref["error"]
    assert np.array_equal(erf.last_acc.numpy(), ref["acc"])
    for leaf, want in zip(eng.leaves, ref["grad"]):
        assert np.array_equal(leaf.grad.numpy(), 3.0 * want)
    f = erf.foci().numpy()
    assert f.shape == (G, dim) and np.array_equal(f, ref["foci"], equal_nan=True)
    assert same_bits(erf.residuals().numpy(), ref["residuals"])
    assert erf.plane()["valid"] and erf.plane()["groups_used"] == ref["n_used"]
    assert erf.plane()["offset"] == ref["offset"] and len(erf.plane()["axis"]) == dim
    eng.finished_rays = {}
    assert erf(eng).shape == (0, 1)
    with pytest.raises(ValueError, match="engine"):
        eng3 = _Engine(block, perm, group.shape[0], dim)
        eng3.dimension = 5 - dim
        erf(eng3)


def _lens(n_rays):
    from test_host_logic import _lens_api
    eng, system, lens, target = _lens_api(n_rays)
    groups = np.arange(n_rays) % 5
    box = ((9.0, 11.0), (-5.0, 5.0), (-5.0, 5.0))           # the target plane is x = 10
    return eng, lens, groups, box


def test_the_optimiser_takes_the_generic_path_on_the_cpu_backend(cpu_backend):
    """SGD_Optimizer with a FlatFieldError on the oracle-backed CPU stand-ins: the step's error is
    the reference's on the traced rays, the parameter gradient is that of the plain torch objective
    under autograd through the same trace, and a few steps lower the error.  The tolerance is the
    1e-9 tests/test_focus_error_host.py applies to the same comparison, or 8 x the quantisation
    difference between the reference and the plain objective on these finished rays, whichever is
    larger (measured on the CPU: 8.2e-10 on the rays, 5.9e-10 on the parameters)."""
    eng, lens, groups, box = _lens(200)
    erf = optimizer.FlatFieldError(groups, box, min_det=ff.MIN_DET)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=2e-3, grad_clip=1e9)
    grads, err_sum, n_terms = opt.raw_gradient()
    assert opt._fused_step is None
    fin = eng.finished_rays
    names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
    block = np.stack([fin[k].detach().numpy() for k in names])
    ids = eng.last_trace["finished_id"].numpy()
    ref = ff.flatfield_error(block, groups, 5, box, (1.0, 0.0, 0.0), perm=ids)
    assert ref["terms"] > 150 and ref["used"].all() and n_terms == block.shape[1]
    assert abs(float(err_sum) - ref["error"]) <= block.shape[1] * ff.EPS * ref["error"]
    assert same_bits(erf.residuals().numpy(), ref["residuals"])
    eng.clear_ray_history()
    eng.optical_system.update()
    eng.ray_trace(3)
    fin = eng.finished_rays
    assert np.array_equal(eng.last_trace["finished_id"].numpy(), ids)
    t = torch.stack([fin[k] for k in names]).double()
    label = np.where(ref["counts"], ref["focus"]["label"], -1)
    e = torch_objective(t, label, 5, ref["used"], (1.0, 0.0, 0.0))
    want = torch.autograd.grad(e, lens.parameters, retain_graph=True)
    on_rays, = torch.autograd.grad(e, t)
    quant = float(np.abs(ref["grad"] - on_rays.numpy()).max() / on_rays.abs().max())
    tol = max(1e-9, 8 * quant)
    print(f"quantisation difference on the finished rays {quant:.2e}, tolerance {tol:.2e}")
    for g, w in zip(grads, want):
        rel = float((g - w).abs().max()) / float(w.abs().max())
        print(f"parameter gradient rel diff {rel:.2e}")
        assert rel <= tol
    errs = [float(opt.single_step(None)) for _ in range(6)]
    print("errors:", errs)
    assert errs[-1] < errs[0]


def test_a_sum_with_a_focus_error_runs_on_the_cpu_backend(cpu_backend):
    eng, lens, groups, box = _lens(200)
    focus = optimizer.FocusError(groups, box, min_det=ff.MIN_DET)
    flat = optimizer.FlatFieldError(groups, box, min_det=ff.MIN_DET)
    both = optimizer.SumError([focus, flat], weights=[1.0, 0.5], reduce="mean")
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, both, 3, learning_rate=1e-3, grad_clip=1e9)
    e = float(opt.single_step(None))
    triples = both.last_errors.numpy()
    assert triples.shape == (2, 3) and triples[0, 1] > 150 and triples[1, 1] == triples[0, 1]
    assert abs(e - (triples[0, 2] + 0.5 * triples[1, 2])) <= 1e-12 * abs(e)
    assert flat.foci().shape == (5, 3) and flat.plane()["valid"]
    assert np.array_equal(flat.last_acc.numpy(), focus.last_acc.numpy())
    assert np.array_equal(flat.foci().numpy(), focus.foci().numpy())


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    L = _lib.lib()
    assert L.tfrt_version() == 107
    assert L.tfrt_flatfield_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_flatfield_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_flatfield_error_workspace_bytes(-1, 4) == 0
    assert 0 < L.tfrt_flatfield_error_workspace_bytes(0, 4) \
        <= L.tfrt_flatfield_error_workspace_bytes(1_000_000, 2 ** 20)
    dummy = ctypes.create_string_buffer((1 << 17) + 64)
    base = ctypes.addressof(dummy)
    p = ctypes.c_void_p((base + 63) // 64 * 64)               # 64-byte aligned

    def call(n=8, G=4, dim=3, x1=1.0, y1=1.0, z1=1.0, ws=1 << 17, stride=8, gstride=8, variant=0,
             group=p, dtype=1, pbits=40, n_source=8, acc=p, table=p, fit=p, err=p, min_det=1e-6,
             axis=(0.6, 0.0, 0.8)):
        return L.tfrt_flatfield_error(p, stride, n, dtype, dim, None, group, n_source, None, G,
                                      0.0, x1, 0.0, y1, 0.0, z1, pbits, min_det, *axis, p, gstride,
                                      err, acc, table, fit, variant, p, ws, None)
    up = float(np.nextafter(1.0, 2.0))
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(dim=1), dict(dim=4),
                dict(x1=0.0), dict(y1=float("nan")), dict(z1=float("inf")), dict(z1=-1.0),
                dict(stride=4), dict(gstride=4), dict(variant=3), dict(group=None),
                dict(n=1 << 31), dict(dtype=7), dict(G=257, variant=1), dict(pbits=41),
                dict(pbits=0), dict(n=1 << 21, pbits=40, stride=1 << 21, gstride=1 << 21),
                dict(n_source=-1), dict(acc=None), dict(table=None), dict(fit=None),
                dict(err=None), dict(min_det=0.0), dict(min_det=float("nan")),
                dict(table=ctypes.c_void_p(p.value + 8)), dict(table=ctypes.c_void_p(p.value + 32)),
                dict(axis=(0.0, 0.0, 0.0)), dict(axis=(1.0, 0.0, 1e-6)), dict(axis=(2.0, 0.0, 0.0)),
                dict(axis=(float("nan"), 0.0, 1.0)), dict(axis=(float("inf"), 0.0, 0.0)),
                dict(axis=(1.0 + 16 * ff.EPS, 0.0, 0.0)), dict(dim=2, axis=(0.6, 0.0, 0.8))):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    # a few ulp are let through; (z1 and the axis' z are not looked at in 2-D)
    assert call(ws=8, axis=(up, 0.0, 0.0)) == -2
    assert call(dim=2, z1=-1.0, ws=8, axis=(0.6, 0.8, 5.0)) == -2


# ------------------------------------------------------------ flatfield_math.h on the host
def _pack(n, dim, G, pbits, box, min_det, axis, e, u, L, counts, label):
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).tobytes()       # noqa: E731
    lo, hi, c, R, iR = box
    pad = lambda v: list(v) + [0.0] * (3 - len(v))                         # noqa: E731
    return (struct.pack("<4q", n, dim, G, pbits)
            + f8(pad(lo) + pad(hi) + pad(c) + [R, iR, min_det] + list(axis))
            + f8(e) + f8(u) + f8(L) + i4(counts) + i4(label))


def test_flatfield_math_on_the_host_under_the_sanitizers(tmp_path):
    """The records, the (G, 8) table, the plane, the error triple and every ray's gradient of
    flatfield_math.h (over focus_math.h) equal the reference's bit for bit, in both dimensions,
    from float32 and float64 rows, with and without a plane and over more than 1,024 groups; the
    program's vectors are exact-size allocations and it runs under the address and
    undefined-behaviour sanitizers.  Nothing is loaded into this process."""
    exe = tmp_path / "flatfield_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    for n, G, dim, dtype in ((257, 7, 3, np.float64), (1000, 7, 2, np.float32),
                             (64, 3, 3, np.float32), (3000, 257, 2, np.float64),
                             (5000, 2100, 3, np.float64), (300, 257, 3, np.float64),
                             (200, 257, 3, np.float64),
                             (1, 3, 3, np.float64), (0, 3, 2, np.float64)):
        block, mask, group, perm, ref = ff.case(n, G, dtype, dim, permuted=True, masked=True,
                                                plane=has_plane(n, G))
        f = ref["focus"]
        e = block[dim:].astype(np.float64)
        box = fr.box_of(ff.DOMAIN[:dim])
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(_pack(n, dim, G, f["pbits"], box, ff.MIN_DET, ref["a"], e, f["u"], f["L"],
                              f["counts"], np.clip(f["label"], 0, G - 1)))
        run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert run.returncode == 0, f"{n} {G} {dim}: {run.stdout}{run.stderr}"
        raw = dst.read_bytes()
        at = 0

        def take(count, dt):
            nonlocal at
            out = np.frombuffer(raw[at:at + count * np.dtype(dt).itemsize], dtype=dt)
            at += count * np.dtype(dt).itemsize
            return out
        acc = take(10 * G, np.int64).reshape(G, 10)
        table = take(8 * G, np.float64).reshape(G, 8)
        fit = take(8, np.float64)
        err = take(3, np.float64)
        gs = take(dim * n, np.float64).reshape(dim, n)
        ge = take(dim * n, np.float64).reshape(dim, n)
        assert at == len(raw)
        check([err, np.concatenate([gs, ge]), acc, table, fit], ref)
