"""
MixingError without a GPU: the numpy reference (tests/mixing_error_reference.py) against torch
autograd of the plain float definition, its quantised form against its plain one, the CPU path of
``ops.mixing_error`` against the reference bit for bit, the properties the definition promises, the
class and its place in the fused step's protocol, and ``csrc/mixing_math.h`` on the host under
the address and undefined-behaviour sanitizers.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import direction_fields_reference as dfr
import mixing_error_reference as mr
import weighted_errors_reference as wr
import tfrt.optimizer as optimizer
from tensorflowraytrace_amd import _lib, errors, fused_step, ops
from tensorflowraytrace_amd.errors import _Columns
from tensorflowraytrace_amd.fused_step import _TermState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "mixing_host", "mixing_main.cpp")
EPS = mr.EPS
N, G, BINS = 4000, 4, (8, 6)


def _scene(two=True, weighted=False, n=N):
    """4,000 rays, 4 groups, 8 x 6 bins (8 with one field), edge bins included: the points of
    tests/density_error_reference.py with a mask, a perm, labels and (weighted) the special
    weights."""
    x, y, mask, perm, weight, group = mr.inputs(n, n_groups=G)
    return dict(x=x, y=y if two else None, group=group, n_groups=G,
                bins=BINS if two else BINS[:1], domain=mr.DOMAIN if two else mr.DOMAIN[:1],
                oob_weight=mr.OOB, mask=mask, perm=perm, weight=weight if weighted else None)


def _autograd(ref, x, y, domain, bins):
    """d plain_torch / d (x, y) on the columns that count, scattered back onto all columns."""
    c = ref["counts"]
    tx = torch.tensor(np.asarray(x, dtype=np.float64)[c], requires_grad=True)
    ty = None if y is None else torch.tensor(np.asarray(y, dtype=np.float64)[c], requires_grad=True)
    w = None if ref["w"] is None else torch.tensor(ref["w"][c])
    e = mr.plain_torch(tx, ty, torch.tensor(ref["label"][c]), G, bins, domain, mr.OOB, w=w)
    e.backward()
    gx, gy = np.zeros(c.shape[0]), np.zeros(c.shape[0])
    gx[c] = tx.grad.numpy()
    if ty is not None:
        gy[c] = ty.grad.numpy()
    return float(e.detach()), gx, gy


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
def test_unquantised_reference_equals_autograd_of_the_plain_definition(two, weighted):
    """The gradient the definition states -- no derivative of m, n_g or N -- against torch autograd
    of the plain float definition, which differentiates all three: 1e-12 of the largest gradient
    entry."""
    kw = _scene(two, weighted)
    ref = mr.mixing_error(quantise=False, **kw)
    assert ref["inside"].sum() > N // 2 and ref["n_penalised"] > N // 32 and ref["groups_used"] == G
    e, gx, gy = _autograd(ref, kw["x"], kw["y"], kw["domain"], kw["bins"])
    top = max(np.abs(gx).max(), np.abs(gy).max())
    dev = max(np.abs(gx - ref["grad_x"]).max(), np.abs(gy - (ref["grad_y"] if two else 0.0)).max())
    print(f"error {ref['error']!r} autograd {e!r}; gradient deviation {dev / top:.2e} of the "
          f"largest entry {top:.3e}")
    assert abs(e - ref["error"]) <= 1e-12 * abs(e)
    assert dev <= 1e-12 * top


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_unquantised_reference_equals_autograd_with_a_direction_field(weighted):
    """Far-field fields: the reference's chain rule (tests/direction_fields_reference.py) against
    autograd through ``d = (end - start) / |end - start|`` into the plain definition."""
    n = 1000
    block = dfr.rays(n, np.float64)
    codes, domain, bins = (7, 8), dfr.DOMAIN, (8, 6)
    group = mr.labels_for(n, G)
    weight = wr.weights(n, 20) if weighted else None
    ref = mr.fields(block, codes, group, G, bins, domain, oob_weight=mr.OOB, weight=weight,
                    quantise=False)
    c = ref["counts"]
    assert ref["inside"].sum() > 150 and ref["n_penalised"] > 50
    t = torch.tensor(block[:, c], requires_grad=True)
    e3 = t[3:] - t[:3]
    d = e3 / torch.sqrt((e3 * e3).sum(dim=0))
    w = None if weight is None else torch.tensor(ref["w"][c])
    e = mr.plain_torch(d[1], d[2], torch.tensor(ref["label"][c]), G, bins, domain, mr.OOB, w=w)
    e.backward()
    top = float(t.grad.abs().max())
    dev = float(np.abs(t.grad.numpy() - ref["grad"][:, c]).max())
    print(f"gradient deviation {dev / top:.2e} of the largest entry {top:.3e}")
    assert dev <= 1e-12 * top and not ref["grad"][:, ~c].any()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
def test_quantised_against_unquantised(two, weighted):
    """What the fixed point costs: every bilinear weight is off by at most 2**-33 of a ray, so a
    cell with c contributions is off by at most c * 2**-33 -- it scales with the rays per cell.
    Measured here, on the CPU, on these inputs (4,000 rays, 4 groups, 8 x 6 bins, or 8 with one
    field), the largest gradient deviation relative to the largest gradient entry and the
    deviation of the error relative to the error: two fields 4.29e-13 and 1.41e-15,
    weighted 1.39e-12 and 5.32e-14; one field 9.20e-14 and 2.08e-15, weighted 4.42e-13 and
    5.39e-15.  Each case is asserted at 8 times its own measured figures."""
    measured = {(True, False): (4.29e-13, 1.41e-15), (True, True): (1.39e-12, 5.32e-14),
                (False, False): (9.20e-14, 2.08e-15), (False, True): (4.42e-13, 5.39e-15)}
    kw = _scene(two, weighted)
    q, p = mr.mixing_error(**kw), mr.mixing_error(quantise=False, **kw)
    top = max(np.abs(p["grad_x"]).max(), np.abs(p["grad_y"]).max() if two else 0.0)
    dev = np.abs(q["grad_x"] - p["grad_x"]).max()
    if two:
        dev = max(dev, np.abs(q["grad_y"] - p["grad_y"]).max())
    rel_e = abs(q["error"] - p["error"]) / p["error"]
    print(f"quantised against plain: gradient {dev / top:.2e} of the largest entry, error "
          f"{rel_e:.2e}")
    g_meas, e_meas = measured[two, weighted]
    assert dev <= 8 * g_meas * top and rel_e <= 8 * e_meas
    assert abs(float(q["Hq"].sum()) / mr.TWO32 - p["H"].sum()) <= 4 * q["inside"].sum() * 2.0 ** -33


@pytest.mark.parametrize("n", [0, 1, 65, 1000, 4097])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
def test_the_cpu_path_equals_the_reference_bit_for_bit(two, weighted, n):
    """``ops.mixing_error`` on CPU tensors: Hq as integers; pulls, group errors, the gradient
    rows, the error triple and the counts bit for bit."""
    for Gn, bins, empty in ((4, (8, 6), None), (3, (7, 3), 1), (5, (33, 32), None),
                            (2, (1, 1), None)):
        x, y, mask, perm, weight, group = mr.inputs(n, n_groups=Gn, empty=empty)
        b = bins if two else bins[:1]
        domain = mr.DOMAIN if two else mr.DOMAIN[:1]
        ref = mr.mixing_error(x, y if two else None, group, Gn, b, domain, mr.OOB, mask=mask,
                              perm=perm, weight=weight if weighted else None)
        rows = torch.full((6, n), 7.0, dtype=torch.float64)
        rows[4], rows[5] = torch.tensor(x), torch.tensor(y)
        grad = torch.full((6, n), float("nan"), dtype=torch.float64)
        grid = ops.density_grid(domain, b[0], b[1] if two else None)
        out = ops.mixing_error(rows, 4, 5 if two else -1, torch.tensor(group), Gn, b, grid, mr.OOB,
                               mask=torch.tensor(mask), perm=torch.tensor(perm), grad=grad,
                               weights=torch.tensor(weight) if weighted else None)
        err, g, hq, pull, ge, used = [o.numpy() for o in out]
        assert np.array_equal(hq, ref["Hq"])
        assert pull.tobytes() == ref["D"].tobytes()
        assert ge.tobytes() == ref["group_errors"].tobytes()
        assert g[4].tobytes() == ref["grad_x"].tobytes()
        if two:
            assert g[5].tobytes() == ref["grad_y"].tobytes()
        assert np.isnan(g[:4]).all() and (two or np.isnan(g[5]).all())
        assert err.tobytes() == np.array([ref["error"], 1.0, ref["error"]]).tobytes()
        assert used[0] == ref["groups_used"] and used[1] == ref["N"]


def test_the_cpu_path_equals_the_reference_with_a_direction_field():
    n = 1000
    block = dfr.rays(n, np.float64)
    group = mr.labels_for(n, G)
    weight = wr.weights(n, 20)
    ref = mr.fields(block, (7, 8), group, G, (8, 6), dfr.DOMAIN, oob_weight=mr.OOB, weight=weight)
    grid = ops.density_grid(dfr.DOMAIN, 8, 6)
    out = ops.mixing_error(torch.tensor(block), 7, 8, torch.tensor(group), G, (8, 6), grid, mr.OOB,
                           dimension=3, weights=torch.tensor(weight))
    assert np.array_equal(out[2].numpy(), ref["Hq"])
    assert out[3].numpy().tobytes() == ref["D"].tobytes()
    assert out[1].numpy().tobytes() == ref["grad"].tobytes()
    assert float(out[0][0]) == ref["error"]


# ------------------------------------------------------------------------------ properties
def _points(n, seed=3, margin=0.0):
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = mr.DOMAIN
    return (rng.uniform(x0 - margin, x1 + margin, n), rng.uniform(y0 - margin, y1 + margin, n))


def test_groups_that_are_copies_of_one_another_are_perfectly_mixed():
    x, y = _points(200)
    xs, ys = np.tile(x, 3), np.tile(y, 3)
    group = np.repeat(np.arange(3), 200)
    w = np.tile(np.random.default_rng(1).uniform(0.1, 1.0, 200), 3)
    for weight in (None, w):
        ref = mr.mixing_error(xs, ys, group, 3, (8, 6), mr.DOMAIN, mr.OOB, weight=weight)
        assert ref["e_mix"] == 0.0 and ref["error"] == 0.0 and not ref["D"].any()
        assert not ref["grad_x"].any() and not ref["grad_y"].any()
        assert np.array_equal(ref["group_errors"], np.zeros(3))


def test_one_used_group_gives_zero():
    x, y = _points(300, margin=0.2)
    group = np.full(300, 2)
    ref = mr.mixing_error(x, y, group, 4, (8, 6), mr.DOMAIN, 0.0)
    assert ref["groups_used"] == 1 and ref["error"] == 0.0 and not ref["D"].any()
    assert np.isnan(ref["group_errors"][[0, 1, 3]]).all() and ref["group_errors"][2] == 0.0
    # nothing at all: no mass, no error, no pull
    none = mr.mixing_error(x, y, np.full(300, -1), 4, (8, 6), mr.DOMAIN, mr.OOB)
    assert none["Nq"] == 0 and none["error"] == 0.0 and not none["D"].any()
    assert np.isnan(none["group_errors"]).all() and not none["grad_x"].any()


def test_one_bin_gives_zero():
    x, y = _points(300)
    group = np.arange(300) % 3
    two = mr.mixing_error(x, y, group, 3, (1, 1), mr.DOMAIN, 0.0)
    one = mr.mixing_error(x, None, group, 3, (1,), mr.DOMAIN[:1], 0.0)
    for ref in (two, one):
        assert ref["error"] == 0.0 and not ref["D"].any() and not ref["grad_x"].any()
        assert np.array_equal(ref["group_errors"], np.zeros(3))


def test_permuting_the_columns_changes_no_bit():
    """The histogram is an integer sum and every float sum runs over bins or groups: the order of
    the columns shows only in the order of the penalties (compared here to their rounding)."""
    kw = _scene(True, True, n=1000)
    n = 1000
    order = np.random.default_rng(8).permutation(n)
    a = mr.mixing_error(**kw)
    moved = dict(kw, x=kw["x"][order], y=kw["y"][order], mask=kw["mask"][order],
                 perm=kw["perm"][order])
    b = mr.mixing_error(**moved)
    assert np.array_equal(a["Hq"], b["Hq"]) and a["D"].tobytes() == b["D"].tobytes()
    assert a["group_errors"].tobytes() == b["group_errors"].tobytes() and a["e_mix"] == b["e_mix"]
    assert a["grad_x"][order].tobytes() == b["grad_x"].tobytes()
    assert a["grad_y"][order].tobytes() == b["grad_y"].tobytes()
    assert abs(a["penalty"] - b["penalty"]) <= 2 * a["n_penalised"] * EPS * a["penalty"]
    # without a ray outside the whole error has the same bits
    inside = dict(kw, x=np.clip(kw["x"], *mr.DOMAIN[0]), y=np.clip(kw["y"], *mr.DOMAIN[1]))
    c = mr.mixing_error(**inside)
    d = mr.mixing_error(**dict(inside, x=inside["x"][order], y=inside["y"][order],
                               mask=kw["mask"][order], perm=kw["perm"][order]))
    assert c["n_penalised"] == 0 and c["error"] == d["error"] > 0.0


def test_relabelling_the_groups_permutes_the_group_errors():
    kw = _scene(True, False, n=1000)
    a = mr.mixing_error(**kw)
    to = np.array([2, 0, 3, 1])
    lab = kw["group"].copy()
    ok = (lab >= 0) & (lab < G)
    lab[ok] = to[lab[ok]]
    b = mr.mixing_error(**dict(kw, group=lab))
    assert b["group_errors"][to].tobytes() == a["group_errors"].tobytes()
    assert b["D"][to].tobytes() == a["D"].tobytes()
    assert a["grad_x"].tobytes() == b["grad_x"].tobytes()
    # (G terms >= 0 in another order: each sum is within (G - 1) eps of the exact one)
    assert abs(a["e_mix"] - b["e_mix"]) <= 2 * G * EPS * a["e_mix"]


def test_a_ray_in_the_outer_half_bin_has_no_derivative_on_that_axis():
    (x0, x1), (y0, y1) = mr.DOMAIN
    bx, by = (x1 - x0) / 8, (y1 - y0) / 6
    x, y = _points(400, seed=5)
    # on the edge x0, inside the outer half bin at x1, in the outer half bin below y0's edge bin
    x[:3] = x0, x1 - 0.3 * bx, x0 + 2.2 * bx
    y[:3] = y0 + 2.6 * by, y0 + 1.7 * by, y0 + 0.4 * by
    group = np.arange(400) % 3
    ref = mr.mixing_error(x, y, group, 3, (8, 6), mr.DOMAIN, mr.OOB)
    assert ref["inside"][:3].all()
    assert ref["grad_x"][0] == 0.0 and ref["grad_x"][1] == 0.0 and ref["grad_y"][2] == 0.0
    assert ref["grad_y"][0] != 0.0 and ref["grad_y"][1] != 0.0 and ref["grad_x"][2] != 0.0
    rows = torch.tensor(np.stack([x, y]))
    out = ops.mixing_error(rows, 0, 1, torch.tensor(group.astype(np.int32)), 3, (8, 6),
                           ops.density_grid(mr.DOMAIN, 8, 6), mr.OOB)
    assert out[1].numpy().tobytes() == np.stack([ref["grad_x"], ref["grad_y"]]).tobytes()


# ------------------------------------------------------------------------------ the class
def test_the_wrapper_checks_its_arguments():
    n = 5
    rows = torch.zeros((2, n), dtype=torch.float64)
    lab = torch.zeros(n, dtype=torch.int32)
    grid = ops.density_grid(mr.DOMAIN, 4, 4)
    ok = dict(rows=rows, row_x=0, row_y=1, group=lab, n_groups=3, bins=(4, 4), grid=grid)
    ops.mixing_error(**ok)
    for bad, match in ((dict(group=lab.long()), "group"), (dict(n_groups=0), "n_groups"),
                       (dict(n_groups=1025), "n_groups"), (dict(bins=(4,)), "bins"),
                       (dict(bins=(0, 4)), "bins"), (dict(bins=(512, 512)), "bins"),
                       (dict(n_groups=32, bins=(256, 256)), "cells"), (dict(row_y=0), "distinct"),
                       (dict(variant=3), "variant"), (dict(bins=(64, 65), variant=1), "variant"),
                       (dict(mask=torch.zeros(5)), "mask"), (dict(perm=torch.zeros(5)), "perm"),
                       (dict(weights=torch.ones(5)), "weights"),
                       (dict(weights=torch.ones(4, dtype=torch.float64)), "one of each"),
                       (dict(grad=torch.zeros((4, 5), dtype=torch.float64)), "grad"),
                       (dict(hq=torch.zeros((3, 4, 4), dtype=torch.int32)), "hq"),
                       (dict(pull=torch.zeros((3, 16), dtype=torch.float64)), "pull"),
                       (dict(group_errors=torch.zeros(4, dtype=torch.float64)), "group_errors"),
                       (dict(used_out=torch.zeros(3, dtype=torch.float64)), "used_out")):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.mixing_error(**kw)


def test_the_class_checks_its_arguments_and_is_exported():
    import tfrt.optimizer
    M = optimizer.MixingError
    assert tfrt.optimizer.MixingError is M and fused_step.MixingError is M \
        and errors.MixingError is M and M in errors._COUPLED
    lab = np.arange(12) % 4
    erf = M(("y_end", "z_end"), lab, mr.DOMAIN, (8, 6))
    assert erf.n_groups == 4 and erf.labels.dtype == torch.int32 and erf.bins == (8, 6)
    assert erf.grid == ops.density_grid(mr.DOMAIN, 8, 6) and erf.weights is None
    assert erf.rows == [4, 5] and erf.seed_rows == 0x30 and erf.on_columns
    assert erf.rows_for(3) == [4, 5]
    with pytest.raises(ValueError, match="2-D engine"):
        erf.rows_for(2)
    far = M(("y_dir", "z_dir"), lab, mr.DOMAIN, 16, weights=np.linspace(1.0, 4.0, 12))
    assert far.has_direction and far.seed_rows == 0x3f and far.rows_for(3) == [7, 8]
    assert far.bins == (16, 16) and float(far.weights.max()) == 1.0
    one = M("y_end", torch.tensor(lab), mr.DOMAIN[:1], 9, n_groups=6)
    assert one.bins == (9,) and one.rows_for(2) == [3] and one.rows_for(3) == [4] \
        and one.n_groups == 6
    assert M(("x_dir", "y_dir"), lab, mr.DOMAIN, (4, 5)).rows_for(2) == [4, 5]
    for bad in (dict(fields=("y_end", "y_end")), dict(fields=("w_end",)),
                dict(domain=mr.DOMAIN[:1]), dict(domain=((0.0, 0.0), (0.0, 1.0))),
                dict(bins=0), dict(bins=(8,)), dict(bins=(8, 6, 2)), dict(bins="many"),
                dict(bins=(512, 512)), dict(bins=(256, 256), n_groups=17),
                dict(oob_weight=-1.0), dict(oob_weight=float("inf")), dict(oob_weight="big"),
                dict(groups=np.zeros(12)), dict(groups=np.zeros((3, 4), dtype=np.int64)),
                dict(groups=lambda src: lab), dict(n_groups=0), dict(n_groups=1025),
                dict(n_groups="some"), dict(weights=-np.ones(12)), dict(weights=np.zeros(12)),
                dict(weights=np.ones((12, 2))), dict(weights=np.ones(11))):
        kw = dict(fields=("y_end", "z_end"), groups=lab, domain=mr.DOMAIN, bins=(8, 6))
        kw.update(bad)
        with pytest.raises(ValueError, match="MixingError"):
            M(**kw)
    assert M(("y_end", "z_end"), lambda src: lab, mr.DOMAIN, 8, n_groups=4).labels is None
    for read in (erf.shares, erf.pooled, erf.group_errors, lambda: erf.groups_used):
        with pytest.raises(RuntimeError, match="no evaluation"):
            read()
    # graph_key: the label buffer and the weight buffer; in-place writes keep it
    k0, f0 = erf.graph_key(), far.graph_key()
    erf.labels.add_(0)
    far.weights.mul_(1.0)
    assert erf.graph_key() == k0 and far.graph_key() == f0 and k0 != f0
    erf.labels = erf.labels.clone()
    far.weights = far.weights.clone()
    assert erf.graph_key() != k0 and far.graph_key() != f0
    for name, value in (("n_groups", 5), ("oob_weight", 0.5), ("splat_variant", 2)):
        other = M(("y_end", "z_end"), erf.labels, mr.DOMAIN, (8, 6))
        base = other.graph_key()
        setattr(other, name, value)
        assert other.graph_key() != base
    assert M(("y_end", "z_end"), erf.labels, mr.DOMAIN, (8, 7)).graph_key() != \
        M(("y_end", "z_end"), erf.labels, mr.DOMAIN, (8, 6)).graph_key()
    # a legal term of a SumError, named in its message
    dens = optimizer.DensityError(("y_end", "z_end"), np.ones((6, 8)), mr.DOMAIN)
    both = optimizer.SumError([dens, erf], reduce="mean")
    assert both.terms == (dens, erf) and both.rows == [4, 5, 4, 5]
    with pytest.raises(ValueError, match="MixingError"):
        optimizer.SumError([erf, object()])


class _Engine:
    def __init__(self, block, ids, n_source, dim):
        names = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end") if dim == 3 \
            else ("x_start", "y_start", "x_end", "y_end")
        self.dimension = dim
        self.leaves = [torch.tensor(r, requires_grad=True) for r in block]
        self.finished_rays = dict(zip(names, self.leaves))
        self.last_trace = {"finished_id": torch.tensor(ids)}
        self._trace_src = {"x_start": torch.zeros(n_source)}


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_the_generic_path_returns_the_error_and_the_gradient_rows(weighted):
    """MixingError.__call__ on CPU tensors: the (1,) error and, through backward, the reference's
    gradient on the fields' rows; the read-outs report the reference's tables."""
    n = 300
    x, y, mask, perm, weight, group = mr.inputs(n, n_groups=G)
    # (the class refuses weights that are not finite or negative)
    ok = np.where(np.isfinite(weight) & (weight >= 0), weight, 0.5)
    ref = mr.mixing_error(x, y, group, G, BINS, mr.DOMAIN, mr.OOB, perm=perm,
                          weight=ok / ok.max() if weighted else None)
    erf = optimizer.MixingError(("y_end", "z_end"), group, mr.DOMAIN, BINS, oob_weight=mr.OOB,
                                n_groups=G, weights=ok if weighted else None)
    erf.labels = erf.labels.cpu()
    if weighted:
        erf.weights = erf.weights.cpu()
    block = np.zeros((6, n))
    block[4], block[5] = x, y
    eng = _Engine(block, perm, n + 3, 3)
    e = erf(eng)
    assert e.shape == (1,) and e.dtype == torch.float64 and float(e.detach()) == ref["error"]
    (3.0 * e.sum()).backward()
    assert np.array_equal(erf.last_hq.numpy(), ref["Hq"])
    assert np.array_equal(eng.leaves[4].grad.numpy(), 3.0 * ref["grad_x"])
    assert np.array_equal(eng.leaves[5].grad.numpy(), 3.0 * ref["grad_y"])
    assert eng.leaves[0].grad is None                  # (a row that is no field: untouched)
    assert erf.groups_used == ref["groups_used"] == G
    assert erf.group_errors().numpy().tobytes() == ref["group_errors"].tobytes()
    nq = np.array([float(v) for v in ref["nq"]])
    assert np.array_equal(erf.shares().numpy(), ref["Hq"].astype(np.float64) / nq[:, None, None])
    assert erf.shares().shape == (G, BINS[1], BINS[0]) and erf.pooled().shape == BINS[::-1]
    assert abs(float(erf.pooled().sum()) - 1.0) < 1e-12
    eng.finished_rays = {}
    assert erf(eng).shape == (1,) and float(erf(eng)) == 0.0
    with pytest.raises(ValueError, match="label"):
        erf(_Engine(block, perm, n, 3))


@pytest.mark.parametrize("fields,weighted", [(("y_end", "z_end"), False), (("z_end",), False),
                                             (("y_dir", "z_end"), False),
                                             (("y_end", "z_end"), True)],
                         ids=["two", "one", "direction", "weighted"])
def test_seed_columns_equals_the_direct_call(fields, weighted):
    """In the manner of tests/test_error_terms_host.py: ``seed_columns(cols, hold)`` on CPU tensors
    leaves exactly what a direct ``ops.mixing_error`` call with the same arguments leaves."""
    n, Gn = 70, 5
    rng = np.random.default_rng(7)
    rows = np.concatenate([rng.uniform(-0.2, 0.2, (3, n)), rng.uniform(-1.3, 1.3, (3, n))])
    rows[3] = 1.0 + 0.1 * rows[3]
    mask = np.where(np.arange(n) % 5 == 4, -1, np.arange(n) % 7).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    src = {"x_start": torch.zeros(n, dtype=torch.float64)}
    cols = _Columns(torch.tensor(rows), torch.tensor(mask), torch.tensor(perm), src, n)
    two = len(fields) == 2
    domain = ((-1.0, 1.0), (-0.9, 1.1))[:2 if two else 1]
    bins = (7, 6) if two else (7,)
    labels = np.where(np.arange(n) % 11 == 10, -1, np.arange(n) % Gn)
    w = np.random.default_rng(3).uniform(0.1, 1.0, n) if weighted else None

    def make():
        term = optimizer.MixingError(fields, labels, domain, bins, oob_weight=0.3, n_groups=Gn,
                                     weights=w)
        term.labels = term.labels.cpu()
        if weighted:
            term.weights = term.weights.cpu()
        return term
    term = make()
    hold = _TermState(torch.zeros((6, n), dtype=torch.float64),
                      torch.zeros(3, dtype=torch.float64), term.seed_rows)
    term.seed_columns(cols, hold)
    other = make()
    nx, ny = bins[0], (bins[1] if two else 1)
    ws = torch.empty(max(_lib.lib().tfrt_mixing_error_workspace_bytes(n, Gn, nx, ny), 1),
                     dtype=torch.uint8)
    grad = torch.zeros((6, n), dtype=torch.float64)
    err = torch.zeros(3, dtype=torch.float64)
    out = ops.mixing_error(cols.rows, other.rows[0], other.rows[1] if two else -1,
                           other.labels_of(src), Gn, bins, other.grid, 0.3, mask=cols.mask,
                           perm=cols.perm, variant=0, dimension=3, weights=other.weights_of(src),
                           grad=grad, err=err, workspace=ws)
    bits = lambda t: t.contiguous().view(torch.int64)     # noqa: E731
    assert torch.equal(bits(hold.g_fin), bits(grad)) and torch.equal(bits(hold.err), bits(err))
    assert float(err[1]) == 1.0 and float(err[0]) > 0.0
    assert set(hold.buffers) == {"workspace", "hq", "pull", "group_errors", "used_out"}
    assert term.last_hq is hold.buffers["hq"] and torch.equal(term.last_hq, out[2])
    assert torch.equal(bits(term.last_pull), bits(out[3])) and bool(out[2].any())
    written = sum(1 << r for r in range(6) if bool(hold.g_fin[r].any()))
    assert written == term.seed_rows
    assert term.seed_rows == (0x3f if "y_dir" in fields else sum(1 << r for r in term.rows))
    before = {k: v.data_ptr() for k, v in hold.buffers.items()}
    term.seed_columns(cols, hold)
    assert {k: v.data_ptr() for k, v in hold.buffers.items()} == before
    assert torch.equal(bits(hold.g_fin), bits(grad)) and torch.equal(bits(hold.err), bits(err))


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build
    _build.build()
    L = _lib.lib()
    ws = L.tfrt_mixing_error_workspace_bytes
    assert ws(10, 0, 4, 4) == 0 and ws(10, 1025, 4, 4) == 0 and ws(10, 4, 512, 512) == 0
    assert ws(10, 32, 256, 256) == 0 and ws(-1, 4, 4, 4) == 0
    assert 0 < ws(0, 4, 4, 4) <= ws(1_000_000, 16, 256, 256)
    dummy = ctypes.create_string_buffer(1 << 17)
    p = ctypes.cast(dummy, ctypes.c_void_p)

    def call(n=8, G=4, nx=4, ny=4, dim=3, fx=4, fy=5, x1=1.0, sx=4.0, oob=0.0, wsb=1 << 17,
             stride=8, gstride=8, variant=0, group=p, n_source=8, used=p, ge=p, pull=p, hq=p,
             err=p, dtype=1):
        return L.tfrt_mixing_error(p, stride, n, dtype, dim, None, fx, fy, group, n_source, None,
                                   G, None, nx, ny, 0.0, x1, sx, 0.0, 1.0, 4.0, oob, p, gstride,
                                   err, used, ge, pull, hq, variant, p, wsb, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=1025), dict(nx=0), dict(ny=0), dict(nx=512, ny=512),
                dict(G=32, nx=256, ny=256), dict(dim=1), dict(dim=4), dict(fx=9), dict(fy=4),
                dict(dim=2, fx=6), dict(fy=-1), dict(x1=0.0), dict(sx=0.0), dict(oob=-1.0),
                dict(stride=4), dict(gstride=4), dict(variant=3), dict(group=None),
                dict(n=1 << 31), dict(dtype=7), dict(nx=33, ny=32, variant=1),
                dict(n_source=-1), dict(used=None), dict(ge=None), dict(pull=None),
                dict(hq=None), dict(err=None)):
        assert call(**bad) == -1, bad
    assert call(wsb=8) == -2


def test_mixing_math_on_the_host_under_the_sanitizers(tmp_path):
    """The margins, every cell's squared difference and pull, every group's error and its term of
    E_mix from mixing_math.h equal the reference's bit for bit; the program's vectors are
    exact-size allocations and it runs under the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "mixing_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
    for n, Gn, bins, two, weighted, empty in (
            (1000, 4, (8, 6), True, False, None), (1000, 4, (8, 6), True, True, None),
            (4097, 3, (7, 3), True, True, 1), (1000, 5, (33, 32), True, False, None),
            (1000, 1, (9,), False, False, None), (65, 2, (1,), False, True, None),
            (1, 3, (4, 4), True, False, None), (0, 2, (4, 4), True, False, None)):
        x, y, mask, perm, weight, group = mr.inputs(n, n_groups=Gn, empty=empty)
        ref = mr.mixing_error(x, y if two else None, group, Gn, bins,
                              mr.DOMAIN if two else mr.DOMAIN[:1], mr.OOB, mask=mask, perm=perm,
                              weight=weight if weighted else None)
        B = ref["bins"]
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(struct.pack("<2q", Gn, B) + ref["Hq"].tobytes() + f8(ref["sq_sum"]))
        run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert run.returncode == 0, f"{n} {Gn} {bins}: {run.stdout}{run.stderr}"
        raw = dst.read_bytes()
        assert len(raw) == 8 * (Gn + B + 1 + 2 + 2 * Gn * B + 3 * Gn)
        ints = np.frombuffer(raw[:8 * (Gn + B + 1)], dtype=np.int64)
        f = np.frombuffer(raw[8 * (Gn + B + 1):], dtype=np.float64)
        assert ints[:Gn].tolist() == list(ref["nq"]) and ints[Gn:Gn + B].tolist() == list(ref["Pq"])
        assert int(ints[-1]) == ref["Nq"]
        assert f[:2].tobytes() == f8([ref["N"], ref["scale"]])
        cells = Gn * B
        assert f[2:2 + cells].tobytes() == f8(ref["sq"])
        assert f[2 + cells:2 + 2 * cells].tobytes() == f8(ref["D"])
        rest = f[2 + 2 * cells:].reshape(3, Gn)
        assert rest[0].tobytes() == f8(ref["group_errors"])
        assert rest[1].tobytes() == f8(ref["term"])
        assert np.array_equal(rest[2] != 0.0, ref["used"])
