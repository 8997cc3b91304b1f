"""MomentError without a GPU: the CPU path of ``ops.moment_error`` against the numpy restatement
(tests/moment_error_reference.py) bit for bit, the limb arithmetic and its bit budget, the gradient
against torch autograd of the plain covariance definition, descent onto a target covariance, the
class and its generic path, the entry's argument checks, and moment_math.h as a stand-alone host
program under the sanitizers.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import direction_fields_reference as dfr
import moment_error_reference as mr
from tensorflowraytrace_amd import ops, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "moment_host", "moment_main.cpp")
MODES = ["covariance", "round"]


def _mode(mode, G, two):
    return dict(shape="round") if mode == "round" else dict(covariance=mr.targets_for(G, two))


def _torch_mode(kw):
    return {k: torch.tensor(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}


def _case(n, G, two, mode, masked=False, permuted=False, dtype=np.float64):
    x, y, mask, group, perm = mr.rays(n, G, dtype)
    domain = mr.DOMAIN if two else mr.DOMAIN[:1]
    kw = _mode(mode, G, two)
    ref = mr.moment_error(x.astype(np.float64), y.astype(np.float64) if two else None, group, G,
                          domain, oob_weight=mr.OOB, mask=mask if masked else None,
                          perm=perm if permuted else None, **kw)
    return (x, y, mask, group, perm, domain, kw), ref


def _cpu(case, G, two, masked, permuted, dim=3):
    x, y, mask, group, perm, domain, kw = case
    n = x.shape[0]
    rows = torch.full((2 * dim, n), 7.0, dtype=torch.tensor(x).dtype)
    rows[dim], rows[dim + 1] = torch.tensor(x), torch.tensor(y)
    g = torch.tensor(group)
    grad = torch.full((2 * dim, n), float("nan"), dtype=torch.float64)
    mb = ops.moment_mbits(g.numel())
    out = ops.moment_error(
        rows, dim, dim + 1 if two else -1, g, G, ops.spot_grid(domain, mb), oob_weight=mr.OOB,
        mask=torch.tensor(mask) if masked else None, perm=torch.tensor(perm) if permuted else None,
        grad=grad, dimension=dim, mbits=mb, **_torch_mode(kw))
    return [t.numpy() for t in out]


def _bits_equal(a, b):
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def assert_equal(got, ref, dim, two):
    """Every output of an evaluation against the reference, bit for bit (also the GPU tests')."""
    err, grad, acc, mom, group_rows, cov, used_out = got
    assert np.array_equal(acc, ref["acc"])
    assert np.array_equal(mom, ref["mom"])
    assert _bits_equal(group_rows, ref["group_rows"]).all()
    assert _bits_equal(cov, ref["cov"]).all()
    assert used_out.tolist() == [ref["groups_used"], int(ref["rays"].sum())]
    assert grad[dim].tobytes() == ref["grad_x"].tobytes()
    if two:
        assert grad[dim + 1].tobytes() == ref["grad_y"].tobytes()
    assert np.isnan(np.delete(grad, [dim, dim + 1][:2 if two else 1], axis=0)).all()
    assert err[1] == ref["terms"]
    assert err[0].tobytes() == np.float64(ref["error"]).tobytes()
    if ref["terms"]:
        assert err[2] == err[0] / err[1]
    else:
        assert np.isnan(err[2])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("G", [1, 7, 300])
def test_cpu_path_equals_the_reference(G, mode):
    """Both modes, one and two fields, 2-D and 3-D blocks, f32 and f64 rows, masked and permuted
    columns, labels -1 and G, NaN target components, empty groups and groups of one ray; n = 0
    and 1."""
    for n in (0, 1, 65, 1000):
        for two in (True, False):
            if mode == "round" and not two:
                continue
            for flags in ((False, False), (True, True)):
                for dtype, dim in ((np.float64, 3), (np.float32, 2)):
                    case, ref = _case(n, G, two, mode, *flags, dtype=dtype)
                    assert_equal(_cpu(case, G, two, *flags, dim=dim), ref, dim, two)
                    if n == 1000 and G == 7:
                        assert 0 < ref["groups_used"] < int(ref["rays"].sum()) < G
                        assert ref["outside"].sum() > 50 and ref["inside"].sum() > 400
                        assert ref["error"] > 0.0


@pytest.mark.parametrize("dim,codes,mode", [
    (d, c, m) for d, c in [(3, (7, 8)), (3, (8,)), (3, (4, 8)), (2, (3, 5)), (2, (2, 3)), (2, (5,))]
    for m in MODES if m == "covariance" or len(c) == 2])
def test_cpu_path_with_direction_fields_equals_the_reference(dim, codes, mode):
    """Direction and mixed codes: the covariance of direction cosines (a divergence, a phase-space
    matrix), and all 2 d rows of every column written through the chain rule."""
    two = len(codes) == 2
    n, G = 1000, 7
    block = dfr.rays(n, np.float64, dimension=dim)
    rng = np.random.default_rng(3)
    group = rng.integers(-1, G - 1, n + 3).astype(np.int32)
    mask = np.where(np.arange(n) % 5 == 4, -1, 0).astype(np.int32)
    domain = tuple(dfr.DOMAIN[i] if c >= 2 * dim else (-0.5, 2.5) for i, c in enumerate(codes))
    kw = _mode(mode, G, two)
    if mode == "covariance":
        kw["covariance"] = kw["covariance"] * 0.1
    ref = mr.fields(block, codes, group, G, domain, oob_weight=mr.OOB, mask=mask, **kw)
    assert ref["inside"].sum() > 150 and ref["outside"].sum() > 50 and ref["groups_used"] >= 3
    grad = torch.full((2 * dim, n), float("nan"), dtype=torch.float64)
    g = torch.tensor(group)
    mb = ops.moment_mbits(g.numel())
    out = ops.moment_error(torch.tensor(block), codes[0], codes[1] if two else -1, g, G,
                           ops.spot_grid(domain, mb), oob_weight=mr.OOB, mask=torch.tensor(mask),
                           grad=grad, dimension=dim, **_torch_mode(kw))
    assert np.array_equal(out[2].numpy(), ref["acc"])
    assert np.array_equal(out[3].numpy(), ref["mom"])
    assert _bits_equal(out[5].numpy(), ref["cov"]).all()
    has_dir = any(c >= 2 * dim for c in codes)
    for row in range(2 * dim):
        if has_dir or row in codes:
            assert grad[row].numpy().tobytes() == ref["grad"][row].tobytes(), row
        else:
            assert np.isnan(grad[row].numpy()).all()
    assert float(out[0][0]) == ref["error"]


@pytest.mark.parametrize("mode", MODES)
def test_permuting_the_columns_changes_no_bit(mode):
    """The records are integer sums and every float sum has a fixed order over the GROUPS: another
    order of the columns gives the same tables and, column by column, the same gradient.  (No
    penalties here: their sum runs over the columns in launch order.)"""
    n, G = 1000, 7
    (x, y, mask, group, perm, domain, kw), _ = _case(n, G, True, mode)
    x = np.clip(x, domain[0][0], domain[0][1])
    y = np.clip(y, domain[1][0], domain[1][1])
    ident = np.arange(n, dtype=np.int32)
    a = _cpu((x, y, mask, group, ident, domain, kw), G, True, False, True)
    sh = np.random.default_rng(1).permutation(n).astype(np.int32)
    b = _cpu((x[sh], y[sh], mask, group, sh, domain, kw), G, True, False, True)
    for i in (0, 2, 3, 4, 5, 6):
        assert a[i].tobytes() == b[i].tobytes(), i
    assert a[1][:, sh].tobytes() == b[1].tobytes()


def test_the_limb_sums_reassemble_to_the_exact_moment():
    """HH 2^mbits + HL 2^h + LL is the Python-integer sum of da * db, for offsets of either sign
    over the whole range |d| <= 2^mbits, and the reference's tables are such sums."""
    rng = np.random.default_rng(11)
    for mbits in (2, 30, 36, 40):
        h = mbits // 2
        top = 1 << mbits
        dx = [int(v) for v in rng.integers(-top, top + 1, 500)] + [top, -top, 0, -1, 1]
        dy = [int(v) for v in rng.integers(-top, top + 1, 500)] + [-top, -top, 0, 1, -1]
        s = mr.limb_sums(dx, dy, h)
        for first, (p, q) in ((0, (dx, dx)), (3, (dx, dy)), (6, (dy, dy))):
            whole = s[first] * (1 << mbits) + s[first + 1] * (1 << h) + s[first + 2]
            assert whole == sum(a * b for a, b in zip(p, q))
    (x, y, mask, group, perm, domain, kw), ref = _case(1000, 7, True, "round")
    for g in range(7):
        if ref["used"][g]:
            at = ref["inside"] & (ref["label"] == g)
            kx, ky = ref["centres"][g]
            dx = [int(v) - kx for v in ref["mx"][at]]
            dy = [int(v) - ky for v in ref["my"][at]]
            assert ref["mom_exact"][g] == [sum(a * a for a in dx),
                                           sum(a * b for a, b in zip(dx, dy)),
                                           sum(b * b for b in dy)]
            # the centre is the grid point nearest to the centroid
            assert abs(kx - sum(int(v) for v in ref["mx"][at]) / int(at.sum())) <= 0.5


@pytest.mark.parametrize("N", [2, 4096, 2 ** 20 - 4, 2 ** 20, 2 ** 24])
def test_the_bit_budget_holds(N):
    """With every ray at the largest offset the definition allows, each limb sum of a source of N
    rays stays below 2^62 in magnitude, and pass 1's sums below 2^61."""
    mbits = ops.moment_mbits(N)
    assert mbits == mr.mbits_of(N) and mbits % 2 == 0 and 2 <= mbits <= 40
    h = mbits // 2
    low, top = (1 << h) - 1, 1 << mbits
    worst = 0
    for d in (top, -top, top - 1, -top + 1, low, -low - 1, -1):
        for e in (top, -top, low, -low - 1, -1):
            al, ah, bl, bh = d & low, d >> h, e & low, e >> h
            worst = max(worst, abs(ah * bh), abs(ah * bl + al * bh), abs(al * bl))
    assert worst <= 1 << (mbits + 1)
    assert N * worst < 1 << 62 and N * top < 1 << 61
    assert N < 1 << (61 - mbits)              # (what ops.moment_error and the entry check)
    if mbits < 40:
        assert N * (1 << (mbits + 3)) >= 1 << 62      # (and no two bits are given away)


@pytest.mark.parametrize("mode", MODES)
def test_gradient_against_autograd_of_the_plain_definition(mode):
    """4,000 points in 5 anisotropic clouds, the domain four times their extent: the gradient
    agrees with float64 autograd of the covariance about the MEAN, no grid, to 1e-9 relative; grid
    effects there are about 2^-40.  Targets of half the clouds' covariance keep D well away from
    a difference of nearly equal numbers."""
    x, y, group, domain, cov = mr.clouds()
    G = 5
    kw = dict(shape="round") if mode == "round" else dict(covariance=0.5 * cov)
    xt = torch.tensor(x, requires_grad=True)
    yt = torch.tensor(y, requires_grad=True)
    e = mr.plain_covariance_error(xt, yt, group, G, kw.get("covariance"), kw.get("shape"))
    e.backward()
    out = _cpu((x, y, None, group, None, domain, kw), G, True, False, False)
    scale = max(float(xt.grad.abs().max()), float(yt.grad.abs().max()))
    assert scale > 1e-3
    assert np.abs(out[1][3] - xt.grad.numpy()).max() <= 1e-9 * scale
    assert np.abs(out[1][4] - yt.grad.numpy()).max() <= 1e-9 * scale
    assert abs(out[0][0] - float(e.detach())) <= 1e-9 * float(e.detach())
    assert np.abs(out[5][:, :3] - cov).max() <= 1e-9 * np.abs(cov).max()
    # the gradient of every used group sums to zero within rounding
    for g in range(G):
        at = group == g
        big = np.abs(out[1][3:5, at]).sum()
        assert abs(out[1][3, at].sum()) <= 1e-9 * big and abs(out[1][4, at].sum()) <= 1e-9 * big


def test_descent_reaches_the_target_covariance_and_keeps_the_centroids():
    """Plain descent on free points: every cloud takes its target covariance -- here the first
    cloud's, for all --, and no centroid moves."""
    x, y, group, domain, cov = mr.clouds(n=1000)
    G = 5
    target = np.broadcast_to(cov[0], (G, 3)).copy()
    c0 = np.array([[x[group == g].mean(), y[group == g].mean()] for g in range(G)])
    first = None
    for step in range(400):
        out = _cpu((x, y, None, group, None, domain, dict(covariance=target)), G, True, False,
                   False)
        first = out[0][0] if first is None else first
        x = x - 0.5 * out[1][3]
        y = y - 0.5 * out[1][4]
    assert out[0][0] < 1e-6 * first
    assert np.abs(out[5][:, :3] - target).max() < 1e-3 * np.abs(target).max()
    c1 = np.array([[x[group == g].mean(), y[group == g].mean()] for g in range(G)])
    assert np.abs(c1 - c0).max() < 1e-9


def test_groups_of_one_ray_nan_targets_empty_groups_and_excluded_labels():
    x = np.array([0.0, 0.1, -0.2, 0.3, 0.5, -0.5, 0.2])
    y = np.array([1.0, 1.2, 0.9, 1.1, 1.5, 0.7, 1.0])
    group = np.array([0, 0, 0, 1, 3, 3, -1], dtype=np.int32)      # 1: one ray; 2: empty; -1: out
    G = 4
    tg = np.array([[0.01, np.nan, 0.02], [0.01, 0.0, 0.01], [0.01, 0.0, 0.01],
                   [np.nan, np.nan, np.nan]])
    kw = dict(covariance=tg)
    ref = mr.moment_error(x, y, group, G, mr.DOMAIN, **kw)
    out = _cpu((x, y, None, group, None, mr.DOMAIN, kw), G, True, False, False)
    assert_equal(out, ref, 3, True)
    err, grad, acc, mom, rows, cov, used = out
    assert acc[:, 0].tolist() == [3, 1, 0, 2] and used.tolist() == [2.0, 3.0]
    assert np.isfinite(rows[1, :2]).all() and np.isnan(rows[2, :2]).all()
    assert np.isnan(cov[1]).all() and np.isnan(cov[2]).all() and not mom[1].any()
    assert cov[0, 4] == 0.0 and (cov[3, 3:] == 0.0).all() and np.isfinite(cov[3, :3]).all()
    assert (grad[3:5, 3:] == 0.0).all() and (grad[3:5, :3] != 0.0).all()
    assert err[1] == 14.0 and err[0] > 0.0


def test_ops_argument_errors():
    rows = torch.zeros((6, 8), dtype=torch.float64)
    g = torch.zeros(8, dtype=torch.int32)
    grid = ops.spot_grid(mr.DOMAIN, 40)
    tg = torch.zeros((2, 3), dtype=torch.float64)
    ok = dict(rows=rows, row_x=4, row_y=5, group=g, n_groups=2, grid=grid, covariance=tg)
    ops.moment_error(**ok)
    for bad in (dict(covariance=None), dict(shape="round"), dict(covariance=None, shape="oval"),
                dict(covariance=None, shape="round", row_y=-1), dict(covariance=tg[:, :1]),
                dict(covariance=tg.float()), dict(covariance=tg[:1]), dict(group=g.long()),
                dict(n_groups=0), dict(n_groups=2 ** 20 + 1), dict(row_y=4), dict(row_x=6),
                dict(variant=3), dict(variant=1, n_groups=257, covariance=None, shape="round"),
                dict(mbits=41), dict(mbits=39), dict(mbits=0), dict(dimension=4),
                dict(acc=torch.zeros((2, 3), dtype=torch.int64)),
                dict(mom=torch.zeros((2, 8), dtype=torch.int64)),
                dict(group_rows=torch.zeros((2, 6), dtype=torch.float64)),
                dict(cov=torch.zeros((2, 6), dtype=torch.float32)),
                dict(used_out=torch.zeros(3, dtype=torch.float64)),
                dict(grad=torch.zeros((6, 4), dtype=torch.float64)),
                dict(mask=torch.zeros(8, dtype=torch.int64))):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match="moment_error"):
            ops.moment_error(**kw)
    assert tuple(ops.moment_covariances(torch.zeros((2, 6)), 2).shape) == (2, 3)
    assert tuple(ops.moment_covariances(torch.zeros((2, 6)), 1).shape) == (2, 1)


def test_the_class_checks_its_arguments_and_is_exported():
    import tfrt.optimizer
    from tensorflowraytrace_amd import errors, fused_step
    M = optimizer.MomentError
    assert tfrt.optimizer.MomentError is M and fused_step.MomentError is M \
        and errors.MomentError is M and M in errors._COUPLED
    lab = np.arange(12) % 4
    tg = np.array([[0.1, 0.0, 0.1], [np.nan, 0.0, 0.2], [0.2, 0.1, 0.3], [0.0, 0.0, 0.0]])
    erf = M(("y_end", "z_end"), lab, mr.DOMAIN, covariance=tg)
    assert erf.n_groups == 4 and erf.labels.dtype == torch.int32 and erf.shape is None
    assert erf.covariance.dtype == torch.float64 and tuple(erf.covariance.shape) == (4, 3)
    assert erf.rows == [4, 5] and erf.seed_rows == 0x30 and erf.on_columns
    with pytest.raises(ValueError, match="2-D engine"):
        erf.rows_for(2)
    far = M(("y_dir", "z_dir"), lab, mr.DOMAIN, shape="round")
    assert far.has_direction and far.seed_rows == 0x3f and far.rows_for(3) == [7, 8]
    assert far.covariance is None and far.shape == "round"
    one = M("y_end", torch.tensor(lab), mr.DOMAIN[:1], covariance=tg[:, 0], n_groups=4)
    assert tuple(one.covariance.shape) == (4, 1) and one.rows_for(2) == [3]
    assert M("y_end", lab, mr.DOMAIN[:1], covariance=0.25).covariance.tolist() == [[0.25]] * 4
    assert M(("y_end", "z_end"), lab, mr.DOMAIN, covariance=[0.1, 0.0, 0.2]) \
        .covariance.tolist() == [[0.1, 0.0, 0.2]] * 4
    inf, neg, ind = tg.copy(), tg.copy(), tg.copy()
    inf[2, 1], neg[0, 2], ind[2, 1] = np.inf, -0.1, 0.3
    for bad in (dict(), dict(covariance=tg, shape="round"), dict(shape="oval"),
                dict(shape="round", fields="y_end", domain=mr.DOMAIN[:1]),
                dict(covariance=tg, fields=("y_end", "y_end")),
                dict(covariance=tg, domain=mr.DOMAIN[:1]), dict(covariance=tg, oob_weight=-1.0),
                dict(covariance=inf), dict(covariance=neg), dict(covariance=ind),
                dict(covariance=-tg), dict(covariance=tg[:3]), dict(covariance=tg[:, :2]),
                dict(covariance="wide"), dict(covariance=tg, groups=np.zeros(3)),
                dict(covariance=tg, groups=lambda src: lab), dict(covariance=tg, n_groups=0),
                dict(shape="round", n_groups=2 ** 20 + 1)):
        kw = dict(fields=("y_end", "z_end"), groups=lab, domain=mr.DOMAIN)
        kw.update(bad)
        with pytest.raises(ValueError, match="MomentError"):
            M(**kw)
    with pytest.raises(TypeError):
        M(("y_end", "z_end"), lab, mr.DOMAIN, shape="round", weights=np.ones(12))
    assert M(("y_end", "z_end"), lambda src: lab, mr.DOMAIN, shape="round", n_groups=4) \
        .labels is None
    for read in (erf.centroids, erf.covariances, erf.residuals, lambda: erf.groups_used):
        with pytest.raises(RuntimeError, match="no evaluation"):
            read()
    # graph_key: the label buffer, the target buffer and the mode; in-place writes keep it
    k0, f0 = erf.graph_key(), far.graph_key()
    erf.labels.add_(0)
    erf.covariance.add_(0.0)
    assert erf.graph_key() == k0 and k0 != f0
    erf.covariance = erf.covariance.clone()
    assert erf.graph_key() != k0
    # a legal term of a SumError, named in its message
    spot = optimizer.SpotError(("y_end", "z_end"), lab, mr.DOMAIN)
    both = optimizer.SumError([spot, far], reduce="mean")
    assert both.terms == (spot, far) and both.rows == [4, 5, 7, 8]
    with pytest.raises(ValueError, match="MomentError"):
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


@pytest.mark.parametrize("mode", MODES)
def test_the_generic_path_returns_the_terms_and_the_gradient_rows(mode):
    """MomentError.__call__ on CPU tensors: (n, k) terms -- an inside ray of a used group carries
    (Dxx^2 + Dxy^2, Dxy^2 + Dyy^2), a penalised ray its penalty per field -- whose sum is the
    reference's error to rounding and, through backward, the reference's gradient on the fields'
    rows; the read-outs report the reference's tables."""
    n, G = 300, 7
    (x, y, mask, group, perm, domain, kw), ref = _case(n, G, True, mode, permuted=True)
    erf = optimizer.MomentError(("y_end", "z_end"), group, domain, oob_weight=mr.OOB, n_groups=G,
                                **kw)
    erf.labels = erf.labels.cpu()
    block = np.zeros((6, n))
    block[4], block[5] = x, y
    eng = _Engine(block, perm, n + 3, 3)
    e = erf(eng)
    assert e.shape == (n, 2) and e.dtype == torch.float64
    (3.0 * e.sum()).backward()
    want = mr.per_ray_terms(ref)
    inside = ref["inside"]
    assert np.array_equal(e.detach().numpy()[inside], want[inside])
    assert (e.detach().numpy()[~inside & ~ref["outside"]] == 0.0).all()
    # (n terms and 2 G group terms in another order: Higham, eq. 4.4, as the sibling tests)
    assert abs(float(e.detach().sum()) - ref["error"]) <= 2.0 * (2 * n + 2 * G) * mr.EPS \
        * ref["abs_sum"]
    assert np.array_equal(erf.last_acc.numpy(), ref["acc"])
    assert np.array_equal(erf.last_mom.numpy(), ref["mom"])
    assert np.array_equal(eng.leaves[4].grad.numpy(), 3.0 * ref["grad_x"])
    assert np.array_equal(eng.leaves[5].grad.numpy(), 3.0 * ref["grad_y"])
    assert eng.leaves[0].grad is None                  # (a row that is no field: untouched)
    assert erf.groups_used == ref["groups_used"] > 2
    assert np.array_equal(erf.centroids().numpy(), ref["centroids"], equal_nan=True)
    assert np.array_equal(erf.covariances().numpy(), ref["cov"][:, :3], equal_nan=True)
    assert np.array_equal(erf.residuals().numpy(), ref["cov"][:, 3:], equal_nan=True)
    eng.finished_rays = {}
    assert erf(eng).shape == (0, 2)
    with pytest.raises(ValueError, match="label"):
        erf(_Engine(block, perm, n, 3))


def test_the_optimiser_takes_the_generic_path_on_the_cpu_backend(cpu_backend):
    """SGD_Optimizer with a MomentError on the oracle-backed CPU stand-ins: the step's error is the
    reference's on the traced rays."""
    from test_host_logic import _lens_api
    eng, system, lens, target = _lens_api(200)
    groups = np.arange(200) % 5
    domain = ((-5.0, 5.0), (-5.0, 5.0))
    erf = optimizer.MomentError(("y_end", "z_end"), groups, domain, shape="round")
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=2e-3, grad_clip=1e9)
    grads, err_sum, n_terms = opt.raw_gradient()
    assert opt._fused_step is None
    fin = eng.finished_rays
    ids = eng.last_trace["finished_id"].numpy()
    ref = mr.moment_error(fin["y_end"].detach().numpy(), fin["z_end"].detach().numpy(), groups, 5,
                          domain, shape="round", perm=ids)
    assert ref["terms"] == n_terms > 300 and ref["groups_used"] == 5 and ref["error"] > 0.0
    assert abs(float(err_sum) - ref["error"]) <= 2.0 * (400 + 10) * mr.EPS * ref["abs_sum"]
    assert any(float(g.abs().max()) > 0 for g in grads)


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from tensorflowraytrace_amd import _build, _lib
    _build.build()
    L = _lib.lib()
    assert L.tfrt_moment_error_workspace_bytes(10, 0) == 0
    assert L.tfrt_moment_error_workspace_bytes(10, 2 ** 20 + 1) == 0
    assert L.tfrt_moment_error_workspace_bytes(-1, 4) == 0
    small = L.tfrt_moment_error_workspace_bytes(0, 4)
    assert 0 < small < L.tfrt_moment_error_workspace_bytes(1_000_000, 2 ** 20)
    dummy = ctypes.create_string_buffer(1 << 17)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 8)

    def call(n=8, G=4, dim=3, fx=4, fy=5, x1=1.0, msx=4.0, oob=0.0, ws=1 << 17, stride=8,
             gstride=8, variant=0, group=p, mbits=40, n_source=8, mode=0, target=p, used=p,
             rows=p, cov=p, acc=p, mom=p, err=p, dtype=1):
        return L.tfrt_moment_error(p, stride, n, dtype, dim, None, fx, fy, group, n_source, None,
                                   G, mode, target, 0.0, x1, msx, 0.0, 1.0, 4.0, mbits, oob, p,
                                   gstride, err, used, rows, cov, acc, mom, variant, p, ws, None)
    for bad in (dict(n=-1), dict(G=0), dict(G=2 ** 20 + 1), dict(dim=1), dict(dim=4), dict(fx=9),
                dict(fy=4), dict(dim=2, fx=6), dict(x1=0.0), dict(msx=0.0), dict(oob=-1.0),
                dict(stride=4), dict(gstride=4), dict(variant=3), dict(variant=-1),
                dict(group=None), dict(n=1 << 31), dict(mbits=42), dict(mbits=39), dict(mbits=0),
                dict(dtype=7), dict(n=1 << 21, stride=1 << 21, gstride=1 << 21),
                dict(G=257, variant=1), dict(n_source=-1),
                dict(target=None), dict(mode=1), dict(mode=2), dict(mode=1, target=None, fy=-1),
                dict(used=None), dict(rows=None), dict(rows=odd), dict(cov=None), dict(acc=None),
                dict(mom=None), dict(err=None)):
        assert call(**bad) == -1, bad
    assert call(ws=8) == -2
    assert call(ws=8, mode=1, target=None) == -2


def test_moment_math_on_the_host_under_the_sanitizers(tmp_path):
    """Every group's centre, covariance, residual (both modes, one and two fields), F and error
    term of moment_math.h equal the reference's bit for bit; the program's vectors are exact-size
    allocations and it runs under the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "moment_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
    for n, G, two, mode in ((1000, 7, True, "covariance"), (1000, 7, True, "round"),
                            (300, 300, True, "covariance"), (1000, 30, False, "covariance"),
                            (65, 3, False, "covariance"), (1, 3, True, "round"),
                            (0, 1, True, "covariance")):
        (x, y, mask, group, perm, domain, kw), ref = _case(n, G, two, mode, True, True)
        one = np.ldexp(1.0, ref["mbits"])
        ms = [one / (d[1] - d[0]) for d in domain] + [0.0]
        lo = [d[0] for d in domain] + [0.0]
        tail = f8(kw["covariance"]) if mode == "covariance" else b""
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(struct.pack("<4q", G, int(two), int(mode == "round"), ref["mbits"])
                        + f8([lo[0], ms[0], lo[1], ms[1]]) + ref["acc"].tobytes()
                        + ref["mom"].tobytes() + tail)
        run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert run.returncode == 0, f"{n} {G} {two} {mode}: {run.stdout}{run.stderr}"
        f = np.frombuffer(dst.read_bytes(), dtype=np.float64).reshape(G, 16)
        assert np.array_equal(f[:, 0] != 0.0, ref["rays"])
        assert np.array_equal(f[:, 1] != 0.0, ref["used"])
        assert np.array_equal(f[:, 2], ref["acc"][:, 0].astype(np.float64))
        assert _bits_equal(f[:, 3:5], ref["group_rows"][:, :2]).all()
        assert _bits_equal(f[:, 5:11], ref["cov"]).all()
        assert _bits_equal(f[:, 13:16], ref["group_rows"][:, 2:5]).all()
        D = np.where(ref["used"][:, None], ref["cov"][:, 3:], 0.0)
        e = ref["acc"][:, 0] * ((D[:, 0] * D[:, 0] + 2.0 * (D[:, 1] * D[:, 1])) + D[:, 2] * D[:, 2])
        assert np.array_equal(f[:, 11], e)
        kx = [c[0] for c in ref["centres"]]
        assert all(f[g, 12] == kx[g] for g in range(G) if ref["used"][g])
