"""
SumError without a GPU: the CPU paths of ``ops.goal_error_columns`` and ``ops.error_combine``
against the numpy restatement of their definitions (tests/error_combine_reference.py) --
gradients, coefficients and the combined error bit for bit, the goal-columns sum within the bound
of a float64 sum of m non-negative terms in any order, m * 2^-52 * sum --, SumError's constructor
and ``set_weights`` errors, ``SumError.__call__`` against the sum of its terms called alone, and
csrc/combine_math.h on the host: tests/combine_host/combine_main.cpp (its own main) compiled with
g++ and the address and undefined-behaviour sanitizers.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import error_combine_reference as ref
from tensorflowraytrace_amd import ops, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "combine_host", "combine_main.cpp")

MASKS = ("none", "partial", "all_negative")
PERMS = ("none", "permutation", "out_of_range")


def goal_case(n, n_rows, fields, mask_kind, perm_kind, seed, dtype=np.float64, n_source=None):
    """(rows, goal (fields, n_source), mask, perm) of a goal-columns case."""
    rng = np.random.default_rng(seed)
    n_source = n + 3 if n_source is None else n_source
    rows = rng.standard_normal((n_rows, n)).astype(dtype)
    goal = rng.standard_normal((len(fields), n_source))
    mask = None
    if mask_kind == "partial":
        mask = np.where(rng.random(n) < 0.3, -1, rng.integers(0, 50, n)).astype(np.int32)
    elif mask_kind == "all_negative":
        mask = np.full(n, -1, dtype=np.int32)
    perm = None
    if perm_kind == "permutation":
        perm = rng.permutation(n_source)[:n].astype(np.int32)
    elif perm_kind == "out_of_range":
        perm = rng.integers(0, max(n_source, 1), n).astype(np.int32)
        bad = rng.random(n) < 0.25
        perm[bad] = rng.choice(np.array([-1, -2 ** 31, n_source, n_source + 7, 2 ** 31 - 1]),
                               int(bad.sum())).astype(np.int32)
    return rows, goal, mask, perm


def check_goal(out, want, fields, n_rows):
    err, grad = out
    assert np.array_equal(ref.bits(grad.numpy()), ref.bits(want["grad"]))
    total, terms, mean = want["error"]
    bound = ref.sum_bound(want["terms_each"])
    assert float(err[1]) == terms
    assert abs(float(err[0]) - total) <= bound
    if terms == 0:
        assert float(err[0]) == 0.0 and np.isnan(float(err[2])) and not grad.any()
    else:
        assert abs(float(err[2]) - mean) <= bound / terms + abs(mean) * ref.EPS


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("perm_kind", PERMS)
@pytest.mark.parametrize("by_ray", [False, True])
def test_goal_columns_cpu_path_equals_the_reference(mask_kind, perm_kind, by_ray):
    for n, n_rows, fields in ((1, 4, (3,)), (65, 6, (4, 5)), (1025, 6, (5, 0, 3)), (0, 6, (4,))):
        rows, goal, mask, perm = goal_case(n, n_rows, fields, mask_kind, perm_kind, seed=n + 1)
        table = np.ascontiguousarray(goal.T) if by_ray else goal
        want = ref.goal_error_columns(rows, fields, table, mask, perm, by_ray)
        out = ops.goal_error_columns(
            torch.as_tensor(rows), fields, torch.as_tensor(table),
            mask=None if mask is None else torch.as_tensor(mask),
            perm=None if perm is None else torch.as_tensor(perm), by_ray=by_ray)
        check_goal(out, want, fields, n_rows)
        if mask_kind == "all_negative" or n == 0:
            assert want["error"][1] == 0


def test_goal_columns_padded_stride_float32_and_untouched_rows():
    """float32 rows give the reference of the upcast values; a padded stride changes nothing; a
    row that is no field keeps what the caller's block held."""
    n, fields = 333, (4, 1)
    rows, goal, mask, perm = goal_case(n, 6, fields, "partial", "out_of_range", 9, np.float32)
    block = torch.zeros((6, n + 7), dtype=torch.float32)
    block[:, :n] = torch.as_tensor(rows)
    grad = torch.full((6, n + 5), 7.0, dtype=torch.float64)
    err, g = ops.goal_error_columns(block[:, :n], fields, torch.as_tensor(goal),
                                    mask=torch.as_tensor(mask), perm=torch.as_tensor(perm),
                                    grad=grad)
    want = ref.goal_error_columns(rows, fields, goal, mask, perm)
    assert g is grad
    for r in range(6):
        if r in fields:
            assert np.array_equal(ref.bits(grad[r, :n].numpy()), ref.bits(want["grad"][r]))
        else:
            assert bool((grad[r] == 7.0).all())
    assert bool((grad[:, n:] == 7.0).all())
    assert abs(float(err[0]) - want["error"][0]) <= ref.sum_bound(want["terms_each"])
    # a goal shorter than the columns: the columns beyond it do not count
    short = ref.goal_error_columns(rows, fields, goal, None, None, n_source=100)
    assert short["error"][1] == 2 * 100
    e2, _ = ops.goal_error_columns(torch.as_tensor(rows), fields, torch.as_tensor(goal),
                                   n_source=100)
    assert float(e2[1]) == 200.0


def test_goal_columns_argument_errors():
    rows = torch.zeros((6, 5), dtype=torch.float64)
    goal = torch.zeros((2, 5), dtype=torch.float64)
    for bad in ((4, 4), (6, 0), (), (-1, 2)):
        with pytest.raises(ValueError, match="fields"):
            ops.goal_error_columns(rows, bad, goal[:len(bad)] if bad else goal)
    with pytest.raises(ValueError, match="rows"):
        ops.goal_error_columns(torch.zeros((5, 5), dtype=torch.float64), (0, 1), goal)
    with pytest.raises(ValueError, match="goal"):
        ops.goal_error_columns(rows, (0, 1), goal.float())
    with pytest.raises(ValueError, match="goal"):
        ops.goal_error_columns(rows, (0, 1, 2), goal)
    with pytest.raises(ValueError, match="n_source"):
        ops.goal_error_columns(rows, (0, 1), goal, n_source=6)
    with pytest.raises(ValueError, match="mask"):
        ops.goal_error_columns(rows, (0, 1), goal, mask=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="perm"):
        ops.goal_error_columns(rows, (0, 1), goal, perm=torch.zeros(5, dtype=torch.int64))


def combine_case(K, n, n_rows, masks, seed, pad=0, zero_terms=()):
    """K terms with the row masks ``masks``: blocks of n + pad columns, triples with random sums
    and counts (``zero_terms``: terms whose count is 0)."""
    rng = np.random.default_rng(seed)
    terms = []
    for k in range(K):
        g = rng.standard_normal((n_rows, n + pad))
        if n:
            g[rng.integers(0, n_rows), rng.integers(0, n)] = -0.0
        count = 0.0 if k in zero_terms else float(rng.integers(1, 5000))
        total = 0.0 if k in zero_terms else float(rng.random() * 10)
        e = np.array([total, count, total / count if count else np.nan])
        terms.append((g, masks[k], e))
    return terms, rng.random(K) * 3.0


def run_combine(terms, weights, reduce, n, n_rows, with_grad=True):
    tt = [(torch.as_tensor(g)[:, :n] if with_grad else None, m, torch.as_tensor(e))
          for g, m, e in terms]
    return ops.error_combine(tt, torch.as_tensor(np.asarray(weights, dtype=np.float64)), reduce,
                             n=n, n_rows=n_rows)


def check_combine(out, want):
    err, grad, coeff = out
    assert np.array_equal(ref.bits(coeff.numpy()), ref.bits(want["coeff"]))
    assert np.array_equal(ref.bits(err.numpy()), ref.bits(np.array(want["error"])))
    if want["grad"] is None:
        assert grad is None
    else:
        assert np.array_equal(ref.bits(grad.numpy()), ref.bits(want["grad"]))


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("K,n_rows,masks", [
    (1, 6, (0b110000,)),
    (2, 6, (0b110000, 0b110000)),              # overlapping
    (2, 6, (0b110000, 0b000011)),              # disjoint, rows 2 and 3 named by nobody
    (3, 4, (0b1100, 0b0100, 0b1111)),
    (8, 6, (0x3f, 0x30, 0x03, 0x11, 0x20, 0x3f, 0x0c, 0x30)),
])
def test_error_combine_cpu_path_equals_the_reference(reduce, K, n_rows, masks):
    for n, pad in ((1, 0), (65, 3), (1025, 0), (0, 0)):
        terms, weights = combine_case(K, n, n_rows, masks, seed=K * 100 + n, pad=pad,
                                      zero_terms=(K - 1,) if K > 1 else ())
        if K > 2:
            weights[1] = 0.0                   # a term switched off
        want = ref.error_combine([(g[:, :n], m, e) for g, m, e in terms], weights, reduce, n,
                                 n_rows)
        check_combine(run_combine(terms, weights, reduce, n, n_rows), want)
        if reduce == "mean" and K > 1:
            assert want["coeff"][K - 1] == 0.0     # no terms: the coefficient is 0, not inf
        # without gradient blocks only the errors are combined
        alone = run_combine(terms, weights, reduce, n, n_rows, with_grad=False)
        assert alone[1] is None
        assert np.array_equal(ref.bits(alone[0].numpy()), ref.bits(np.array(want["error"])))


def test_one_term_with_weight_one_returns_its_own_bits():
    n = 257
    terms, _ = combine_case(1, n, 6, (0b110100,), seed=5)
    g = terms[0][0]
    g[2, :5] = [-0.0, 0.0, np.inf, -np.inf, 5e-324]
    err, out, coeff = run_combine(terms, [1.0], "sum", n, 6)
    for r in (2, 4, 5):
        assert np.array_equal(ref.bits(out[r].numpy()), ref.bits(g[r]))
    for r in (0, 1, 3):
        assert np.array_equal(ref.bits(out[r].numpy()), ref.bits(np.zeros(n)))
    assert float(coeff[0]) == 1.0 and float(err[0]) == terms[0][2][0] and float(err[1]) == 1.0


def test_error_combine_argument_errors():
    e = torch.zeros(3, dtype=torch.float64)
    g = torch.zeros((6, 4), dtype=torch.float64)
    w = torch.ones(1, dtype=torch.float64)
    with pytest.raises(ValueError, match="terms"):
        ops.error_combine([], torch.ones(0, dtype=torch.float64))
    with pytest.raises(ValueError, match="terms"):
        ops.error_combine([(g, 1, e)] * 9, torch.ones(9, dtype=torch.float64))
    with pytest.raises(ValueError, match="n_rows"):
        ops.error_combine([(g, 1, e)], w, n_rows=5)
    with pytest.raises(ValueError, match="weights"):
        ops.error_combine([(g, 1, e)], torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="reduce"):
        ops.error_combine([(g, 1, e)], w, reduce="max")
    with pytest.raises(ValueError, match="row_mask"):
        ops.error_combine([(g, 1 << 6, e)], w)
    with pytest.raises(ValueError, match="grad"):
        ops.error_combine([(g, 1, e)], w, n=5)
    with pytest.raises(ValueError, match="every term"):
        ops.error_combine([(g, 1, e), (None, 1, e)], torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="error"):
        ops.error_combine([(g, 1, e.float())], w)


def _density(**kw):
    return optimizer.DensityError(("y_end", "z_end"), np.ones((3, 4)), ((-1.0, 1.0), (-1.0, 1.0)),
                                  **kw)


def test_sum_error_constructor_and_set_weights_errors():
    S = optimizer.SumError
    d = _density()
    g = optimizer.GoalError(("y_end",), torch.zeros(4, 1))
    s = S([d, g])
    assert s.terms == (d, g) and s.reduce == "sum"
    assert s.weights.dtype == torch.float64 and s.weights.tolist() == [1.0, 1.0]
    assert s.rows == [4, 5, 4]
    with pytest.raises(ValueError, match="1 .. 8 terms"):
        S([])
    with pytest.raises(ValueError, match="1 .. 8 terms"):
        S([_density() for _ in range(9)])
    with pytest.raises(ValueError, match="sequence"):
        S(d)
    with pytest.raises(ValueError, match="RowwiseError"):
        S([d, optimizer.RowwiseError(lambda rays: rays["y_end"] ** 2)])
    with pytest.raises(ValueError, match="nested SumError"):
        S([d, S([g])])
    with pytest.raises(ValueError, match="twice"):
        S([d, g, d])
    with pytest.raises(ValueError, match="terms must be"):
        S([d, lambda engine: 0.0])
    with pytest.raises(ValueError, match="reduce"):
        S([d], reduce="max")
    for bad in ([1.0], [1.0, -0.5], [1.0, np.nan], [np.inf, 1.0], "ab", [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="weights"):
            S([d, g], weights=bad)
        with pytest.raises(ValueError, match="weights"):
            s.set_weights(bad)
    ptr, key = s.weights.data_ptr(), s.graph_key()
    s.set_weights([0.25, 0.0])
    assert s.weights.tolist() == [0.25, 0.0]
    assert s.weights.data_ptr() == ptr and s.graph_key() == key
    assert S([d, g], reduce="mean").graph_key() != key
    # exported where the terms are, and through the tfrt shim
    import tfrt.optimizer
    assert tfrt.optimizer.SumError is S
    # a sum of terms never takes the fused 2-D step
    from tensorflowraytrace_amd.fused_step import FusedStep

    class _Eng:
        dimension, ray_shard = 2, None

        @staticmethod
        def _custom_ops():
            return False

    class _Opt:
        engine, error_function, parameters = _Eng(), s, []
    assert FusedStep.eligible2d(_Opt()) is False and FusedStep.eligible(_Opt(), (), {}) is False


class _Engine:
    """What the terms' generic paths read of an engine: the finished rays, their source rays and
    the source set."""
    dimension = 3

    def __init__(self, n, n_source, seed):
        rng = np.random.default_rng(seed)
        self.leaves = {f: torch.tensor(rng.uniform(-1.2, 1.2, n), requires_grad=True)
                       for f in ("y_end", "z_end")}
        self.finished_rays = dict(self.leaves)
        self.last_trace = {"finished_id": torch.as_tensor(rng.permutation(n_source)[:n])}
        self._trace_src = {"x_start": torch.zeros(n_source, dtype=torch.float64),
                           "aim": torch.as_tensor(rng.standard_normal((n_source, 2)))}


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_the_generic_path_is_the_weighted_sum_of_its_terms_called_alone(reduce):
    """SumError.__call__ on CPU tensors against the terms called alone and combined by the
    reference; the gradient on the finished rays' fields is the combination of the terms' own."""
    n, n_source = 300, 320
    d = _density(oob_weight=0.3)
    d.goal = d.goal.cpu()
    g = optimizer.GoalError(("y_end", "z_end"), lambda src: 0.5 * src["aim"])
    weights = [0.7, 1e-3]
    s = optimizer.SumError([d, g], weights, reduce)
    s.weights = s.weights.cpu()

    eng = _Engine(n, n_source, 3)
    alone, grads = [], []
    for term in (d, g):
        e = term(eng)
        gy, gz = torch.autograd.grad(e.sum(), [eng.leaves["y_end"], eng.leaves["z_end"]])
        alone.append((float(e.detach().sum()), float(e.numel())))
        grads.append(np.stack([np.zeros(n)] * 4 + [gy.numpy(), gz.numpy()]))
    assert alone[0][1] == 1.0 and alone[1][1] == 2.0 * n
    triples = [np.array([t, m, t / m]) for t, m in alone]
    want = ref.error_combine([(grads[k], 0b110000, triples[k]) for k in range(2)], weights,
                             reduce, n, 6)

    e = s(eng)
    assert e.shape == (1,)
    gy, gz = torch.autograd.grad(e.sum(), [eng.leaves["y_end"], eng.leaves["z_end"]])
    assert float(e.detach()) == want["error"][0]
    assert np.array_equal(ref.bits(s.last_coefficients.numpy()), ref.bits(want["coeff"]))
    assert np.array_equal(s.last_errors[:, :2].numpy(), np.stack(triples)[:, :2])
    scale = np.abs(want["grad"]).max()
    assert np.abs(gy.numpy() - want["grad"][4]).max() <= 4 * ref.EPS * scale
    assert np.abs(gz.numpy() - want["grad"][5]).max() <= 4 * ref.EPS * scale
    # a weight of 0 switches a term off; the term is still evaluated
    s.set_weights([1.0, 0.0])
    d.last_hq = None
    e0 = s(eng)
    assert d.last_hq is not None
    assert float(e0.detach()) == alone[0][0] * (1.0 if reduce == "sum" else 1.0 / alone[0][1])
    # no finished ray: the density term is its goal's square, the goal term has no terms
    eng.finished_rays = {}
    e1 = s(eng)
    assert abs(float(e1.detach()) - 1.0) <= 12 * ref.EPS and float(s.last_errors[1, 1]) == 0.0
    assert float(s.last_coefficients[1]) == 0.0


def test_combine_math_on_the_host_under_the_sanitizers(tmp_path):
    """combine_math.h in a program of its own (exact-size allocations: an index past a block or the
    goal table would be found) gives the reference's bits."""
    exe = tmp_path / "combine_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
    masks8 = (0x3f, 0x30, 0x03, 0x11, 0x20, 0x3f, 0x0c, 0x30)
    for K, n, n_rows, reduce in ((1, 7, 6, "sum"), (3, 65, 4, "mean"), (8, 130, 6, "mean"),
                                 (2, 0, 6, "sum")):
        masks = tuple(m & ((1 << n_rows) - 1) for m in masks8[:K])
        terms, weights = combine_case(K, n, n_rows, masks, seed=K + n,
                                      zero_terms=(K - 1,) if K > 1 else ())
        want = ref.error_combine(terms, weights, reduce, n, n_rows)
        m, n_source = 97, 40
        rows, goal, _, perm = goal_case(m, 4, (2,), "none", "out_of_range", 17, n_source=n_source)
        gwant = ref.goal_error_columns(rows, (2,), goal, None, perm)
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(
            struct.pack("<6q", K, n, n_rows, 0 if reduce == "sum" else 1, m, n_source)
            + f8(weights) + f8([t[2][1] for t in terms]) + f8([t[2][0] for t in terms])
            + np.asarray(masks, dtype=np.int32).tobytes() + f8(np.stack([t[0] for t in terms]))
            + f8(rows[2]) + perm.astype(np.int64).tobytes() + f8(goal[0]))
        run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert run.returncode == 0, f"{K} {n} {n_rows} {reduce}: {run.stdout}{run.stderr}"
        got = np.frombuffer(dst.read_bytes(), dtype=np.float64)
        assert got.size == K + 1 + n_rows * n + 2 * m
        assert np.array_equal(ref.bits(got[:K]), ref.bits(want["coeff"]))
        assert ref.bits(got[K:K + 1])[0] == ref.bits(np.array([want["error"][0]]))[0]
        out = got[K + 1:K + 1 + n_rows * n].reshape(n_rows, n)
        if n:
            assert np.array_equal(ref.bits(out), ref.bits(want["grad"]))
        term, seed = got[K + 1 + n_rows * n:].reshape(2, m)
        assert np.array_equal(ref.bits(term), ref.bits(gwant["terms_each"][0]))
        assert np.array_equal(ref.bits(seed), ref.bits(gwant["grad"][2]))
