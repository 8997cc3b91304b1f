"""
The error terms' module (tensorflowraytrace_amd/errors.py) and the protocol between a built-in
term and the fused step, on CPU tensors: ``term.seed_columns(cols, hold)`` goes through the
wrappers' CPU paths and the library's host-only sizing entries and must leave exactly what a direct
``ops.*`` call with the same arguments leaves.  No GPU.
"""
import numpy as np
import pytest
import torch

from tensorflowraytrace_amd import _lib, errors, fused_step, ops
from tensorflowraytrace_amd.errors import (DensityError, GoalError, RowwiseError, SpotError,
                                           SumError, TransportError, _Columns)
from tensorflowraytrace_amd.fused_step import _StepState, _TermState

N = 70                                  # more than one wavefront's worth, no multiple of 64
G = 5
DOMAIN = ((-1.0, 1.0), (-0.9, 1.1))
CPU = torch.device("cpu")
REMOVED_SLOTS = {"density_ws", "hq", "spot_ws", "acc", "transport_ws", "rank2", "goal_ws"}


def _goal_map(ny=6, nx=7):
    gy, gx = np.meshgrid(np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
    return np.exp(-(gx ** 2 + gy ** 2) / 0.5)


@pytest.fixture(scope="module")
def cols():
    """70 columns: starts near the origin, ends on a plane a unit away and partly outside
    DOMAIN; every fifth column masked out; the trace's order a non-identity permutation."""
    rng = np.random.default_rng(7)
    rows = np.concatenate([rng.uniform(-0.2, 0.2, (3, N)), rng.uniform(-1.3, 1.3, (3, N))])
    rows[3] = 1.0 + 0.1 * rows[3]
    mask = np.where(np.arange(N) % 5 == 4, -1, np.arange(N) % 7).astype(np.int32)
    perm = rng.permutation(N).astype(np.int32)
    assert not np.array_equal(perm, np.arange(N))
    src = {"x_start": torch.zeros(N, dtype=torch.float64)}
    return _Columns(torch.tensor(rows), torch.tensor(mask), torch.tensor(perm), src, N)


def _weights():
    return np.random.default_rng(3).uniform(0.1, 1.0, N)


def _labels():
    return np.where(np.arange(N) % 11 == 10, -1, np.arange(N) % G)


def _term(kind, fields, weights=False):
    two = len(fields) == 2
    domain = DOMAIN if two else DOMAIN[:1]
    w = _weights() if weights else None
    if kind == "goal":
        return GoalError(fields, torch.tensor(np.random.default_rng(5).normal(size=(N, len(fields)))))
    if kind == "density":
        goal = _goal_map() if two else _goal_map()[0]
        return DensityError(fields, goal, domain, oob_weight=0.3, weights=w)
    if kind == "spot":
        return SpotError(fields, _labels(), domain, oob_weight=0.3, n_groups=G, weights=w)
    goal = _goal_map() if two else _goal_map()[0]
    return TransportError(fields, goal, domain, directions=3, knots=16)


def _direct(term, cols):
    """(err, grad, kept buffer) of a direct ops call with the arguments ``seed_columns`` passes,
    into fresh buffers of the shapes and initial values the step gives them."""
    L = _lib.lib()
    grad = torch.zeros((6, N), dtype=torch.float64)
    err = torch.zeros(3, dtype=torch.float64)
    row_x, row_y = term.rows[0], (term.rows[1] if len(term.rows) == 2 else -1)
    if isinstance(term, GoalError):
        ws = torch.empty(max(L.tfrt_goal_error_columns_workspace_bytes(N), 1), dtype=torch.uint8)
        ops.goal_error_columns(cols.rows, term.rows, term.table(cols.src, by_ray=True),
                               mask=cols.mask, perm=cols.perm, by_ray=True, grad=grad, err=err,
                               workspace=ws)
        return err, grad, None
    if isinstance(term, DensityError):
        goal = term.goal_on(CPU)
        nx, ny = goal.shape[-1], (goal.shape[0] if goal.dim() == 2 else 1)
        ws = torch.empty(max(L.tfrt_density_error_workspace_bytes(N, nx, ny), 1), dtype=torch.uint8)
        w = term.weights_of(cols.src)
        hq = torch.zeros(goal.shape, dtype=torch.int64)
        ops.density_error(cols.rows, row_x, row_y, goal, term.grid, term.oob_weight, mask=cols.mask,
                          variant=0, dimension=3, weights=w,
                          perm=cols.perm if w is not None else None, grad=grad, err=err, hq=hq,
                          workspace=ws)
        return err, grad, hq
    if isinstance(term, SpotError):
        labels, w = term.labels_of(cols.src), term.weights_of(cols.src)
        qbits, grid = term.grid_for(N)
        ws = torch.empty(max(L.tfrt_spot_error_workspace_bytes(N, G), 1), dtype=torch.uint8)
        acc = torch.zeros((G, 4 if w is None else 8), dtype=torch.int64)
        ops.spot_error(cols.rows, row_x, row_y, labels, G, grid, term.oob_weight, mask=cols.mask,
                       perm=cols.perm, variant=0, qbits=qbits, dimension=3, weights=w,
                       wbits=None if w is None else ops.spot_wbits(N), grad=grad, err=err, acc=acc,
                       workspace=ws)
        return err, grad, acc
    tables, angles = term.tables_on(CPU)
    K = term.n_directions
    ws = torch.empty(max(L.tfrt_transport_error_workspace_bytes(N, K), 1), dtype=torch.uint8)
    rank2 = torch.zeros((K, N), dtype=torch.int32)
    ops.transport_error(cols.rows, row_x, row_y, tables, term.grid, angles, mask=cols.mask,
                        dimension=3, grad=grad, err=err, rank2=rank2, workspace=ws)
    return err, grad, rank2


def _bits(t):
    return t.contiguous().view(torch.int64)


CASES = [(kind, fields, False) for kind in ("goal", "density", "spot", "transport")
         for fields in (("y_end", "z_end"), ("z_end",))]
CASES += [(kind, fields, weights) for kind in ("density", "spot")
          for fields, weights in ((("y_dir", "z_end"), False), (("y_end", "z_end"), True))]


@pytest.mark.parametrize("kind,fields,weights", CASES,
                         ids=[f"{k}-{'+'.join(f)}{'-weighted' if w else ''}" for k, f, w in CASES])
def test_seed_columns_equals_the_direct_call(cols, kind, fields, weights):
    term = _term(kind, fields, weights)
    hold = _TermState(torch.zeros((6, N), dtype=torch.float64),
                      torch.zeros(3, dtype=torch.float64), term.seed_rows)
    term.seed_columns(cols, hold)
    err, grad, kept = _direct(_term(kind, fields, weights), cols)
    assert torch.equal(_bits(hold.g_fin), _bits(grad))
    assert torch.equal(_bits(hold.err), _bits(err)) and float(err[1]) > 0
    name = {"density": "hq", "spot": "acc", "transport": "rank2"}.get(kind)
    assert set(hold.buffers) == {"workspace"} | ({name} if name else set())
    if name:
        last = getattr(term, "last_" + name)
        assert last is hold.buffers[name] and torch.equal(last, kept) and bool(kept.any())
    # the rows it writes are the rows it says it writes
    written = sum(1 << r for r in range(6) if bool(hold.g_fin[r].any()))
    assert written == term.seed_rows
    assert term.seed_rows == (0x3f if "y_dir" in fields else sum(1 << r for r in term.rows))
    # a second step allocates nothing and leaves the same bits
    before = {k: v.data_ptr() for k, v in hold.buffers.items()}
    term.seed_columns(cols, hold)
    assert {k: v.data_ptr() for k, v in hold.buffers.items()} == before
    assert torch.equal(_bits(hold.g_fin), _bits(grad)) and torch.equal(_bits(hold.err), _bits(err))


def test_the_classes_are_the_same_objects_everywhere():
    import tfrt.optimizer as optimizer
    for name in ("GoalError", "RowwiseError", "DensityError", "SpotError", "TransportError",
                 "SumError"):
        assert getattr(errors, name) is getattr(fused_step, name) is getattr(optimizer, name)


def test_every_built_in_term_has_the_protocol():
    for cls in (GoalError, DensityError, SpotError, TransportError):
        for name in ("rows_for", "graph_key", "seed_rows", "seed_columns"):
            assert hasattr(cls, name), (cls.__name__, name)
    assert not hasattr(RowwiseError, "seed_columns")
    assert not REMOVED_SLOTS & set(_TermState.__slots__)
    assert REMOVED_SLOTS & set(_StepState.__slots__) == {"goal_ws"}     # (tfrt_goal_error3d's)
    assert "term" in _StepState.__slots__


def test_a_sum_errors_graph_key_is_the_tuple_it_was():
    terms = [_term("goal", ("y_end", "z_end")), _term("density", ("y_end", "z_end"), True),
             _term("spot", ("y_dir", "z_end")), _term("transport", ("z_end",))]
    both = SumError(terms, [1.0, 2.0, 0.0, 0.5], "mean")
    want = (tuple((id(t), t.graph_key() if isinstance(t, (DensityError, SpotError, TransportError))
                   else (id(t.goal), t.fields, t.rowwise)) for t in terms),
            both.weights.data_ptr(), both.reduce)
    assert both.graph_key() == want
    assert terms[0].graph_key() == (id(terms[0].goal), ("y_end", "z_end"), False)


# ------------------------------------------------------------------ the wrappers' checks
def _density(rows, row_x, row_y, **kw):
    goal = torch.tensor(_goal_map() if row_y >= 0 else _goal_map()[0])
    goal = goal / torch.linalg.norm(goal)
    return ops.density_error(rows, row_x, row_y, goal,
                             ops.density_grid(DOMAIN, 7, 6 if row_y >= 0 else None), **kw)


def _spot(rows, row_x, row_y, **kw):
    n = rows.shape[1]
    return ops.spot_error(rows, row_x, row_y, torch.zeros(n, dtype=torch.int32), 1,
                          ops.spot_grid(DOMAIN, ops.spot_qbits(n)), **kw)


def _transport(rows, row_x, row_y, **kw):
    cs = ops.transport_directions(3)
    tables = torch.as_tensor(ops.transport_tables(_goal_map(), DOMAIN, cs, 16))
    return ops.transport_error(rows, row_x, row_y, tables, ops.transport_grid(DOMAIN),
                               torch.as_tensor(cs), **kw)


def _goal(rows, row_x, row_y, **kw):
    return ops.goal_error_columns(rows, (row_x, row_y),
                                  torch.zeros((2, rows.shape[1]), dtype=torch.float64), **kw)


@pytest.mark.parametrize("call", [_density, _spot], ids=["density_error", "spot_error"])
def test_plain_rows_must_lie_inside_the_block(call):
    rows = torch.tensor(np.random.default_rng(1).uniform(-1, 1, (2, 9)))
    call(rows, 0, 1)
    call(rows, 1, -1)
    for row_x, row_y in ((2, -1), (5, -1), (2, 1), (5, 0), (0, 2), (0, 0), (1, 1), (-1, 0), (0, -2)):
        with pytest.raises(ValueError, match="rows must be distinct"):
            call(rows, row_x, row_y)


@pytest.mark.parametrize("call", [_density, _spot, _transport, _goal],
                         ids=["density_error", "spot_error", "transport_error",
                              "goal_error_columns"])
def test_a_bad_mask_is_refused(call):
    rows = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (4, 9)))
    call(rows, 2, 3, mask=torch.zeros(9, dtype=torch.int32))
    for bad in (torch.zeros(9, dtype=torch.int64), torch.zeros(8, dtype=torch.int32),
                torch.zeros(18, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="mask"):
            call(rows, 2, 3, mask=bad)
    with pytest.raises(ValueError, match="grad"):
        call(rows, 2, 3, grad=torch.zeros((4, 9), dtype=torch.float32))
    with pytest.raises(ValueError, match="grad"):
        call(rows, 2, 3, grad=torch.zeros((3, 9), dtype=torch.float64))
