"""
The declarative error terms of the optimiser, and what the fused step (fused_step.FusedStep) asks
of one.

The error functions of the reference's optimisation scripts all have one form
(dev/hexalens.py:144-168):  ``squared_difference(stack(finished[fields]), goal)`` with ``goal``
a function of fields the finished rays inherit unchanged from their source rays.  ``GoalError``
states that form declaratively.  A ``RowwiseError`` is torch code that works row by row on the
finished rays.  The coupled errors take all finished rays of a step into one evaluation (one
process): a ``DensityError`` -- the finished rays, taken together, must land with a given density
-- is ``tfrt_density_error`` (four launches: clear, splat, bins, seed); a ``SpotError`` -- rays of
one group must meet in one point -- ``tfrt_spot_error`` (clear, accumulate, seed, finish); a
``TransportError`` -- the same target density by sliced optimal transport --
``tfrt_transport_error`` (per direction keys, radix sort, sorted keys, ranks; then seed and
finish); a ``FocusError`` -- rays of one group, taken as lines, must pass through one point of
space -- ``tfrt_focus_error`` (clear, accumulate, solve, seed, finish); a ``DistortionError`` --
the groups' centroids must be a scaled or affine copy of the object points --
``tfrt_distortion_error`` (clear, SpotError's accumulate, fit, seed); a ``FlatFieldError`` -- the
foci of all groups must lie in one plane with a given normal -- ``tfrt_flatfield_error`` (clear,
FocusError's accumulate, fit, seed); a ``CentroidError`` -- every group's centroid must lie at a
given target, or the centroids of the groups of one parent must coincide --
``tfrt_centroid_error`` (clear, SpotError's accumulate, with parents their records, table, seed);
a ``MomentError`` -- the covariance of every group's rays, the size and the shape of its spot, must
be a given matrix, or must be round -- ``tfrt_moment_error`` (clear, SpotError's accumulate on a
finer grid, the integer centres, the limb products about them, table, seed); a ``MixingError``
-- every group of rays must land with the same density, whatever that density is: with ``Hq`` the
int64 bilinear histogram of ``DensityError`` kept per group, ``p_gb = Hq_gb / nq_g`` a group's
density and ``m_b = Pq_b / Nq`` the pooled one (``nq``, ``Pq``, ``Nq``: the integer margins), the
error is ``sum_g (nq_g / Nq) * B * sum_b (p_gb - m_b)**2`` plus ``DensityError``'s penalties and
the pull on a cell ``D_gb = (2 * B / N) * (p_gb - m_b)``, ``N = Nq * 2**-32`` --
``tfrt_mixing_error`` (clear, splat, margins, pulls, finish, seed).
A ``SumError`` is a weighted sum of such terms and of ``GoalError``s: every term's launches into a
seed block of its own (a ``GoalError`` through ``tfrt_goal_error_columns``), then ONE
``tfrt_error_combine`` for the step's seed block and error.

Each is an ordinary error function (``__call__(engine)``): the generic path gives the same
numbers, which is what the parity tests compare.

The protocol between a built-in term (``GoalError``, ``DensityError``, ``SpotError``,
``TransportError``, ``FocusError``, ``DistortionError``, ``FlatFieldError``, ``CentroidError``,
``MomentError``, ``MixingError``) and the fused 3-D step:

* ``rows``, ``fields``, ``rows_for(dimension)``: the rows of the ray block (the field codes) the
  term reads;
* ``graph_key()``: what a captured step has baked in of the term;
* ``seed_rows``: the bitmask of the rows of a (6, N) seed block the term writes;
* ``seed_columns(cols, hold)``: the term's launches on the step's fixed-shape columns ``cols`` (a
  ``_Columns``).  ``hold`` has the term's (6, capN) float64 seed block ``g_fin``, zeroed once, its
  error triple ``err`` and a dict ``buffers`` that the term fills on first use -- and again when a
  shape they depend on changes -- with the buffers its kind keeps, under the names its
  ``evaluate`` takes them by.  The rows of ``seed_rows`` of ``hold.g_fin`` are written for every
  column, and ``hold.err``; the term's ``last_hq`` / ``last_acc`` / ``last_rank2`` are those
  buffers.  Nothing is read back.
"""
import collections

import numpy as np
import torch

from . import _lib, ops

# What a step offers every term: the (6, N) view ``rows`` of the finished rows at the rays' own
# columns, the int32 ``mask`` (column i counts if mask[i] >= 0), the trace's order ``perm`` (the
# source ray of column i; None: the source's own order), the source set ``src`` and N.
_Columns = collections.namedtuple("_Columns", "rows mask perm src n")

_GEO3 = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
_GEO2 = ("x_start", "y_start", "x_end", "y_end")
# the fields of the coupled errors (DensityError, SpotError): a row of the geometry block or a
# direction cosine of the finished ray's last link; the index is the field code of
# tfrt_density_error_fields / tfrt_spot_error_fields
_FIELDS3 = _GEO3 + ("x_dir", "y_dir", "z_dir")
_FIELDS2 = _GEO2 + ("x_dir", "y_dir")


def _source_key(src):
    """(key, vals) of the source set ``src``: a cache key made of the versions of its fields, and
    the tensors it is made of -- kept with the key, they stay alive and their ids stay theirs."""
    if hasattr(src, "cache_key"):      # rays made in place (sources.DeviceRaySet): lazy fields
        return src.cache_key, [src]
    vals = list(src.values()) if hasattr(src, "values") else [src[k] for k in src.keys()]
    return tuple((id(v), getattr(v, "_version", None)) for v in vals), vals


def _source_size(src):
    """(ray count, device) of the source set ``src``."""
    if hasattr(src, "n_rays"):
        return src.n_rays, src.device
    return src["x_start"].shape[0], src["x_start"].device


def _xy(codes):
    """(row_x, row_y) as the column errors take them: -1 for the y of one field."""
    return codes[0], codes[1] if len(codes) == 2 else -1


def _workspace(n_bytes, device):
    return torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=device)


class _Term:
    """What the built-in terms share of the fused step's protocol (module docstring)."""
    has_direction = False
    # True: a step with this error alone runs on every source ray's fixed-shape column
    # (FusedStep._rowwise3d / _rowwise2d); False: the goal steps (_goal3d / _goal2d)
    on_columns = False

    @property
    def seed_rows(self):
        """The bitmask of the rows of a (6, N) seed block that ``seed_columns`` writes: the
        fields' own, all six with a direction field (the chain rule onto start and end)."""
        return 0x3f if self.has_direction else sum(1 << r for r in self.rows)


class GoalError(_Term):
    """``error = squared_difference(stack([finished[f] for f in fields], axis=1), goal)``.

    ``goal``: a callable taking the field dict of the SOURCE rays and returning one goal row per
    source ray, shape (N, len(fields)) (or (N,) for a single field); or such a tensor.  Finished
    rays look their row up through the source-ray index the trace carries, which equals
    evaluating the same expression on the fields a finished ray inherits (engine.py:2242-2281).

    Example (dev/hexalens.py:154-157, magnification m)::

        erf = GoalError(("y_end", "z_end"), lambda src: -m * src["object_coords"][:, 1:])

    On a 2-D engine the fields come from ``x_start, y_start, x_end, y_end`` (``rows_for(2)``);
    dev/optimize_single_arc.py's error is ``GoalError(("y_end",), zeros)``.
    """

    def __init__(self, fields=("y_end", "z_end"), goal=None, rowwise=False):
        self.fields = tuple(fields)
        # ``rowwise=True`` states that a callable ``goal`` computes row i from ray i's fields alone
        # (dev/hexalens.py:154-157 does: a multiple of the ray's object coordinates).  The fused
        # step may then evaluate it on the source in whatever order it traces the rays, instead of
        # permuting a table made in source order -- for a source re-drawn every step that saves a
        # random gather per step.  Leave it False for goals that depend on a ray's POSITION in the
        # source (a table closed over by the callable, a linspace over the rays, ...).
        self.rowwise = bool(rowwise)
        if not self.fields or any(f not in _GEO3 for f in self.fields):
            raise ValueError(f"GoalError: fields must be taken from {_GEO3}, got {fields!r}")
        if goal is None:
            raise ValueError("GoalError: a goal (callable or tensor) is required")
        if len(set(self.fields)) != len(self.fields):
            raise ValueError(f"GoalError: duplicate fields in {fields!r}")
        self.rows = [_GEO3.index(f) for f in self.fields]
        self.goal = goal
        self._cache = None

    def rows_for(self, dimension):
        """Rows of the ray block of a ``dimension``-D trace that the fields are read from (a 3-D
        block is x_start .. z_end, a 2-D one x_start, y_start, x_end, y_end)."""
        if dimension == 3:
            return self.rows
        bad = [f for f in self.fields if f not in _GEO2]
        if bad:
            raise ValueError(f"GoalError: field(s) {bad} do not exist on a {dimension}-D engine "
                             f"(fields of its rays: {_GEO2})")
        return [_GEO2.index(f) for f in self.fields]

    def table(self, src, by_ray=False):
        """(len(fields), N) contiguous float64 goal table of the source set ``src``; with
        ``by_ray`` the (N, len(fields)) contiguous form the callable returns (no transposed copy:
        tfrt_goal_error3d takes either layout)."""
        key, vals = _source_key(src)
        key = (key, bool(by_ray))
        if self._cache is not None and self._cache[0] == key:
            return self._cache[1]
        g = self.goal(src) if callable(self.goal) else self.goal
        n, dev = _source_size(src)
        g = torch.as_tensor(g, dtype=torch.float64, device=dev).detach()
        if g.dim() == 1:
            g = g.reshape(-1, 1)
        if tuple(g.shape) != (n, len(self.fields)):
            raise ValueError(f"GoalError: goal has shape {tuple(g.shape)}, expected "
                             f"({n}, {len(self.fields)}) -- one row per source ray")
        table = g.contiguous() if by_ray else g.t().contiguous()
        self._cache = (key, table, vals)     # the keyed tensors stay alive with the key
        return table

    def graph_key(self):
        """What a captured step has baked in: the goal, the fields and the order the goal is
        evaluated in."""
        return (id(self.goal), self.fields, self.rowwise)

    def seed_columns(self, cols, hold):
        """tfrt_goal_error_columns on the step's columns: it reads the goal table in the source's
        order and looks a column's row up through the trace's order ``cols.perm`` itself (no
        permuted copy that could go stale when a source is re-drawn and re-ordered inside the
        graph)."""
        if not hold.buffers:
            hold.buffers["workspace"] = _workspace(
                _lib.lib().tfrt_goal_error_columns_workspace_bytes(cols.n), cols.rows.device)
        # (the table in the layout the goal has: no transposed copy per step)
        ops.goal_error_columns(cols.rows, self.rows, self.table(cols.src, by_ray=True),
                               mask=cols.mask, perm=cols.perm, by_ray=True, grad=hold.g_fin,
                               err=hold.err, **hold.buffers)

    def __call__(self, engine):
        """The same error through the generic path (arbitrary-error-function contract)."""
        self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros((0, len(self.fields)), dtype=torch.float64)
        ids = engine.last_trace["finished_id"].long()
        table = self.table(engine._trace_src)
        out = torch.stack([fin[f] for f in self.fields], dim=1).double()
        return (out - table[:, ids].t()) ** 2


class RowwiseError:
    """An error function of the FINISHED rays that works row by row:
    ``error = fn(rays)`` with ``rays[field]`` the fields of the finished rays (geometry and every
    inherited source field, tfrt/engine.py:2242-2281) and the result one row of error terms per
    ray, shape (n,) or (n, k) -- row i a function of row i of the fields alone.  That is what the
    reference's optimisation scripts compute under their tape (dev/hexalens.py:144-168 is one
    instance; any element-wise torch code qualifies, a mean over the rays does not).

    It is an ordinary ``error_function(engine)``; stating the row-wise contract lets the optimiser
    evaluate ``fn`` on fixed-shape tensors -- every source ray's column, a mask for the rays that
    finished (tfrt_scene3d.in_place == 2) -- so that the step reads no ray count back and its
    launches, ``fn``'s own torch kernels and their autograd included, are captured in one HIP graph
    like a ``GoalError``'s (fused_step.FusedStep).  Columns of rays that did not finish hold finite
    stand-in values (the source ray); their error terms are masked out of the sum and their
    gradients are never read.  On 2-D engines the same holds with one process and no ray shards
    (tfrt_trace2d_rows / tfrt_trace2d_backward_rows; 2-D traces keep the source's order)."""

    on_columns = True

    def __init__(self, fn):
        if not callable(fn):
            raise ValueError("RowwiseError: fn must be callable")
        self.fn = fn
        self.rows = []          # (no built-in goal kernel)

    def __call__(self, engine):
        return self.fn(engine.finished_rays)


def _field_codes(what, fields, dimension):
    """The field codes of ``fields`` on a ``dimension``-D engine."""
    names = _FIELDS3 if dimension == 3 else _FIELDS2
    bad = [f for f in fields if f not in names]
    if bad:
        raise ValueError(f"{what}: field(s) {bad} do not exist on a {dimension}-D engine "
                         f"(fields of its rays: {names})")
    return [names.index(f) for f in fields]


def _source_buffer(owner, name, given, convert, src, what, noun, keep=False):
    """``owner.<name>``, a buffer with one entry per SOURCE ray of the source set ``src``, on the
    source's device: the tensor given (moved once; a new buffer re-captures a graph), or the
    result of the callable ``given`` on the source's field dict, converted by ``convert(value,
    device)`` and cached in ``owner._caches[name]`` by the versions of the source's fields as
    ``GoalError.table`` is.  ``keep``: a new result of the callable is copied into the buffer
    there is (same shape), so its address -- part of a step's signature -- stays and a step that
    is being captured records the evaluation.  What ``SpotError.labels_of`` and the errors'
    ``weights_of`` share."""
    n, dev = _source_size(src)
    value = getattr(owner, name)
    if callable(given):
        key, vals = _source_key(src)
        hit = owner._caches.get(name)
        if hit is None or hit[0] != key:
            new = convert(given(src), dev)
            if keep and value is not None and value.shape == new.shape \
                    and value.device == new.device:
                value.copy_(new)
            else:
                value = new
                setattr(owner, name, value)
            owner._caches[name] = (key, vals)        # the keyed tensors stay alive with the key
    elif value.device != dev:
        value = value.to(dev)
        setattr(owner, name, value)
    if value.numel() != n:
        raise ValueError(f"{what}: {value.numel()} {noun}s for {n} source rays -- one {noun} per "
                         "source ray")
    return value


def _as_weights(what, weights, device):
    """The weights of ``DensityError`` / ``SpotError`` as they are kept: float64 on ``device``,
    divided by their maximum once (only ratios matter), values in [0, 1].  While a step is being
    captured the values cannot be read: the checks are those of the eager steps before it, and the
    kernels leave out a ray whose weight is not finite or not in [0, 1]."""
    w = weights if isinstance(weights, torch.Tensor) else torch.as_tensor(np.asarray(weights))
    if w.dim() != 1 or not w.dtype.is_floating_point:
        raise ValueError(f"{what}: weights must be floats of shape (N,), one weight per source "
                         f"ray; got shape {tuple(w.shape)}, {w.dtype}")
    w = w.detach().to(device=device, dtype=torch.float64)
    if w.numel() == 0:
        raise ValueError(f"{what}: at least one weight must be > 0")
    if not (w.is_cuda and torch.cuda.is_current_stream_capturing()):
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError(f"{what}: weights must be finite and >= 0")
        if not bool((w > 0).any()):
            raise ValueError(f"{what}: at least one weight must be > 0")
    return (w / w.max()).contiguous()


def _init_weights(erf, what, weights):
    """``erf.weights_given`` / ``erf.weights`` from the constructor's ``weights``."""
    from . import config
    erf.weights_given = weights
    erf.weights = None
    if weights is not None and not callable(weights):
        erf.weights = _as_weights(what, weights, config.get_device())


def _weights_key(erf):
    """The weights' part of a ``graph_key``: the buffer's address and shape (overwriting it in
    place is seen by replays, another buffer re-captures)."""
    w = erf.weights
    return (erf.weights_given is not None,
            None if w is None else (w.data_ptr(), tuple(w.shape)))


def _fields_and_domain(what, fields, domain):
    """(fields, domain) of a DensityError or TransportError as they are kept: one or two distinct
    field names, one finite (lo, hi) per field."""
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    if len(names) not in (1, 2) or any(f not in _FIELDS3 for f in names) \
            or len(set(names)) != len(names):
        raise ValueError(f"{what}: one or two distinct fields out of {_FIELDS3}, got {fields!r}")
    try:
        domain = tuple((float(d[0]), float(d[1])) for d in domain)
    except (IndexError, TypeError) as e:
        raise ValueError(f"{what}: domain must be ((x0, x1), (y0, y1)) or ((x0, x1),)") from e
    if len(domain) != len(names) \
            or any(not (np.isfinite(a) and np.isfinite(b) and b > a) for a, b in domain):
        raise ValueError(f"{what}: domain needs one finite (lo, hi), lo < hi, per field; got {domain!r}")
    return names, domain


def _goal_bins(what, goal, domain, bins, dev):
    """(g, ||g||) of a goal given as an array -- (ny, nx), or (nx,) for one field -- or as a
    callable evaluated at the centres of ``bins`` bins: float64 on ``dev``, finite, non-negative,
    not all zero."""
    from . import config
    k = len(domain)
    if callable(goal):
        if bins is None:
            raise ValueError(f"{what}: a callable goal needs bins=nx or bins=(nx, ny)")
        counts = (int(bins),) * k if np.ndim(bins) == 0 else tuple(int(b) for b in bins)
        if len(counts) != k or any(c < 1 for c in counts):
            raise ValueError(f"{what}: bins must give one count >= 1 per field, got {bins!r}")
        centres = []
        for (lo, hi), c in zip(domain, counts):
            edges = torch.linspace(lo, hi, c + 1, dtype=torch.float64, device=dev)
            centres.append((edges[:-1] + edges[1:]) / 2.0)
        if k == 2:
            goal = goal(*torch.meshgrid(centres[0], centres[1], indexing="xy"))
        else:
            goal = goal(centres[0])
    g = config.as_f64(goal, dev).detach()
    if g.dim() != k or g.numel() < 1 or g.numel() > ops.DENSITY_MAX_BINS:
        raise ValueError(f"{what}: goal must have {k} dimension(s) and between 1 and "
                         f"{ops.DENSITY_MAX_BINS} bins, got shape {tuple(g.shape)}")
    if not bool(torch.isfinite(g).all()) or bool((g < 0).any()):
        raise ValueError(f"{what}: goal must be finite and non-negative")
    norm = float(torch.linalg.norm(g))
    if norm == 0.0:
        raise ValueError(f"{what}: goal is zero everywhere")
    return g, norm


def _as_labels(what, groups, device):
    """The group labels of ``SpotError`` / ``FocusError`` as they are kept: int32 on ``device``,
    one per source ray."""
    g = groups if isinstance(groups, torch.Tensor) else torch.as_tensor(np.asarray(groups))
    if g.dim() != 1 or g.dtype.is_floating_point or g.dtype.is_complex or g.dtype == torch.bool:
        raise ValueError(f"{what}: groups must be integers of shape (N,), one label per "
                         f"source ray; got shape {tuple(g.shape)}, {g.dtype}")
    return g.detach().to(device=device, dtype=torch.int32).contiguous()


def _init_groups(erf, what, groups, n_groups, most):
    """``erf.groups`` / ``erf.labels`` / ``erf.n_groups`` from the constructor's ``groups`` and
    ``n_groups`` (default: ``max + 1`` of given labels, read once here; at most ``most``)."""
    from . import config
    erf.groups = groups
    erf.labels = None
    erf._caches = {}
    if callable(groups):
        if n_groups is None:
            raise ValueError(f"{what}: callable groups need n_groups")
    else:
        erf.labels = _as_labels(what, groups, config.get_device())
        if n_groups is None:
            if erf.labels.numel() == 0:
                raise ValueError(f"{what}: no labels and no n_groups")
            n_groups = int(erf.labels.max()) + 1
    try:
        erf.n_groups = int(n_groups)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: n_groups must be an integer, got {n_groups!r}") from e
    if not 1 <= erf.n_groups <= most:
        raise ValueError(f"{what}: n_groups must lie in 1 .. {most}, got {n_groups!r}")


class _CoupledError(_Term):
    """What the coupled errors share: all finished rays of a step enter one evaluation (one
    process).  The class's name stands in front of its messages."""
    on_columns = True
    weights_given = None

    def rows_for(self, dimension):
        """Field codes on a ``dimension``-D trace: the row of the ray block a geometry field is
        read from, ``2 * dimension + axis`` for a direction cosine."""
        if dimension == 3:
            return self.rows
        return _field_codes(type(self).__name__, self.fields, dimension)

    def weights_of(self, src):
        """The float64 weight buffer of the source set ``src`` on its device, one weight in [0, 1]
        per source ray (None without weights): the tensor given, or the callable's result,
        normalised and cached as ``SpotError.labels_of`` caches its labels."""
        if self.weights_given is None:
            return None
        what = type(self).__name__
        return _source_buffer(self, "weights", self.weights_given,
                              lambda v, dev: _as_weights(what, v, dev), src, what, "weight",
                              keep=True)

    def _finished_block(self, engine, fin, codes, ids=False):
        """What the generic path hands the kernels: (block, weights, ids, dimension, codes) --
        the (k, n) field columns of the finished rays ``fin`` with ``dimension = codes = None``,
        or with a direction field the (2 * dimension, n) geometry block and the field codes; the
        weight buffer (None without weights) and, with weights or ``ids``, the int32 source ray
        of every column."""
        weights = None if self.weights_given is None else self.weights_of(engine._trace_src)
        ids = engine.last_trace["finished_id"].to(torch.int32).contiguous() \
            if ids or weights is not None else None
        if self.has_direction:
            dim = engine.dimension
            block = torch.stack([fin[f] for f in (_GEO3 if dim == 3 else _GEO2)], dim=0)
            return block, weights, ids, dim, tuple(codes)
        return torch.stack([fin[f] for f in self.fields], dim=0), weights, ids, None, None

    @staticmethod
    def _held(hold, name, shape, dtype, device, workspace_bytes):
        """``hold.buffers`` with the zeroed buffer ``name`` of ``shape`` and a workspace of
        ``workspace_bytes()`` bytes, and nothing else: made on first use, and again when the
        shape changes (or the holder was another kind's)."""
        held = hold.buffers
        if name not in held or tuple(held[name].shape) != tuple(shape):
            held.clear()
            held["workspace"] = _workspace(workspace_bytes(), device)
            held[name] = torch.zeros(tuple(shape), dtype=dtype, device=device)
        return held


class DensityError(_CoupledError):
    """The finished rays, taken together, must land with the density ``goal`` on the target: a
    soft (bilinear) histogram of the rays against the goal, both L2-normalised, summed squared
    difference -- ``analyze.DistributionDifferential`` (tfrt/analyze.py:134-290) with a gradient.

    ``fields``: one or two fields of a finished ray, x and (if present) y, e.g.
    ``("y_end", "z_end")``: geometry fields, or the direction cosines ``x_dir``, ``y_dir``,
    ``z_dir`` of the ray's last link -- ``("y_dir", "z_dir")`` is a far-field intensity, a position
    with a direction a phase-space density.  For a ray, in float64 and every operation rounded on
    its own: ``e = end - start``, ``L = sqrt(e_x*e_x + e_y*e_y + e_z*e_z)`` (summed left to right),
    ``d = e / L``; a ray with a non-finite coordinate or without a length (``L`` not finite or not
    ``> 0``) counts as one with a non-finite coordinate.  The gradient of a direction field goes
    back onto the start and the end of the link:
    ``G_b = ((gv of the field of axis b, else 0) - t * d_b) / L`` with ``t = sum_k gv_k * d_(a_k)``,
    ``+G`` on the end rows and ``-G`` on the start rows.  With float32 ray state the subtraction
    cancels: a direction is good to about ``eps32 * max|coordinate| / L``, not to ``eps32``.
    ``goal``: a non-negative array, shape (ny, nx) for two fields -- the
    second field is the FIRST index, as ``analyze.histogram2D`` returns it -- or (nx,) for one; or a
    callable, evaluated once at the bin centres exactly as ``DistributionDifferential`` does (the
    bin counts then come from ``bins``: nx, or (nx, ny)).  It is kept L2-normalised in float64 on
    the device as ``goal`` (``g`` below); an all-zero goal is a ValueError.  ``domain``:
    ``((x0, x1), (y0, y1))``, or ``((x0, x1),)`` for one field.  At least one bin per axis, at most
    65,536 bins.  ``sx = nx / (x1 - x0)`` (and ``sy``) are computed once, in float64, on the host.

    For every finished ray of the trace, coordinates converted to float64, every operation
    rounded on its own:

    * a ray with a non-finite coordinate contributes nothing and gets zero gradient;
    * a ray outside the closed domain on any axis contributes nothing to the histogram and adds
      ``oob_weight * (ex**2 + ey**2)`` to the error, ``ex = max(x0 - x, 0) + max(x - x1, 0)``; its
      gradient is the derivative of that expression;
    * a ray inside is spread bilinearly over bin centres: ``u = (x - x0) * sx - 0.5``,
      ``i0 = floor(u)``, ``t = u - i0``; weight ``1 - t`` goes to column ``clamp(i0, 0, nx - 1)``
      and ``t`` to column ``clamp(i0 + 1, 0, nx - 1)`` (the outer half bin piles onto the edge bin:
      total weight 1, derivative 0 there); y alike, the four weights are the products; one field:
      two weights;
    * each weight ``w`` is added to its bin as the integer ``rint(w * 2**32)`` (half to even) in an
      int64 histogram ``Hq`` -- integer addition is associative, so ``Hq`` does not depend on the
      order of the atomics; ``H = Hq / 2**32``;
    * ``s = ||H||``; ``s == 0``: the histogram part is ``sum(g**2)`` and every pull is 0; otherwise
      ``h = H / s``, ``r = h - g``, ``E_hist = sum(r**2)`` and the pull on bin b is
      ``D_b = (2 / s) * (r_b - h_b * sum_c(h_c * r_c))``;
    * gradient of a ray inside (quantisation treated as the identity):
      ``dE/dx = sx * ((1 - ty) * (D[j0, i1] - D[j0, i0]) + ty * (D[j1, i1] - D[j1, i0]))`` with
      the clamped indices, ``dE/dy`` symmetric;
    * ``error = E_hist + sum of the penalties``: ONE error term, so the reported mean is the sum.
      Every reduction has a fixed shape and order: two runs give the same bits.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.density_error`` over the
    finished rays' columns under a ``torch.autograd.Function``), which also serves sources that
    are not traced in place, ``deterministic=True`` and 2-D engines.  On a 3-D engine that traces
    its source in place the optimiser runs it on the fused, graph-replayed step under the
    conditions of a ``RowwiseError`` (``FusedStep._rowwise3d`` with ``tfrt_density_error`` in the
    place of ``fn`` and its autograd).  The fused 2-D step does not take it
    (``FusedStep.eligible2d`` is false): 2-D engines use the generic path.  One process: the
    histogram couples the rays, ray shards would each normalise their own.

    ``weights``: None -- every finished ray is one unit of light --, or a radiant power per
    SOURCE ray: a float tensor or array of shape (N,) in the source's own order, finite and
    ``>= 0`` with at least one ``> 0`` (a ValueError otherwise), or a callable on the source's
    field dict that returns one (``lambda src: cos`` of the start direction for a Lambertian
    emitter sampled uniformly in angle; evaluated and cached as ``SpotError``'s ``groups``).  Only
    ratios matter: the weights are divided by their maximum once, in float64, and kept on the
    device as ``weights`` (values in [0, 1]); that buffer may be overwritten in place between steps
    (a replayed graph reads it), another buffer re-captures.  A finished ray finds its weight ``w``
    through the source-ray index the trace carries.  A ray without a source ray, or whose ``w`` is
    not finite or not in [0, 1], counts as one with a non-finite coordinate.  Then, each product
    rounded on its own:

    * a ray inside adds ``rint(((bx * by) * w) * 2**32)`` to each of its bins (``bx * w`` with one
      field) and its gradient is the expression above multiplied by ``w`` last;
    * a ray outside has its penalty and its gradient multiplied by ``w`` last;
    * ``s``, ``E_hist`` and the pulls come from the weighted histogram exactly as above; with a
      direction field the gradient carries ``w`` when it enters the chain rule.

    Weighted and unweighted run on the same paths (fused, generic, 2-D, ``deterministic=True``),
    the weighted one with kernels of its own (tfrt_density_error_weighted).

    ``goal`` may be overwritten in place between steps (a replayed graph reads the buffer);
    ``last_hq`` is the int64 histogram of the last evaluation (the weighted one with weights).  ``splat_variant`` (0: by the number
    of bins; 1: histogram in LDS; 2: global atomics) is tfrt_density_error's, for measuring."""

    splat_variant = 0

    def __init__(self, fields, goal, domain, oob_weight=0.0, bins=None, weights=None):
        from . import config
        self.fields, self.domain = _fields_and_domain("DensityError", fields, domain)
        self.rows = [_FIELDS3.index(f) for f in self.fields]
        self.has_direction = any(f.endswith("_dir") for f in self.fields)
        k = len(self.fields)
        self.oob_weight = float(oob_weight)
        if not (self.oob_weight >= 0.0 and np.isfinite(self.oob_weight)):
            raise ValueError("DensityError: oob_weight must be finite and >= 0")
        dev = config.get_device()
        g, norm = _goal_bins("DensityError", goal, self.domain, bins, dev)
        self.goal = (g / norm).contiguous()
        nx = self.goal.shape[-1]
        self.grid = ops.density_grid(domain, nx, self.goal.shape[0] if k == 2 else None)
        self.last_hq = None
        self._caches = {}
        _init_weights(self, "DensityError", weights)

    @property
    def g(self):
        return self.goal

    def goal_on(self, device):
        """The goal buffer on ``device`` (moved once; a new buffer re-captures a graph)."""
        if self.goal.device != device:
            self.goal = self.goal.to(device)
        return self.goal

    def graph_key(self):
        """What a captured step has baked in: the goal buffer's address, the weight buffer's and
        the constants."""
        return (self.goal.data_ptr(), tuple(self.goal.shape), self.grid, self.oob_weight,
                self.splat_variant) + _weights_key(self)

    def evaluate(self, rows, row_x, row_y, mask=None, dimension=None, weights=None, perm=None,
                 **buffers):
        """``ops.density_error`` of the columns of ``rows`` with this goal, domain and weight
        (``dimension`` given: ``rows`` is the geometry block, ``row_x`` / ``row_y`` field codes;
        ``weights``: the buffer of ``weights_of``, ``perm``: the source ray of every column)."""
        out = ops.density_error(rows, row_x, row_y, self.goal_on(rows.device), self.grid,
                                self.oob_weight, mask=mask, variant=self.splat_variant,
                                dimension=dimension, weights=weights,
                                perm=perm if weights is not None else None, **buffers)
        self.last_hq = out[2]
        return out

    def seed_columns(self, cols, hold):
        """tfrt_density_error on the step's columns -- with weights it reads the source's weight
        buffer through the trace's order ``cols.perm``, inside the kernel, as a SpotError its
        labels --: the histogram goes into ``hold.buffers["hq"]``, made anew when the goal's
        shape changes."""
        goal = self.goal_on(cols.rows.device)
        nx, ny = goal.shape[-1], (goal.shape[0] if goal.dim() == 2 else 1)
        held = self._held(hold, "hq", goal.shape, torch.int64, cols.rows.device,
                          lambda: _lib.lib().tfrt_density_error_workspace_bytes(cols.n, nx, ny))
        self.evaluate(cols.rows, *_xy(self.rows), mask=cols.mask, dimension=3,
                      weights=self.weights_of(cols.src), perm=cols.perm, grad=hold.g_fin,
                      err=hold.err, **held)

    def __call__(self, engine):
        """The error as a (1,) tensor through the generic path; the gradient rows come back in
        ``backward``."""
        codes = self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return (self.goal * self.goal).sum().reshape(1)
        block, weights, ids, dim, codes = self._finished_block(engine, fin, codes)
        return _DensityTerms.apply(block, self, weights, ids, dim, codes)


class _DensityTerms(torch.autograd.Function):
    """DensityError over the finished rays, no mask.  ``dimension=None, codes=None``: ``block`` is
    the (k, n) field columns; else it is the (2 * dimension, n) geometry block and ``codes`` the
    field codes (a direction field).  ``weights`` (or None) with ``ids``, the source ray of every
    column."""

    @staticmethod
    def forward(ctx, block, erf, weights=None, ids=None, dimension=None, codes=None):
        rows = block.detach().contiguous()
        if codes is None:
            codes = (0, 1)[:rows.shape[0]]
        err, grad, _ = erf.evaluate(rows, *_xy(codes), dimension=dimension, weights=weights,
                                    perm=ids)
        ctx.save_for_backward(grad)
        ctx.dtype = block.dtype
        return err[:1].clone()

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        return (upstream * grad).to(ctx.dtype), None, None, None, None, None


class TransportError(_CoupledError):
    """The finished rays, taken together, must land with the density ``goal`` on the target --
    measured by sliced optimal transport (sliced Wasserstein-2) from the rays that actually arrive:
    along each of K directions the landing points are sorted, the ray of rank r belongs at the
    goal's quantile (r + 1/2) / n, and the error is the squared distance to that target.  In one
    dimension this IS the optimal transport, and its gradient is exact almost everywhere because
    the assignment is locally constant; in two it is averaged over the directions.  Unlike
    ``DensityError``, whose gradient comes from a ray's four neighbouring bins, the pull is global:
    a beam that starts beside the target, a lens that over-focuses into one spot, a goal with
    empty stretches all have a signal.  It needs no transport map (``GoalError`` with ranks does);
    lost rays simply take no part.

    ``fields``, ``goal``, ``domain``, ``bins``: as for ``DensityError`` -- one or two geometry
    fields of a finished ray, e.g. ``("y_end", "z_end")``; ``goal`` a non-negative array of shape
    (ny, nx), the second field the FIRST index, or (nx,) for one field, or a callable evaluated at
    the centres of ``bins`` bins; ``domain`` one finite ``(lo, hi)`` per field; the same
    ValueErrors.  Direction fields (``x_dir`` ...) and ``weights=`` are refused with a ValueError:
    weighted quantiles and the chain rule of a direction are not built yet.
    ``directions``: with two fields K angles -- an int K means ``theta_k = pi * k / K``,
    k = 0 .. K-1 (default 8), an array gives them --, 1 <= K <= 64; one field: K = 1, the axis
    itself.  ``c_k = cos(theta_k)``, ``s_k = sin(theta_k)`` are computed once on the host in
    float64.  ``knots``: Q, the intervals of a quantile table, 2 <= Q <= 65,536.

    The quantile tables ``tables``, (K, Q + 1) float64 on the device, are built on the host
    (``ops.transport_tables``): every goal bin is split into 4 x 4 sub-points at the sub-cells'
    centres, in normalised coordinates xi, eta in [0, 1], each with the bin's mass; empty ones are
    dropped; per direction ``p = c * xi + s * eta`` (one field: ``p = xi``) is sorted stably,
    ``cm = (cumsum(w) - w / 2) / sum(w)`` and ``T_k = np.interp(arange(Q + 1) / Q, cm, p_sorted)``:
    non-decreasing by construction.

    For every finished ray and direction, coordinates converted to float64, every operation
    rounded on its own:

    * a ray counts if both coordinates are finite (and, on the fused step, it has finished);
    * ``xi = (x - x0) * ix`` with ``ix = 1 / (x1 - x0)`` computed once on the host, ``eta`` alike;
      ``p = c * xi + s * eta`` (two products, one sum);
    * its sort key: ``a = min(0, c) + min(0, s)``, ``b = max(0, c) + max(0, s)``,
      ``lo = a - (b - a)``, ``scale = 2**26 / (3 * (b - a))``,
      ``q = clamp(floor((p - lo) * scale), 0, 2**26 - 2)``; a ray that does not count has
      ``q = 2**26 - 1`` (the width 26 is ``ops.TRANSPORT_KEY_BITS``: two 13-bit digits of the
      radix sort) -- a ray up to one domain width outside still has a key of its own, farther out
      the keys clamp and the rays tie;
    * its rank among the n_valid rays that count: ``first`` keys are smaller than q, ``count`` are
      equal to q, ``rank2 = 2 * first + count`` (int32; -1 for a ray that does not count) and
      ``u = (first + count * 0.5) / n_valid``.  Ties share the mid-rank on purpose: the result
      does not depend on the order of the rays, so the fused step (coherent order) and the generic
      path (finished order) give every ray the same bits;
    * target and residual: ``z = u * Q``, ``m = min(floor(z), Q - 1)``, ``f = z - m``,
      ``t = T[m] + f * (T[m + 1] - T[m])``, ``d = p - t``; the term is ``d * d``;
    * gradient, accumulated from zero in the order k = 0 .. K-1:
      ``gx += ((2 * d) * c) * ix``, ``gy += ((2 * d) * s) * iy``; zeros for a ray that does not
      count.  The targets are constants, as ``SpotError``'s centroids are;
    * ``error = {sum of all terms, K * n_valid, sum / terms}`` -- the sum convention of
      ``GoalError`` and ``SpotError``; the mean of no terms is NaN.  The sum has a fixed shape and
      order: two runs give the same bits in the error, the gradient and ``rank2``.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.transport_error`` over
    the finished rays' columns under a ``torch.autograd.Function``, which returns the
    (n_finished, K) terms), which also serves 2-D engines, ``deterministic=True``, fewer than 4,096
    rays and sources that are not traced in place.  On a 3-D engine that traces its source in
    place the optimiser runs it on the fused, graph-replayed step under the conditions of a
    ``DensityError`` (``FusedStep._rowwise3d`` with ``tfrt_transport_error``: 11 K + 2 launches,
    n_valid stays on the device).  One process: the ranks couple all rays.

    ``set_goal(goal)`` rebuilds the tables into the same device buffer, so a replayed graph sees
    the new goal; another shape is a ValueError.  ``last_rank2`` is the (K, n) int32 ``rank2`` of
    the last evaluation, ``last_count`` its n_valid (read from the device when asked for)."""

    def __init__(self, fields, goal, domain, directions=None, knots=1024, bins=None,
                 weights=None):
        from . import config
        self.fields, self.domain = _fields_and_domain("TransportError", fields, domain)
        if any(f.endswith("_dir") for f in self.fields):
            raise ValueError("TransportError: direction fields (x_dir, y_dir, z_dir) are not "
                             f"supported, only geometry fields; got {fields!r}")
        if weights is not None:
            raise ValueError("TransportError: weights= is not supported (weighted quantiles are "
                             "not built yet)")
        self.rows = [_FIELDS3.index(f) for f in self.fields]
        k = len(self.fields)
        try:
            self.knots = int(knots)
        except (TypeError, ValueError) as e:
            raise ValueError(f"TransportError: knots must be an integer, got {knots!r}") from e
        if self.knots != knots or not 2 <= self.knots <= ops.TRANSPORT_MAX_KNOTS:
            raise ValueError(f"TransportError: knots must lie in 2 .. {ops.TRANSPORT_MAX_KNOTS}, "
                             f"got {knots!r}")
        try:
            cs = ops.transport_directions(8 if directions is None else directions, k)
        except (TypeError, ValueError) as e:
            raise ValueError(f"TransportError: directions must be a count in 1 .. "
                             f"{ops.TRANSPORT_MAX_DIRECTIONS} or as many finite angles, got "
                             f"{directions!r}") from e
        self.directions = cs                       # (K, 2) numpy: cos, sin
        self.bins = bins
        dev = config.get_device()
        g, _ = _goal_bins("TransportError", goal, self.domain, bins, dev)
        self.goal_shape = tuple(g.shape)
        self.angles = torch.as_tensor(cs, dtype=torch.float64).contiguous().to(dev)
        self.tables = torch.as_tensor(
            ops.transport_tables(g.cpu().numpy(), self.domain, cs, self.knots)).contiguous().to(dev)
        self.grid = ops.transport_grid(self.domain)
        self.last_rank2 = None

    @property
    def n_directions(self):
        return self.tables.shape[0]

    @property
    def last_count(self):
        """n_valid of the last evaluation (a device read)."""
        if self.last_rank2 is None:
            raise RuntimeError("TransportError: no evaluation yet")
        return int((self.last_rank2[0] >= 0).sum()) if self.last_rank2.shape[1] else 0

    def set_goal(self, goal):
        """Another goal of the same shape: the tables are rebuilt on the host and copied into the
        device buffer there is."""
        g, _ = _goal_bins("TransportError", goal, self.domain, self.bins, torch.device("cpu"))
        if tuple(g.shape) != self.goal_shape:
            raise ValueError(f"TransportError: set_goal needs a goal of shape {self.goal_shape}, "
                             f"got {tuple(g.shape)}")
        new = ops.transport_tables(g.numpy(), self.domain, self.directions, self.knots)
        self.tables.copy_(torch.as_tensor(new))

    def tables_on(self, device):
        """(tables, angles) on ``device`` (moved once; new buffers re-capture a graph)."""
        if self.tables.device != device:
            self.tables, self.angles = self.tables.to(device), self.angles.to(device)
        return self.tables, self.angles

    def graph_key(self):
        """What a captured step has baked in: the table buffer's address, K, Q, the directions'
        buffer and the domain."""
        return (self.tables.data_ptr(), self.n_directions, self.knots, self.angles.data_ptr(),
                self.domain)

    def evaluate(self, rows, row_x, row_y, mask=None, dimension=None, **buffers):
        """``ops.transport_error`` of the columns of ``rows`` with these tables and this domain
        (``dimension`` given: ``rows`` is the geometry block)."""
        tables, angles = self.tables_on(rows.device)
        out = ops.transport_error(rows, row_x, row_y, tables, self.grid, angles, mask=mask,
                                  dimension=dimension, **buffers)
        self.last_rank2 = out[2]
        return out

    def seed_columns(self, cols, hold):
        """tfrt_transport_error on the step's columns: the ranks go into the (K, N) int32
        ``hold.buffers["rank2"]``; n_valid never leaves the device."""
        K = self.n_directions
        held = self._held(hold, "rank2", (K, cols.n), torch.int32, cols.rows.device,
                          lambda: _lib.lib().tfrt_transport_error_workspace_bytes(cols.n, K))
        self.evaluate(cols.rows, *_xy(self.rows), mask=cols.mask, dimension=3, grad=hold.g_fin,
                      err=hold.err, **held)

    def __call__(self, engine):
        """The (n_finished, K) error terms through the generic path; the gradient rows come back
        in ``backward``."""
        self.rows_for(engine.dimension)           # (a field the engine's rays do not have)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros((0, self.n_directions), dtype=torch.float64)
        return _TransportTerms.apply(torch.stack([fin[f] for f in self.fields], dim=0), self)


def _transport_terms(erf, v, rank2):
    """The (n, K) terms of a TransportError evaluation from its ranks, the definition's operations
    as torch ops; ``v``: the (k, n) float64 fields.  Zeros for a ray that does not count."""
    tables, angles = erf.tables_on(v.device)
    x0, ix, y0, iy = erf.grid
    two = v.shape[0] == 2
    Q = erf.knots
    xi = (v[0] - x0) * ix
    eta = (v[1] - y0) * iy if two else None
    counts = rank2[0] >= 0
    nv = counts.sum().double()
    terms = []
    for k in range(tables.shape[0]):
        p = erf.directions[k, 0] * xi + erf.directions[k, 1] * eta if two else xi
        z = ((rank2[k].double() * 0.5) / nv) * float(Q)
        fm = torch.clamp(torch.floor(torch.where(counts, z, torch.zeros_like(z))),
                         min=0.0, max=float(Q - 1))
        m = fm.long()
        t0 = tables[k][m]
        d = p - (t0 + (z - fm) * (tables[k][m + 1] - t0))
        terms.append(torch.where(counts, d * d, torch.zeros_like(d)))
    return torch.stack(terms, dim=1).contiguous()


class _TransportTerms(torch.autograd.Function):
    """TransportError over the (k, n) field columns of the finished rays, no mask.  Returns the
    (n, K) terms; the gradient has summed the K directions into a ray's rows, so one weight per
    ray is all that can be applied afterwards (the optimiser passes ones)."""

    @staticmethod
    def forward(ctx, columns, erf):
        rows = columns.detach().contiguous()
        _, grad, rank2 = erf.evaluate(rows, 0, 1 if rows.shape[0] == 2 else -1)
        ctx.save_for_backward(grad)
        ctx.dtype = columns.dtype
        return _transport_terms(erf, rows.double(), rank2)

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        if upstream.shape[1] > 1 and not torch.equal(upstream,
                                                     upstream[:, :1].expand_as(upstream)):
            raise ValueError("TransportError: the upstream gradient must weigh the K terms of a "
                             "ray alike")
        return (upstream[:, 0] * grad).to(ctx.dtype), None


class SpotError(_CoupledError):
    """Rays that left the same object point must meet in one point -- wherever that is: the sum
    over the finished rays of the squared distance to the CENTROID of their own group, the squared
    RMS spot size times the ray count.  Where the spots lie (magnification, distortion, field
    curvature) is left to the lens; no target is needed in advance.

    ``fields``: one or two fields of a finished ray, e.g. ``("y_end", "z_end")``: geometry
    fields, or the direction cosines ``x_dir``, ``y_dir``, ``z_dir`` of the ray's last link --
    ``("y_dir", "z_dir")`` asks the rays of one object point to leave PARALLEL (collimation, afocal
    systems: a spot in direction space; ``centroids()`` are then mean direction cosines).  The
    direction, its non-finite case, the chain rule back onto the start and end rows and the
    float32 caveat (a direction is good to about ``eps32 * max|coordinate| / L``) are
    ``DensityError``'s.
    ``groups``: an integer tensor or array of shape (N,), one label per SOURCE ray in the source's
    own order -- finished rays look theirs up through the source-ray index the trace carries --, or
    a callable on the source's field dict that returns such labels (evaluated and cached as
    ``GoalError.table`` is; it then needs ``n_groups``).  The labels are kept as int32 on the
    device (``labels``) and may be overwritten in place between steps (a replayed graph reads the
    buffer).  Labels outside ``[0, n_groups)`` -- ``-1`` -- exclude a ray.  ``n_groups``: G, by
    default ``max + 1`` of a tensor, read once here; at most 2**20.  ``domain``:
    ``((x0, x1), (y0, y1))``, or ``((x0, x1),)`` for one field: rays outside it take a penalty
    instead of pulling their spot.

    For every finished ray of the trace, coordinates converted to float64, every operation rounded
    on its own, the first case that applies:

    * a non-finite coordinate: no error, zero gradient;
    * a label outside ``[0, n_groups)``: no error, zero gradient;
    * outside the closed domain on any axis: the ray is in no spot and adds
      ``oob_weight * (ex**2 + ey**2)``, ``ex = max(x0 - x, 0) + max(x - x1, 0)``; its gradient is
      the derivative of that expression;
    * inside: ``qx = min(max(rint((x - x0) * qsx), 0), 2**qbits)`` (half to even),
      ``qsx = 2**qbits / (x1 - x0)``, ``qbits = min(52, 62 - bit_length(N))``; ``{1, qx, qy}`` is
      added to the ray's group in an int64 table -- integer addition is associative, so the table
      does not depend on the order of the atomics.

    A group with rays has the centroid ``cx = x0 + (Sx / count) / qsx``; a ray inside has
    ``dx = x - cx``, the error terms ``dx**2`` and ``dy**2`` and the gradient ``2 * dx``, ``2 * dy``.
    That gradient is exact without differentiating through the centroid, because the residuals of
    a group sum to zero (up to the quantisation: at most half a step ``1 / qsx`` per centroid).
    ``error = sum of the terms + sum of the penalties`` over ``len(fields) * n_finished`` terms;
    every sum has a fixed shape and order: two runs give the same bits.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.spot_error`` over the
    finished rays' columns under a ``torch.autograd.Function``), which also serves sources that are
    not traced in place, ``deterministic=True``, fewer than 4,096 rays and 2-D engines
    (``FusedStep.eligible2d`` is false).  Its ``backward`` returns ``upstream * gradient``: exact
    when ``upstream`` is constant within a group (the optimiser passes ones) -- a radiant power
    per ray belongs in ``weights`` (below), which moves the centroid with it, not in ``upstream``;
    with a direction field the two fields of a ray must also carry the same upstream factor (a
    ``ValueError`` otherwise), because the kernel's chain rule sums both into the geometry rows.  On a 3-D engine that traces
    its source in place the optimiser runs it on the fused, graph-replayed step under the
    conditions of a ``RowwiseError`` (``FusedStep._rowwise3d`` with ``tfrt_spot_error`` in the
    place of ``fn`` and its autograd), with the same kernels and the same ``qbits``.  One process:
    with ray shards over several ranks the generic path runs and each shard forms the centroids of
    its own rays.

    ``weights``: None -- every ray of a spot counts alike --, or a radiant power per SOURCE ray,
    given, normalised (divided by the maximum, float64, values in [0, 1]), kept as ``weights`` and
    looked up exactly as ``DensityError``'s: a tensor or array of shape (N,), or a callable on the
    source's field dict (an apodised pupil, a spectrum).  The spot is then the WEIGHTED one.  With
    ``wbits = min(20, 62 - bit_length(N) - ceil(qbits / 2))`` (``ops.spot_wbits(N)``) a ray's
    weight ``w`` enters as the integer ``wq = rint(w * 2**wbits)`` (half to even), and
    ``wr = wq * 2**-wbits`` -- exact -- is the weight used everywhere, so the weighted residuals of
    a group sum to zero in the quantised quantities.  After the label's case above:

    * no source ray, ``w`` not finite or not in [0, 1], or ``wq == 0``: the ray is in no spot, no
      error, zero gradient;
    * outside the domain: the penalty and its gradient are multiplied by ``wr`` last;
    * inside: with ``h = qbits // 2`` the product ``wq * qx`` is added in two limbs, so that the
      position keeps its full ``qbits``: ``Xhi += wq * (qx >> h)``, ``Xlo += wq * (qx & (2**h - 1))``
      (y alike), ``W += wq``, ``count += 1`` -- a record is eight int64
      ``{W, Xhi, Xlo, Yhi, Ylo, count, 0, 0}``, every sum below ``N * 2**wbits * 2**ceil(qbits / 2)
      < 2**62``.

    A group with ``W > 0`` has ``X = ldexp(Xhi, h) + Xlo`` and the centroid
    ``cx = x0 + (X / W) / qsx``; a ray inside has ``dx = x - cx``, the terms ``wr * (dx * dx)`` and
    ``wr * (dy * dy)`` and the gradient ``(2 * dx) * wr``, ``(2 * dy) * wr`` -- again exact without
    a derivative of the centroid, because the WEIGHTED residuals of a group sum to zero.  The
    number of terms stays ``len(fields) * n_finished``.  Weighted and unweighted run on the same
    paths; the weighted one has kernels of its own (tfrt_spot_error_weighted: a table of six planes
    in LDS up to ``ops.SPOT_WEIGHTED_LDS_GROUPS`` groups, global atomics above).

    ``last_acc`` is the (G, 4) int64 table ``{count, Sx, Sy, 0}`` of the last evaluation -- with
    weights the (G, 8) table above --, ``centroids()`` the (G, k) float64 centroids made from it,
    weighted with weights (NaN for a group without rays).
    ``splat_variant`` (0: by G; 1: table in LDS; 2: global atomics) is tfrt_spot_error's, for
    measuring."""

    splat_variant = 0

    def __init__(self, fields, groups, domain, oob_weight=0.0, n_groups=None, weights=None):
        self.fields, self.domain = _fields_and_domain("SpotError", fields, domain)
        self.rows = [_FIELDS3.index(f) for f in self.fields]
        self.has_direction = any(f.endswith("_dir") for f in self.fields)
        self.oob_weight = float(oob_weight)
        if not (self.oob_weight >= 0.0 and np.isfinite(self.oob_weight)):
            raise ValueError("SpotError: oob_weight must be finite and >= 0")
        _init_groups(self, "SpotError", groups, n_groups, ops.SPOT_MAX_GROUPS)
        self._grids = {}
        self.last_acc = None
        self.last_grid = None
        self.last_qbits = None
        _init_weights(self, "SpotError", weights)
        if self.weights is not None and self.labels is not None \
                and self.weights.numel() != self.labels.numel():
            raise ValueError(f"SpotError: {self.weights.numel()} weights for "
                             f"{self.labels.numel()} labels -- one of each per source ray")

    def labels_of(self, src):
        """The int32 label buffer of the source set ``src`` on its device, one label per source
        ray: the tensor given (moved once; a new buffer re-captures a graph), or the callable's
        result, cached by the versions of the source's fields as ``GoalError.table`` is."""
        return _source_buffer(self, "labels", self.groups,
                              lambda v, dev: _as_labels("SpotError", v, dev), src, "SpotError",
                              "label")

    def grid_for(self, n_source):
        """(qbits, grid constants) for a source of ``n_source`` rays: both paths of a step use the
        source's ray count, so the fused and the generic step quantise alike."""
        hit = self._grids.get(n_source)
        if hit is None:
            qbits = ops.spot_qbits(n_source)
            hit = self._grids[n_source] = (qbits, ops.spot_grid(self.domain, qbits))
        return hit

    def graph_key(self):
        """What a captured step has baked in: the label buffer's address, the weight buffer's
        with ``wbits``, and the constants."""
        lab, w = self.labels, self.weights
        return (None if lab is None else (lab.data_ptr(), tuple(lab.shape)), self.n_groups,
                self.domain, self.oob_weight, self.splat_variant) + _weights_key(self) \
            + (None if w is None else ops.spot_wbits(w.numel()),)

    def evaluate(self, rows, row_x, row_y, labels, mask=None, perm=None, dimension=None,
                 weights=None, **buffers):
        """``ops.spot_error`` of the columns of ``rows`` with these labels, domain and weight
        (``dimension`` given: ``rows`` is the geometry block, ``row_x`` / ``row_y`` field codes;
        ``weights``: the buffer of ``weights_of``)."""
        qbits, grid = self.grid_for(labels.numel())
        out = ops.spot_error(rows, row_x, row_y, labels, self.n_groups, grid, self.oob_weight,
                             mask=mask, perm=perm, variant=self.splat_variant, qbits=qbits,
                             dimension=dimension, weights=weights,
                             wbits=None if weights is None else ops.spot_wbits(labels.numel()),
                             **buffers)
        self.last_acc, self.last_grid, self.last_qbits = out[2], grid, qbits
        return out

    def seed_columns(self, cols, hold):
        """tfrt_spot_error on the step's columns: it reads the source's label buffer and the
        trace's order ``cols.perm`` -- the kernel looks a column's label up itself, so no permuted
        copy can go stale when a source is re-drawn and re-ordered inside the graph -- and, looked
        up like the labels, the weights; the group records go into ``hold.buffers["acc"]``,
        (G, 4), with weights (G, 8)."""
        labels, weights = self.labels_of(cols.src), self.weights_of(cols.src)
        G = self.n_groups
        held = self._held(hold, "acc", (G, 4 if weights is None else 8), torch.int64,
                          cols.rows.device,
                          lambda: _lib.lib().tfrt_spot_error_workspace_bytes(cols.n, G))
        self.evaluate(cols.rows, *_xy(self.rows), labels, mask=cols.mask, perm=cols.perm,
                      dimension=3, weights=weights, grad=hold.g_fin, err=hold.err, **held)

    def centroids(self):
        """(G, k) float64 centroids of the last evaluation, NaN for a group without rays."""
        if self.last_acc is None:
            raise RuntimeError("SpotError: no evaluation yet")
        return ops.spot_centroids(self.last_acc, self.last_grid, len(self.fields), self.last_qbits)

    def __call__(self, engine):
        """The (n_finished, k) error terms through the generic path; the gradient rows come back
        in ``backward``."""
        codes = self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros((0, len(self.fields)), dtype=torch.float64)
        labels = self.labels_of(engine._trace_src)
        block, weights, ids, dim, codes = self._finished_block(engine, fin, codes, ids=True)
        return _SpotTerms.apply(block, self, labels, ids, weights, dim, codes)


def _spot_terms(erf, v, labels, ids, acc, weights, inside=None):
    """The (n, k) terms of a SpotError evaluation from its records: an inside ray's squared
    distances to its group's centroid (``inside``, (k, n), where the caller has them already), a
    penalised ray's ``oob_weight * ex**2`` per field, both times ``wr`` with ``weights``; zeros for
    a ray in no spot.  ``v``: the (k, n) float64 fields."""
    k = v.shape[0]
    lo = torch.tensor([d[0] for d in erf.domain], dtype=torch.float64, device=v.device)[:, None]
    hi = torch.tensor([d[1] for d in erf.domain], dtype=torch.float64, device=v.device)[:, None]
    zero = torch.zeros((), dtype=torch.float64, device=v.device)
    ex = torch.maximum(lo - v, zero) + torch.maximum(v - hi, zero)
    out = ((v < lo) | (v > hi)).any(dim=0, keepdim=True)
    # (a ray that does not count has a zero gradient and, outside, no penalty either: its label
    # and its weight decide, which the kernel has looked up)
    s = ids.long()
    s_ok = (s >= 0) & (s < labels.numel())
    s = s.clamp(0, labels.numel() - 1)
    lab = labels[s]
    spot = s_ok & (lab >= 0) & (lab < erf.n_groups) & torch.isfinite(v).all(dim=0)
    if inside is None:
        centre = ops.spot_centroids(acc, erf.last_grid, k, erf.last_qbits).t()[
            :, lab.long().clamp(0, erf.n_groups - 1)]
        dv = v - centre
        inside = dv * dv
    penalty = erf.oob_weight * (ex * ex)
    if weights is not None:
        wbits = ops.spot_wbits(labels.numel())
        w = weights[s]
        wq = torch.where((w >= 0.0) & (w <= 1.0), torch.round(w * float(np.ldexp(1.0, wbits))),
                         torch.zeros_like(w))
        wr = wq * float(np.ldexp(1.0, -wbits))
        spot = spot & (wq > 0)
        penalty, inside = penalty * wr, wr * inside
    return torch.where(spot[None, :], torch.where(out, penalty, inside), zero).t().contiguous()


class _SpotTerms(torch.autograd.Function):
    """SpotError over the finished rays, no mask; ``ids``: the source ray of every column.
    ``dimension=None, codes=None``: ``block`` is the (k, n) field columns; else it is the
    (2 * dimension, n) geometry block and ``codes`` the field codes (a direction field).  Returns
    the (n, k) terms (``_spot_terms``): a penalised ray's ``oob_weight * ex**2`` per field, an
    inside ray's squared distances to its group's centroid.  Over plain columns without
    ``weights`` the latter are (gradient / 2)**2 -- the kernel's own dx * dx, the halving is
    exact --; with ``weights`` or a direction field that is no longer the term, and they come from
    the records' centroids."""

    @staticmethod
    def forward(ctx, block, erf, labels, ids, weights=None, dimension=None, codes=None):
        rows = block.detach().contiguous()
        ctx.chained = codes is not None
        if codes is None:
            codes = (0, 1)[:rows.shape[0]]
        err, grad, acc = erf.evaluate(rows, *_xy(codes), labels, perm=ids, dimension=dimension,
                                      weights=weights)
        ctx.save_for_backward(grad)
        ctx.dtype = block.dtype
        if ctx.chained:
            link = ops._link_torch(rows, dimension)
            v = torch.stack([ops._link_field_torch(link, c, dimension) for c in codes], dim=0)
            return _spot_terms(erf, v, labels, ids, acc, weights)
        half = 0.5 * grad
        return _spot_terms(erf, rows.double(), labels, ids, acc, weights,
                           inside=half * half if weights is None else None)

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        if not ctx.chained:
            return (upstream.t() * grad).to(ctx.dtype), None, None, None, None, None, None
        # the kernel's chain rule has summed both fields' gradients into the rows: one weight per
        # ray is all that can be applied afterwards (the optimiser passes ones)
        if upstream.shape[1] == 2 and not torch.equal(upstream[:, 0], upstream[:, 1]):
            raise ValueError("SpotError with a direction field: the upstream gradient must weigh "
                             "both fields of a ray alike")
        return (upstream[:, 0] * grad).to(ctx.dtype), None, None, None, None, None, None


class FocusError(_CoupledError):
    """Rays that left the same object point, taken as LINES, must pass through one common point
    of space -- wherever along the beam that is: the sum over the finished rays of the squared
    distance of their group's FOCUS from the ray's own line, in the scene's units.  A
    ``SpotError`` asks the rays to meet in one point of the target surface and charges defocus
    and field curvature to the lens as spot size; here the axial position is free too, and the
    solved points (``foci()``) are a direct read-out of the focal surface.  It is also the
    objective of concentrators and fibre coupling: everything through one small region, wherever
    it is.

    ``groups``, ``n_groups``: as for ``SpotError`` -- one integer label per SOURCE ray (a tensor
    or array of shape (N,), kept as int32 on the device as ``labels`` and overwritable in place,
    or a callable on the source's field dict, which needs ``n_groups``); labels outside
    ``[0, n_groups)`` exclude a ray.  ``domain``: the closed box ``((x0, x1), (y0, y1), (z0, z1))``
    -- ``((x0, x1), (y0, y1))`` on a 2-D engine -- that the END of a finished ray's last link must
    lie in to count; it should contain the target.  ``min_det``: finite and > 0; a group has a
    focus if it has at least two rays and ``det(A / count) >= min_det`` (below) -- a definition:
    a collimated group has no focus.  Choose it well above ``2**-pbits``, the size of the
    quantisation.  There are no ``fields`` (all ``2 * dimension`` geometry rows are read and
    seeded) and no ``weights``.

    For every finished ray of the trace, coordinates converted to float64, every operation
    rounded on its own, sums of products left to right:

    * the line: ``v = end - start``, ``L = sqrt(v . v)``, ``u = v / L`` (``DensityError``'s
      direction); a ray counts if its link has a direction, its label lies in ``[0, n_groups)``
      and its end lies in the box; everything else has no term and zero gradient;
    * with ``c`` the box centre, ``R`` its largest half-width and ``iR = 1 / R`` computed once:
      ``m = (end - c) * iR``; ``P = I - u u^T`` (``P_aa = 1 - u_a * u_a``,
      ``P_ab = -(u_a * u_b)``), ``w = u . m``, ``t = m - w * u``;
    * ``{1, rint(P_ab * 2**pbits) (a <= b), rint(t_a * 2**pbits)}`` (half to even) is added to the
      ray's group in an int64 table of ten slots ``{count, Pxx, Pxy, Pxz, Pyy, Pyz, Pzz, tx, ty,
      tz}`` (2-D: the z slots stay 0), ``pbits = min(40, 60 - bit_length(N))``
      (``ops.focus_pbits(N)``) -- integer addition is associative, so the table does not depend on
      the order of the atomics;
    * a group's ``A = Aq * 2**-pbits / count``, ``b = bq * 2**-pbits / count``, the determinant
      and ``x = A^-1 b`` by the cofactor expressions of include/tfrt_hip.h (tfrt_focus_error); its
      focus is ``c + R * x``;
    * a counting ray of a group with a focus: ``q = m - x``, ``a = u . q``,
      ``rho = R * (q - a * u)``, the term ``rho . rho``; with ``lever = (R * a) / L`` the gradient
      is ``(2 * rho) * (1 - lever)`` on the end rows and ``(2 * rho) * lever`` on the start rows:
      the lever rule of the foot point along the link.  It is exact without a derivative of the
      focus, because the focus minimises the group's sum (up to the quantisation, relative
      ``2**-pbits``).  With float32 ray state the lever inherits the direction's
      ``eps32 * max|coordinate| / L``;
    * ``error = {sum of the terms, number of terms, sum / number}``, NaN without terms; every sum
      has a fixed shape and order: two runs give the same bits.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.focus_error`` over the
    finished rays' geometry block under a ``torch.autograd.Function`` that returns the
    (n_finished, 1) terms), which also serves sources that are not traced in place,
    ``deterministic=True``, fewer than 4,096 rays, several ranks (each shard then solves the foci
    of its own rays) and 2-D engines.  Its ``backward`` returns ``upstream * gradient``: exact when
    ``upstream`` is constant within a group (the optimiser passes ones).  On a 3-D engine that
    traces its source in place the optimiser runs it on the fused, graph-replayed step under the
    conditions of a ``DensityError`` (``FusedStep._rowwise3d`` with ``tfrt_focus_error``: clear,
    accumulate, solve, seed, finish), and it is a legal term of a ``SumError``.

    ``last_acc`` is the (G, 10) int64 table of the last evaluation, ``foci()`` the (G, d) float64
    foci in scene coordinates made from it (NaN for a group without a focus).  ``splat_variant``
    (0: by G; 1: table in LDS; 2: global atomics) is tfrt_focus_error's, for measuring."""

    splat_variant = 0
    has_direction = True          # (every geometry row is read and seeded)

    def __init__(self, groups, domain, n_groups=None, min_det=1e-12):
        what = type(self).__name__
        try:
            self.grid = ops.focus_grid(domain)
        except ValueError as e:
            raise ValueError(f"{what}: domain must be ((x0, x1), (y0, y1), (z0, z1)) -- "
                             f"((x0, x1), (y0, y1)) on a 2-D engine --, finite with lo < hi; got "
                             f"{domain!r}") from e
        self.domain = tuple((float(d[0]), float(d[1])) for d in domain)
        self.dimension = len(self.domain)
        self.fields = _GEO3 if self.dimension == 3 else _GEO2
        self.rows = list(range(2 * self.dimension))
        try:
            self.min_det = float(min_det)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: min_det must be a number, got {min_det!r}") from e
        if not (self.min_det > 0.0 and np.isfinite(self.min_det)):
            raise ValueError(f"{what}: min_det must be finite and > 0, got {min_det!r}")
        _init_groups(self, what, groups, n_groups, ops.FOCUS_MAX_GROUPS)
        self.last_acc = None
        self.last_foci = None

    def labels_of(self, src):
        """The int32 label buffer of the source set ``src`` on its device, one label per source
        ray, given or computed and cached as ``SpotError.labels_of`` does."""
        what = type(self).__name__
        return _source_buffer(self, "labels", self.groups,
                              lambda v, dev: _as_labels(what, v, dev), src, what, "label")

    def rows_for(self, dimension):
        """All ``2 * dimension`` rows of the geometry block; the box must have the engine's
        dimension."""
        if dimension != self.dimension:
            raise ValueError(f"{type(self).__name__}: a {dimension}-D engine needs a domain of "
                             f"{dimension} axes, got {self.domain!r}")
        return self.rows

    def graph_key(self):
        """What a captured step has baked in: the label buffer's address and the constants."""
        lab = self.labels
        return (None if lab is None else (lab.data_ptr(), tuple(lab.shape)), self.n_groups,
                self.grid, self.min_det, self.splat_variant)

    def evaluate(self, rows, labels, mask=None, perm=None, **buffers):
        """``ops.focus_error`` of the geometry block ``rows`` with these labels, box and
        ``min_det``."""
        out = ops.focus_error(rows, labels, self.n_groups, self.grid, self.min_det, mask=mask,
                              perm=perm, dimension=self.dimension, variant=self.splat_variant,
                              **buffers)
        self.last_acc, self.last_foci = out[2], out[3]
        return out

    def seed_columns(self, cols, hold):
        """tfrt_focus_error on the step's columns: it reads the source's label buffer through the
        trace's order ``cols.perm`` inside the kernels, as a SpotError does; the records go into
        ``hold.buffers["acc"]``, (G, 10), the solved table into ``hold.buffers["foci"]``."""
        self.rows_for(3)
        labels = self.labels_of(cols.src)
        G = self.n_groups
        held = self._held(hold, "acc", (G, ops.FOCUS_SLOTS), torch.int64, cols.rows.device,
                          lambda: _lib.lib().tfrt_focus_error_workspace_bytes(cols.n, G))
        if "foci" not in held:
            held["foci"] = torch.zeros((G, 4), dtype=torch.float64, device=cols.rows.device)
        self.evaluate(cols.rows, labels, mask=cols.mask, perm=cols.perm, grad=hold.g_fin,
                      err=hold.err, **held)

    def foci(self):
        """(G, d) float64 foci of the last evaluation in scene coordinates, NaN for a group
        without a focus."""
        if self.last_foci is None:
            raise RuntimeError(f"{type(self).__name__}: no evaluation yet")
        return ops.focus_points(self.last_foci, self.grid, self.dimension)

    def __call__(self, engine):
        """The (n_finished, 1) error terms through the generic path; the gradient rows come back
        in ``backward``."""
        self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros((0, 1), dtype=torch.float64)
        labels = self.labels_of(engine._trace_src)
        ids = engine.last_trace["finished_id"].to(torch.int32).contiguous()
        block = torch.stack([fin[f] for f in self.fields], dim=0)
        return _FocusTerms.apply(block, self, labels, ids)


class _FocusTerms(torch.autograd.Function):
    """FocusError over the (2 * dimension, n) geometry block of the finished rays, no mask;
    ``ids``: the source ray of every column.  Returns the (n, 1) terms, made from the solved
    table with the definition's operations as torch ops (``ops.focus_terms``)."""

    @staticmethod
    def forward(ctx, block, erf, labels, ids):
        rows = block.detach().contiguous()
        _, grad, _, foci = erf.evaluate(rows, labels, perm=ids)
        ctx.save_for_backward(grad)
        ctx.dtype = block.dtype
        return ops.focus_terms(rows, labels, erf.n_groups, erf.grid, foci, perm=ids,
                               dimension=erf.dimension)[:, None].contiguous()

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        return (upstream[:, 0] * grad).to(ctx.dtype), None, None, None


class DistortionError(_CoupledError):
    """The image must be an undistorted copy of the object -- at whatever scale and offset the
    lens gives: the distortion term of a lens merit function.  A ``SpotError`` makes the rays of
    an object point meet and leaves where the spots lie to the lens; a ``GoalError`` pins them to
    image points known in advance.  Here every group g has an object point ``p_g``, the centroids
    ``c_g`` of the groups' finished rays are fitted by ``c ~ A p + t`` over all groups, and the
    error is the sum over the rays inside the domain of the squared distance of their GROUP'S
    CENTROID from its fitted target ``A p_g + t``.  Neither the magnification nor the image
    centre is needed; both can be read afterwards (``fit_parameters()``).  It says nothing about
    spot size: add a ``SpotError`` in a ``SumError`` for that.

    ``fields``, ``groups``, ``domain``, ``oob_weight`` and ``n_groups`` are exactly
    ``SpotError``'s: one or two fields (positions or direction cosines), one label per SOURCE ray
    (or a callable with ``n_groups``), the label ``-1`` excludes a ray, rays outside the closed
    domain take the penalty ``oob_weight * (ex**2 + ey**2)`` and are in no group.  There are no
    ``weights``.  ``points``: (G, k) floats, the object coordinates of each group in the order of
    the fields, finite (a ``ValueError`` otherwise); kept as float64 on the device (``points``)
    and overwritable in place between steps -- a replayed graph reads the buffer.
    ``fit``: ``"scale"`` -- a scalar magnification M, sign free, ``A = M I``, and a free offset
    -- or ``"affine"`` -- a free k x k matrix and offset (with one field that is the scale fit).
    ``min_cond``: finite and >= 0, the affine fit's guard (below).

    For every finished ray, the four cases of ``SpotError`` in its order; a ray inside enters its
    group's record ``{count, Sx, Sy, 0}`` with the same ``qbits`` and ``qsx``.  A group with
    ``count > 0`` is USED: its weight ``w = count``, its centroid ``c`` as ``SpotError`` computes
    it.  Every float64 operation is rounded on its own; with one field the y components are 0.0:

    * ``W = sum w``, ``pm = (sum w p) / W``, ``cm = (sum w c) / W``;
    * ``dp = p - pm``, ``dc = c - cm``, ``Spp = sum w dp dp^T``, ``Scp = sum w dc dp^T`` (each
      entry ``w * (d1 * d2)``);
    * ``"scale"``: ``M = tr(Scp) / tr(Spp)``; valid iff at least two groups are used and
      ``tr(Spp) > 0``.  ``"affine"``: ``A = Scp Spp^-1`` by cofactors; valid iff
      ``det(Spp) > min_cond * (tr(Spp) / 2)**2`` (scale-free: collinear object points have no
      affine fit);
    * ``r = c - (cm + A dp)`` per used group, ``t = cm - A pm`` for reporting;
    * ``error = sum w rx**2 + sum w ry**2 + penalties`` over ``len(fields) * n_finished`` terms;
      a ray inside gets the gradient ``2 rx``, ``2 ry`` of its group (chained onto start and end
      rows with a direction field, as ``SpotError``'s).  No derivative of the fit is needed,
      because ``(A, t)`` minimises the error (up to the quantisation of the records).  Without a
      valid fit the rays inside add no error and get a zero gradient; the penalties remain.

    Every sum over the groups has a fixed shape and order (include/tfrt_hip.h at
    tfrt_distortion_error): two runs give the same bits.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.distortion_error`` over
    the finished rays' columns under a ``torch.autograd.Function`` that returns the (n_finished,
    k) terms -- a ray inside carries its group's ``rx**2``, ``ry**2``), which also serves sources
    that are not traced in place, ``deterministic=True``, fewer than 4,096 rays, several ranks
    (each shard then fits its own rays) and 2-D engines.  Its ``backward`` returns ``upstream *
    gradient``, exact when ``upstream`` is constant (the optimiser passes ones); with a direction
    field both fields of a ray must carry the same factor.  On a 3-D engine that traces its
    source in place the optimiser runs it on the fused, graph-replayed step wherever a
    ``SpotError`` runs there (``FusedStep._rowwise3d`` with ``tfrt_distortion_error``: clear,
    accumulate, fit, seed), and it is a legal term of a ``SumError``.

    ``last_acc`` is the (G, 4) int64 record table of the last evaluation, ``centroids()`` the
    (G, k) centroids made from it, ``residuals()`` the (G, k) residuals (NaN for a group without
    rays) and ``fit_parameters()`` the fit.  ``splat_variant`` is ``SpotError``'s."""

    splat_variant = 0

    def __init__(self, fields, groups, points, domain, fit="scale", oob_weight=0.0, n_groups=None,
                 min_cond=1e-9):
        from . import config
        what = "DistortionError"
        self.fields, self.domain = _fields_and_domain(what, fields, domain)
        self.rows = [_FIELDS3.index(f) for f in self.fields]
        self.has_direction = any(f.endswith("_dir") for f in self.fields)
        self.oob_weight = float(oob_weight)
        if not (self.oob_weight >= 0.0 and np.isfinite(self.oob_weight)):
            raise ValueError(f"{what}: oob_weight must be finite and >= 0")
        if fit not in ops.DISTORTION_FITS:
            raise ValueError(f"{what}: fit must be 'scale' or 'affine', got {fit!r}")
        self.fit = fit
        try:
            self.min_cond = float(min_cond)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: min_cond must be a number, got {min_cond!r}") from e
        if not (self.min_cond >= 0.0 and np.isfinite(self.min_cond)):
            raise ValueError(f"{what}: min_cond must be finite and >= 0, got {min_cond!r}")
        _init_groups(self, what, groups, n_groups, ops.SPOT_MAX_GROUPS)
        k = len(self.fields)
        try:
            p = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) \
                else np.asarray(points)
            p = np.ascontiguousarray(p, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: points must be numbers of shape ({self.n_groups}, {k})") \
                from e
        if p.ndim == 1 and k == 1:
            p = p[:, None]
        if p.shape != (self.n_groups, k):
            raise ValueError(f"{what}: points must have shape (n_groups, fields) = "
                             f"({self.n_groups}, {k}), got {p.shape}")
        if not np.isfinite(p).all():
            bad = np.nonzero(~np.isfinite(p).all(axis=1))[0][:5].tolist()
            raise ValueError(f"{what}: points must be finite; rows {bad} are not")
        self.points = torch.as_tensor(p).to(config.get_device())
        self._grids = {}
        self.last_acc = self.last_grid = self.last_qbits = None
        self.last_fit = self.last_residual = None

    def labels_of(self, src):
        """The int32 label buffer of the source set ``src`` on its device, one label per source
        ray, given or computed and cached as ``SpotError.labels_of`` does."""
        return _source_buffer(self, "labels", self.groups,
                              lambda v, dev: _as_labels("DistortionError", v, dev), src,
                              "DistortionError", "label")

    grid_for = SpotError.grid_for      # (the records are SpotError's: the same qbits and grid)

    def points_on(self, device):
        """The object points on ``device`` (moved once; a new buffer re-captures a graph)."""
        if self.points.device != device:
            self.points = self.points.to(device)
        return self.points

    def graph_key(self):
        """What a captured step has baked in: the addresses of the label buffer and of the
        ``points`` buffer, and the constants."""
        lab = self.labels
        return (None if lab is None else (lab.data_ptr(), tuple(lab.shape)), self.n_groups,
                self.domain, self.oob_weight, self.splat_variant, self.points.data_ptr(),
                self.fit, self.min_cond)

    def evaluate(self, rows, row_x, row_y, labels, mask=None, perm=None, dimension=None,
                 **buffers):
        """``ops.distortion_error`` of the columns of ``rows`` with these labels, points, domain
        and fit (``dimension`` given: ``rows`` is the geometry block, ``row_x`` / ``row_y`` field
        codes)."""
        qbits, grid = self.grid_for(labels.numel())
        out = ops.distortion_error(rows, row_x, row_y, labels, self.n_groups,
                                   self.points_on(rows.device), grid, fit=self.fit,
                                   min_cond=self.min_cond, oob_weight=self.oob_weight, mask=mask,
                                   perm=perm, variant=self.splat_variant, qbits=qbits,
                                   dimension=dimension, **buffers)
        self.last_acc, self.last_grid, self.last_qbits = out[2], grid, qbits
        self.last_fit, self.last_residual = out[3], out[4]
        return out

    def seed_columns(self, cols, hold):
        """tfrt_distortion_error on the step's columns: labels through the trace's order inside
        the kernels, as a SpotError; the records go into ``hold.buffers["acc"]``, (G, 4), the fit
        into ``["fit_out"]``, (8,), the residual table into ``["residual"]``, (G, 2)."""
        labels = self.labels_of(cols.src)
        G = self.n_groups
        dev = cols.rows.device
        held = self._held(hold, "acc", (G, 4), torch.int64, dev,
                          lambda: _lib.lib().tfrt_distortion_error_workspace_bytes(cols.n, G))
        if "residual" not in held:
            held["fit_out"] = torch.zeros(8, dtype=torch.float64, device=dev)
            held["residual"] = torch.zeros((G, 2), dtype=torch.float64, device=dev)
        self.evaluate(cols.rows, *_xy(self.rows), labels, mask=cols.mask, perm=cols.perm,
                      dimension=3, grad=hold.g_fin, err=hold.err, **held)

    def _last(self, name):
        value = getattr(self, name)
        if value is None:
            raise RuntimeError("DistortionError: no evaluation yet")
        return value

    def centroids(self):
        """(G, k) float64 centroids of the last evaluation, NaN for a group without rays."""
        return ops.spot_centroids(self._last("last_acc"), self.last_grid, len(self.fields),
                                  self.last_qbits)

    def residuals(self):
        """(G, k) float64 residuals ``c - (A p + t)`` of the last evaluation: NaN for a group
        without rays, zeros without a valid fit."""
        return self._last("last_residual")[:, :len(self.fields)]

    def fit_parameters(self):
        """The fit of the last evaluation, read from the device: a dict with ``matrix`` (k, k) and
        ``offset`` (k,) float64 CPU tensors (NaN without a valid fit), ``valid``,
        ``groups_used`` and, for ``fit="scale"``, ``magnification``."""
        f = self._last("last_fit").detach().cpu()
        k = len(self.fields)
        out = dict(matrix=f[:4].reshape(2, 2)[:k, :k].clone(), offset=f[4:4 + k].clone(),
                   valid=bool(f[6] != 0.0), groups_used=int(f[7]))
        if self.fit == "scale":
            out["magnification"] = float(f[0])
        return out

    def __call__(self, engine):
        """The (n_finished, k) error terms through the generic path; the gradient rows come back
        in ``backward``."""
        codes = self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros((0, len(self.fields)), dtype=torch.float64)
        labels = self.labels_of(engine._trace_src)
        block, _, ids, dim, codes = self._finished_block(engine, fin, codes, ids=True)
        return _DistortionTerms.apply(block, self, labels, ids, dim, codes)


class _DistortionTerms(torch.autograd.Function):
    """DistortionError over the finished rays, no mask; ``ids``: the source ray of every column;
    ``block``, ``dimension`` and ``codes`` as for ``_SpotTerms``.  Returns the (n, k) terms: a
    penalised ray's ``oob_weight * ex**2`` per field, an inside ray's squared residuals of its
    GROUP (their sum over the rays is the groups' ``w * r**2``), zeros for the rest."""

    @staticmethod
    def forward(ctx, block, erf, labels, ids, dimension=None, codes=None):
        rows = block.detach().contiguous()
        ctx.chained = codes is not None
        if codes is None:
            codes = (0, 1)[:rows.shape[0]]
        _, grad, acc, _, residual = erf.evaluate(rows, *_xy(codes), labels, perm=ids,
                                                 dimension=dimension)
        ctx.save_for_backward(grad)
        ctx.dtype = block.dtype
        if ctx.chained:
            link = ops._link_torch(rows, dimension)
            v = torch.stack([ops._link_field_torch(link, c, dimension) for c in codes], dim=0)
        else:
            v = rows.double()
        s = ids.long().clamp(0, labels.numel() - 1)
        r = residual[labels[s].long().clamp(0, erf.n_groups - 1), :v.shape[0]].t()
        return _spot_terms(erf, v, labels, ids, acc, None, inside=r * r)

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        if not ctx.chained:
            return (upstream.t() * grad).to(ctx.dtype), None, None, None, None, None
        if upstream.shape[1] == 2 and not torch.equal(upstream[:, 0], upstream[:, 1]):
            raise ValueError("DistortionError with a direction field: the upstream gradient must "
                             "weigh both fields of a ray alike")
        return (upstream[:, 0] * grad).to(ctx.dtype), None, None, None, None, None


class CentroidError(_CoupledError):
    """Where the CENTROID of a group of rays lies, without charging the spread of the group.  A
    ``GoalError`` pins every ray, so it charges spot size with position; a ``SpotError`` charges
    the spread alone; a ``DistortionError`` moves centroids towards a fitted copy of the object,
    scale and offset free.  Here every group's centroid is pinned to a target given in advance
    (``targets``) -- telecentricity or a prescribed chief-ray angle with direction fields (the
    MEAN direction of a bundle, its cone as wide as it is), a prescribed image height (f-theta,
    a fisheye law), a magnification without pulling against the spot term -- or the centroids of
    several groups are registered onto each other, wherever they meet (``parents``): the lateral
    colour of an object point (one group per wavelength band), the overlap of several emitters'
    beams, "all chief rays parallel, whatever the direction".

    ``fields``, ``groups``, ``domain``, ``oob_weight`` and ``n_groups`` are exactly
    ``DistortionError``'s: one or two fields (positions or direction cosines), one label per
    SOURCE ray (or a callable with ``n_groups``), kept as int32 on the device and overwritable
    between replays, the label ``-1`` excludes a ray, rays outside the closed domain take the
    penalty ``oob_weight * (ex**2 + ey**2)`` and are in no group.  There are no ``weights``.
    Giving both ``targets`` and ``parents`` is a ``ValueError``.

    * ``targets``: (G, k) floats (or (G,) with one field), kept as float64 on the device
      (``self.targets``, moved once) and overwritable in place between replayed steps; the
      buffer's address is part of ``graph_key()``.  A row with a NaN leaves that group unpinned
      (no error, zero gradient for its rays inside the domain); infinite entries are refused.
    * ``parents``: (G,) integers, kept as int32 on the device (``self.parents``), overwritable in
      place, its address in the graph key.  ``n_parents`` defaults to ``max + 1`` (at least 1),
      read once, 1 .. ``ops.SPOT_MAX_GROUPS``.  A group whose parent label lies outside
      ``[0, n_parents)`` is left out.
    * neither: one parent for all groups -- all centroids must coincide.

    For every finished ray, the four cases of ``SpotError`` in its order; a ray inside enters its
    group's record ``{count, Sx, Sy, 0}`` with the same ``qbits`` and ``qsx``.  Every float64
    operation is rounded on its own; with one field the y components are 0.0
    (include/tfrt_hip.h, tfrt_centroid_error):

    * a group with ``count > 0`` has rays: ``w = count``, ``c = x0 + (Sx / count) / qsx`` as
      ``SpotError`` computes it;
    * with ``parents`` the record of parent p is the INTEGER sum of the records of its groups
      that have rays and a legal label, ``C_p`` is formed from it by the same expression, and
      ``t_g = C_parent(g)``; with ``targets`` ``t_g = targets[g]``;
    * a group is USED if it has rays and a target (a finite row; a legal label):
      ``r = c - t``, ``e_g = w * (rx * rx)`` and ``w * (ry * ry)``;
    * the residual table is ``r`` for a used group, 0.0 for one with rays that is not used, NaN
      for one without rays;
    * ``error = (sum w rx**2 + sum w ry**2) + penalties`` over ``len(fields) * n_finished``
      terms, the sums over the groups in ``DistortionError``'s fixed shape and order: two runs
      give the same bits;
    * a ray inside gets the gradient ``2 rx``, ``2 ry`` of its group (chained onto start and end
      rows with a direction field, as ``SpotError``'s), a ray outside the penalty's derivative,
      every other ray zeros.  That is the exact gradient up to the quantisation of the records,
      and no centroid is differentiated: with ``targets``, ``d/dx_i`` of ``count_g |c_g -
      t_g|**2`` is ``2 r_g`` because ``d c_g / d x_i = 1 / count_g``; with ``parents``, ``C_p``
      minimises the sum of its groups' terms, so its derivative drops out.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.centroid_error`` over
    the finished rays' columns under a ``torch.autograd.Function`` that returns the (n_finished,
    k) terms -- a ray inside carries its group's ``rx**2``, ``ry**2``), which also serves sources
    that are not traced in place, ``deterministic=True``, fewer than 4,096 rays, several ranks
    and 2-D engines.  Its ``backward`` returns ``upstream * gradient``, exact when ``upstream`` is
    constant (the optimiser passes ones); with a direction field both fields of a ray must carry
    the same factor.  On a 3-D engine that traces its source in place the optimiser runs it on
    the fused, graph-replayed step wherever a ``SpotError`` runs there (``FusedStep._rowwise3d``
    with ``tfrt_centroid_error``: clear, accumulate, [parents,] table, seed), and it is a legal
    term of a ``SumError``.

    ``last_acc`` is the (G, 4) int64 record table of the last evaluation, ``centroids()`` the
    (G, k) centroids made from it, ``residuals()`` the (G, k) residuals, ``parent_centroids()``
    the (P, k) common centroids (``parents`` mode), ``groups_used`` the number of used groups
    (read from the device).  ``splat_variant`` is ``SpotError``'s."""

    splat_variant = 0

    def __init__(self, fields, groups, domain, targets=None, parents=None, oob_weight=0.0,
                 n_groups=None, n_parents=None):
        from . import config
        what = "CentroidError"
        self.fields, self.domain = _fields_and_domain(what, fields, domain)
        self.rows = [_FIELDS3.index(f) for f in self.fields]
        self.has_direction = any(f.endswith("_dir") for f in self.fields)
        self.oob_weight = float(oob_weight)
        if not (self.oob_weight >= 0.0 and np.isfinite(self.oob_weight)):
            raise ValueError(f"{what}: oob_weight must be finite and >= 0")
        if targets is not None and parents is not None:
            raise ValueError(f"{what}: give targets or parents, not both")
        _init_groups(self, what, groups, n_groups, ops.SPOT_MAX_GROUPS)
        G, k = self.n_groups, len(self.fields)
        dev = config.get_device()
        self.targets = self.parents = None
        self.n_parents = 0
        if targets is not None:
            if n_parents is not None:
                raise ValueError(f"{what}: n_parents goes with parents, not with targets")
            try:
                t = targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) \
                    else np.asarray(targets)
                t = np.ascontiguousarray(t, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{what}: targets must be numbers of shape ({G}, {k})") from e
            if t.ndim == 1 and k == 1:
                t = t[:, None]
            if t.shape != (G, k):
                raise ValueError(f"{what}: targets must have shape (n_groups, fields) = "
                                 f"({G}, {k}), got {t.shape}")
            if np.isinf(t).any():
                bad = np.nonzero(np.isinf(t).any(axis=1))[0][:5].tolist()
                raise ValueError(f"{what}: targets must be finite, or NaN for a group that is "
                                 f"not pinned; rows {bad} are infinite")
            self.targets = torch.as_tensor(t).to(dev)
        else:
            if parents is None:
                p = torch.zeros(G, dtype=torch.int32)
            else:
                p = parents if isinstance(parents, torch.Tensor) \
                    else torch.as_tensor(np.asarray(parents))
                if p.dim() != 1 or p.dtype.is_floating_point or p.dtype.is_complex \
                        or p.dtype == torch.bool or p.shape[0] != G:
                    raise ValueError(f"{what}: parents must be integers of shape (n_groups,) = "
                                     f"({G},); got shape {tuple(p.shape)}, {p.dtype}")
                p = p.detach().to(dtype=torch.int32)
            if n_parents is None:
                n_parents = max(int(p.max()) + 1, 1)
            try:
                self.n_parents = int(n_parents)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{what}: n_parents must be an integer, got {n_parents!r}") from e
            if not 1 <= self.n_parents <= ops.SPOT_MAX_GROUPS:
                raise ValueError(f"{what}: n_parents must lie in 1 .. {ops.SPOT_MAX_GROUPS}, got "
                                 f"{n_parents!r}")
            self.parents = p.to(dev).contiguous()
        self._grids = {}
        self.last_acc = self.last_grid = self.last_qbits = None
        self.last_residual = self.last_used = self.last_parent_acc = None

    def labels_of(self, src):
        """The int32 label buffer of the source set ``src`` on its device, one label per source
        ray, given or computed and cached as ``SpotError.labels_of`` does."""
        return _source_buffer(self, "labels", self.groups,
                              lambda v, dev: _as_labels("CentroidError", v, dev), src,
                              "CentroidError", "label")

    grid_for = SpotError.grid_for      # (the records are SpotError's: the same qbits and grid)

    def _mode_on(self, device):
        """(targets, parents) on ``device`` (moved once; a new buffer re-captures a graph)."""
        name = "targets" if self.targets is not None else "parents"
        if getattr(self, name).device != device:
            setattr(self, name, getattr(self, name).to(device))
        return self.targets, self.parents

    def graph_key(self):
        """What a captured step has baked in: the addresses of the label buffer and of the
        ``targets`` or ``parents`` buffer, and the constants."""
        lab = self.labels
        mode = self.targets if self.targets is not None else self.parents
        return (None if lab is None else (lab.data_ptr(), tuple(lab.shape)), self.n_groups,
                self.domain, self.oob_weight, self.splat_variant, self.targets is not None,
                mode.data_ptr(), self.n_parents)

    def evaluate(self, rows, row_x, row_y, labels, mask=None, perm=None, dimension=None,
                 **buffers):
        """``ops.centroid_error`` of the columns of ``rows`` with these labels, targets or
        parents and domain (``dimension`` given: ``rows`` is the geometry block, ``row_x`` /
        ``row_y`` field codes)."""
        qbits, grid = self.grid_for(labels.numel())
        targets, parents = self._mode_on(rows.device)
        out = ops.centroid_error(rows, row_x, row_y, labels, self.n_groups, grid, targets=targets,
                                 parents=parents,
                                 n_parents=None if parents is None else self.n_parents,
                                 oob_weight=self.oob_weight, mask=mask, perm=perm,
                                 variant=self.splat_variant, qbits=qbits, dimension=dimension,
                                 **buffers)
        self.last_acc, self.last_grid, self.last_qbits = out[2], grid, qbits
        self.last_residual, self.last_used, self.last_parent_acc = out[3], out[4], out[5]
        return out

    def seed_columns(self, cols, hold):
        """tfrt_centroid_error on the step's columns: labels through the trace's order inside the
        kernels, as a SpotError; the records go into ``hold.buffers["acc"]``, (G, 4), the residual
        table into ``["residual"]``, (G, 2), the counts into ``["used_out"]``, (2,), and with
        parents their records into ``["parent_acc"]``, (P, 4)."""
        labels = self.labels_of(cols.src)
        G, P = self.n_groups, self.n_parents
        dev = cols.rows.device
        held = self._held(hold, "acc", (G, 4), torch.int64, dev,
                          lambda: _lib.lib().tfrt_centroid_error_workspace_bytes(cols.n, G))
        by_parent = self.parents is not None
        if "residual" not in held or ("parent_acc" in held) != by_parent \
                or (by_parent and held["parent_acc"].shape[0] != P):
            held.pop("parent_acc", None)
            held["residual"] = torch.zeros((G, 2), dtype=torch.float64, device=dev)
            held["used_out"] = torch.zeros(2, dtype=torch.float64, device=dev)
            if by_parent:
                held["parent_acc"] = torch.zeros((P, 4), dtype=torch.int64, device=dev)
        self.evaluate(cols.rows, *_xy(self.rows), labels, mask=cols.mask, perm=cols.perm,
                      dimension=3, grad=hold.g_fin, err=hold.err, **held)

    def _last(self, name):
        value = getattr(self, name)
        if value is None:
            raise RuntimeError("CentroidError: no evaluation yet")
        return value

    def centroids(self):
        """(G, k) float64 centroids of the last evaluation, NaN for a group without rays."""
        return ops.spot_centroids(self._last("last_acc"), self.last_grid, len(self.fields),
                                  self.last_qbits)

    def residuals(self):
        """(G, k) float64 residuals ``c - t`` of the last evaluation: NaN for a group without
        rays, zeros for a group with rays and no target."""
        return self._last("last_residual")[:, :len(self.fields)]

    def parent_centroids(self):
        """(P, k) float64 common centroids of the last evaluation (``parents`` mode), NaN for a
        parent without rays."""
        if self.parents is None:
            raise RuntimeError("CentroidError: parent_centroids() needs parents, not targets")
        return ops.centroid_parent_centroids(self._last("last_parent_acc"), self.last_grid,
                                             len(self.fields))

    @property
    def groups_used(self):
        """The number of used groups of the last evaluation, read from the device."""
        return int(self._last("last_used")[0])

    def __call__(self, engine):
        """The (n_finished, k) error terms through the generic path; the gradient rows come back
        in ``backward``."""
        codes = self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros((0, len(self.fields)), dtype=torch.float64)
        labels = self.labels_of(engine._trace_src)
        block, _, ids, dim, codes = self._finished_block(engine, fin, codes, ids=True)
        return _CentroidTerms.apply(block, self, labels, ids, dim, codes)


class _CentroidTerms(torch.autograd.Function):
    """CentroidError over the finished rays, no mask; ``ids``: the source ray of every column;
    ``block``, ``dimension`` and ``codes`` as for ``_SpotTerms``.  Returns the (n, k) terms: a
    penalised ray's ``oob_weight * ex**2`` per field, an inside ray's squared residuals of its
    GROUP (their sum over the rays is the groups' ``w * r**2``), zeros for the rest."""

    @staticmethod
    def forward(ctx, block, erf, labels, ids, dimension=None, codes=None):
        rows = block.detach().contiguous()
        ctx.chained = codes is not None
        if codes is None:
            codes = (0, 1)[:rows.shape[0]]
        _, grad, acc, residual = erf.evaluate(rows, *_xy(codes), labels, perm=ids,
                                              dimension=dimension)[:4]
        ctx.save_for_backward(grad)
        ctx.dtype = block.dtype
        if ctx.chained:
            link = ops._link_torch(rows, dimension)
            v = torch.stack([ops._link_field_torch(link, c, dimension) for c in codes], dim=0)
        else:
            v = rows.double()
        s = ids.long().clamp(0, labels.numel() - 1)
        r = residual[labels[s].long().clamp(0, erf.n_groups - 1), :v.shape[0]].t()
        return _spot_terms(erf, v, labels, ids, acc, None, inside=r * r)

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        if not ctx.chained:
            return (upstream.t() * grad).to(ctx.dtype), None, None, None, None, None
        if upstream.shape[1] == 2 and not torch.equal(upstream[:, 0], upstream[:, 1]):
            raise ValueError("CentroidError with a direction field: the upstream gradient must "
                             "weigh both fields of a ray alike")
        return (upstream[:, 0] * grad).to(ctx.dtype), None, None, None, None, None


class MomentError(_CoupledError):
    """What the spot of a group of rays LOOKS like: the covariance of the group's finished rays
    -- the size and the shape of its spot -- must be a given matrix, or must be round.  A
    ``SpotError`` pulls the second moment of every group to zero, alike on both axes; a
    ``CentroidError`` says where the spot lies.  Here a spot gets a prescribed size (an
    illumination patch of a given width, a detector under-filled by a margin, a beam of a given
    divergence with ``("y_dir", "z_dir")``), an anamorphic shape (a line generator, a diode beam
    to be circularised), a waist at the target plane (``("y_end", "y_dir")`` with ``txy = 0``: a
    beam matrix in phase space) -- or, with ``shape="round"``, equal and uncorrelated widths on
    both axes at whatever size: the astigmatism term of an imaging merit function, beside the
    ``SpotError`` that sets the size.

    ``fields``, ``groups``, ``domain``, ``oob_weight`` and ``n_groups`` are exactly
    ``SpotError``'s: one or two fields (positions or direction cosines), one label per SOURCE ray
    (or a callable with ``n_groups``), kept as int32 on the device and overwritable between
    replays, the label ``-1`` excludes a ray, rays outside the closed domain take the penalty
    ``oob_weight * (ex**2 + ey**2)`` and are in no group.  There are no ``weights``.  Exactly one
    of ``covariance`` and ``shape`` is given (``ValueError`` otherwise):

    * ``covariance``: (G, 3) floats ``{txx, txy, tyy}`` in scene units squared -- (G, 1) or (G,)
      with one field; a single row serves every group --, kept as (G, 3) float64 on the device
      (``self.covariance``, moved once) and overwritable in place between replayed steps; the
      buffer's address is part of ``graph_key()``.  A NaN component is free (no error, no
      gradient from it); finite ``txx < 0``, ``tyy < 0`` or ``txy**2 > txx * tyy`` are refused.
    * ``shape="round"`` (two fields): ``s = (Cxx + Cyy) / 2`` is free.

    For every finished ray, the four cases of ``SpotError`` in its order.  Float64, every
    operation rounded on its own, integers exact (include/tfrt_hip.h, tfrt_moment_error); N is
    the source's ray count:

    * the grid: ``mbits = min(40, 2 * ((61 - bit_length(N)) // 2))`` (``ops.moment_mbits(N)``),
      ``h = mbits // 2``, ``ms = 2**mbits / (x1 - x0)`` per axis,
      ``m = min(max(rint((x - x0) * ms), 0), 2**mbits)``;
    * pass 1: a ray inside adds ``{1, mx, my}`` to its group's int64 record ``{n, Sx, Sy, 0}``;
    * a group with ``n >= 2`` is USED; its integer centre is ``kx = (2 * Sx + n) // (2 * n)``,
      ``cx = x0 + kx / ms``: within half a grid step of the centroid;
    * pass 2: a ray inside a used group has ``dx = mx - kx``, split as ``dxl = dx & (2**h - 1)``,
      ``dxh = dx >> h``; for (a, b) in xx, xy, yy the group's second record of nine int64 takes
      ``HH += ah * bh``, ``HL += ah * bl + al * bh``, ``LL += al * bl`` -- below ``2**62`` for any
      N, and ``HH * 2**mbits + HL * 2**h + LL`` is the exact ``sum(da * db)``;
    * ``Mf = (ldexp(HH, mbits) + ldexp(HL, h)) + LL``, ``C_ab = (Mf / n) / (ms_a * ms_b)``: the
      covariance about the centre (the ``(c - k)**2`` correction, below a quarter of a grid step
      squared, is dropped by definition);
    * the residual: ``D_ab = C_ab - t_ab`` (0 where ``t_ab`` is NaN); round: ``Dxx = Cxx - s``,
      ``Dyy = Cyy - s``, ``Dxy = Cxy``;
    * ``error = sum over used groups of n * ((Dxx**2 + 2 * Dxy**2) + Dyy**2) + penalties`` over
      ``len(fields) * n_finished`` terms, the sum over the groups in ``CentroidError``'s fixed
      shape and order: two runs give the same bits;
    * a ray inside a used group gets ``gx = Fxx * (x - cx) + Fxy * (y - cy)``,
      ``gy = Fxy * (x - cx) + Fyy * (y - cy)`` with ``F = 4 * D`` and its own float64 ``x``
      (chained onto start and end rows with a direction field), a ray outside the penalty's
      derivative, every other ray zeros.  No centre is differentiated, because the residuals of a
      group sum to zero, and ``s`` is not, because it minimises the error.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.moment_error`` over the
    finished rays' columns under a ``torch.autograd.Function`` that returns the (n_finished, k)
    terms -- a ray inside a used group carries ``(Dxx**2 + Dxy**2, Dxy**2 + Dyy**2)`` of its
    group, ``(Dxx**2)`` with one field), which also serves sources that are not traced in place,
    ``deterministic=True``, fewer than 4,096 rays, several ranks and 2-D engines.  Its
    ``backward`` returns ``upstream * gradient``, exact when ``upstream`` is constant; with a
    direction field both fields of a ray must carry the same factor.  On a 3-D engine that traces
    its source in place the optimiser runs it on the fused, graph-replayed step wherever a
    ``CentroidError`` runs there (``FusedStep._rowwise3d`` with ``tfrt_moment_error``: clear,
    accumulate, centres, pass 2, table, seed), and it is a legal term of a ``SumError``.

    ``last_acc`` / ``last_mom`` are the (G, 4) and (G, 9) int64 record tables of the last
    evaluation, ``centroids()`` the (G, k) centres, ``covariances()`` the (G, 3) ``{Cxx, Cxy,
    Cyy}`` ((G, 1) with one field), ``residuals()`` the ``D`` alike -- NaN for a group that is
    not used --, ``groups_used`` the number of used groups (read from the device).
    ``splat_variant`` is ``ops.moment_error``'s ``variant``."""

    splat_variant = 0

    def __init__(self, fields, groups, domain, covariance=None, shape=None, oob_weight=0.0,
                 n_groups=None):
        from . import config
        what = "MomentError"
        self.fields, self.domain = _fields_and_domain(what, fields, domain)
        self.rows = [_FIELDS3.index(f) for f in self.fields]
        self.has_direction = any(f.endswith("_dir") for f in self.fields)
        self.oob_weight = float(oob_weight)
        if not (self.oob_weight >= 0.0 and np.isfinite(self.oob_weight)):
            raise ValueError(f"{what}: oob_weight must be finite and >= 0")
        if (covariance is None) == (shape is None):
            raise ValueError(f"{what}: give exactly one of covariance and shape")
        _init_groups(self, what, groups, n_groups, ops.SPOT_MAX_GROUPS)
        G, k = self.n_groups, len(self.fields)
        k3 = 3 if k == 2 else 1
        self.shape, self.covariance = shape, None
        if shape is not None:
            if shape != "round":
                raise ValueError(f"{what}: shape must be 'round', got {shape!r}")
            if k != 2:
                raise ValueError(f"{what}: shape='round' needs two fields")
        else:
            try:
                t = covariance.detach().cpu().numpy() if isinstance(covariance, torch.Tensor) \
                    else np.asarray(covariance)
                t = np.array(t, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{what}: covariance must be numbers of shape ({G}, {k3})") from e
            if k3 == 1 and t.ndim <= 1 and t.size in (1, G):
                t = t.reshape(-1, 1)
            if t.ndim == 1 and t.shape[0] == k3:
                t = t[None, :]
            if t.ndim != 2 or t.shape[1] != k3 or t.shape[0] not in (1, G):
                raise ValueError(f"{what}: covariance must have shape (n_groups, {k3}) = "
                                 f"({G}, {k3}) or one such row, got {t.shape}")
            t = np.broadcast_to(t, (G, k3)).copy()
            if np.isinf(t).any():
                raise ValueError(f"{what}: covariance must be finite, or NaN for a free component")
            with np.errstate(invalid="ignore"):
                bad = t[:, 0] < 0
                if k3 == 3:
                    bad |= (t[:, 2] < 0) | (t[:, 1] * t[:, 1] > t[:, 0] * t[:, 2])
            if bad.any():
                raise ValueError(f"{what}: covariance rows {np.nonzero(bad)[0][:5].tolist()} are "
                                 "not positive semi-definite (txx >= 0, tyy >= 0, "
                                 "txy**2 <= txx * tyy)")
            self.covariance = torch.as_tensor(t).to(config.get_device())
        self._grids = {}
        self.last_acc = self.last_mom = self.last_grid = self.last_mbits = None
        self.last_rows = self.last_cov = self.last_used = None

    def labels_of(self, src):
        """The int32 label buffer of the source set ``src`` on its device, one label per source
        ray, given or computed and cached as ``SpotError.labels_of`` does."""
        return _source_buffer(self, "labels", self.groups,
                              lambda v, dev: _as_labels("MomentError", v, dev), src,
                              "MomentError", "label")

    def grid_for(self, n_source):
        """(mbits, grid constants) for a source of ``n_source`` rays: both paths of a step use
        the source's ray count, so the fused and the generic step quantise alike."""
        hit = self._grids.get(n_source)
        if hit is None:
            mbits = ops.moment_mbits(n_source)
            hit = self._grids[n_source] = (mbits, ops.spot_grid(self.domain, mbits))
        return hit

    def covariance_on(self, device):
        """The target buffer on ``device`` (moved once; a new buffer re-captures a graph); None
        with ``shape``."""
        if self.covariance is not None and self.covariance.device != device:
            self.covariance = self.covariance.to(device)
        return self.covariance

    def graph_key(self):
        """What a captured step has baked in: the addresses of the label buffer and of the
        target buffer, the mode and the constants."""
        lab, t = self.labels, self.covariance
        return (None if lab is None else (lab.data_ptr(), tuple(lab.shape)), self.n_groups,
                self.domain, self.oob_weight, self.splat_variant, self.shape,
                None if t is None else t.data_ptr())

    def evaluate(self, rows, row_x, row_y, labels, mask=None, perm=None, dimension=None,
                 **buffers):
        """``ops.moment_error`` of the columns of ``rows`` with these labels, target and domain
        (``dimension`` given: ``rows`` is the geometry block, ``row_x`` / ``row_y`` field
        codes)."""
        mbits, grid = self.grid_for(labels.numel())
        out = ops.moment_error(rows, row_x, row_y, labels, self.n_groups, grid,
                               covariance=self.covariance_on(rows.device), shape=self.shape,
                               oob_weight=self.oob_weight, mask=mask, perm=perm,
                               variant=self.splat_variant, mbits=mbits, dimension=dimension,
                               **buffers)
        self.last_acc, self.last_mom, self.last_grid, self.last_mbits = out[2], out[3], grid, mbits
        self.last_rows, self.last_cov, self.last_used = out[4], out[5], out[6]
        return out

    def seed_columns(self, cols, hold):
        """tfrt_moment_error on the step's columns: labels through the trace's order inside the
        kernels, as a SpotError; the records go into ``hold.buffers["acc"]``, (G, 4), and
        ``["mom"]``, (G, 9), the per-group rows into ``["group_rows"]``, (G, 8), covariances and
        residuals into ``["cov"]``, (G, 6), the counts into ``["used_out"]``, (2,)."""
        labels = self.labels_of(cols.src)
        G = self.n_groups
        dev = cols.rows.device
        held = self._held(hold, "acc", (G, 4), torch.int64, dev,
                          lambda: _lib.lib().tfrt_moment_error_workspace_bytes(cols.n, G))
        if "mom" not in held:
            held["mom"] = torch.zeros((G, 9), dtype=torch.int64, device=dev)
            held["group_rows"] = torch.zeros((G, 8), dtype=torch.float64, device=dev)
            held["cov"] = torch.zeros((G, 6), dtype=torch.float64, device=dev)
            held["used_out"] = torch.zeros(2, dtype=torch.float64, device=dev)
        self.evaluate(cols.rows, *_xy(self.rows), labels, mask=cols.mask, perm=cols.perm,
                      dimension=3, grad=hold.g_fin, err=hold.err, **held)

    def _last(self, name):
        value = getattr(self, name)
        if value is None:
            raise RuntimeError("MomentError: no evaluation yet")
        return value

    def centroids(self):
        """(G, k) float64 centres of the last evaluation -- the grid point nearest to each
        group's centroid --, NaN for a group without rays."""
        return self._last("last_rows")[:, :len(self.fields)]

    def covariances(self):
        """(G, 3) float64 ``{Cxx, Cxy, Cyy}`` of the last evaluation ((G, 1) with one field), NaN
        for a group of fewer than two rays."""
        return ops.moment_covariances(self._last("last_cov"), len(self.fields))

    def residuals(self):
        """(G, 3) float64 ``{Dxx, Dxy, Dyy}`` of the last evaluation ((G, 1) with one field), NaN
        for a group of fewer than two rays."""
        return self._last("last_cov")[:, 3:(6 if len(self.fields) == 2 else 4)]

    @property
    def groups_used(self):
        """The number of used groups of the last evaluation, read from the device."""
        return int(self._last("last_used")[0])

    def __call__(self, engine):
        """The (n_finished, k) error terms through the generic path; the gradient rows come back
        in ``backward``."""
        codes = self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros((0, len(self.fields)), dtype=torch.float64)
        labels = self.labels_of(engine._trace_src)
        block, _, ids, dim, codes = self._finished_block(engine, fin, codes, ids=True)
        return _MomentTerms.apply(block, self, labels, ids, dim, codes)


class _MomentTerms(torch.autograd.Function):
    """MomentError over the finished rays, no mask; ``ids``: the source ray of every column;
    ``block``, ``dimension`` and ``codes`` as for ``_SpotTerms``.  Returns the (n, k) terms: a
    penalised ray's ``oob_weight * ex**2`` per field, for an inside ray of a used group
    ``(Dxx**2 + Dxy**2, Dxy**2 + Dyy**2)`` of its GROUP (their sum over the rays is the groups'
    ``n * |D|**2``), zeros for the rest."""

    @staticmethod
    def forward(ctx, block, erf, labels, ids, dimension=None, codes=None):
        rows = block.detach().contiguous()
        ctx.chained = codes is not None
        if codes is None:
            codes = (0, 1)[:rows.shape[0]]
        out = erf.evaluate(rows, *_xy(codes), labels, perm=ids, dimension=dimension)
        grad, acc, cov = out[1], out[2], out[5]
        ctx.save_for_backward(grad)
        ctx.dtype = block.dtype
        if ctx.chained:
            link = ops._link_torch(rows, dimension)
            v = torch.stack([ops._link_field_torch(link, c, dimension) for c in codes], dim=0)
        else:
            v = rows.double()
        s = ids.long().clamp(0, labels.numel() - 1)
        D = cov[labels[s].long().clamp(0, erf.n_groups - 1), 3:]
        D = torch.where(torch.isnan(D), torch.zeros_like(D), D)      # (a group that is not used)
        cross = D[:, 1] * D[:, 1]
        inside = torch.stack([D[:, 0] * D[:, 0] + cross, cross + D[:, 2] * D[:, 2]], dim=0)
        return _spot_terms(erf, v, labels, ids, acc, None, inside=inside[:v.shape[0]])

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        if not ctx.chained:
            return (upstream.t() * grad).to(ctx.dtype), None, None, None, None, None
        if upstream.shape[1] == 2 and not torch.equal(upstream[:, 0], upstream[:, 1]):
            raise ValueError("MomentError with a direction field: the upstream gradient must "
                             "weigh both fields of a ray alike")
        return (upstream[:, 0] * grad).to(ctx.dtype), None, None, None, None, None


class FlatFieldError(FocusError):
    """The foci of all groups must lie in ONE plane with the normal ``axis`` -- a flat field --,
    wherever along the normal that plane has to stand: the sum, over the finished rays that count,
    of the squared distance of their group's focus from the plane, in the scene's units.  A
    ``FocusError`` frees the axial position of every object point's focus, so field curvature is
    no longer charged to the lens; a sensor is flat, and this is the term that says so:
    ``SumError([FocusError, FlatFieldError])`` is "a sharp image on a flat sensor, wherever along
    the axis it has to stand".

    ``groups``, ``domain``, ``n_groups``, ``min_det``: a ``FocusError``'s, and everything up to a
    group's focus ``x = A^-1 b`` is that class's, bit for bit -- which rays count, the box
    constants, the int64 records, the cofactor solve, "a focus needs two rays and
    ``det(A / count) >= min_det``".  ``axis``: ``dimension`` finite numbers, not all zero, default
    ``(1, 0, 0)`` (``(1, 0)`` with a 2-D domain); ``a = axis / sqrt(axis . axis)`` is formed once.

    Float64, every operation rounded on its own (include/tfrt_hip.h, tfrt_flatfield_error):

    * a group with a focus is USED: ``n = count``, ``h = a . x``, and by the same cofactors
      ``y = A^-1 a``;
    * ``W = sum n``, ``hbar = (sum n * h) / W`` over the used groups; the plane
      ``a . p = a . c + R * hbar`` is VALID with at least two used groups;
    * ``r = h - hbar``, ``e_g = (R * r) * (R * r)``, ``error = {sum n * e_g, number of counting
      rays in used groups, sum / number}``; without a valid plane the sum is 0.0 and every
      gradient zero;
    * the height ``hbar`` is not differentiated, because it minimises the sum; the FOCUS is: the
      group's adjoint is ``mu = (2 * (R * r)) * y``, and a counting ray of a used group, with
      ``focus_term``'s ``q``, ``alpha``, ``rho`` and ``lever`` and ``beta = mu . u``,
      ``muP = mu - beta * u``, ``k = beta / L``, gets ``muP * (1 - lever) - k * rho`` on the end
      rows and ``muP * lever + k * rho`` on the start rows -- the lever rule applied to the part
      of the adjoint across the ray, plus a term from turning the ray;
    * every float sum over the groups has a fixed shape and order: two runs give the same bits.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.flatfield_error`` over
    the finished rays' geometry block under a ``torch.autograd.Function`` that returns the
    (n_finished, 1) terms ``e_g`` of every ray's group), which serves the cases a ``FocusError``'s
    generic path serves.  Its ``backward`` returns ``upstream * gradient``: exact when ``upstream``
    is ONE constant (the optimiser passes ones), because the plane couples the groups.  On a 3-D
    engine that traces its source in place the optimiser runs it on the fused, graph-replayed
    step wherever a ``FocusError`` runs there (``tfrt_flatfield_error``: clear, accumulate, fit,
    seed), and it is a legal term of a ``SumError``.

    ``last_acc`` is the (G, 10) int64 record table of the last evaluation; ``foci()`` the (G, d)
    foci in scene coordinates, ``heights()`` the (G,) ``a . focus``, ``residuals()`` the (G,)
    ``R * r`` (NaN for an unused group, zeros without a plane), ``plane()`` the plane."""

    def __init__(self, groups, domain, axis=None, n_groups=None, min_det=1e-12):
        super().__init__(groups, domain, n_groups=n_groups, min_det=min_det)
        d = self.dimension
        if axis is None:
            axis = (1.0, 0.0, 0.0)[:d]
        try:
            self.unit_axis = ops.flatfield_axis(axis, d)
        except ValueError as e:
            raise ValueError(f"FlatFieldError: axis must be {d} finite numbers, not all zero (the "
                             f"domain has {d} axes); got {axis!r}") from e
        self.axis = tuple(float(v) for v in axis)
        self.last_table = None
        self.last_fit = None

    def graph_key(self):
        """A ``FocusError``'s, and the axis."""
        return super().graph_key() + (self.unit_axis,)

    def evaluate(self, rows, labels, mask=None, perm=None, **buffers):
        """``ops.flatfield_error`` of the geometry block ``rows`` with these labels, box, axis
        and ``min_det``."""
        out = ops.flatfield_error(rows, labels, self.n_groups, self.grid, self.axis, self.min_det,
                                  mask=mask, perm=perm, dimension=self.dimension,
                                  variant=self.splat_variant, **buffers)
        self.last_acc, self.last_table, self.last_fit = out[2], out[3], out[4]
        self.last_foci = out[3]               # (``foci()`` reads the first d entries of a row)
        return out

    def seed_columns(self, cols, hold):
        """tfrt_flatfield_error on the step's columns, as ``FocusError.seed_columns``: the
        records go into ``hold.buffers["acc"]``, (G, 10), the groups' table into
        ``hold.buffers["table"]``, (G, 8), the plane into ``hold.buffers["fit_out"]``."""
        self.rows_for(3)
        labels = self.labels_of(cols.src)
        G = self.n_groups
        dev = cols.rows.device
        held = self._held(hold, "acc", (G, ops.FOCUS_SLOTS), torch.int64, dev,
                          lambda: _lib.lib().tfrt_flatfield_error_workspace_bytes(cols.n, G))
        if "table" not in held:
            held["table"] = torch.zeros((G, ops.FLATFIELD_ROW), dtype=torch.float64, device=dev)
            held["fit_out"] = torch.zeros(8, dtype=torch.float64, device=dev)
        self.evaluate(cols.rows, labels, mask=cols.mask, perm=cols.perm, grad=hold.g_fin,
                      err=hold.err, **held)

    def _last(self, name):
        v = getattr(self, name)
        if v is None:
            raise RuntimeError("FlatFieldError: no evaluation yet")
        return v

    def heights(self):
        """(G,) float64 ``a . focus`` of the last evaluation in scene coordinates, NaN for a group
        without a focus."""
        f = self.foci()
        a = self.unit_axis
        h = a[0] * f[:, 0] + a[1] * f[:, 1]
        return h + a[2] * f[:, 2] if self.dimension == 3 else h

    def residuals(self):
        """(G,) float64 signed distances ``R * r`` of the foci from the plane in the scene's
        units: NaN for an unused group, zeros without a valid plane."""
        t, fit = self._last("last_table"), self._last("last_fit")
        a = self.unit_axis
        h = a[0] * t[:, 0] + a[1] * t[:, 1]
        if self.dimension == 3:
            h = h + a[2] * t[:, 2]
        r = torch.where(fit[4] != 0.0, self.grid[9] * (h - fit[0]), torch.zeros_like(h))
        return torch.where(t[:, 3] != 0.0, r, torch.full_like(r, float("nan")))

    def plane(self):
        """The plane of the last evaluation: ``axis`` (the unit normal, d floats), ``offset``
        (``axis . p = offset`` in scene coordinates; NaN without a used group), ``valid`` (at
        least two groups had a focus) and ``groups_used``."""
        fit = self._last("last_fit").cpu()
        return dict(axis=self.unit_axis[:self.dimension], offset=float(fit[1]),
                    valid=bool(fit[4] != 0.0), groups_used=int(fit[3]))

    def __call__(self, engine):
        """The (n_finished, 1) error terms through the generic path; the gradient rows come back
        in ``backward``."""
        self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros((0, 1), dtype=torch.float64)
        labels = self.labels_of(engine._trace_src)
        ids = engine.last_trace["finished_id"].to(torch.int32).contiguous()
        block = torch.stack([fin[f] for f in self.fields], dim=0)
        return _FlatFieldTerms.apply(block, self, labels, ids)


class _FlatFieldTerms(torch.autograd.Function):
    """FlatFieldError over the (2 * dimension, n) geometry block of the finished rays, no mask;
    ``ids``: the source ray of every column.  Returns the (n, 1) terms, ``e_g`` of every counting
    ray's used group (``ops.flatfield_terms``).  ``backward`` is ``upstream * gradient``: exact
    when ``upstream`` is one constant, because the plane couples the groups."""

    @staticmethod
    def forward(ctx, block, erf, labels, ids):
        rows = block.detach().contiguous()
        _, grad, _, table, _ = erf.evaluate(rows, labels, perm=ids)
        ctx.save_for_backward(grad)
        ctx.dtype = block.dtype
        return ops.flatfield_terms(rows, labels, erf.n_groups, erf.grid, table, perm=ids,
                                   dimension=erf.dimension)[:, None].contiguous()

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        return (upstream[:, 0] * grad).to(ctx.dtype), None, None, None


class MixingError(_CoupledError):
    """Every group of rays must land with the SAME density on the target -- whatever that density
    is: the R, G, B and W dies of an LED behind a mixing rod or a collimator (colour uniformity in
    the near field with ``("y_end", "z_end")``, in the far field with ``("y_dir", "z_dir")``), an
    emitter array that must survive a dead die, a homogeniser whose output must not depend on
    where the light entered (the groups are the input zones), a beam combiner.  A ``DensityError``
    per group needs a goal in advance and pins every group to it; here the pooled shape stays
    free -- a ``DensityError`` beside it in a ``SumError`` states that one.

    ``fields``, ``domain``, ``oob_weight``, ``weights`` and the bilinear splat are exactly
    ``DensityError``'s; ``bins`` is ``nx`` or ``(nx, ny)``, at most 65,536 bins.  ``groups`` and
    ``n_groups`` are ``SpotError``'s: one label per SOURCE ray (a tensor, or a callable with
    ``n_groups``), kept as int32 on the device (``labels``) and overwritable in place between
    replays, looked up through the trace's order inside the kernel; ``n_groups`` (G) at most 1,024
    and ``n_groups * bins`` at most ``2**20``.

    For every finished ray, float64 and int64, every operation rounded on its own
    (include/tfrt_hip.h, tfrt_mixing_error), B the number of bins:

    * the classification of ``DensityError`` (with ``weights``: the weighted one), then: a ray
      without a source ray, or whose label lies outside ``[0, G)``, counts as one with a
      non-finite coordinate -- nothing, zero gradient, no penalty;
    * a ray outside the closed domain adds ``oob_weight * (ex**2 + ey**2)``, times ``w`` last
      with weights; its gradient is the derivative of that;
    * a ray inside adds ``rint(b * 2**32)`` (``rint((b * w) * 2**32)`` with weights) to its two
      or four bins of ITS OWN GROUP's plane of the int64 histogram ``Hq[G, ny, nx]``;
    * the margins are integer sums, free of order: ``nq_g = sum_b Hq[g, b]``,
      ``Pq_b = sum_g Hq[g, b]``, ``Nq = sum_g nq_g``;
    * ``p_gb = Hq_gb / nq_g`` is the group's density, ``m_b = Pq_b / Nq`` the pooled one,
      ``e_g = B * sum_b (p_gb - m_b)**2`` the mean squared difference in units of the uniform
      density, ``E_mix = sum_g (nq_g / Nq) * e_g`` and ``error = E_mix + penalties``: ONE error
      term, ``{error, 1, error}``, as ``DensityError``.  A group with ``nq_g == 0`` is unused: it
      adds nothing, pulls nothing and its ``e_g`` reads as NaN; with ``Nq == 0`` everything is 0;
    * the pull ``D_gb = (2 * B / N) * (p_gb - m_b)`` with ``N = Nq * 2**-32``; a ray inside gets
      ``DensityError``'s gradient expression on its own group's plane of ``D``, times ``w`` last,
      chained onto start and end rows with a direction field.  No ``m``, ``n_g`` or ``N`` is
      differentiated: ``m`` is the mass-weighted mean of the ``p_g`` and so minimises the error,
      and a ray inside carries total weight 1 wherever it stands.
    * every float sum has a fixed shape and order -- over the bins of a group the fixed-shape
      workgroup sum, over the groups ``CentroidError``'s --: two runs give the same bits.

    It is an ordinary ``error_function(engine)`` (the generic path: ``ops.mixing_error`` over the
    finished rays' columns under a ``torch.autograd.Function``), which also serves sources that
    are not traced in place, ``deterministic=True``, fewer than 4,096 rays, several ranks and 2-D
    engines.  On a 3-D engine that traces its source in place the optimiser runs it on the fused,
    graph-replayed step exactly where a ``DensityError`` runs (``FusedStep._rowwise3d`` with
    ``tfrt_mixing_error``: clear, splat, margins, pulls, finish, seed), and it is a legal term of
    a ``SumError``.

    ``last_hq`` is the (G, ny, nx) int64 histogram of the last evaluation ((G, nx) with one
    field), ``shares()`` the densities ``p`` of that shape (NaN for an unused group), ``pooled()``
    the pooled density ``m``, ``group_errors()`` the (G,) ``e_g``, ``groups_used`` the number of
    used groups (read from the device).  ``splat_variant`` (0: by the number of cells; 1: table in
    LDS; 2: global atomics) is tfrt_mixing_error's, for measuring."""

    splat_variant = 0

    def __init__(self, fields, groups, domain, bins, oob_weight=0.0, n_groups=None, weights=None):
        what = "MixingError"
        self.fields, self.domain = _fields_and_domain(what, fields, domain)
        self.rows = [_FIELDS3.index(f) for f in self.fields]
        self.has_direction = any(f.endswith("_dir") for f in self.fields)
        k = len(self.fields)
        try:
            self.oob_weight = float(oob_weight)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: oob_weight must be finite and >= 0") from e
        if not (self.oob_weight >= 0.0 and np.isfinite(self.oob_weight)):
            raise ValueError(f"{what}: oob_weight must be finite and >= 0")
        try:
            counts = (int(bins),) * k if np.ndim(bins) == 0 else tuple(int(b) for b in bins)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: bins must be nx or (nx, ny), got {bins!r}") from e
        if len(counts) != k or any(c < 1 for c in counts) \
                or int(np.prod(counts, dtype=np.int64)) > ops.DENSITY_MAX_BINS:
            raise ValueError(f"{what}: bins must give one count >= 1 per field and at most "
                             f"{ops.DENSITY_MAX_BINS} bins, got {bins!r}")
        self.bins = counts
        _init_groups(self, what, groups, n_groups, ops.MIXING_MAX_GROUPS)
        if self.n_groups * int(np.prod(counts, dtype=np.int64)) > ops.MIXING_MAX_CELLS:
            raise ValueError(f"{what}: n_groups * bins must not exceed {ops.MIXING_MAX_CELLS}, "
                             f"got {self.n_groups} groups of {bins!r} bins")
        self.grid = ops.density_grid(self.domain, counts[0], counts[1] if k == 2 else None)
        self.last_hq = self.last_pull = self.last_group_errors = self.last_used = None
        _init_weights(self, what, weights)
        if self.weights is not None and self.labels is not None \
                and self.weights.numel() != self.labels.numel():
            raise ValueError(f"{what}: {self.weights.numel()} weights for "
                             f"{self.labels.numel()} labels -- one of each per source ray")

    def labels_of(self, src):
        """The int32 label buffer of the source set ``src`` on its device, one label per source
        ray, given or computed and cached as ``SpotError.labels_of`` does."""
        return _source_buffer(self, "labels", self.groups,
                              lambda v, dev: _as_labels("MixingError", v, dev), src,
                              "MixingError", "label")

    def graph_key(self):
        """What a captured step has baked in: the addresses of the label buffer and of the weight
        buffer, the grid, ``n_groups`` and the constants."""
        lab = self.labels
        return (None if lab is None else (lab.data_ptr(), tuple(lab.shape)), self.n_groups,
                self.bins, self.grid, self.oob_weight, self.splat_variant) + _weights_key(self)

    def evaluate(self, rows, row_x, row_y, labels, mask=None, perm=None, dimension=None,
                 weights=None, **buffers):
        """``ops.mixing_error`` of the columns of ``rows`` with these labels, bins, domain and
        weight (``dimension`` given: ``rows`` is the geometry block, ``row_x`` / ``row_y`` field
        codes; ``weights``: the buffer of ``weights_of``)."""
        if weights is not None and weights.numel() != labels.numel():
            raise ValueError(f"MixingError: {weights.numel()} weights for {labels.numel()} "
                             "labels -- one of each per source ray")
        out = ops.mixing_error(rows, row_x, row_y, labels, self.n_groups, self.bins, self.grid,
                               self.oob_weight, mask=mask, perm=perm, variant=self.splat_variant,
                               dimension=dimension, weights=weights, **buffers)
        self.last_hq, self.last_pull = out[2], out[3]
        self.last_group_errors, self.last_used = out[4], out[5]
        return out

    def seed_columns(self, cols, hold):
        """tfrt_mixing_error on the step's columns: labels and weights through the trace's order
        ``cols.perm`` inside the kernels, as a SpotError; the histogram goes into
        ``hold.buffers["hq"]``, (G, ny, nx), the pulls into ``["pull"]``, the groups' errors into
        ``["group_errors"]``, (G,), and the counts into ``["used_out"]``, (2,)."""
        labels, weights = self.labels_of(cols.src), self.weights_of(cols.src)
        G = self.n_groups
        dev = cols.rows.device
        shape = (G,) + tuple(reversed(self.bins))
        nx, ny = self.bins[0], (self.bins[1] if len(self.bins) == 2 else 1)
        held = self._held(hold, "hq", shape, torch.int64, dev,
                          lambda: _lib.lib().tfrt_mixing_error_workspace_bytes(cols.n, G, nx, ny))
        if "pull" not in held:
            held["pull"] = torch.zeros(shape, dtype=torch.float64, device=dev)
            held["group_errors"] = torch.zeros(G, dtype=torch.float64, device=dev)
            held["used_out"] = torch.zeros(2, dtype=torch.float64, device=dev)
        self.evaluate(cols.rows, *_xy(self.rows), labels, mask=cols.mask, perm=cols.perm,
                      dimension=3, weights=weights, grad=hold.g_fin, err=hold.err, **held)

    def _last(self, name):
        value = getattr(self, name)
        if value is None:
            raise RuntimeError("MixingError: no evaluation yet")
        return value

    def shares(self):
        """(G, ny, nx) float64 densities ``p_gb = Hq_gb / nq_g`` of the last evaluation ((G, nx)
        with one field), NaN for a group without mass."""
        hq = self._last("last_hq")
        flat = hq.reshape(hq.shape[0], -1)
        nq = flat.sum(dim=1)
        p = flat.double() / torch.where(nq > 0, nq, torch.ones_like(nq)).double()[:, None]
        p = torch.where((nq > 0)[:, None], p, torch.full_like(p, float("nan")))
        return p.reshape(hq.shape)

    def pooled(self):
        """(ny, nx) float64 pooled density ``m_b = Pq_b / Nq`` of the last evaluation ((nx,) with
        one field), NaN when nothing landed."""
        hq = self._last("last_hq")
        pq = hq.sum(dim=0)
        return pq.double() / pq.sum().double()

    def group_errors(self):
        """(G,) float64 ``e_g`` of the last evaluation, NaN for a group without mass."""
        return self._last("last_group_errors")

    @property
    def groups_used(self):
        """The number of groups with mass in the last evaluation, read from the device."""
        return int(self._last("last_used")[0])

    def __call__(self, engine):
        """The error as a (1,) tensor through the generic path; the gradient rows come back in
        ``backward``."""
        codes = self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return torch.zeros(1, dtype=torch.float64)
        labels = self.labels_of(engine._trace_src)
        block, weights, ids, dim, codes = self._finished_block(engine, fin, codes, ids=True)
        return _MixingTerms.apply(block, self, labels, ids, weights, dim, codes)


class _MixingTerms(torch.autograd.Function):
    """MixingError over the finished rays, no mask; ``ids``: the source ray of every column;
    ``block``, ``dimension`` and ``codes`` as for ``_DensityTerms``; ``weights`` or None."""

    @staticmethod
    def forward(ctx, block, erf, labels, ids, weights=None, dimension=None, codes=None):
        rows = block.detach().contiguous()
        if codes is None:
            codes = (0, 1)[:rows.shape[0]]
        out = erf.evaluate(rows, *_xy(codes), labels, perm=ids, dimension=dimension,
                           weights=weights)
        ctx.save_for_backward(out[1])
        ctx.dtype = block.dtype
        return out[0][:1].clone()

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        return (upstream * grad).to(ctx.dtype), None, None, None, None, None, None


# the coupled errors: all finished rays of a step enter one evaluation (one process)
_COUPLED = (DensityError, SpotError, TransportError, FocusError, DistortionError, FlatFieldError,
            CentroidError, MomentError, MixingError)


class SumError:
    """A weighted sum of error terms on ONE step: ``error = sum_k c_k * term_k``.  A real design
    is never one term: transport to find the target and density for the detail, a spot size with
    a magnification pinned by a goal, a near field and a far field at once.  Every term reads the
    same finished rays of one trace and the reverse sweep is linear in its seed, so the combined
    step is one trace, K error evaluations, one combination and one reverse sweep.

    ``terms``: 1 to 8 distinct instances of ``GoalError``, ``DensityError``, ``SpotError``,
    ``TransportError``, ``FocusError``, ``DistortionError``, ``FlatFieldError``,
    ``CentroidError``, ``MomentError`` or ``MixingError``; a ``RowwiseError``, a nested ``SumError`` or the same object twice is a ValueError.  ``weights``: K finite values >= 0, default all ones, kept as the (K,) float64
    device tensor ``weights``; ``set_weights(values)`` validates on the host and overwrites that
    buffer in place, so a replayed graph sees the new values without a re-capture (as
    ``TransportError.set_goal``).  A weight of 0 switches a term off for a phase; the term is
    still evaluated.  ``reduce``: ``"sum"``, ``c_k = w_k`` and ``term_k`` the term's error sum; or
    ``"mean"``, ``c_k = w_k / terms_k`` with ``terms_k`` the term's own count of error terms
    (0.0 for a term without any), read on the device.  Every product and every sum is rounded on
    its own, the terms in index order (tfrt_error_combine); the sum reports itself as ONE error
    term, ``{E, 1, E}``, as a ``DensityError`` does.

    After an evaluation ``last_errors`` is the (K, 3) tensor of the terms' own triples {sum, terms,
    mean} and ``last_coefficients`` the (K,) ``c_k``; each term keeps its own ``last_hq`` /
    ``centroids()`` / ``last_rank2`` / ``foci()`` / ``fit_parameters()`` / ``plane()`` as when it
    runs alone.

    It is an ordinary ``error_function(engine)`` -- the generic path returns the (1,) tensor
    ``sum_k c_k * term_k(engine).sum()`` (``terms_k = numel``) under torch autograd, which serves
    2-D engines, fewer than 4,096 rays, ``deterministic=True`` and sources not traced in place.
    On a 3-D engine that traces its source in place the optimiser runs it on the fused,
    graph-replayed step under the conditions of a ``DensityError``: every term evaluates into a
    seed block of its own (a ``GoalError`` through tfrt_goal_error_columns, its goal row looked up
    through the trace's order inside the kernel), and one tfrt_error_combine launch writes the
    step's seed block and error.  One process."""

    on_columns = True

    def __init__(self, terms, weights=None, reduce="sum"):
        from . import config
        try:
            terms = tuple(terms)
        except TypeError as e:
            raise ValueError("SumError: terms must be a sequence of error terms") from e
        if not 1 <= len(terms) <= ops.COMBINE_MAX_TERMS:
            raise ValueError(f"SumError: 1 .. {ops.COMBINE_MAX_TERMS} terms, got {len(terms)}")
        for t in terms:
            if isinstance(t, SumError):
                raise ValueError("SumError: a nested SumError is not supported -- list its terms "
                                 "(and multiply the weights) instead")
            if isinstance(t, RowwiseError):
                raise ValueError("SumError: a RowwiseError cannot be a term (its error is torch "
                                 "code of its own); state it as a GoalError")
            if not isinstance(t, (GoalError,) + _COUPLED):
                raise ValueError("SumError: terms must be GoalError, DensityError, SpotError, "
                                 "TransportError, FocusError, DistortionError, FlatFieldError or "
                                 "CentroidError instances, or MomentError or MixingError ones; "
                                 "got "
                                 f"{type(t).__name__}")
        if len(set(id(t) for t in terms)) != len(terms):
            raise ValueError("SumError: the same term object is listed twice (a term keeps the "
                             "buffers of its last evaluation); make a second instance")
        if reduce not in ("sum", "mean"):
            raise ValueError(f"SumError: reduce must be 'sum' or 'mean', got {reduce!r}")
        self.terms, self.reduce = terms, reduce
        values = self._as_values(len(terms), [1.0] * len(terms) if weights is None else weights)
        self.weights = torch.as_tensor(values).to(config.get_device())
        # every term's rows, in term order: a step's buffers are keyed on them
        self.rows = [r for t in terms for r in t.rows]
        self.fields = tuple(t.fields for t in terms)
        self.last_errors = self.last_coefficients = None

    @staticmethod
    def _as_values(K, weights):
        try:
            w = np.asarray(weights.detach().cpu() if isinstance(weights, torch.Tensor)
                           else weights, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"SumError: weights must be {K} numbers, got {weights!r}") from e
        if w.shape != (K,):
            raise ValueError(f"SumError: {K} weights for {K} terms, got shape {w.shape}")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError(f"SumError: weights must be finite and >= 0, got {w.tolist()}")
        return np.ascontiguousarray(w)

    def set_weights(self, values):
        """Other weights, checked on the host and copied into the device buffer there is."""
        self.weights.copy_(torch.as_tensor(self._as_values(len(self.terms), values)))

    def weights_on(self, device):
        """The weight buffer on ``device`` (moved once; a new buffer re-captures a graph)."""
        if self.weights.device != device:
            self.weights = self.weights.to(device)
        return self.weights

    def rows_for(self, dimension):
        return [r for t in self.terms for r in t.rows_for(dimension)]

    def graph_key(self):
        """What a captured step has baked in: the terms' keys, the weight buffer's address and
        ``reduce``."""
        return (tuple((id(t), t.graph_key()) for t in self.terms), self.weights.data_ptr(),
                self.reduce)

    def __call__(self, engine):
        """The error as a (1,) tensor through the generic path: the terms called one by one, then
        tfrt_error_combine's operations in its order as torch ops."""
        total, triples, coeffs = None, [], []
        for k, term in enumerate(self.terms):
            e = term(engine)
            s = e.sum().double()
            w = self.weights_on(s.device)[k]
            if self.reduce == "sum":
                c = w
            else:
                c = w / float(e.numel()) if e.numel() > 0 else torch.zeros_like(w)
            p = c * s
            total = p if total is None else total + p
            with torch.no_grad():
                n = torch.full_like(w, float(e.numel()))
                triples.append(torch.stack([s.detach(), n, s.detach() / n if e.numel() > 0
                                            else torch.full_like(w, float("nan"))]))
                coeffs.append(c.detach())
        self.last_errors, self.last_coefficients = torch.stack(triples), torch.stack(coeffs)
        return total.reshape(1)

