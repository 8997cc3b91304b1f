"""
The optimiser step as ONE fixed launch sequence (no host read inside, hipGraph-replayable).

``SGD_Optimizer.single_step`` of the reference (tfrt/optimizer.py:187-320) is

    system.update() -> engine.ray_trace(depth) -> error_function(engine) -> tape.gradient
    -> non-finite -> 0, scale, clip, accumulate -> SGD apply

The generic path of this package keeps the user's ``error_function`` arbitrary torch code, which
costs a blocking read of the ray counts (the finished set has a data-dependent length), ~25
stock torch kernels for the error and its reverse, and autograd bookkeeping: ~0.75 ms per step
whatever the ray count -- the part that caps ray-parallel strong scaling.

The error functions of the reference's optimisation scripts all have one form
(dev/hexalens.py:144-168):  ``squared_difference(stack(finished[fields]), goal)`` with ``goal``
a function of fields the finished rays inherit unchanged from their source rays.  ``GoalError``
states that form declaratively; an optimiser given a ``GoalError`` runs ``FusedStep``:

    system.update()                     constraints, parameters -> faces   (torch + tfrt_param_faces_*)
    tfrt_trace3d_forward                into persistent buffers, counts stay on the device
    tfrt_goal_error3d                   error sum (fixed order) + gradient seed 2 (output - goal)
    tfrt_trace3d_backward               -> d error / d faces   (coherent rays: both as ONE launch,
                                        tfrt_trace3d_backward_goal)
    autograd through update()           -> d error / d parameters           (tfrt_param_faces_backward ...)
    [one all-reduce over ray shards]
    tfrt_sgd_process_dev / tfrt_csr_matvec   non-finite -> 0, scale, clip, accumulate, SGD apply
                                        (tfrt_sgd_momentum_multi with apply_momentum=True,
                                        tfrt_adam_multi for an Adam_Optimizer)

A 2-D engine (one process, no ray shards) runs ``FusedStep._goal2d`` instead of ``_goal3d``:
``tfrt_trace2d_forward``, then ``tfrt_trace2d_backward_goal`` -- error, seed and the reverse sweep of
every pass in ONE launch -- and autograd from the merged segments and arcs to the parameters.  With a
``RowwiseError`` (``_rowwise2d``) the error comes from ``tfrt_trace2d_rows`` (every source ray's
fixed-shape column), ``fn`` and its autograd, and ``tfrt_trace2d_backward_rows`` sweeps from that
gradient; ``_rowwise3d`` does the same on a 3-D engine with an in-place trace that leaves the
finished rows at the rays' own columns.  A ``DensityError`` -- the finished rays, taken together,
must land with a given density -- takes ``_rowwise3d`` too, with ``tfrt_density_error`` (four
launches: clear, splat, bins, seed) in the place of ``fn`` and its autograd; a ``SpotError`` -- rays
of one group must meet in one point -- likewise with ``tfrt_spot_error`` (clear, accumulate, seed,
finish); a ``TransportError`` -- the same target density by sliced optimal transport -- with
``tfrt_transport_error`` (per direction keys, radix sort, sorted keys, ranks; then seed and finish).
A ``SumError`` -- a weighted sum of such terms and of ``GoalError``s -- takes ``_rowwise3d`` as well:
every term's launches into a seed block of its own (a ``GoalError`` through
``tfrt_goal_error_columns``), then ONE ``tfrt_error_combine`` for the step's seed block and error.

The four bodies share one skeleton: ``_enqueue_gradient`` does what comes before the trace, the
body its launches over a ``_StepState``, ``_publish_lazily`` and ``_enqueue_apply`` what comes after.

Every launch has step-independent arguments (learning-rate dependent scalars live in a small
device table), so after a few eager steps the sequence is captured once in a HIP graph
(``torch.cuda.CUDAGraph``) and replayed: one graph launch per step.  With ray shards over several
processes the collective splits it in two graphs (RCCL is called eagerly between them).

``GoalError`` is also an ordinary error function (``__call__(engine)``): the generic path gives
the same numbers, which is what the parity tests compare.
"""
import contextlib
import ctypes
import gc

import numpy as np
import torch

from . import _lib, ops
from . import distributed as tdist
from ._lib import RayOut, check

_GEO3 = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end")
_GEO2 = ("x_start", "y_start", "x_end", "y_end")
# the fields of the coupled errors (DensityError, SpotError): a row of the geometry block or a
# direction cosine of the finished ray's last link; the index is the field code of
# tfrt_density_error_fields / tfrt_spot_error_fields
_FIELDS3 = _GEO3 + ("x_dir", "y_dir", "z_dir")
_FIELDS2 = _GEO2 + ("x_dir", "y_dir")

_CLASS_FLAGS = (("finished", _lib.COMPILE_FINISHED), ("active", _lib.COMPILE_ACTIVE),
                ("stopped", _lib.COMPILE_STOPPED), ("dead", _lib.COMPILE_DEAD))


class _NotInPlace(RuntimeError):
    """The fixed-shape path of a RowwiseError needs an in-place trace; this step takes the generic
    path instead."""


class GoalError:
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
        if hasattr(src, "cache_key"):      # rays made in place (sources.DeviceRaySet): lazy fields
            vals, key = [src], src.cache_key
        else:
            vals = list(src.values()) if hasattr(src, "values") else [src[k] for k in src.keys()]
            key = tuple((id(v), getattr(v, "_version", None)) for v in vals)
        key = (key, bool(by_ray))
        if self._cache is not None and self._cache[0] == key:
            return self._cache[1]
        g = self.goal(src) if callable(self.goal) else self.goal
        if hasattr(src, "n_rays"):
            n, dev = src.n_rays, src.device
        else:
            n, dev = src["x_start"].shape[0], src["x_start"].device
        g = torch.as_tensor(g, dtype=torch.float64, device=dev).detach()
        if g.dim() == 1:
            g = g.reshape(-1, 1)
        if tuple(g.shape) != (n, len(self.fields)):
            raise ValueError(f"GoalError: goal has shape {tuple(g.shape)}, expected "
                             f"({n}, {len(self.fields)}) -- one row per source ray")
        table = g.contiguous() if by_ray else g.t().contiguous()
        self._cache = (key, table, vals)     # the keyed tensors stay alive with the key
        return table

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


def _geometry_block(engine, fin):
    """(dimension, the (2 * dimension, n) block of the finished rays' geometry fields)."""
    dim = engine.dimension
    return dim, torch.stack([fin[f] for f in (_GEO3 if dim == 3 else _GEO2)], dim=0)


def _source_buffer(owner, name, given, convert, src, what, noun, keep=False):
    """``owner.<name>``, a buffer with one entry per SOURCE ray of the source set ``src``, on the
    source's device: the tensor given (moved once; a new buffer re-captures a graph), or the
    result of the callable ``given`` on the source's field dict, converted by ``convert(value,
    device)`` and cached in ``owner._caches[name]`` by the versions of the source's fields as
    ``GoalError.table`` is.  ``keep``: a new result of the callable is copied into the buffer
    there is (same shape), so its address -- part of a step's signature -- stays and a step that
    is being captured records the evaluation.  What ``SpotError.labels_of`` and the errors'
    ``weights_of`` share."""
    if hasattr(src, "n_rays"):
        n, dev = src.n_rays, src.device
    else:
        n, dev = src["x_start"].shape[0], src["x_start"].device
    value = getattr(owner, name)
    if callable(given):
        if hasattr(src, "cache_key"):      # rays made in place (sources.DeviceRaySet)
            vals, key = [src], src.cache_key
        else:
            vals = list(src.values()) if hasattr(src, "values") else [src[k] for k in src.keys()]
            key = tuple((id(v), getattr(v, "_version", None)) for v in vals)
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


class DensityError:
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

    def rows_for(self, dimension):
        """Field codes on a ``dimension``-D trace: the row of the ray block a geometry field is
        read from, ``2 * dimension + axis`` for a direction cosine."""
        if dimension == 3:
            return self.rows
        return _field_codes("DensityError", self.fields, dimension)

    def goal_on(self, device):
        """The goal buffer on ``device`` (moved once; a new buffer re-captures a graph)."""
        if self.goal.device != device:
            self.goal = self.goal.to(device)
        return self.goal

    def weights_of(self, src):
        """The float64 weight buffer of the source set ``src`` on its device, one weight in [0, 1]
        per source ray (None without weights): the tensor given, or the callable's result,
        normalised and cached as ``SpotError.labels_of`` caches its labels."""
        if self.weights_given is None:
            return None
        return _source_buffer(self, "weights", self.weights_given,
                              lambda v, dev: _as_weights("DensityError", v, dev), src,
                              "DensityError", "weight", keep=True)

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

    def __call__(self, engine):
        """The error as a (1,) tensor through the generic path; the gradient rows come back in
        ``backward``."""
        codes = self.rows_for(engine.dimension)
        fin = engine.finished_rays
        if not bool(fin):
            return (self.goal * self.goal).sum().reshape(1)
        weights = ids = None
        if self.weights_given is not None:
            weights = self.weights_of(engine._trace_src)
            ids = engine.last_trace["finished_id"].to(torch.int32).contiguous()
        if self.has_direction:
            dim, block = _geometry_block(engine, fin)
            return _DensityTerms.apply(block, self, weights, ids, dim, tuple(codes))
        return _DensityTerms.apply(torch.stack([fin[f] for f in self.fields], dim=0), self,
                                   weights, ids)


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
        err, grad, _ = erf.evaluate(rows, codes[0], codes[1] if len(codes) == 2 else -1,
                                    dimension=dimension, weights=weights, perm=ids)
        ctx.save_for_backward(grad)
        ctx.dtype = block.dtype
        return err[:1].clone()

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        return (upstream * grad).to(ctx.dtype), None, None, None, None, None


class TransportError:
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

    def rows_for(self, dimension):
        """The rows of a ``dimension``-D geometry block the fields are read from."""
        if dimension == 3:
            return self.rows
        return _field_codes("TransportError", self.fields, dimension)

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


class SpotError:
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
        from . import config
        self.fields = (fields,) if isinstance(fields, str) else tuple(fields)
        if len(self.fields) not in (1, 2) or any(f not in _FIELDS3 for f in self.fields) \
                or len(set(self.fields)) != len(self.fields):
            raise ValueError(f"SpotError: one or two distinct fields out of {_FIELDS3}, got {fields!r}")
        self.rows = [_FIELDS3.index(f) for f in self.fields]
        self.has_direction = any(f.endswith("_dir") for f in self.fields)
        k = len(self.fields)
        try:
            domain = tuple((float(d[0]), float(d[1])) for d in domain)
        except (IndexError, TypeError) as e:
            raise ValueError("SpotError: domain must be ((x0, x1), (y0, y1)) or ((x0, x1),)") from e
        if len(domain) != k or any(not (np.isfinite(a) and np.isfinite(b) and b > a) for a, b in domain):
            raise ValueError(f"SpotError: domain needs one finite (lo, hi), lo < hi, per field; got {domain!r}")
        self.domain = domain
        self.oob_weight = float(oob_weight)
        if not (self.oob_weight >= 0.0 and np.isfinite(self.oob_weight)):
            raise ValueError("SpotError: oob_weight must be finite and >= 0")
        self.groups = groups
        self.labels = None
        self._caches = {}
        if callable(groups):
            if n_groups is None:
                raise ValueError("SpotError: callable groups need n_groups")
        else:
            self.labels = self._as_labels(groups, config.get_device())
            if n_groups is None:
                if self.labels.numel() == 0:
                    raise ValueError("SpotError: no labels and no n_groups")
                n_groups = int(self.labels.max()) + 1
        try:
            self.n_groups = int(n_groups)
        except (TypeError, ValueError) as e:
            raise ValueError(f"SpotError: n_groups must be an integer, got {n_groups!r}") from e
        if not 1 <= self.n_groups <= ops.SPOT_MAX_GROUPS:
            raise ValueError(f"SpotError: n_groups must lie in 1 .. {ops.SPOT_MAX_GROUPS}, got "
                             f"{n_groups!r}")
        self._grids = {}
        self.last_acc = None
        self.last_grid = None
        self.last_qbits = None
        _init_weights(self, "SpotError", weights)
        if self.weights is not None and self.labels is not None \
                and self.weights.numel() != self.labels.numel():
            raise ValueError(f"SpotError: {self.weights.numel()} weights for "
                             f"{self.labels.numel()} labels -- one of each per source ray")

    @staticmethod
    def _as_labels(groups, device):
        g = groups if isinstance(groups, torch.Tensor) else torch.as_tensor(np.asarray(groups))
        if g.dim() != 1 or g.dtype.is_floating_point or g.dtype.is_complex or g.dtype == torch.bool:
            raise ValueError("SpotError: groups must be integers of shape (N,), one label per "
                             f"source ray; got shape {tuple(g.shape)}, {g.dtype}")
        return g.detach().to(device=device, dtype=torch.int32).contiguous()

    def rows_for(self, dimension):
        """Field codes on a ``dimension``-D trace: the row of the ray block a geometry field is
        read from, ``2 * dimension + axis`` for a direction cosine."""
        if dimension == 3:
            return self.rows
        return _field_codes("SpotError", self.fields, dimension)

    def labels_of(self, src):
        """The int32 label buffer of the source set ``src`` on its device, one label per source
        ray: the tensor given (moved once; a new buffer re-captures a graph), or the callable's
        result, cached by the versions of the source's fields as ``GoalError.table`` is."""
        return _source_buffer(self, "labels", self.groups, self._as_labels, src, "SpotError",
                              "label")

    def weights_of(self, src):
        """The float64 weight buffer of the source set ``src`` on its device, one weight in [0, 1]
        per source ray (None without weights): the tensor given, or the callable's result,
        normalised and cached as the labels are."""
        if self.weights_given is None:
            return None
        return _source_buffer(self, "weights", self.weights_given,
                              lambda v, dev: _as_weights("SpotError", v, dev), src, "SpotError",
                              "weight", keep=True)

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
        ids = engine.last_trace["finished_id"]
        labels = self.labels_of(engine._trace_src)
        weights = self.weights_of(engine._trace_src)
        ids = ids.to(torch.int32).contiguous()
        if self.has_direction:
            dim, block = _geometry_block(engine, fin)
            return _SpotTerms.apply(block, self, labels, ids, weights, dim, tuple(codes))
        columns = torch.stack([fin[f] for f in self.fields], dim=0)
        return _SpotTerms.apply(columns, self, labels, ids, weights)


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
        err, grad, acc = erf.evaluate(rows, codes[0], codes[1] if len(codes) == 2 else -1, labels,
                                      perm=ids, dimension=dimension, weights=weights)
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


# the coupled errors: all finished rays of a step enter one evaluation (one process)
_COUPLED = (DensityError, SpotError, TransportError)


class SumError:
    """A weighted sum of error terms on ONE step: ``error = sum_k c_k * term_k``.  A real design
    is never one term: transport to find the target and density for the detail, a spot size with
    a magnification pinned by a goal, a near field and a far field at once.  Every term reads the
    same finished rays of one trace and the reverse sweep is linear in its seed, so the combined
    step is one trace, K error evaluations, one combination and one reverse sweep.

    ``terms``: 1 to 8 distinct instances of ``GoalError``, ``DensityError``, ``SpotError`` or
    ``TransportError``; a ``RowwiseError``, a nested ``SumError`` or the same object twice is a
    ValueError.  ``weights``: K finite values >= 0, default all ones, kept as the (K,) float64
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
    ``centroids()`` / ``last_rank2`` as when it runs alone.

    It is an ordinary ``error_function(engine)`` -- the generic path returns the (1,) tensor
    ``sum_k c_k * term_k(engine).sum()`` (``terms_k = numel``) under torch autograd, which serves
    2-D engines, fewer than 4,096 rays, ``deterministic=True`` and sources not traced in place.
    On a 3-D engine that traces its source in place the optimiser runs it on the fused,
    graph-replayed step under the conditions of a ``DensityError``: every term evaluates into a
    seed block of its own (a ``GoalError`` through tfrt_goal_error_columns, its goal row looked up
    through the trace's order inside the kernel), and one tfrt_error_combine launch writes the
    step's seed block and error.  One process."""

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
                raise ValueError("SumError: terms must be GoalError, DensityError, SpotError or "
                                 f"TransportError instances, got {type(t).__name__}")
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
        return (tuple((id(t), t.graph_key() if isinstance(t, _COUPLED)
                       else (id(t.goal), t.fields, t.rowwise)) for t in self.terms),
                self.weights.data_ptr(), self.reduce)

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


class _TermState:
    """What one term of a SumError owns in a step's state: its seed block and error triple, and
    the buffers its kind of error keeps (the names a ``_StepState`` has for a single error)."""
    __slots__ = ("g_fin", "err", "row_mask", "density_ws", "hq", "spot_ws", "acc", "transport_ws",
                 "rank2", "goal_ws")

    def __init__(self, g_fin, err, row_mask):
        for name in self.__slots__:
            setattr(self, name, None)
        self.g_fin, self.err, self.row_mask = g_fin, err, row_mask


class _RowFields:
    """Field mapping handed to a RowwiseError on the fixed-shape path: geometry = the rows of the
    in-place finished block, everything else = the source's own fields in the trace's order."""

    def __init__(self, geo, inherited):
        self._geo, self._inh = geo, inherited

    def __getitem__(self, key):
        if key in self._geo:
            return self._geo[key]
        return self._inh(key)

    def keys(self):
        return list(self._geo.keys())

    def __bool__(self):
        return True


class _HyperTable:
    """(n_parameters, 3) float64 {scale, clip, sgd_learning_rate} on the device -- (n_parameters, 5)
    with {momentum, nesterov} appended for the momentum rule, (n_parameters, 6) {scale, clip,
    adam_learning_rate, beta1, beta2, epsilon} for the Adam rule -- refreshed through a ring of
    pinned host buffers only when a value changes."""

    def __init__(self, n, device, slots=8, width=3):
        self.width = width
        self.dev = torch.zeros((n, width), dtype=torch.float64, device=device)
        self._host = [torch.zeros((n, width), dtype=torch.float64).pin_memory()
                      for _ in range(slots)]
        self._events = [None] * slots
        self._at = 0
        self._current = None

    def set(self, rows):
        if rows == self._current:
            return
        k = self._at
        self._at = (k + 1) % len(self._host)
        if self._events[k] is not None:
            self._events[k].synchronize()     # the copy that last used this buffer is long done
        self._host[k].copy_(torch.tensor(rows, dtype=torch.float64))
        self.dev.copy_(self._host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev.device))
        self._events[k] = ev
        self._current = rows



class _Override:
    """``with _override(sc, field=value, ...)``: sets fields of a scene struct for the span of the
    block and puts back the values they had, also when the block raises.  The struct is cached by
    the scene and shared with every other trace of it: whatever a step points it at (its gradient
    blocks, the block the trace's set-up launch clears, the in-place mode of this trace) must be
    gone when the step's launches are enqueued."""
    __slots__ = ("_sc", "_new", "_old")

    def __init__(self, sc, fields):
        self._sc, self._new = sc, fields

    def __enter__(self):
        sc = self._sc
        self._old = [(name, getattr(sc, name)) for name in self._new]
        for name, value in self._new.items():
            setattr(sc, name, value)
        return sc

    def __exit__(self, *exc):
        for name, value in self._old:
            setattr(self._sc, name, value)
        return False


def _override(sc, **fields):
    return _Override(sc, fields)


class _StepState:
    """The persistent buffers of one signature -- outputs, tape, seeds and gradient blocks of the
    trace -- and what the last enqueued step left for publishing its ray sets."""
    __slots__ = (
        "sig", "dim", "N", "M", "Ms", "Ma", "P", "dt", "flags", "capN",
        "full", "aux", "outs", "no_outs", "counts", "ints", "ws", "wsb",
        "err", "goal_ws", "gws", "fields",
        "g_fin", "g_fv", "g_n",                              # 3-D gradient blocks
        "g_prim", "g_seg", "g_arc", "g_index",               # 2-D: one block, views into it
        "rows", "row_face", "row_passes", "row_outs",        # a RowwiseError's fixed-shape columns
        "density_ws", "hq",                                  # a DensityError's workspace and histogram
        "spot_ws", "acc",                                    # a SpotError's workspace and group records
        "transport_ws", "rank2",                             # a TransportError's workspace and ranks
        "terms", "terms_key", "term_errs", "coeff",          # a SumError's per-term states
        "chain_ws", "inherited",                             # made on first use
        "sched", "sched_key", "sched_checked",               # the in-place trace's wavefront schedule
        "block", "stream", "perm", "inplace")                # of the last enqueued step

    def __init__(self, sig, block, dim, P, flags, fields, workspace_bytes):
        """What 2-D and 3-D share, for ray blocks of ``2 * dim`` rows.  ``fields``: the rows the
        error is read from; ``workspace_bytes``: (of the trace, of the error sum)."""
        for name in self.__slots__:
            setattr(self, name, None)
        n_rows, dev = 2 * dim, block.device
        N = block.shape[1]
        capN = max(N, 1)
        self.sig, self.dim, self.N, self.P, self.flags, self.capN = sig, dim, N, P, flags, capN
        self.dt = ops._DT[block.dtype]
        ints = ops._IntPool(dev, True, _lib.COUNTS_PER_PASS * (P + 1), flags, capN, P)
        caps = {"finished": capN, "active": capN * max(P, 1), "stopped": capN, "dead": capN}
        full, aux, outs = {}, {"counts": ints.counts}, {}
        for name, flag in _CLASS_FLAGS:
            if flags & flag:
                rays = torch.empty((n_rows, caps[name]), dtype=block.dtype, device=dev)
                ids, faces = ints.take(caps[name]), ints.take(caps[name])
                full[name], aux[name + "_id"], aux[name + "_face"] = rays, ids, faces
                outs[name] = ops._ray_out(rays, ids, faces)
            else:
                aux[name + "_id"] = aux[name + "_face"] = None
                outs[name] = ops._ray_out(None, None, None)
        # the rays still active after the last pass are not copied out by a fused step
        aux["unfinished"] = torch.empty((n_rows, 0), dtype=block.dtype, device=dev)
        aux["unfinished_id"] = torch.empty(0, dtype=torch.int32, device=dev)
        self.full, self.aux, self.outs = full, aux, outs
        self.no_outs = {name: ops._ray_out(None, None, None) for name, _ in _CLASS_FLAGS}
        self.counts, self.ints = ints.counts, ints
        wsb, gws = workspace_bytes
        self.ws, self.wsb = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev), wsb
        self.err = torch.zeros(3, dtype=torch.float64, device=dev)
        self.goal_ws, self.gws = torch.zeros(max(gws, 1), dtype=torch.uint8, device=dev), gws
        self.fields = (ctypes.c_int32 * n_rows)(*(list(fields) + [0] * n_rows)[:n_rows])

    def __getitem__(self, name):
        """``state["N"]``: the fields by name, as bench.py and the tests read them."""
        return getattr(self, name)


class FusedStep:
    """Runs ``SGD_Optimizer.single_step`` for a ``GoalError`` or a ``RowwiseError`` as a fixed
    launch sequence, on 3-D engines and on 2-D ones (one process), and for a ``DensityError``, a
    ``SpotError``, a ``TransportError`` or a ``SumError`` of them on 3-D engines; see the module
    docstring.
    One instance per optimizer."""

    # coherent rays: error, gradient seed and reverse sweep as ONE launch (tfrt_trace3d_backward_goal);
    # False: tfrt_goal_error3d + tfrt_trace3d_backward (what a trace in natural order always runs)
    fold_backward = True
    folded_backward = False           # what the last enqueued step did
    in_place = False                  # ... its trace ran all passes in one launch, rays in place
    face_sums = False                 # ... its sweep left four sums per face (tfrt_scene3d.face_sums)
    # Several ranks: capture the RCCL all-reduce inside the step's graph (one graph per step) instead
    # of calling it eagerly between two graphs.  "auto": only with a one-rank group -- the form has
    # been replayed with a one-rank RCCL group (tests/test_gpu_zz_rccl.py), never yet with several
    # RCCL ranks (no multi-GPU box in this round's pool), and a capture that goes wrong ACROSS ranks
    # does not raise, it hangs; the split form is plain eager torch.distributed and costs ~10 us
    # per step.  True: always try (bench.py --collective-in-graph).
    capture_collective = "auto"
    collective_in_graph = False
    # engine.wave_schedule == "auto": a schedule is made when the step has more groups of 64 rays
    # than this (None: the wavefronts the chip holds of k_trace_inplace, 4 SIMDs x 5 per CU -- a
    # launch that is resident all at once has no order to gain from)
    schedule_min_waves = None

    def __init__(self, optimizer, graph="auto", graph_warmup=3):
        self.opt = optimizer
        self.graph_mode = graph           # "auto" / True: capture after the warm-up; False: never
        self.graph_warmup = int(graph_warmup)
        self._state = None                # _StepState of the current signature
        self._graphs = None               # (signature, graph A, graph B or None, grads)
        self._stream = None               # the side stream steps are captured on
        self._last_sig = None             # signature of the last eager step
        self._eager_steps = 0
        self.tests_total = None           # device int64: ray-face tests of all fused steps
        self.steps = 0
        self.graph_replays = 0
        self.capture_error = None
        self.collective_capture_error = None
        self.untapped = False             # a parameter reached the faces without boundaries.tap
        self._tap_checks = 0              # eager steps that compared leaf and alias gradients
        self._goal_perm = None            # the goal rows in the trace's (coherent) order, keyed
        self._goal_pending = None         # (error sum left to the update's launch, its stream)
        self._hyper = self._hyper_apply = None    # _HyperTable of the update / of an accumulated one
        self._err_view = None             # {sum, terms, mean} of the last step
        # several ranks: [gradients, error sums] as the collective reduces them
        self._flat_buf = self._flat = self._err_sink = None
        self._flat_views = False

    # ------------------------------------------------------------------------ eligibility
    @staticmethod
    def eligible(optimizer, args, kwargs):
        eng = optimizer.engine
        erf = optimizer.error_function
        if not isinstance(erf, (GoalError, RowwiseError, SumError) + _COUPLED) or args or kwargs:
            return False
        if isinstance(erf, SumError) and eng.dimension != 3:
            return False            # (a sum of terms takes the generic path on a 2-D engine)
        if (isinstance(erf, (RowwiseError, SumError) + _COUPLED) and eng.dimension == 3
                and not FusedStep.rowwise_ready(eng)):
            return False
        if isinstance(erf, (SumError,) + _COUPLED) and tdist.is_distributed():
            return False            # (the histogram / the centroids / the ranks couple the rays: one process)
        if not bool(eng.optical_system):
            return False
        if eng.dimension == 2 and not FusedStep.eligible2d(optimizer):
            return False
        try:
            eng._reaction()
        except RuntimeError:
            return False
        return all(isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float64
                   and p.is_contiguous() for p in optimizer.parameters)

    @staticmethod
    def eligible2d(optimizer):
        """A 2-D engine takes the fused step with a GoalError over fields its rays have or with a
        RowwiseError, in one process without ray shards, and with the projection in the kernels
        (no operation with a main() of its own); everything else keeps the generic path."""
        eng, erf = optimizer.engine, optimizer.error_function
        if not isinstance(erf, (GoalError, RowwiseError)) or tdist.is_distributed() \
                or eng._custom_ops():
            return False
        if eng.ray_shard not in (None, "auto"):
            return False
        if isinstance(erf, RowwiseError):
            return True
        try:
            erf.rows_for(2)
        except ValueError:
            return False
        return True

    @staticmethod
    def rowwise_ready(eng):
        """A RowwiseError runs on the fixed-shape path once the engine traces this source in place
        (its rays are ordered and an earlier trace -- of the generic path -- left no wavefront
        over); until then, and whenever that stops holding, the step takes the generic path."""
        return (eng.in_place is not False and eng.coherent is not False and not eng.deterministic
                and getattr(eng, "_visit_all_key", None) is not None
                and not getattr(eng, "_rowwise_off", False))

    # -------------------------------------------------------------------------- buffers
    def _buffers(self, block, fv, P, flags, index=False):
        """The state of a 3-D trace for this (N, M, P, dtype, flags), made when the signature
        changes; ``index``: with the (2, M) block of d error / d (n_in, n_out) too."""
        N, M = block.shape[1], fv.shape[0]
        dt = ops._DT[block.dtype]
        # (the error function's rows are baked into `fields` and into which rows of g_fin are
        # ever written: another GoalError gets fresh, zeroed buffers)
        rows = self.opt.error_function.rows
        sig = (N, M, P, dt, flags, str(block.device), tuple(rows), bool(index))
        st = self._state
        if st is None or st.sig != sig:
            L = _lib.lib()
            st = _StepState(sig, block, 3, P, flags, rows,
                            (L.tfrt_trace3d_workspace_bytes(N, M, P, dt),
                             L.tfrt_goal_error3d_workspace_bytes(max(N, 1))))
            dev = block.device
            st.M = M
            st.g_fin = torch.zeros((6, st.capN), dtype=torch.float64, device=dev)
            st.g_fv = torch.zeros((max(M, 1), 9), dtype=torch.float64, device=dev)
            if index:
                st.g_n = torch.zeros((2, max(M, 1)), dtype=torch.float64, device=dev)
            self._install(st)
        st.block, st.stream = block, ops._stream(block)
        return st

    def _buffers2d(self, block, det, P, flags, rows, index):
        """The state of a 2-D trace over the (detached) merged segments and arcs ``det`` for this
        (N, Ms, Ma, P, dtype, flags, fields).  ``rows``: the ray-block rows of a GoalError's
        fields, None for a RowwiseError (which gets its fixed-shape columns); ``index``: which of
        (seg_n_in, seg_n_out, arc_n_in, arc_n_out) take a gradient."""
        N = block.shape[1]
        Ms, Ma = (0 if g is None else g.shape[0] for g in det)
        dt = ops._DT[block.dtype]
        index = tuple(i is not None for i in index)
        sig = (2, N, Ms, Ma, P, dt, flags, str(block.device), tuple(rows or ()), rows is None,
               index)
        st = self._state
        if st is None or st.sig != sig:
            L = _lib.lib()
            st = _StepState(sig, block, 2, P, flags, rows or (),
                            (L.tfrt_trace2d_workspace_bytes(N, Ms, Ma, P, dt),
                             L.tfrt_trace2d_backward_goal_workspace_bytes(N)))
            dev = block.device
            st.Ms, st.Ma = Ms, Ma
            # (segment and arc gradients in one block, the index gradients asked for behind them:
            # one clearing launch per step)
            n_index = 2 * (Ms + Ma) if any(index) else 0
            at = 4 * Ms + 5 * Ma
            g = st.g_prim = torch.zeros(max(at + n_index, 1), dtype=torch.float64, device=dev)
            st.g_seg, st.g_arc = g[:4 * Ms].view(Ms, 4), g[4 * Ms:at].view(Ma, 5)
            st.g_index = [None] * 4
            if n_index:
                cuts = (at, at + Ms, at + 2 * Ms, at + 2 * Ms + Ma, at + n_index)
                st.g_index = [g[a:b] if want else None
                              for a, b, want in zip(cuts, cuts[1:], index)]
            if rows is None:
                # (every column is written by each step's tfrt_trace2d_rows: no clearing)
                st.rows = torch.empty((4, st.capN), dtype=block.dtype, device=dev)
                st.row_face = torch.empty(st.capN, dtype=torch.int32, device=dev)
            self._install(st)
        st.block, st.stream = block, ops._stream(block)
        return st

    def _install(self, st):
        """New buffers: whatever was captured wrote into the old ones."""
        self._state = st
        self._graphs = None
        dev = st.err.device
        if self.tests_total is None or self.tests_total.device != dev:
            self.tests_total = torch.zeros(1, dtype=torch.int64, device=dev)

    # ------------------------------------------------------- the C-ABI entries called twice
    def _lengths(self):
        eng = self.opt.engine
        return float(eng.new_ray_length), float(eng.dead_ray_length or 0.0)

    def _trace_forward(self, st, sc, outs):
        """tfrt_trace3d_forward / tfrt_trace2d_forward (one argument list) of the step's rays into
        the ray sets ``outs``; counts and tape stay on the device."""
        name = "tfrt_trace3d_forward" if st.dim == 3 else "tfrt_trace2d_forward"
        block = st.block
        check(getattr(_lib.lib(), name)(
            ops._p(block), block.shape[1], st.N, ctypes.byref(sc), *self._lengths(), st.P, st.dt,
            st.flags, ctypes.byref(outs["finished"]), ctypes.byref(outs["active"]),
            ctypes.byref(outs["stopped"]), ctypes.byref(outs["dead"]),
            None, None,      # (the rays still active after the last pass are not copied out)
            ops._p(st.counts), ops._p(st.ws), st.wsb, st.stream), name)

    def _trace3d_backward(self, st, sc, seeds, capacity):
        """tfrt_trace3d_backward from the finished rays' gradient ``seeds`` (6, capacity) into the
        face-gradient block (and the index block the struct points at)."""
        block = st.block
        check(_lib.lib().tfrt_trace3d_backward(
            ops._p(block), block.shape[1], st.N, ctypes.byref(sc), *self._lengths(), st.P, st.dt,
            ops._p(seeds), capacity, None, 0, None, 0, None, 0, ops._p(st.g_fv), None,
            ops._p(st.counts), ops._p(st.ws), st.wsb, st.stream), "tfrt_trace3d_backward")

    @staticmethod
    def _goal_finish(pending, stream):
        """The second stage of an error sum (the launch tfrt_goal_error3d would have made)."""
        check(_lib.lib().tfrt_goal_finish(ctypes.byref(pending), stream), "tfrt_goal_finish")

    # ---------------------------------------------------------------- the launch sequence
    def _enqueue_gradient(self):
        """update -> trace -> error -> reverse sweep -> parameter gradients.  Returns
        (grads, error tensor {sum, terms, mean}).  Nothing here waits for the device."""
        opt, eng = self.opt, self.opt.engine
        eng.clear_ray_history()
        from . import boundaries
        with boundaries.collect_taps() as tap_log:
            eng.optical_system.update()
        src = eng._source_set()
        if not src:
            raise RuntimeError("FusedStep: the optical system has no source rays")
        inputs = eng._trace_inputs(src)
        P, flags = int(opt.trace_depth), eng._flags() | _lib.COMPILE_FINISHED
        rowwise = isinstance(opt.error_function, (RowwiseError, SumError) + _COUPLED)
        if eng.dimension == 2:
            body = self._rowwise2d if rowwise else self._goal2d
        else:
            body = self._rowwise3d if rowwise else self._goal3d
        grads, st = body(src, inputs, tap_log, P, flags)
        self._publish_lazily(st, src)
        return ([None] * len(opt.parameters) if grads is None else grads), st.err

    # ------------------------------------------------------------------------------ 3-D
    def _goal3d(self, src, inputs, tap_log, P, flags):
        """tfrt_trace3d_forward -> error + gradient seed -> reverse sweep; coherent rays: the last
        two as one launch, and from 64 rays on the trace in place."""
        erf = self.opt.error_function
        block, scene, fv = inputs
        perm = self.opt.engine._trace_perm
        goal, goal_by_ray = self._goal_rows(erf, src, perm)
        fvc = self._faces(fv)
        index = self._index3d(scene, fvc)
        st = self._buffers(block, fvc, P, flags, any(n is not None for n in index))
        sink = self._err_sink
        if tdist.is_distributed() and sink is not None and st.err.data_ptr() != sink.data_ptr():
            st.err = sink               # (the error sums land in the collective's buffer)
        sc = scene.struct(fvc)
        # (the reverse sweep runs for the faces or the indices; it is given the face-gradient block
        # either way: the in-place chain sums its face terms per wavefront into it)
        need_back = bool((fv.requires_grad or st.g_n is not None) and st.M > 0)
        # coherent rays: error, gradient seed and the whole reverse sweep are ONE launch
        # (tfrt_trace3d_backward_goal); the face-gradient block it accumulates into is cleared by
        # the trace's set-up launch
        folded = bool(self.fold_backward and need_back and sc.coherent_rays
                      and not sc.deterministic and 1 <= P <= 8)
        # all passes in one launch, rays in place (tfrt_scene3d.in_place): the folded reverse sweep
        # needs no ray set, so none is compacted here -- _publish_lazily does it if somebody asks
        inplace = bool(folded and sc.in_place and st.N >= 64 and P >= 1)
        self.folded_backward, self.in_place = folded, inplace
        st.perm = perm
        st.inplace = (block, self._lengths()[1]) if inplace else None
        # (the folded sweep is one of the two chain kernels, which write the four-sum form)
        four = self.face_sums = self._four_sums(fv, sc, folded)
        clear = {"clear_buffer": st.g_fv.data_ptr(), "clear_count": st.g_fv.numel()} if folded \
            else {}
        sched = self._wave_schedule(st) if inplace else None
        # (in_place, wave_schedule, face_sums: the reverse sweep is given the same values as the
        # forward)
        with _override(sc, in_place=1 if inplace else 0, face_sums=1 if four else 0,
                       wave_schedule=None if sched is None else sched.data_ptr()):
            with _override(sc, **clear):
                self._trace_forward(st, sc, st.no_outs if inplace else st.outs)
            with self._index_grads3d(sc, st, need_back):
                self._goal_backward3d(st, sc, (goal, goal_by_ray), folded, need_back)
        if inplace:
            self._make_wave_schedule(st, perm)
        if not need_back:
            return None, st
        with ops.FaceSums() if four else contextlib.nullcontext():
            return self._parameter_gradients(*self._outs3d(fv, st, index), tap_log), st

    @staticmethod
    def _four_sums(fv, sc, chain_sweep):
        """Whether this step's reverse sweep leaves the faces' four sums (tfrt_scene3d.face_sums)
        instead of their nine vertex gradients: the sweep is one of the two chain kernels, not
        ``deterministic``, and the merged faces come straight from the parametric update whose
        gather expands the sums -- a vertex-parametrised boundary, a custom ``_update`` or
        anything else between the update and the faces reads a true (M, 9) gradient."""
        return bool(chain_sweep and not sc.deterministic and sc.coherent_rays
                    and fv.requires_grad and ops.faces_from_param_update(fv))

    def _wave_schedule(self, st):
        """The wavefront schedule this in-place step runs with (engine.wave_schedule), or None:
        the caller's tensor, checked once per version, or the one _make_wave_schedule left."""
        given = self.opt.engine.wave_schedule
        if isinstance(given, torch.Tensor):
            key = (id(given), given._version)
            if st.sched_checked != key:
                if given.device != st.block.device:
                    raise RuntimeError("FusedStep: wave_schedule must be on the rays' device")
                ops.check_wave_schedule(given, st.N)
                st.sched_checked = key
            return given
        if given != "auto":
            if given is not False:
                raise ValueError("OpticalEngine.wave_schedule must be 'auto', False or an int32 "
                                 f"tensor, got {given!r}")
            return None
        return st.sched if st.sched_key is not None else None

    def _make_wave_schedule(self, st, perm):
        """engine.wave_schedule == "auto": after the first in-place step of these rays in this
        order over this scene (what the key holds; N, M and P are the state's own), one launch
        behind the trace that has just left its work rows turns them into the schedule of the
        steps that follow.  The buffer is persistent and read by address: a later build -- another
        order, another topology -- needs no new capture.  Never inside a capture, never per step:
        a source re-drawn in place keeps its wavefronts' places on the key grid, and a schedule
        gone stale costs time, not correctness."""
        eng = self.opt.engine
        if not isinstance(eng.wave_schedule, str) or eng.wave_schedule != "auto":
            return
        G = ops.wave_groups(st.N)
        least = self.schedule_min_waves
        if least is None:
            least = 20 * torch.cuda.get_device_properties(st.block.device).multi_processor_count
        key = (id(perm), eng.optical_system.scene_signature())
        if G <= least or st.sched_key == key or torch.cuda.is_current_stream_capturing():
            return
        if st.sched is None:
            st.sched = torch.empty(G, dtype=torch.int32, device=st.block.device)
        ops.wave_schedule(st.N, st.M, st.P, st.block.dtype, st.ws, out=st.sched)
        st.sched_key = key

    def _goal_rows(self, erf, src, perm):
        """The goal table of the step's rays and whether it is (N, fields) rows instead of
        (fields, N) columns."""
        if perm is None:
            return erf.table(src), False
        # coherent order: the trace runs over src[perm] (its ray ids are positions in that
        # order), so the goal rows go along; the ray sets are restored when somebody asks
        # (keyed by the goal TABLE, not by the geometry the order was made from: a goal may
        # read any source field, and erf.table() is itself cached by the versions of all of
        # them -- a field changed in place re-evaluates it and, through the key, re-gathers)
        rowwise = bool(erf.rowwise and callable(erf.goal) and hasattr(src, "permuted"))
        base = None if rowwise else erf.table(src)
        gkey = (id(erf), src.cache_key if rowwise else id(base), id(perm), rowwise)
        cached = self._goal_perm
        if cached is None or cached[0] != gkey:
            if rowwise:
                # made in the trace's order, left in the layout the callable returns
                rows, by_ray = erf.table(src.permuted(perm), by_ray=True), True
            else:
                rows, by_ray = ops.gather_rows(base, perm), False
            cached = self._goal_perm = (gkey, rows, perm, by_ray, base)   # (holds `base`: its id stays its own)
        return cached[1], cached[3]

    def _goal_backward3d(self, st, sc, goal_rows, folded, need_back):
        """Error, gradient seed and reverse sweep of _goal3d.  One rank: nothing on the device
        waits for the error sum, so its second stage is left to the parameter update's launch
        (_enqueue_apply); with several ranks the sum goes into the collective and is finished
        here."""
        L = _lib.lib()
        goal, by_ray = goal_rows
        n_fields = len(self.opt.error_function.rows)
        strides = (1, goal.shape[1]) if by_ray else (goal.shape[1], 1)
        block, stream = st.block, st.stream
        several = tdist.is_distributed()
        pending = _lib.GoalPending()
        self._goal_pending = None
        if folded:
            if st.chain_ws is None:
                cwb = L.tfrt_trace3d_backward_goal_workspace_bytes(st.N)
                st.chain_ws = (torch.zeros(max(cwb, 1), dtype=torch.uint8, device=block.device), cwb)
            check(L.tfrt_trace3d_backward_goal(
                ops._p(block), block.shape[1], st.N, ctypes.byref(sc), *self._lengths(), st.P,
                st.dt, ctypes.byref(st.outs["finished"]), st.fields, n_fields, ops._p(goal),
                *strides, ops._p(st.err), ops._p(self.tests_total), ops._p(st.chain_ws[0]),
                st.chain_ws[1], ctypes.byref(pending), None, 0, None, 0, None, 0,
                ops._p(st.g_fv), None, ops._p(st.counts), ops._p(st.ws), st.wsb, stream),
                "tfrt_trace3d_backward_goal")
            if several:
                self._goal_finish(pending, stream)
        else:
            # error + gradient seed; the same launch clears the face-gradient block the reverse
            # sweep accumulates into and adds the trace's test count to the running total
            goal_args = (
                ops._p(st.full["finished"]), st.capN, ops._p(st.aux["finished_id"]), st.dt,
                ops._p(st.counts), st.P, st.fields, n_fields, ops._p(goal), *strides,
                ops._p(st.g_fin), ops._p(st.err), ops._p(st.g_fv) if need_back else None,
                st.g_fv.numel() if need_back else 0, ops._p(self.tests_total),
                ops._p(st.goal_ws), st.gws)
            if several:
                check(L.tfrt_goal_error3d(*goal_args, stream), "tfrt_goal_error3d")
            else:
                check(L.tfrt_goal_error3d_deferred(*goal_args, ctypes.byref(pending), stream),
                      "tfrt_goal_error3d_deferred")
        if not several:
            self._goal_pending = (pending, stream)
        if need_back and not folded:
            self._trace3d_backward(st, sc, st.g_fin, st.capN)

    @staticmethod
    def _faces(fv):
        fvc = fv.detach()
        if fvc.dtype != torch.float64 or not fvc.is_contiguous():
            raise RuntimeError("FusedStep: merged faces must be contiguous float64")
        return fvc

    @staticmethod
    def _index3d(scene, fvc):
        """(n_in, n_out) of "value" mode when they take a gradient (the merged columns update()
        made, Scene3DArgs.n_in_arg / n_out_arg), None where not."""
        if scene.n_table is not None or fvc.shape[0] == 0:
            return (None, None)
        return tuple(n if isinstance(n, torch.Tensor) and n.requires_grad else None
                     for n in (scene.n_in_arg, scene.n_out_arg))

    @staticmethod
    def _outs3d(fv, st, index):
        """What the parameter gradients are taken from: the faces and the indices that take one."""
        outs, g_outs = ([fv], [st.g_fv]) if fv.requires_grad else ([], [])
        for k, n in enumerate(index):
            if n is not None:
                outs.append(n)
                g_outs.append(st.g_n[k, :n.shape[0]])
        return outs, g_outs

    @staticmethod
    def _index_grads3d(sc, st, on):
        """Scope in which tfrt_scene3d.grad_n_in / grad_n_out point at the step's index block
        (cleared here, in the captured sequence)."""
        g = st.g_n
        if not on or g is None:
            return _override(sc)
        g.zero_()
        return _override(sc, grad_n_in=g[0].data_ptr(), grad_n_out=g[1].data_ptr())

    def _rowwise3d(self, src, inputs, tap_log, P, flags):
        """In-place trace with the finished rows at the rays' own columns -> ``erf.fn`` on
        fixed-shape tensors + its autograd (torch), or a DensityError's / a SpotError's / a
        TransportError's launches (tfrt_density_error, tfrt_spot_error, tfrt_transport_error), or
        a SumError's terms and tfrt_error_combine -> reverse sweep.  No ray count is read;
        everything is capturable."""
        eng = self.opt.engine
        block, scene, fv = inputs
        perm = eng._trace_perm
        fvc = self._faces(fv)
        index = self._index3d(scene, fvc)
        st = self._buffers(block, fvc, P, flags, any(n is not None for n in index))
        N, M, dev = st.N, st.M, block.device
        sc = scene.struct(fvc)
        if not (scene.in_place and sc.coherent_rays
                and _lib.lib().tfrt_trace3d_in_place(ctypes.byref(sc), N, P) == 1):
            eng._rowwise_off = True      # (this source is not traced in place: generic path)
            raise _NotInPlace()
        if st.rows is None:
            st.rows = torch.zeros((6, st.capN), dtype=block.dtype, device=dev)
            st.row_face = torch.full((st.capN,), -1, dtype=torch.int32, device=dev)
            st.row_passes = torch.zeros(st.capN, dtype=torch.int32, device=dev)
            st.row_outs = dict(st.no_outs,
                               finished=ops._ray_out(st.rows, st.row_passes, st.row_face))
        need_back = bool((fv.requires_grad or st.g_n is not None) and M > 0)
        self.folded_backward, self.in_place = False, True
        self._goal_pending = None
        st.perm, st.inplace = perm, (block, self._lengths()[1])
        # (an in-place tape is swept by k_backward_chain, which writes the four-sum form)
        four = self.face_sums = self._four_sums(fv, sc, need_back)
        clear = {"clear_buffer": st.g_fv.data_ptr(), "clear_count": st.g_fv.numel()} if need_back \
            else {}
        grads = None
        # (in_place == 2: the finished rows at the rays' own columns; the reverse sweep is given
        # the same values as the forward)
        with _override(sc, in_place=2, face_sums=1 if four else 0, **clear):
            self._trace_forward(st, sc, st.row_outs)
            erf = self.opt.error_function
            if isinstance(erf, (SumError,) + _COUPLED):
                if isinstance(erf, SumError):
                    g64 = self._sum_seeds3d(st, src, perm, erf, need_back)
                else:
                    g64 = self._term_seeds3d(st, src, perm, erf, st)
                with torch.no_grad():
                    self.tests_total += st.row_passes[:st.N].sum() * st.M
                if not need_back:
                    g64 = None
            else:
                g64 = self._rowwise_seeds3d(st, src, perm, need_back)
            if g64 is not None:
                with self._index_grads3d(sc, st, True):
                    self._trace3d_backward(st, sc, g64, g64.shape[1])
                with ops.FaceSums() if four else contextlib.nullcontext():
                    grads = self._parameter_gradients(*self._outs3d(fv, st, index), tap_log)
        return grads, st

    def _term_seeds3d(self, st, src, perm, erf, hold):
        """The launches of one built-in error ``erf`` on the fixed-shape columns of ``st``, into
        the seed block, the error triple and the buffers of ``hold``: the step's state itself for
        a single error, a ``_TermState`` for a term of a SumError.  Returns the seed block."""
        if isinstance(erf, DensityError):
            return self._density_seeds3d(st, src, perm, erf, hold)
        if isinstance(erf, TransportError):
            return self._transport_seeds3d(st, erf, hold)
        if isinstance(erf, SpotError):
            return self._spot_seeds3d(st, src, perm, erf, hold)
        return self._goal_seeds3d(st, src, perm, erf, hold)

    def _sum_seeds3d(self, st, src, perm, erf, need_back):
        """A SumError on the fixed-shape columns: every term evaluates into a private, once-zeroed
        (6, capN) seed block and its own triple -- coupled terms through their ``evaluate`` with
        buffers of their own, GoalError terms through tfrt_goal_error_columns --, then ONE
        tfrt_error_combine writes the step's seed block ``st.g_fin`` (all six rows, every column)
        and ``st.err``; without a reverse sweep only the errors are combined.  Nothing is read
        back: the coefficients of ``reduce="mean"`` come from the triples on the device."""
        dev = st.rows.device
        key = tuple(id(t) for t in erf.terms)
        if st.terms is None or st.terms_key != key:
            K = len(erf.terms)
            st.term_errs = torch.zeros((K, 3), dtype=torch.float64, device=dev)
            st.coeff = torch.zeros(K, dtype=torch.float64, device=dev)
            st.terms = []
            for k, t in enumerate(erf.terms):
                mask = 0x3f if getattr(t, "has_direction", False) \
                    else sum(1 << r for r in t.rows)
                st.terms.append(_TermState(
                    torch.zeros((6, st.capN), dtype=torch.float64, device=dev), st.term_errs[k],
                    mask))
            st.terms_key = key
            self._graphs = None
        for t, hold in zip(erf.terms, st.terms):
            self._term_seeds3d(st, src, perm, t, hold)
        ops.error_combine(
            [(h.g_fin if need_back else None, h.row_mask, h.err) for h in st.terms],
            erf.weights_on(dev), erf.reduce, n=st.N, n_rows=6, out=st.g_fin, err=st.err,
            coeff=st.coeff)
        erf.last_errors, erf.last_coefficients = st.term_errs, st.coeff
        return st.g_fin

    def _goal_seeds3d(self, st, src, perm, erf, hold):
        """A GoalError term on the fixed-shape columns: tfrt_goal_error_columns reads ``st.rows``,
        the mask ``st.row_face`` and the goal table in the source's order, which it looks up
        through the trace's order ``perm`` itself (no permuted copy that could go stale when a
        source is re-drawn and re-ordered inside the graph), and writes the fields' rows of the
        term's seed block for every column."""
        if hold.goal_ws is None:
            wsb = _lib.lib().tfrt_goal_error_columns_workspace_bytes(st.N)
            hold.goal_ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=st.rows.device)
        # (the table in the layout the goal has: no transposed copy per step)
        ops.goal_error_columns(st.rows[:, :st.N], erf.rows, erf.table(src, by_ray=True),
                               mask=st.row_face, perm=perm, by_ray=True, grad=hold.g_fin,
                               err=hold.err, workspace=hold.goal_ws)
        return hold.g_fin

    def _density_seeds3d(self, st, src, perm, erf, hold):
        """A DensityError on the fixed-shape columns: tfrt_density_error reads ``st.rows`` and the
        mask ``st.row_face`` -- with weights also the source's weight buffer through the trace's
        order ``perm``, inside the kernel, as a SpotError's labels -- and writes its rows of the persistent seed block for every column --
        the two rows of position fields (the other rows were zeroed when the state was made, and
        the field codes are part of its signature), all six with a direction field --, the error
        into ``hold.err`` and the histogram into ``hold.hq``.  Returns the (6, capN) seed block."""
        dev = st.rows.device
        goal = erf.goal_on(dev)
        if hold.hq is None or hold.hq.shape != goal.shape:
            nx, ny = goal.shape[-1], (goal.shape[0] if goal.dim() == 2 else 1)
            wsb = _lib.lib().tfrt_density_error_workspace_bytes(st.N, nx, ny)
            hold.density_ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
            hold.hq = torch.zeros(goal.shape, dtype=torch.int64, device=dev)
        rows = erf.rows
        erf.evaluate(st.rows[:, :st.N], rows[0], rows[1] if len(rows) == 2 else -1,
                     mask=st.row_face, dimension=3, weights=erf.weights_of(src), perm=perm,
                     grad=hold.g_fin, err=hold.err, hq=hold.hq, workspace=hold.density_ws)
        return hold.g_fin

    def _transport_seeds3d(self, st, erf, hold):
        """A TransportError on the fixed-shape columns: tfrt_transport_error reads ``st.rows`` and
        the mask ``st.row_face`` and writes its two rows of the persistent seed block for every
        column (the other rows were zeroed when the state was made), the error into ``hold.err``
        and the ranks into ``hold.rank2``; n_valid never leaves the device.  Returns the
        (6, capN) seed block."""
        dev = st.rows.device
        K = erf.n_directions
        if hold.rank2 is None or tuple(hold.rank2.shape) != (K, st.N):
            wsb = _lib.lib().tfrt_transport_error_workspace_bytes(st.N, K)
            hold.transport_ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
            hold.rank2 = torch.zeros((K, st.N), dtype=torch.int32, device=dev)
        rows = erf.rows
        erf.evaluate(st.rows[:, :st.N], rows[0], rows[1] if len(rows) == 2 else -1,
                     mask=st.row_face, dimension=3, grad=hold.g_fin, err=hold.err,
                     rank2=hold.rank2, workspace=hold.transport_ws)
        return hold.g_fin

    def _spot_seeds3d(self, st, src, perm, erf, hold):
        """A SpotError on the fixed-shape columns: tfrt_spot_error reads ``st.rows``, the mask
        ``st.row_face``, the source's label buffer and the trace's order ``perm`` -- the kernel
        looks a column's label up itself, so no permuted copy can go stale when a source is
        re-drawn and re-ordered inside the graph -- and writes its rows of the persistent seed
        block for every column (two for position fields, the others zeroed when the state was
        made; all six with a direction field), the error into ``hold.err`` and the group records
        into ``hold.acc`` ((G, 4), with weights -- looked up like the labels -- (G, 8)).  Returns
        the (6, capN) seed block."""
        dev = st.rows.device
        labels = erf.labels_of(src)
        weights = erf.weights_of(src)
        record = 4 if weights is None else 8
        if hold.acc is None or tuple(hold.acc.shape) != (erf.n_groups, record):
            wsb = _lib.lib().tfrt_spot_error_workspace_bytes(st.N, erf.n_groups)
            hold.spot_ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
            hold.acc = torch.zeros((erf.n_groups, record), dtype=torch.int64, device=dev)
        rows = erf.rows
        erf.evaluate(st.rows[:, :st.N], rows[0], rows[1] if len(rows) == 2 else -1, labels,
                     mask=st.row_face, perm=perm, dimension=3, weights=weights, grad=hold.g_fin,
                     err=hold.err, acc=hold.acc, workspace=hold.spot_ws)
        return hold.g_fin

    def _rowwise_seeds3d(self, st, src, perm, need_back):
        """A RowwiseError on the fixed-shape columns: ``fn`` and its autograd (torch), the masked
        error sum into ``st.err``.  Returns the columns' float64 gradient, None without one."""
        N, M, dev = st.N, st.M, st.rows.device
        if perm is None:
            inherited = src.__getitem__
        else:
            if st.inherited is None:
                st.inherited = {}
            cache = st.inherited

            def inherited(key):
                v = src[key]
                hit = cache.get(key)
                if hit is None or hit[0] is not v or hit[1] is not perm or hit[2] != v._version:
                    hit = cache[key] = (v, perm, v._version, v.index_select(0, perm.long()))
                return hit[3]
        leaf, e = self._rowwise_terms(st, _GEO3, inherited)
        mask = st.row_face[:N] >= 0
        err_sum = torch.where(mask.unsqueeze(1), e.double(), torch.zeros((), dtype=torch.float64,
                                                                       device=dev)).sum()
        terms = mask.sum().double() * e.shape[1]
        with torch.no_grad():
            st.err[0] = err_sum.detach()
            st.err[1] = terms
            st.err[2] = torch.where(terms > 0, err_sum.detach() / torch.clamp(terms, min=1.0),
                                    torch.full_like(terms, float("nan")))
            self.tests_total += st.row_passes[:N].sum() * M
        if need_back and err_sum.requires_grad:
            with torch.autograd.set_multithreading_enabled(False):
                g_rows, = torch.autograd.grad(err_sum, [leaf])
            return g_rows.to(torch.float64).contiguous()
        return None

    def _rowwise_terms(self, st, names, inherited):
        """The user's error function, row by row on every source ray's column: ``st.rows`` (a leaf
        of its own autograd graph) under the geometry ``names``, every other field through
        ``inherited``.  Returns the leaf and the error terms as (N, k)."""
        leaf = st.rows.detach().requires_grad_(True)
        geo = {name: leaf[k] for k, name in enumerate(names)}
        e = self.opt.error_function.fn(_RowFields(geo, inherited))
        if e.dim() == 1:
            e = e.reshape(-1, 1)
        # (3-D has always taken terms of more than two dimensions -- it sums them all and counts
        # e.shape[1] per ray --; 2-D hands the terms to a kernel as a matrix and refuses them.
        # Both behaviours are kept.)
        if e.shape[0] != st.N or (st.dim == 2 and e.dim() != 2):
            raise RuntimeError(f"RowwiseError: fn returned {tuple(e.shape)}, expected one row "
                               f"per ray ({st.N})")
        return leaf, e

    def _parameter_gradients(self, outs, g_outs, tap_log):
        """d error / d parameters from d error / d geometry (``g_outs``: the faces' gradient in 3-D,
        the merged segments' and arcs' in 2-D) through update()'s graph."""
        opt = self.opt
        grads = [None] * len(opt.parameters)
        # Inside a graph capture: differentiate w.r.t. the aliases update() read the parameters
        # through (see boundaries.tap), never w.r.t. the leaves.  Outside a capture the leaf is
        # differentiated too -- its gradient is the total whatever route update() took -- and
        # the first eager steps compare the two: a parameter that reaches the faces (partly)
        # without an alias (a custom _update reading the leaf) must never be captured.
        capturing = torch.cuda.is_current_stream_capturing()
        inputs, owner = [], []
        for i, p in enumerate(opt.parameters):
            taps = tap_log.get(id(p), [])
            if not taps:
                self.untapped = True
            checked = self._tap_checks >= self.graph_warmup and not self.untapped
            if (capturing or checked) and taps:
                inputs.extend(taps)
                owner.extend([i] * len(taps))
            else:
                inputs.extend(taps + [p])
                owner.extend([i] * len(taps) + [-1 - i])
        with torch.autograd.set_multithreading_enabled(False):
            got = torch.autograd.grad(outs, inputs, grad_outputs=g_outs, allow_unused=True)
        total = {}
        for i, g in zip(owner, got):
            if g is None:
                continue
            if i < 0:
                total[-1 - i] = g
            else:
                grads[i] = g if grads[i] is None else grads[i] + g
        for i, g in total.items():
            if (not self.untapped and self._tap_checks < self.graph_warmup
                    and not self._same_gradient(grads[i], g)):
                self.untapped = True
                self.capture_error = RuntimeError(
                    f"FusedStep: parameter {i} reaches the faces without boundaries.tap "
                    "(its leaf gradient differs from the sum over its aliases): the step "
                    "is never captured in a launch graph")
            grads[i] = g
        if not capturing:
            self._tap_checks += 1
        return grads

    @staticmethod
    def _same_gradient(aliases, leaf):
        """Whether the sum over a parameter's aliases is its leaf gradient (one host read per
        parameter, first steps only).  Relative to the gradient's largest entry: the aliases are
        summed in another order than autograd's own accumulation, entries near zero may differ by
        more than any relative bound."""
        if aliases is None or not bool(torch.isfinite(leaf).eq(torch.isfinite(aliases)).all()):
            return False
        finite = dict(nan=0.0, posinf=0.0, neginf=0.0)
        return float(torch.nan_to_num(aliases - leaf, **finite).abs().max()) \
            <= 1e-9 * float(torch.nan_to_num(leaf, **finite).abs().max())

    # ------------------------------------------------------------------------------ 2-D
    def _setup2d(self, inputs, P, flags, rows):
        """State, scene struct and what the reverse sweep differentiates of a 2-D step: the
        (tensor, gradient block) pairs of the merged segments, arcs and indices that take one."""
        block, scene, _ = inputs
        geo = [None if k is None else k["geo"] for k in (scene.segments, scene.arcs)]
        det = [None if g is None else g.detach() for g in geo]
        if any(g is not None and (g.dtype != torch.float64 or not g.is_contiguous()) for g in det):
            raise RuntimeError("FusedStep: merged segments / arcs must be contiguous float64")
        # the per-primitive indices of "value" mode that take a gradient (seg_n_in, seg_n_out,
        # arc_n_in, arc_n_out; None where not), as merged by update() from the boundaries' fields
        index = [n if isinstance(n, torch.Tensor) and n.requires_grad and n.shape[0] > 0 else None
                 for n in scene.index_args()]
        st = self._buffers2d(block, det, P, flags, rows, index)
        st.perm = st.inplace = None       # (2-D traces keep the source's order and compact)
        back = [(g, grad) for g, grad in zip(geo, (st.g_seg, st.g_arc))
                if g is not None and g.requires_grad and g.shape[0] > 0]
        back += [(n, g) for n, g in zip(index, st.g_index) if n is not None]
        return st, scene.struct(det[0], det[1]), back

    @staticmethod
    def _index_grads2d(sc, st, on):
        """Scope in which the 2-D scene struct's index-gradient fields point at the step's blocks."""
        return _override(sc, **{name: g.data_ptr() for name, g in zip(ops._GRAD_INDEX_2D, st.g_index)
                                if on and g is not None})

    def _goal2d(self, src, inputs, tap_log, P, flags):
        """tfrt_trace2d_forward -> tfrt_trace2d_backward_goal (error, seed and the reverse sweep of
        every pass in one launch); the parameter gradients come through update()'s graph from the
        merged segments and arcs.  One process, rays in natural order."""
        erf = self.opt.error_function
        rows = erf.rows_for(2)
        goal = erf.table(src)
        st, sc, back = self._setup2d(inputs, P, flags, rows)
        block = st.block
        self._trace_forward(st, sc, st.outs)
        if back:
            st.g_prim.zero_()
        pending = _lib.GoalPending()
        with self._index_grads2d(sc, st, bool(back)):
            check(_lib.lib().tfrt_trace2d_backward_goal(
                ops._p(block), block.shape[1], st.N, ctypes.byref(sc), self._lengths()[0],
                P, st.dt, ctypes.byref(st.outs["finished"]), st.fields, len(rows), ops._p(goal),
                goal.shape[1], 1, ops._p(st.err), ops._p(self.tests_total),
                ops._p(st.goal_ws), st.gws, ctypes.byref(pending),
                ops._p(st.g_seg) if back and st.Ms else None,
                ops._p(st.g_arc) if back and st.Ma else None,
                ops._p(st.counts), ops._p(st.ws), st.wsb, st.stream),
                "tfrt_trace2d_backward_goal")
        # (nothing on the device waits for the error sum: the parameter update's launch finishes it)
        self._goal_pending = (pending, st.stream)
        self.folded_backward, self.in_place = True, False
        if not back:
            return None, st
        return self._parameter_gradients([b[0] for b in back], [b[1] for b in back], tap_log), st

    def _rowwise2d(self, src, inputs, tap_log, P, flags):
        """_goal2d for a RowwiseError: tfrt_trace2d_forward -> tfrt_trace2d_rows (every source
        ray's column, a mask for the rays that finished) -> ``erf.fn`` on those columns + its
        autograd (torch) -> tfrt_trace2d_backward_rows seeded with the columns' gradient.  No ray
        count is read; everything is capturable."""
        st, sc, back = self._setup2d(inputs, P, flags, None)
        block, N = st.block, st.N
        L = _lib.lib()
        finished = ctypes.byref(st.outs["finished"])
        self._trace_forward(st, sc, st.outs)
        # the finished rows at their source rays' columns
        check(L.tfrt_trace2d_rows(
            ops._p(block), block.shape[1], N, P, st.dt, finished,
            ops._p(st.rows), st.rows.shape[1], ops._p(st.row_face), ops._p(st.counts),
            ops._p(st.ws), st.wsb, st.stream), "tfrt_trace2d_rows")
        # (natural order: column i is source ray i, whose own fields are the inherited ones)
        leaf, e = self._rowwise_terms(st, _GEO2, src.__getitem__)
        e = e.double()
        # No reduction over the rays in torch (a sum over a million entries inside a replayed graph
        # is not reliable): the gradient of the masked sum is the mask itself, and the sum is
        # formed by the sweep's launch and finished by the parameter update's, as for a GoalError
        g64 = None
        if back and e.requires_grad:
            mask = (st.row_face[:N] >= 0).unsqueeze(1).expand_as(e).double()
            with torch.autograd.set_multithreading_enabled(False):
                g_rows, = torch.autograd.grad(e, [leaf], grad_outputs=mask)
            g64 = g_rows.to(torch.float64).contiguous()
            st.g_prim.zero_()
        e = e.detach().contiguous()
        pending = _lib.GoalPending()
        with self._index_grads2d(sc, st, g64 is not None):
            check(L.tfrt_trace2d_backward_rows(
                ops._p(block), block.shape[1], N, ctypes.byref(sc), self._lengths()[0], P,
                st.dt, finished, ops._p(e), e.shape[1], 1, e.shape[1],
                None if g64 is None else ops._p(g64), 0 if g64 is None else g64.shape[1],
                ops._p(st.err), ops._p(self.tests_total), ops._p(st.goal_ws), st.gws,
                ctypes.byref(pending),
                ops._p(st.g_seg) if g64 is not None and st.Ms else None,
                ops._p(st.g_arc) if g64 is not None and st.Ma else None,
                ops._p(st.counts), ops._p(st.ws), st.wsb, st.stream),
                "tfrt_trace2d_backward_rows")
        # (nothing on the device waits for the error sum: the parameter update's launch finishes it)
        self._goal_pending = (pending, st.stream)
        self.folded_backward, self.in_place = False, False
        if g64 is None:
            return None, st
        return self._parameter_gradients([b[0] for b in back], [b[1] for b in back], tap_log), st

    # ------------------------------------------------------------------------ publishing
    def _publish_lazily(self, st, src):
        """Leaves the engine a function that cuts the ray sets of the step ``st`` last enqueued
        (or a replayed graph last ran) when somebody asks for them."""
        eng = self.opt.engine
        P, flags, perm, inplace = st.P, st.flags, st.perm, st.inplace
        eng._trace_src = src
        eng._trace_sig = (src.n_rays if hasattr(src, "n_rays") else src["x_start"].shape[0], P, flags)

        def publish():
            if inplace is not None:
                # the trace ran in place and compacted nothing: the ray sets are gathered from its
                # tape now, into the reference's (per-pass, stable) order of the traced rays
                # (with a coherent order: in the SOURCE's order, through the inverse of the order)
                block, dead_len = inplace
                o = st.outs
                # (`perm` is inverted now, not when the step was enqueued: a replayed graph
                # re-orders a re-drawn source into the same tensor behind Python's back)
                check(_lib.lib().tfrt_trace3d_compact(
                    ops._p(block), block.shape[1], st.N, dead_len, P, st.dt, flags,
                    ctypes.byref(o["finished"]), ctypes.byref(o["active"]),
                    ctypes.byref(o["stopped"]), ctypes.byref(o["dead"]), None, None,
                    ops._p(st.counts), st.M,
                    None if perm is None else ops._p(ops.inverse_order(perm)), ops._p(st.ws),
                    st.wsb, ops._stream(block)), "tfrt_trace3d_compact")
                return ops._finish_trace(dict(st.full), dict(st.aux), P, None)
            out = ops._finish_trace(dict(st.full), dict(st.aux), P, None)
            if st.dim == 2:
                out["n_segments"] = st.Ms
            return out if perm is None else ops.restore_order(out, perm)
        eng._pending_trace = publish

    # ------------------------------------------------------------------------ the update
    def _enqueue_apply(self, grads, accumulators):
        """non-finite -> 0, scale, clip, accumulate, SGD apply (optimizer.py:223-257, 316) with
        the step-dependent scalars read from the device table: rows of {scale, clip,
        sgd_learning_rate}, with {momentum, nesterov} appended for the momentum rule
        (tfrt_sgd_momentum_multi, the optimizer's velocity buffers), or {scale, clip,
        adam_learning_rate, beta1, beta2, epsilon} for the Adam rule (tfrt_adam_multi, the
        optimizer's m / v buffers and its step state, which the launch advances)."""
        opt = self.opt
        L = _lib.lib()
        k = len(grads)
        rule = opt._rule
        batched = (rule.min_batch <= k <= 8 and all(a is None for a in accumulators)
                   and len({ops._stream(p).value for p in opt.parameters}) == 1)
        pending, self._goal_pending = self._goal_pending, None

        def arr(ts, ctype=ctypes.c_void_p):
            return (ctype * len(ts))(*ts)

        def launch(idx, gs, row, stream, *finish):
            """The rule's entry over parameters ``idx`` (consecutive ones) with gradients ``gs``;
            ``row``: address of the first one's row; ``finish``: the pending sum to finish."""
            name = rule.entry + ("_finish" if finish else "")
            check(getattr(L, name)(
                len(gs), arr([g.data_ptr() for g in gs]), None,
                arr([opt.parameters[i].data_ptr() for i in idx]),
                *[arr([getattr(opt, a)[i].data_ptr() for i in idx]) for a in rule.states],
                arr([g.numel() for g in gs], ctypes.c_int64), ctypes.c_void_p(row),
                *[ctypes.c_void_p(getattr(opt, a).data_ptr() + stride * idx[0])
                  for a, stride in rule.extras], *finish, stream), name)
        hyper, row_bytes = self._hyper.dev.data_ptr(), 8 * self._hyper.width
        with torch.no_grad():
            if batched:
                # every parameter tensor in one launch (the device table holds the scalars of
                # parameter i in row i), which also finishes the error sum left on its stream
                stream = ops._stream(opt.parameters[0])
                if pending is not None and pending[1].value == stream.value:
                    launch(range(k), grads, hyper, stream, ctypes.byref(pending[0]))
                    return
                if pending is not None:      # (recorded on another stream: finished on its own)
                    self._goal_finish(*pending)
                launch(range(k), grads, hyper, stream)
                return
            if pending is not None:
                self._goal_finish(*pending)
            for i, (g, p) in enumerate(zip(grads, opt.parameters)):
                stream = ops._stream(p)
                row = hyper + row_bytes * i
                if accumulators[i] is not None:
                    # (the row's first three scalars: tfrt_sgd_process_dev reads no further)
                    processed = torch.empty_like(g)
                    check(L.tfrt_sgd_process_dev(ops._p(g), ops._p(processed), None, g.numel(),
                                                 _lib.F64, ctypes.c_void_p(row), stream),
                          "tfrt_sgd_process_dev")
                    g = opt._matrix_product(opt._acc_cache, i, accumulators[i],
                                            processed).contiguous()
                    row = self._hyper_apply.dev.data_ptr() + row_bytes * i
                if rule is _lib.SGD:
                    check(L.tfrt_sgd_process_dev(ops._p(g), None, ops._p(p), g.numel(), _lib.F64,
                                                 ctypes.c_void_p(row), stream),
                          "tfrt_sgd_process_dev")
                else:
                    # (a one-tensor batch; its row of the rule's state and a ticket of its own:
                    # parameters may sit on different streams)
                    launch([i], [g], row, stream)

    def _fix_grads(self, grads):
        opt = self.opt
        out = []
        for g, p in zip(grads, opt.parameters):
            if g is None:
                if not opt.suppress_warnings:
                    print("Warning: SGD_Optimizer.process_gradient encountered a possible issue:  "
                          "The gradient was likely None, which can mean that the error does not "
                          "depend on it.  The gradient will be set to zero and future instances "
                          "of this message will be suppressed.")
                    opt.suppress_warnings = True
                g = torch.zeros_like(p)
            out.append(g.contiguous())
        return out

    def _sequence(self, accumulators, world):
        """The whole step; with several ranks the collective sits between the two halves."""
        if world > 1:
            # one persistent buffer [grad p_0 ... grad p_k, sum of errors, terms, -]: the face
            # updates' reverse kernels write the parameter gradients straight into it (ops.GradSink)
            # and the error kernel its sums, so the collective needs no concatenation before and
            # no slicing after
            opt = self.opt
            n = sum(p.numel() for p in opt.parameters)
            flat = self._flat_buf
            if flat is None or flat.numel() != n + 3 or flat.device != opt.parameters[0].device:
                flat = self._flat_buf = torch.zeros(n + 3, dtype=torch.float64,
                                                    device=opt.parameters[0].device)
            self._err_sink = flat[n:]
            with ops.GradSink(flat[:n]) as sink:
                grads, err = self._enqueue_gradient()
            fixed = self._fix_grads(grads)
            if (err.data_ptr() == flat[n:].data_ptr() and sink.at == n
                    and all(sink.holds(g) for g in fixed)):
                self._flat, self._flat_views = flat, True
            else:       # (a gradient from somewhere else: a parameter with several aliases, ...)
                self._flat = torch.cat([g.reshape(-1) for g in fixed] + [err[:2]])
                self._flat_views = False
            return fixed
        grads, err = self._enqueue_gradient()
        grads = self._fix_grads(grads)
        self._enqueue_apply(grads, accumulators)
        self._err_view = err
        return grads

    def _after_reduce(self, grads, accumulators):
        flat = self._flat
        if self._flat_views:             # the gradients ARE slices of the reduced buffer
            red, o = grads, flat.numel() - 3
        else:
            o, red = 0, []
            for g in grads:
                red.append(flat[o:o + g.numel()].reshape(g.shape))
                o += g.numel()
        self._enqueue_apply(red, accumulators)
        mean = torch.where(flat[o + 1] > 0, flat[o] / torch.clamp(flat[o + 1], min=1.0),
                           torch.full_like(flat[o], float("nan")))
        self._err_view = torch.stack([flat[o], flat[o + 1], mean])

    # ------------------------------------------------------------------------------ step
    def _hyper_rows(self, lr_scale):
        # (the rule's own values -- the phase's momentum, the Adam rates -- ride in the table too:
        # a phase change or a reassignment replays)
        opt = self.opt
        rows, apply_rows = [], []
        for i in range(len(opt.parameters)):
            scale = float(lr_scale * opt.individual_lr[i] * opt.learning_rate)
            clip = float(opt.grad_clip if opt.clip_mode == "common" else
                         opt.individual_lr[i] * opt.clip_scale * opt.learning_rate * lr_scale)
            rows.append(opt._kernel_row(scale, clip))
            apply_rows.append(opt._kernel_row(1.0, float("inf")))
        return tuple(rows), tuple(apply_rows)

    def _signature(self, accumulators):
        """Everything a captured graph has baked in and the caller could have changed."""
        opt, eng = self.opt, self.opt.engine
        src = eng.optical_system._amalgamated_sources
        if src and hasattr(src, "identity"):
            src_id = src.identity        # (rays re-drawn in place: the buffers stay)
        else:
            src_id = tuple(id(src[f]) for f in (_GEO3 if eng.dimension == 3 else _GEO2)) if src else ()
        return (tuple(id(a) for a in accumulators), tuple(p.data_ptr() for p in opt.parameters),
                src_id, int(opt.trace_depth),
                eng._flags(), eng.new_ray_length, eng.dead_ray_length, eng._trace_mode(),
                id(opt.error_function), id(getattr(opt.error_function, "goal", None)),
                getattr(opt.error_function, "fields", None),
                tdist.world_size(), eng.optical_system.scene_signature(), bool(eng.deterministic),
                id((getattr(eng, "_order_cache", None) or (None, None, None))[2]),
                getattr(eng, "_visit_all_key", None) is not None, eng.in_place,
                id(eng.wave_schedule) if isinstance(eng.wave_schedule, torch.Tensor)
                else eng.wave_schedule,
                self._index_signature()) + self._rule_signature() + self._density_signature()

    def _rule_signature(self):
        """The update rule's part of the signature: the rule and the addresses of its state."""
        opt, rule = self.opt, self.opt._rule
        return (rule.name, tuple(t.data_ptr() for a in rule.states for t in getattr(opt, a)),
                tuple(getattr(opt, a).data_ptr() for a, _ in rule.extras))

    def _density_signature(self):
        """A DensityError's part of the signature: the goal buffer's address (overwriting the goal
        in place is seen by replays, another buffer re-captures), its shape and the constants; a
        SpotError's: the label buffer's address and shape, G and the constants."""
        erf = self.opt.error_function
        return erf.graph_key() if isinstance(erf, (SumError,) + _COUPLED) else ()

    def _index_signature(self):
        """The refractive-index fields that take a gradient (boundary, field, identity of a tensor
        the caller gave).  Their values change in place every step -- a captured update() merges
        them by address --; another tensor, or an index that starts or stops taking a gradient,
        changes the sequence.  (A field update() computes, e.g. a scalar broadcast from a
        material_dict entry, is made inside the captured update(): its identity does not count.)"""
        system = self.opt.engine.optical_system
        sig = []
        for name in system._boundary_sets:
            for b in getattr(system, "_" + name):
                fields = getattr(b, "_fields", {})
                for f in ("n_in", "n_out"):
                    v = fields.get(f)
                    if isinstance(v, torch.Tensor) and v.requires_grad:
                        sig.append((id(b), f, id(v) if v.is_leaf else None))
        return tuple(sig)

    def step(self, accumulators, lr_scale):
        """One optimiser step.  Returns the error tensor {sum, n_terms, mean} (device)."""
        opt = self.opt
        dev = opt.parameters[0].device
        world = 2 if tdist.is_distributed() else 1      # > 1: the collective splits the sequence
        width = opt._rule.width
        if self._hyper is None or self._hyper.width != width:
            # (a captured graph reads the table it was captured with: a new one invalidates it)
            self._graphs = None
            self._hyper = _HyperTable(len(opt.parameters), dev, width=width)
            self._hyper_apply = _HyperTable(len(opt.parameters), dev, width=width)
        opt._state_buffers()         # allocated before the first capture, updated in place after
        rows, apply_rows = self._hyper_rows(lr_scale)
        self._hyper.set(rows)
        self._hyper_apply.set(apply_rows)
        self.steps += 1

        sig = self._signature(accumulators)
        want_graph = self.graph_mode in ("auto", True) and self.capture_error is None
        if want_graph and self._graphs is not None and self._graphs[0] == sig:
            return self._replay()
        if (want_graph and self._eager_steps >= self.graph_warmup and self._stable(sig)
                and not self.untapped):
            return self._capture(sig, accumulators, world)   # (runs this step, then tries to capture)
        self._eager(accumulators, world)
        self._eager_steps += 1
        self._last_sig = sig
        if (self._eager_steps == 3 and self._state is not None
                and getattr(opt.engine, "_trace_perm", None) is not None):
            # (ONE host read, early on: did the sorted source leave wavefronts to the grouped
            # kernel?  Many: coherent="auto" goes back to natural order for this source)
            opt.engine._note_left_over(int(self._state.counts[-1]), self._state.P)
            self._last_sig = self._signature(accumulators)   # (what the note changes is no instability)
        return self._err_view

    def _eager(self, accumulators, world):
        grads = self._sequence(accumulators, world)
        if world > 1:
            torch.distributed.all_reduce(self._flat, op=torch.distributed.ReduceOp.SUM)
            self._after_reduce(grads, accumulators)

    def _replay(self):
        _, ga, gb, _grads = self._graphs
        ga.replay()
        if gb is not None:
            torch.distributed.all_reduce(self._flat, op=torch.distributed.ReduceOp.SUM)
            gb.replay()
        self.graph_replays += 1
        # (a replay re-draws a device-made source behind Python's back: what the source and its
        # distributions had materialised for an earlier draw is stale now)
        for source in getattr(self.opt.engine.optical_system, "_sources", ()):
            note = getattr(source, "note_external_update", None)
            if note is not None:
                note()
        self._republish()
        return self._err_view

    def _stable(self, sig):
        return self._last_sig == sig

    def _republish(self):
        eng = self.opt.engine
        eng.clear_ray_history()
        self._publish_lazily(self._state, eng._trace_src)

    def _capture(self, sig, accumulators, world):
        """Run THIS step eagerly on the capture stream, then capture the sequence there (capturing
        executes nothing).  The eager run on that stream matters: autograd remembers the stream
        on which a leaf's gradient accumulator was created; accumulators left over from steps on
        the caller's stream would make the backward inside the capture fork to that stream, and
        ending the capture then crashes inside the HIP runtime."""
        dev = self.opt.parameters[0].device
        if self._stream is None:
            self._stream = torch.cuda.Stream(dev)
        side, cur = self._stream, torch.cuda.current_stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._eager(accumulators, world)
            err_now = self._err_view.clone()
        cur.wait_stream(side)
        self._last_sig = sig
        self._eager_steps += 1
        # the step itself is done; capturing is an optimisation of the following ones: anything in
        # update() that a capture does not allow (a host->device copy, a blocking read) turns it
        # off for this optimizer and the steps go on eagerly
        # No cyclic garbage collection while a stream captures: the collector may run at any
        # allocation, and an unreachable cycle that holds a CUDAGraph or an event of an earlier
        # optimiser (e.g. the previous FusedStep <-> SGD_Optimizer pair) is then destroyed inside
        # the capture -- the HIP runtime refuses the destroy call and the process aborts.
        gc_was_on = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            torch.cuda.synchronize(dev)
            # (the device is idle: one read tells whether the visiting-order trace of the step just
            # run left wavefronts to the grouped kernel; if not, the captured sequence omits it)
            if self._state is not None:
                self.opt.engine._note_left_over(int(self._state.counts[-1]), self._state.P)
            sig = self._signature(accumulators)
            pool = torch.cuda.graph_pool_handle()
            ga, gb, grads = None, None, None
            want = self.capture_collective
            if want == "auto":
                want = torch.distributed.is_initialized() and torch.distributed.get_world_size() == 1
            if world > 1 and want and torch.distributed.get_backend() == "nccl":
                # RCCL collectives can be captured: update ... gradients | all-reduce | apply as ONE
                # graph, one launch per step (two graphs with an eager collective between them
                # otherwise: gloo, or a runtime that refuses the capture)
                try:
                    g1 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g1, pool=pool, stream=side):
                        grads = self._sequence(accumulators, world)
                        torch.distributed.all_reduce(self._flat, op=torch.distributed.ReduceOp.SUM)
                        self._after_reduce(grads, accumulators)
                    ga, self.collective_in_graph = g1, True
                except Exception as e:       # noqa: BLE001  (fall back to the split form)
                    self.collective_capture_error = e
                    torch.cuda.synchronize(dev)
                    ga = None
            if ga is None:
                self.collective_in_graph = False
                ga = torch.cuda.CUDAGraph()
                with torch.cuda.graph(ga, pool=pool, stream=side):
                    grads = self._sequence(accumulators, world)
                if world > 1:
                    gb = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gb, pool=pool, stream=side):
                        self._after_reduce(grads, accumulators)
            self._graphs = (sig, ga, gb, grads)
        except Exception as e:
            self.capture_error = e
            self._graphs = None
            torch.cuda.synchronize(dev)
        finally:
            if gc_was_on:
                gc.enable()
        self._republish()
        return err_now
