"""
The optimiser step as ONE fixed launch sequence (no host read inside, hipGraph-replayable).

``SGD_Optimizer.single_step`` of the reference (tfrt/optimizer.py:187-320) is

    system.update() -> engine.ray_trace(depth) -> error_function(engine) -> tape.gradient
    -> non-finite -> 0, scale, clip, accumulate -> SGD apply

The generic path of this package keeps the user's ``error_function`` arbitrary torch code, which
costs a blocking read of the ray counts (the finished set has a data-dependent length), ~25
stock torch kernels for the error and its reverse, and autograd bookkeeping: ~0.75 ms per step
whatever the ray count -- the part that caps ray-parallel strong scaling.

The error terms that state their form declaratively are in errors.py; an optimiser given a
``GoalError`` runs ``FusedStep``:

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
finished rows at the rays' own columns.  A coupled error (``DensityError``, ``SpotError``,
``TransportError``, ``FocusError``, ``DistortionError``, ``FlatFieldError``, ``CentroidError``,
``MomentError``, ``MixingError``) takes ``_rowwise3d`` too, with the term's own launches
(``term.seed_columns``, errors.py) in the place of ``fn`` and its autograd.  A ``SumError`` takes
``_rowwise3d`` as well (``_sum_seeds3d``): every term's ``seed_columns`` into a seed block of its
own, then ONE ``tfrt_error_combine`` for the step's seed block and error.

The four bodies share one skeleton: ``_enqueue_gradient`` does what comes before the trace, the
body its launches over a ``_StepState``, ``_publish_lazily`` and ``_enqueue_apply`` what comes after.

Every launch has step-independent arguments (learning-rate dependent scalars live in a small
device table), so after a few eager steps the sequence is captured once in a HIP graph
(``torch.cuda.CUDAGraph``) and replayed: one graph launch per step.  With ray shards over several
processes the collective splits it in two graphs (RCCL is called eagerly between them).
"""
import contextlib
import ctypes
import gc

import torch

from . import _lib, ops
from . import distributed as tdist
from ._lib import RayOut, check

# (the error terms are reached through this module too: optimizer.py and the tests import them here)
from .errors import (_COUPLED, _GEO2, _GEO3, _Columns, CentroidError, DensityError,  # noqa: F401
                     DistortionError, FlatFieldError, FocusError, GoalError, MixingError,
                     MomentError, RowwiseError, SpotError, SumError, TransportError)

_CLASS_FLAGS = (("finished", _lib.COMPILE_FINISHED), ("active", _lib.COMPILE_ACTIVE),
                ("stopped", _lib.COMPILE_STOPPED), ("dead", _lib.COMPILE_DEAD))


class _NotInPlace(RuntimeError):
    """The fixed-shape path of a RowwiseError needs an in-place trace; this step takes the generic
    path instead."""


class _TermState:
    """What one built-in term owns in a step's state (the ``hold`` of ``term.seed_columns``): its
    (6, capN) seed block and error triple, the rows of the block it writes, and ``buffers``, which
    the term fills with what its kind of error keeps."""
    __slots__ = ("g_fin", "err", "row_mask", "buffers")

    def __init__(self, g_fin, err, row_mask):
        self.g_fin, self.err, self.row_mask, self.buffers = g_fin, err, row_mask, {}


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
        "term",                                              # a single coupled error's _TermState
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
    ``SpotError``, a ``TransportError``, a ``FocusError``, a ``DistortionError``, a
    ``FlatFieldError``, a ``CentroidError``, a ``MomentError``, a ``MixingError`` or a ``SumError``
    of them on 3-D engines;
    see the module docstring.
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
        rowwise = opt.error_function.on_columns
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
        fixed-shape tensors + its autograd (torch), or a coupled error's own launches
        (``erf.seed_columns``, errors.py), or a SumError's terms and tfrt_error_combine -> reverse
        sweep.  No ray count is read; everything is capturable."""
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
            if isinstance(erf, RowwiseError):
                g64 = self._rowwise_seeds3d(st, src, perm, need_back)
            else:
                cols = _Columns(st.rows[:, :N], st.row_face, perm, src, N)
                if isinstance(erf, SumError):
                    self._sum_seeds3d(st, cols, erf, need_back)
                else:                   # a single coupled error: its launches write the step's own
                    if st.term is None:
                        st.term = _TermState(st.g_fin, st.err, erf.seed_rows)
                    erf.seed_columns(cols, st.term)
                with torch.no_grad():
                    self.tests_total += st.row_passes[:N].sum() * M
                g64 = st.g_fin if need_back else None
            if g64 is not None:
                with self._index_grads3d(sc, st, True):
                    self._trace3d_backward(st, sc, g64, g64.shape[1])
                with ops.FaceSums() if four else contextlib.nullcontext():
                    grads = self._parameter_gradients(*self._outs3d(fv, st, index), tap_log)
        return grads, st

    def _sum_seeds3d(self, st, cols, erf, need_back):
        """A SumError on the fixed-shape columns ``cols``: every term's ``seed_columns`` into a
        private, once-zeroed (6, capN) seed block, its own triple and buffers of its own, then ONE
        tfrt_error_combine writes the step's seed block ``st.g_fin`` (all six rows, every column)
        and ``st.err``; without a reverse sweep only the errors are combined.  Nothing is read
        back: the coefficients of ``reduce="mean"`` come from the triples on the device."""
        dev = st.rows.device
        key = tuple(id(t) for t in erf.terms)
        if st.terms is None or st.terms_key != key:
            K = len(erf.terms)
            st.term_errs = torch.zeros((K, 3), dtype=torch.float64, device=dev)
            st.coeff = torch.zeros(K, dtype=torch.float64, device=dev)
            st.terms = [_TermState(torch.zeros((6, st.capN), dtype=torch.float64, device=dev),
                                   st.term_errs[k], t.seed_rows)
                        for k, t in enumerate(erf.terms)]
            st.terms_key = key
            self._graphs = None
        for t, hold in zip(erf.terms, st.terms):
            t.seed_columns(cols, hold)
        ops.error_combine(
            [(h.g_fin if need_back else None, h.row_mask, h.err) for h in st.terms],
            erf.weights_on(dev), erf.reduce, n=st.N, n_rows=6, out=st.g_fin, err=st.err,
            coeff=st.coeff)
        erf.last_errors, erf.last_coefficients = st.term_errs, st.coeff

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
                self._index_signature()) + self._rule_signature() + self._error_signature()

    def _rule_signature(self):
        """The update rule's part of the signature: the rule and the addresses of its state."""
        opt, rule = self.opt, self.opt._rule
        return (rule.name, tuple(t.data_ptr() for a in rule.states for t in getattr(opt, a)),
                tuple(getattr(opt, a).data_ptr() for a, _ in rule.extras))

    def _error_signature(self):
        """The error function's own part of the signature, its ``graph_key()``: the addresses and
        shapes of the buffers its launches read (overwriting one in place is seen by replays,
        another buffer re-captures) and its constants.  A RowwiseError has none."""
        key = getattr(self.opt.error_function, "graph_key", None)
        return () if key is None else key()

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
