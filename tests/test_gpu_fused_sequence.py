"""
The launch sequence of the fused optimiser step (fused_step.FusedStep), entry point by entry point.

``_lib.lib()`` hands back a recording proxy that forwards every call unchanged and notes the name of
the C-ABI entry; the ordered ``tfrt_*`` names of one steady-state eager step (graph=False) are
compared with lists written down from the module as it was before its four paths were given one
skeleton.  A change to fused_step.py that adds, drops or re-orders a launch fails here by name.
Replayed graphs are not covered (a replay calls nothing from Python).

The scoped override of the cached scene struct has a host-side case of its own (no GPU).
"""
import importlib

import pytest


class _Recording:
    """Forwards every attribute of the ctypes handle; calls of tfrt_* entries are logged by name."""

    def __init__(self, handle, log):
        self._handle, self._log = handle, log

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.startswith("tfrt_"):
            return fn
        log = self._log

        def call(*args):
            log.append(name)
            return fn(*args)
        self.__dict__[name] = call
        return call


@pytest.fixture
def log(monkeypatch):
    # (every module of the package calls _lib.lib() at use; none binds the handle once)
    from tensorflowraytrace_amd import _lib
    calls = []
    proxy = _Recording(_lib.lib(), calls)
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    return calls


def _steady_step(opt, log, steps, accumulators=None, **kw):
    """The entry points of step number ``steps``; it and the one before it must be fused steps
    (a RowwiseError's first steps take the generic path) that made the same calls."""
    seen, fused = [], []
    for _ in range(steps):
        del log[:]
        opt.single_step(accumulators, **kw)
        seen.append(list(log))
        fused.append(0 if opt._fused_step is None else opt._fused_step.steps)
    assert fused[-1] == fused[-2] + 1 == fused[-3] + 2, "the last steps were not fused ones"
    assert opt._fused_step.graph_replays == 0
    assert seen[-1] == seen[-2], "the recorded step is not a steady-state one"
    return seen[-1]


# ---------------------------------------------------------------------------------- scenes
def _lens3d(n_rays, k=3, coherent=None, in_place=None, **kw):
    from test_gpu_fused_step import _make
    opt, eng, *_rest, acc = _make(n_rays, "eager", k=k, **kw)
    if coherent is not None:
        eng.coherent = coherent
    if in_place is not None:
        eng.in_place = in_place
    return opt, acc


def _optimizer2d(make, momentum=False, adam=False):
    import torch
    from tfrt.optimizer import Adam_Optimizer, SGD_Optimizer
    eng, params, erf = make(torch.float64)
    cls = Adam_Optimizer if adam else SGD_Optimizer
    return cls(eng, params, erf, 4, learning_rate=0.02, grad_clip=0.05,
               sgd_learning_rate=1.0, apply_momentum=momentum, fused=True, graph=False)


def _lens3d_adam(n_rays, **kw):
    from test_gpu_adam import _make
    opt, _eng, _lens, acc = _make(n_rays, "eager", **kw)
    return opt, acc


def _index2d(error):
    def make(ray_dtype):
        from test_gpu_index_gradients import _lens, _rowwise_fn
        from tfrt.optimizer import RowwiseError
        eng, params, erf = _lens(ray_dtype)
        return eng, params, RowwiseError(_rowwise_fn) if error == "rowwise" else erf
    return make


def _case(name):
    """(optimizer, accumulators, steps, keyword arguments of single_step) of a named case."""
    from test_gpu_fused_2d import SCENES
    from test_gpu_fused_2d_rowwise import _rowwise
    if name == "3d_goal_natural":                       # two parameters, plain rule
        return _lens3d(2000) + (6, {})
    if name == "3d_goal_coherent_per_pass":
        return _lens3d(20000, k=6, coherent=True, in_place=False) + (6, {})
    if name == "3d_goal_in_place":
        return _lens3d(8192) + (9, {})
    if name == "3d_rowwise_in_place":
        from test_gpu_rowwise import _make
        return _make(6000, "eager")[0], None, 10, {}
    if name in ("3d_density", "3d_spot", "3d_transport"):
        # (the scenes and the ray count of those modules' fused-equals-generic tests)
        make = importlib.import_module("test_gpu_" + name[3:])._make
        return make(8192, "eager")[0], None, 10, {}
    if name == "3d_sum":
        from test_gpu_combine import DIRECTIONS, _make
        return _make(8192, "eager", lambda n: (
            ("transport", "density", "goal"), (40.0 / (n * DIRECTIONS), 1.0, 1.0), "sum",
            0.05))[0], None, 10, {}
    if name == "2d_goal":
        return _optimizer2d(SCENES["mixed"]), None, 6, {}
    if name == "2d_rowwise":
        return _optimizer2d(_rowwise(SCENES["mixed"])), None, 6, {}
    if name in ("3d_goal_index", "3d_rowwise_index"):
        from test_gpu_index_gradients import _lens3d as index_lens
        return index_lens(8192, name.split("_")[1], "eager")[0], None, 10, {}
    if name in ("2d_goal_index", "2d_rowwise_index"):
        return _optimizer2d(_index2d(name.split("_")[1])), None, 6, {}
    if name == "apply_one_parameter":
        return _optimizer2d(SCENES["single_arc"]), None, 6, {}
    if name == "apply_one_parameter_momentum":
        return _optimizer2d(SCENES["single_arc"], momentum=True), None, 6, {"momentum": 0.9}
    if name == "apply_two_parameters_momentum":
        return _lens3d(2000, apply_momentum=True) + (6, {"momentum": 0.9})
    if name == "apply_accumulator":
        return _lens3d(2000, accumulators=True) + (6, {})
    if name == "apply_accumulator_momentum":
        return _lens3d(2000, accumulators=True, apply_momentum=True) + (6, {"momentum": 0.9})
    if name == "apply_one_parameter_adam":
        return _optimizer2d(SCENES["single_arc"], adam=True), None, 6, {}
    if name == "apply_two_parameters_adam":
        return _lens3d_adam(2000) + (6, {})
    if name == "apply_accumulator_adam":
        return _lens3d_adam(2000, accumulators=True) + (6, {})
    raise KeyError(name)


# What the module made of one steady-state step before the refactoring (recorded on an MI355X).
# update() of the parametric 3-D lens and its reverse are launches of their own; the 2-D scenes'
# update() is torch code.
_UPDATE3D, _UPDATE3D_BACK = "tfrt_param_faces_forward_multi", "tfrt_param_faces_backward_multi"
_UNFOLDED3D = [_UPDATE3D, "tfrt_trace3d_forward", "tfrt_goal_error3d_deferred",
               "tfrt_trace3d_backward", _UPDATE3D_BACK]
_FOLDED3D = [_UPDATE3D, "tfrt_trace3d_forward", "tfrt_trace3d_backward_goal", _UPDATE3D_BACK]
# (the error is summed in torch: no pending sum for the update's launch to finish)
_ROWWISE3D = [_UPDATE3D, "tfrt_trace3d_in_place", "tfrt_trace3d_forward", "tfrt_trace3d_backward",
              _UPDATE3D_BACK, "tfrt_sgd_process_multi"]
_GOAL2D = ["tfrt_trace2d_forward", "tfrt_trace2d_backward_goal"]
_ROWWISE2D = ["tfrt_trace2d_forward", "tfrt_trace2d_rows", "tfrt_trace2d_backward_rows"]
EXPECTED = {
    # (case, error function's path)                   # the step's launches, then the update's
    "3d_goal_natural": _UNFOLDED3D + ["tfrt_sgd_process_multi_finish"],
    "3d_goal_coherent_per_pass": _FOLDED3D + ["tfrt_sgd_process_multi_finish"],
    "3d_goal_in_place": _FOLDED3D + ["tfrt_sgd_process_multi_finish"],
    "3d_rowwise_in_place": _ROWWISE3D,
    "2d_goal": _GOAL2D + ["tfrt_sgd_process_multi_finish"],
    "2d_rowwise": _ROWWISE2D + ["tfrt_sgd_process_multi_finish"],
    "3d_goal_index": _FOLDED3D + ["tfrt_sgd_process_multi_finish"],
    "3d_rowwise_index": _ROWWISE3D,
    "2d_goal_index": _GOAL2D + ["tfrt_sgd_process_multi_finish"],
    "2d_rowwise_index": _ROWWISE2D + ["tfrt_sgd_process_multi_finish"],
    # one parameter: the plain rule takes the per-parameter path, the momentum rule one launch
    "apply_one_parameter": _GOAL2D + ["tfrt_goal_finish", "tfrt_sgd_process_dev"],
    "apply_one_parameter_momentum": _GOAL2D + ["tfrt_sgd_momentum_multi_finish"],
    # two parameters, plain rule: "3d_goal_natural"
    "apply_two_parameters_momentum": _UNFOLDED3D + ["tfrt_sgd_momentum_multi_finish"],
    # an accumulator on the first of two parameters: the per-parameter path
    "apply_accumulator": _UNFOLDED3D + ["tfrt_goal_finish", "tfrt_sgd_process_dev",
                                        "tfrt_csr_matvec", "tfrt_sgd_process_dev",
                                        "tfrt_sgd_process_dev"],
    "apply_accumulator_momentum": _UNFOLDED3D + ["tfrt_goal_finish", "tfrt_sgd_process_dev",
                                                 "tfrt_csr_matvec", "tfrt_sgd_momentum_multi",
                                                 "tfrt_sgd_momentum_multi"],
    # the Adam rule on the same scenes: one launch from one parameter on, like momentum
    "apply_one_parameter_adam": _GOAL2D + ["tfrt_adam_multi_finish"],
    "apply_two_parameters_adam": _UNFOLDED3D + ["tfrt_adam_multi_finish"],
    "apply_accumulator_adam": _UNFOLDED3D + ["tfrt_goal_finish", "tfrt_sgd_process_dev",
                                             "tfrt_csr_matvec", "tfrt_adam_multi",
                                             "tfrt_adam_multi"],
}
# The coupled errors and a SumError of a transport, a density and a goal term, recorded on an
# MI355X before the error terms moved to errors.py: the error's launches stand where a
# RowwiseError's torch code does.  The host's sizing queries (``*_workspace_bytes``) are no
# launches; they are dropped from both lists before these cases are compared.
_COLUMNS3D = _ROWWISE3D[:3], _ROWWISE3D[3:]
COUPLED = {
    "3d_density": ["tfrt_density_error_workspace_bytes", "tfrt_density_error_fields"],
    "3d_spot": ["tfrt_spot_error_workspace_bytes", "tfrt_spot_error_fields"],
    "3d_transport": ["tfrt_transport_error_workspace_bytes", "tfrt_transport_error"],
    "3d_sum": ["tfrt_transport_error_workspace_bytes", "tfrt_transport_error",
               "tfrt_density_error_workspace_bytes", "tfrt_density_error_fields",
               "tfrt_goal_error_columns_workspace_bytes", "tfrt_goal_error_columns",
               "tfrt_error_combine"],
}
EXPECTED.update({name: _COLUMNS3D[0] + calls + _COLUMNS3D[1] for name, calls in COUPLED.items()})


def _launches(calls):
    return [name for name in calls if not name.endswith("_workspace_bytes")]


# (folded reverse sweep, in-place trace) of the recorded step
MODES = {
    "3d_goal_natural": (False, False), "3d_goal_coherent_per_pass": (True, False),
    "3d_goal_in_place": (True, True), "3d_rowwise_in_place": (False, True),
    "3d_density": (False, True), "3d_spot": (False, True), "3d_transport": (False, True),
    "3d_sum": (False, True),
    "3d_goal_index": (True, True), "3d_rowwise_index": (False, True),
    "2d_goal": (True, False), "2d_rowwise": (False, False),
}


def record(name, log):
    opt, acc, steps, kw = _case(name)
    return opt, _steady_step(opt, log, steps, acc, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_steady_state_step_makes_the_recorded_launches(name, log):
    opt, calls = record(name, log)
    fs = opt._fused_step
    if name in MODES:
        assert (fs.folded_backward, fs.in_place) == MODES[name]
    if name in COUPLED:
        assert _launches(calls) == _launches(EXPECTED[name])
    else:
        assert calls == EXPECTED[name]


# --------------------------------------------------------------------------- host side
def test_scoped_override_sets_and_restores_struct_fields():
    from tensorflowraytrace_amd import _lib
    from tensorflowraytrace_amd.fused_step import _override
    sc = _lib.Scene3D()
    sc.in_place, sc.clear_count, sc.grad_n_in = 1, 7, 4096
    before = (sc.in_place, sc.clear_buffer, sc.clear_count, sc.grad_n_in, sc.grad_n_out)
    with _override(sc, in_place=2, clear_buffer=8192, clear_count=9, grad_n_in=None,
                   grad_n_out=64) as inside:
        assert inside is sc
        assert (sc.in_place, sc.clear_buffer, sc.clear_count, sc.grad_n_in, sc.grad_n_out) == \
            (2, 8192, 9, None, 64)
        with _override(sc, in_place=0):               # scopes nest
            assert sc.in_place == 0 and sc.clear_count == 9
        assert sc.in_place == 2
    assert (sc.in_place, sc.clear_buffer, sc.clear_count, sc.grad_n_in, sc.grad_n_out) == before
    with pytest.raises(ZeroDivisionError):
        with _override(sc, in_place=2, clear_buffer=8192):
            assert sc.in_place == 2
            1 / 0
    assert (sc.in_place, sc.clear_buffer, sc.clear_count, sc.grad_n_in, sc.grad_n_out) == before
    with _override(sc):                               # no field: nothing to do
        pass
    assert (sc.in_place, sc.clear_buffer, sc.clear_count, sc.grad_n_in, sc.grad_n_out) == before
