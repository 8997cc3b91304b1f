"""
The momentum rule of SGD_Optimizer's generic path on the host (``cpu_backend`` stand-ins, CPU
tensors: eager torch ops) against a float64 numpy restatement of the Keras rule

    v = m*v - lr*g;   p += m*v - lr*g  (nesterov)  |  p += v

with one persistent velocity tensor per parameter, updated in place, and ``m == 0`` meaning
plain ``p -= lr*g`` with ``v`` untouched.
"""
import numpy as np
import pytest
import torch

from test_host_logic import _lens_api


def _restate(p, v, g, m, lr, nesterov):
    """One step of the rule in numpy float64, every product and difference rounded on its own."""
    v = m * v - lr * g
    p = p + ((m * v - lr * g) if nesterov else v)
    return p, v


def _spy(opt, ops, monkeypatch):
    """Per step: the parameters / velocities just before the update, the processed gradients and
    the parameters / velocities after it."""
    log = []
    orig_apply = opt.apply_gradients
    orig_process = ops.sgd_process

    def snap():
        return ([p.detach().numpy().copy() for p in opt.parameters],
                [None if v is None else v.numpy().copy() for v in opt._velocity])

    def sgd_process(grad, scale, clip, param=None, sgd_learning_rate=0.0):
        if param is not None and (not log or "pre" in log[-1] and "post" in log[-1]):
            log.append({"pre": None})
        if param is not None and log[-1]["pre"] is None:
            log[-1]["pre"] = snap()          # (plain SGD applies inside the processing)
        return orig_process(grad, scale, clip, param=param, sgd_learning_rate=sgd_learning_rate)

    def apply_gradients(grads, skip=None):
        if not log or "post" in log[-1]:
            log.append({"pre": None})
        if log[-1]["pre"] is None:
            log[-1]["pre"] = snap()
        log[-1]["g"] = [g.detach().numpy().copy() for g in grads]
        orig_apply(grads, skip=skip)
        log[-1]["post"] = snap()

    monkeypatch.setattr(ops, "sgd_process", sgd_process)
    opt.apply_gradients = apply_gradients
    return log


@pytest.mark.parametrize("nesterov", [True, False])
def test_generic_momentum_step_equals_the_numpy_restatement(cpu_backend, monkeypatch, nesterov):
    import tfrt.optimizer as optimizer
    from tensorflowraytrace_amd import ops
    eng, system, lens, target = _lens_api(200)

    def erf(engine):
        fin = engine.finished_rays
        return (torch.stack([fin["y_end"], fin["z_end"]], 1) + fin["object_coords"][:, 1:]) ** 2

    opt = optimizer.SGD_Optimizer(eng, lens.parameters, erf, 3, learning_rate=5e-3, grad_clip=1e-2,
                                  apply_momentum=True, nesterov=nesterov)
    assert opt.nesterov is nesterov
    log = _spy(opt, ops, monkeypatch)
    schedule = [0.6, 0.6, 0.6, 0.0, 0.0, 0.9, 0.9, 0.9]
    velocity_ids = None
    for m in schedule:
        opt.single_step(None, momentum=m)
        if velocity_ids is None:
            velocity_ids = [id(v) for v in opt._velocity]
            ptrs = [v.data_ptr() for v in opt._velocity]
        # the velocity buffers are the same tensors, updated in place, from the first step on
        assert [id(v) for v in opt._velocity] == velocity_ids
        assert [v.data_ptr() for v in opt._velocity] == ptrs
    assert len(log) == len(schedule)
    lr = opt.sgd_learning_rate
    moved = 0.0
    for m, rec in zip(schedule, log):
        (p0, v0), (p1, v1) = rec["pre"], rec["post"]
        for i in range(len(p0)):
            g = rec["g"][i]
            if m == 0.0:
                # plain SGD; the velocity keeps its value to the last bit
                assert v1[i].tobytes() == (v0[i] if v0[i] is not None else np.zeros_like(g)).tobytes()
                np.testing.assert_allclose(p1[i], p0[i] - lr * g, rtol=0, atol=1e-17)
            else:
                v_prev = v0[i] if v0[i] is not None else np.zeros_like(g)
                pw, vw = _restate(p0[i], v_prev, g, m, lr, nesterov)
                np.testing.assert_array_equal(v1[i], vw)
                np.testing.assert_array_equal(p1[i], pw)
            moved = max(moved, float(np.abs(v1[i]).max()))
    assert moved > 0.0                                   # the velocity did build up


def test_momentum_defaults_keep_todays_behaviour(cpu_backend):
    import tfrt.optimizer as optimizer
    eng, system, lens, target = _lens_api(100)
    opt = optimizer.SGD_Optimizer(eng, lens.parameters, lambda e: None, 3)
    assert opt.apply_momentum is False and opt.nesterov is True
    assert opt._velocity == [None, None]
