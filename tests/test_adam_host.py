"""
The Adam rule of Adam_Optimizer's generic path on the host (``cpu_backend`` stand-ins, CPU tensors:
eager torch ops) against a float64 numpy restatement of the Keras rule (non-amsgrad)

    t = t + 1;  p1 = p1 * beta1;  p2 = p2 * beta2          (running products, not pow())
    lr_t = adam_learning_rate * sqrt(1 - p2) / (1 - p1)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * (g * g)
    param -= lr_t * m / (sqrt(v) + epsilon)

on the processed gradient ``g`` (non-finite -> 0, scale, clip), with persistent ``m``, ``v`` and
``{t, p1, p2}`` per parameter, updated in place.
"""
import numpy as np
import torch

from test_host_logic import _lens_api


def _restate(p, m, v, st, g, lr, beta1, beta2, eps):
    """One step of the rule in numpy float64, every operation rounded on its own.  ``st`` is
    {t, p1, p2}; returns the new (p, m, v, st)."""
    st = np.array([st[0] + 1.0, st[1] * beta1, st[2] * beta2])
    lr_t = lr * np.sqrt(1.0 - st[2]) / (1.0 - st[1])
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    p = p - lr_t * m / (np.sqrt(v) + eps)
    return p, m, v, st


def _erf(engine):
    fin = engine.finished_rays
    return (torch.stack([fin["y_end"], fin["z_end"]], 1) + fin["object_coords"][:, 1:]) ** 2


def test_generic_adam_step_equals_the_numpy_restatement(cpu_backend, monkeypatch):
    import tfrt.optimizer as optimizer
    eng, system, lens, target = _lens_api(200)
    extra = torch.zeros(3, dtype=torch.float64, requires_grad=True)   # the error ignores it: None
    params = list(lens.parameters) + [extra]
    # (raw gradients of 130 to 380 here: at scale 1e-4 the clip of 0.02 catches the larger ones only)
    opt = optimizer.Adam_Optimizer(eng, params, _erf, 3, learning_rate=1e-4, grad_clip=2e-2,
                                   adam_learning_rate=2e-3, beta1=0.8, beta2=0.99, epsilon=1e-6)
    opt.suppress_warnings = True
    assert opt._fused_step is None and opt.update_rule == "adam"

    # the raw gradient of every step, with non-finite entries planted in the first parameter's
    raw, orig_raw = [], opt.raw_gradient
    poison = [np.nan, np.inf, -np.inf]

    def raw_gradient(*a, **k):
        grads, err, n = orig_raw(*a, **k)
        grads = [g.clone() for g in grads]
        for j, bad in enumerate(poison):
            grads[0][2 * j + len(raw) % 2] = bad
        raw.append([g.numpy().copy() for g in grads])
        return grads, err, n

    monkeypatch.setattr(opt, "raw_gradient", raw_gradient)
    # (update() applies the lens's thickness constraints before the trace: the parameters a step
    # starts from are the ones apply_gradients finds, not the ones the last step left)
    pre, orig_apply = [], opt.apply_gradients

    def apply_gradients(grads, skip=None):
        assert skip is None or not any(skip)
        pre.append([p.detach().numpy().copy() for p in params])
        orig_apply(grads, skip=skip)

    monkeypatch.setattr(opt, "apply_gradients", apply_gradients)
    steps = 8
    want = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape),
             np.array([0.0, 1.0, 1.0])) for p in params]
    ids = None
    clipped = untouched = 0
    for step in range(steps):
        if step == 5:                       # plain attributes, reassigned between steps
            opt.adam_learning_rate, opt.beta2 = 1e-3, 0.95
        opt.single_step(None, lr_scale=1.0 - 0.05 * step, momentum=0.9)
        scale = (1.0 - 0.05 * step) * 1e-4
        lr, b1, b2, eps = opt.adam_learning_rate, opt.beta1, opt.beta2, opt.epsilon
        for i, (_, m, v, st) in enumerate(want):
            p, g = pre[step][i], raw[step][i]
            g = np.where(np.isfinite(g), g, 0.0) * scale
            clipped += int((np.abs(g) > 2e-2).sum())
            untouched += int(((np.abs(g) < 2e-2) & (g != 0.0)).sum())
            g = np.where(g < -2e-2, -2e-2, np.where(g > 2e-2, 2e-2, g))
            want[i] = _restate(p, m, v, st, g, lr, b1, b2, eps)
            np.testing.assert_array_equal(params[i].detach().numpy(), want[i][0])
            np.testing.assert_array_equal(opt._adam_m[i].numpy(), want[i][1])
            np.testing.assert_array_equal(opt._adam_v[i].numpy(), want[i][2])
            np.testing.assert_array_equal(opt._adam_state[i].numpy(), want[i][3])
        # the state buffers are the same tensors, updated in place, from the first step on
        now = [id(t) for t in opt._adam_m + opt._adam_v] + [opt._adam_state.data_ptr()]
        ids = ids or now
        assert now == ids
    assert clipped > 0 and untouched > 0
    assert all(np.isfinite(w[0]).all() for w in want)
    assert float(opt._adam_state[0, 0]) == steps
    assert np.abs(want[0][1]).max() > 0 and np.abs(want[2][1]).max() == 0      # (None gradient)

    # reset_state: in place, and the next step is a first step again
    opt.reset_state()
    assert [id(t) for t in opt._adam_m + opt._adam_v] + [opt._adam_state.data_ptr()] == ids
    assert all(float(t.abs().max()) == 0.0 for t in opt._adam_m + opt._adam_v)
    np.testing.assert_array_equal(opt._adam_state.numpy(), [[0.0, 1.0, 1.0]] * 3)


def test_adam_phases_set_the_attributes(cpu_backend):
    import tfrt.optimizer as optimizer
    eng, system, lens, target = _lens_api(100)
    opt = optimizer.Adam_Optimizer(eng, lens.parameters, _erf, 3, learning_rate=1.0)
    opt.training_routine([{"steps": 1, "beta1": 0.5, "adam_learning_rate": 1e-4},
                          {"steps": 1, "epsilon": 1e-5}], report_frequency=0, show_time=False)
    assert (opt.beta1, opt.adam_learning_rate, opt.epsilon, opt.beta2) == (0.5, 1e-4, 1e-5, 0.999)
    assert float(opt._adam_state[0, 0]) == 2.0
    np.testing.assert_array_equal(opt._adam_state[:, 1].numpy(), [0.25, 0.25])


def test_adam_constructor_accepts_and_ignores_the_sgd_arguments(cpu_backend):
    import tfrt.optimizer
    import tensorflowraytrace_amd.optimizer as native
    assert tfrt.optimizer.Adam_Optimizer is native.Adam_Optimizer
    assert issubclass(native.Adam_Optimizer, native.SGD_Optimizer)
    eng, system, lens, target = _lens_api(100)
    runs = []
    for kw in ({}, dict(sgd_learning_rate=7.0, momentum=0.5, apply_momentum=True, nesterov=False)):
        eng, system, lens, target = _lens_api(100)
        opt = native.Adam_Optimizer(eng, lens.parameters, _erf, 3, learning_rate=1.0, **kw)
        assert (opt.adam_learning_rate, opt.beta1, opt.beta2, opt.epsilon) == (1e-3, 0.9, 0.999, 1e-7)
        assert opt.update_rule == "adam"
        for _ in range(3):
            opt.single_step(None, momentum=0.7)
        assert all(v is None for v in opt._velocity)            # no SGD state was ever made
        runs.append([p.detach().numpy().copy() for p in lens.parameters])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
        assert np.isfinite(a).all()
