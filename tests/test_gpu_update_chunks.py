"""
More than eight tensors through ``ops.sgd_momentum`` and ``ops.adam``: the launches take eight
tensors each, so a ninth starts a second one at an offset into the table of rows and, for Adam,
into the state.  Seventeen tensors (launches of 8, 8 and 1, with workgroup-boundary sizes and
tensors without elements in the first two), every one with a row and an initial Adam state of its
own, two calls in a row; parameters, state buffers and processed gradients bit for bit against the
numpy restatements of test_gpu_momentum.py and test_gpu_adam.py.
"""
import numpy as np
import pytest
import torch

from test_gpu_adam import _gradient, _on_dev, _restate as _restate_adam, _same
from test_gpu_momentum import _restate as _restate_momentum

pytestmark = pytest.mark.gpu
SIZES = [1, 255, 256, 257, 0, 64, 3, 1, 513, 2, 0, 256, 7, 1, 1, 300, 5]


def _out(sizes):
    return [torch.full((n,), 7.0, dtype=torch.float64, device="cuda:0") for n in sizes]


def test_sgd_momentum_seventeen_tensors_bitwise():
    from tensorflowraytrace_amd import ops
    rng = np.random.default_rng(1700)
    # {scale, clip, sgd_learning_rate, momentum, nesterov}: no two tensors alike, some with m == 0
    rows = [(0.5 + 0.1 * k, 0.05 + 0.03 * k, 0.01 + 0.002 * k,
             0.0 if k % 4 == 0 else (0.9, 0.6, 0.98)[k % 4 - 1] - 0.001 * k, float(k % 2))
            for k in range(len(SIZES))]
    assert len(set(rows)) == len(rows)
    p = [rng.standard_normal(n) for n in SIZES]
    v = [rng.standard_normal(n) * 1e-3 for n in SIZES]
    p_d, v_d = _on_dev(p), _on_dev(v)
    for _ in range(2):
        g = [_gradient(rng, n, r[1] / r[0]) for n, r in zip(SIZES, rows)]
        out = _out(SIZES)
        ops.sgd_momentum(_on_dev(g), p_d, v_d, rows, processed=out)
        torch.cuda.synchronize()
        for k, r in enumerate(rows):
            gw, p[k], v[k] = _restate_momentum(g[k], p[k], v[k], *r[:4], r[4] != 0.0)
            assert _same(out[k], gw) and _same(p_d[k], p[k]) and _same(v_d[k], v[k]), k


def test_adam_seventeen_tensors_bitwise():
    from tensorflowraytrace_amd import ops
    rng = np.random.default_rng(1701)
    count = len(SIZES)
    # {scale, clip, adam_learning_rate, beta1, beta2, epsilon} and {t, p1, p2}: no two tensors alike
    rows = [(0.5 + 0.1 * k, 0.05 + 0.03 * k, 1e-3 * (1 + k), 0.9 - 0.01 * k, 0.999 - 0.002 * k,
             1e-7 * (1 + k)) for k in range(count)]
    st = np.array([[float(k), 0.8 - 0.03 * k, 0.99 - 0.01 * k] for k in range(count)])
    t0 = st[:, 0].copy()
    p = [rng.standard_normal(n) for n in SIZES]
    m = [rng.standard_normal(n) * 1e-2 for n in SIZES]
    v = [rng.random(n) * 1e-3 for n in SIZES]
    p_d, m_d, v_d = _on_dev(p), _on_dev(m), _on_dev(v)
    st_d = torch.tensor(st, dtype=torch.float64, device="cuda:0")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    for _ in range(2):
        g = [_gradient(rng, n, r[1] / r[0]) for n, r in zip(SIZES, rows)]
        out = _out(SIZES)
        ops.adam(_on_dev(g), p_d, m_d, v_d, rows, st_d, ticket, processed=out)
        torch.cuda.synchronize()
        for k, r in enumerate(rows):
            gw, p[k], m[k], v[k], st[k] = _restate_adam(g[k], p[k], m[k], v[k], st[k], *r)
            assert _same(out[k], gw) and _same(p_d[k], p[k]), k
            assert _same(m_d[k], m[k]) and _same(v_d[k], v[k]), k
        assert _same(st_d, st)
        assert int(ticket) == 0
    # every tensor's step count advanced by exactly 2, the ones without elements included
    assert st_d[:, 0].cpu().numpy().tolist() == (t0 + 2.0).tolist()
    assert all(np.isfinite(x).all() for x in p)
