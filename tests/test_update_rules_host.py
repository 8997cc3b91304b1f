"""
The description of each update rule that the optimiser classes carry (``_lib.UpdateRule``: C entry,
row of the device table, state lists, trailing arguments, smallest batched launch), on the host,
against the C ABI's signatures and the rows the fused step writes into its device table.
"""
import pytest
import torch

from test_host_logic import _lens_api


def _erf(engine):
    fin = engine.finished_rays
    return torch.stack([fin["y_end"], fin["z_end"]], 1) ** 2


@pytest.mark.parametrize("name, entry, width, n_states, n_extras, min_batch", [
    ("sgd", "tfrt_sgd_process_multi", 3, 0, 0, 2),
    ("momentum", "tfrt_sgd_momentum_multi", 5, 1, 0, 1),
    ("adam", "tfrt_adam_multi", 6, 2, 2, 1)])
def test_rule_description(cpu_backend, name, entry, width, n_states, n_extras, min_batch):
    import tfrt.optimizer as optimizer
    from tensorflowraytrace_amd import _lib
    from tensorflowraytrace_amd.fused_step import FusedStep
    eng, system, lens, target = _lens_api(50)
    cls = optimizer.Adam_Optimizer if name == "adam" else optimizer.SGD_Optimizer
    opt = cls(eng, lens.parameters, _erf, 3, learning_rate=0.5, grad_clip=0.25,
              sgd_learning_rate=0.125, momentum=0.75, apply_momentum=name == "momentum",
              nesterov=True)
    rule = opt._rule
    assert opt.update_rule == rule.name == name
    assert (rule.entry, rule.width, len(rule.states), len(rule.extras), rule.min_batch) == \
        (entry, width, n_states, n_extras, min_batch)
    # the C entries: count, grad, processed, param, [states], n, rows, [extras], (pending,) stream
    n_args = 7 + n_states + n_extras
    assert len(_lib.SIGNATURES[entry][1]) == n_args
    assert len(_lib.SIGNATURES[entry + "_finish"][1]) == n_args + 1
    # state lists with one slot per parameter; the trailing arguments' strides: {t, p1, p2} float64
    # and one int32 ticket per parameter
    assert all(len(getattr(opt, a)) == len(opt.parameters) for a in rule.states)
    assert [s for _, s in rule.extras] == [24, 4][:n_extras]
    # the rows of the device table
    rows, apply_rows = FusedStep(opt)._hyper_rows(0.5)
    tail = {"sgd": (0.125,), "momentum": (0.125, 0.75, 1.0),
            "adam": (0.001, 0.9, 0.999, 1e-7)}[name]
    assert rows == ((0.25, 0.25) + tail,) * len(opt.parameters)
    assert apply_rows == ((1.0, float("inf")) + tail,) * len(opt.parameters)
    assert all(len(r) == rule.width for r in rows + apply_rows)
