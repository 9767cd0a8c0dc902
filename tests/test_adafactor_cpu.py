"""`flasht5_amd.Adafactor` without a GPU: the argument checks and the host-side schedule are HF's, nothing runs on the CPU."""
import math

import pytest
import torch
from transformers.optimization import Adafactor as HFAdafactor


@pytest.mark.parametrize("kw", [dict(lr=1e-3), dict(lr=1e-3, relative_step=True), dict(relative_step=False, warmup_init=True)])
def test_argument_checks_raise_what_hf_raises(kw):
    from flasht5_amd import Adafactor
    p = [torch.nn.Parameter(torch.zeros(4, 4))]
    with pytest.raises(ValueError) as hf:
        HFAdafactor(p, **kw)
    with pytest.raises(ValueError) as ours:
        Adafactor(p, **kw)
    assert str(ours.value) == str(hf.value)


def test_cpu_parameter_raises_and_is_not_touched():
    from flasht5_amd import Adafactor
    p = torch.nn.Parameter(torch.ones(4, 4))
    p.grad = torch.ones(4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Adafactor([p]).step()
    assert torch.equal(p.detach(), torch.ones(4, 4))


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("kw", [dict(), dict(warmup_init=True), dict(lr=3e-4, relative_step=False), dict(decay_rate=-0.5)])
def test_schedule_values_equal_hf(step, kw):
    """beta2t and rho against HF's own expressions: `_get_lr` with scale_parameter off returns rel_step_sz itself"""
    from flasht5_amd import Adafactor
    group = Adafactor([torch.nn.Parameter(torch.zeros(2))], **kw).param_groups[0]
    beta2t, rho = Adafactor._schedule(group, step)
    assert beta2t == 1.0 - math.pow(step, group["decay_rate"])
    assert rho == HFAdafactor._get_lr({**group, "scale_parameter": False}, {"step": step, "RMS": 0.0})


def test_graphed_train_step_takes_adafactor_and_still_refuses_sgd():
    from flasht5_amd import Adafactor, GraphedTrainStep
    lin = torch.nn.Linear(8, 8)
    GraphedTrainStep(lin, Adafactor(lin.parameters()))
    with pytest.raises(TypeError):
        GraphedTrainStep(lin, torch.optim.SGD(lin.parameters(), lr=0.1))
