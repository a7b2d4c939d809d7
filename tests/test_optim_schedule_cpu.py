"""Host side of the optimiser options: the tri-stage schedule against the reference's own class (golden:
tests/golden/tri_stage.json, written by tests/golden/make_tri_stage_golden.py), the translation of torch schedulers
and optimisers into the engine's descriptions.  No GPU."""
import json
import os

import pytest
import torch

from conftest import GOLDEN


def _golden():
    with open(os.path.join(GOLDEN, "tri_stage.json")) as f:
        return json.load(f)


def test_tri_stage_matches_reference_golden():
    """Every step 0 .. max_steps + 2 of the default ratios 0.1 / 0.4 / 0.5 at max_steps 10, 37, 1000 and of a
    configuration without warm-up: 1e-6 relative (the reference's tables are f32).  Where the reference's own table
    lookup raises (max_steps 37: the floors lose two steps and step 37 indexes past the decay table) the port raises
    the same exception class."""
    from w2v2_speaker_amd.optim.schedule import TriStageLearningRateLambdaLRFunction as Tri
    cases = _golden()
    assert sorted(c["config"]["max_steps"] for c in cases) == [10, 37, 100, 1000]
    assert any(c["config"]["warmup_stage_ratio"] == 0 for c in cases)
    for c in cases:
        fn = Tri(**c["config"])
        assert len(c["factors"]) == c["config"]["max_steps"] + 3
        for step, want in enumerate(c["factors"]):
            if want is None:
                with pytest.raises(IndexError):
                    fn(step)
                assert c["raises"][str(step)] == "IndexError"
            else:
                assert fn(step) == pytest.approx(want, rel=1e-6, abs=0), (c["config"], step)
        assert fn(c["config"]["max_steps"] + 50) == pytest.approx(c["config"]["final_lr"] / c["config"]["base_lr"], rel=1e-12)


def test_tri_stage_rejects_bad_ratios():
    from w2v2_speaker_amd.optim.schedule import TriStageLearningRateLambdaLRFunction as Tri
    lrs = dict(initial_lr=1e-6, base_lr=1e-4, final_lr=1e-7)
    with pytest.raises(ValueError):
        Tri(100, -0.1, 0.6, 0.5, **lrs)                  # a ratio outside [0, 1]
    with pytest.raises(ValueError):
        Tri(100, 0.1, 0.4, 0.4, **lrs)                   # ratios that do not add up to 1


def _dummy(algo):
    p = torch.nn.Parameter(torch.zeros(1))
    if algo == "adam":
        return p, torch.optim.Adam([p], lr=3e-3, betas=(0.8, 0.99))
    return p, torch.optim.SGD([p], lr=3e-3, momentum=0.7, nesterov=True)


def _second(opt):
    g = opt.param_groups[0]
    return g["betas"][0] if "betas" in g else g["momentum"]


@pytest.mark.parametrize("algo", ["adam", "sgd"])
@pytest.mark.parametrize("kind", ["one_cycle", "lambda"])
def test_from_torch_scheduler_follows_the_torch_scheduler(algo, kind):
    """.at(step) == the lr and beta1 / momentum a real torch scheduler leaves in the param group, 50 steps."""
    from torch.optim.lr_scheduler import LambdaLR, OneCycleLR
    from w2v2_speaker_amd.optim.schedule import (LambdaSchedule, OneCycle, TriStageLearningRateLambdaLRFunction,
                                                 from_torch_scheduler)
    p, opt = _dummy(algo)
    if kind == "one_cycle":
        sched = OneCycleLR(opt, max_lr=1e-2, total_steps=50, pct_start=0.3)
    else:
        sched = LambdaLR(opt, TriStageLearningRateLambdaLRFunction(50, 0.1, 0.4, 0.5, 1e-5, 3e-3, 1e-6))
    ours = from_torch_scheduler(sched)
    assert isinstance(ours, OneCycle if kind == "one_cycle" else LambdaSchedule)
    for step in range(50):
        lr, second = ours.at(step)
        assert lr == pytest.approx(opt.param_groups[0]["lr"], rel=1e-12), step
        assert second == pytest.approx(_second(opt), rel=1e-12), step
        p.grad = torch.ones(1)
        opt.step()
        if step < 49:
            sched.step()
    if kind == "lambda":
        assert ours.at(0)[1] == (0.8 if algo == "adam" else 0.7)         # not cycled: the optimiser's own value


def test_from_torch_scheduler_rejects_other_classes():
    from w2v2_speaker_amd.optim.schedule import from_torch_scheduler
    _, opt = _dummy("sgd")
    with pytest.raises(NotImplementedError, match="StepLR"):
        from_torch_scheduler(torch.optim.lr_scheduler.StepLR(opt, 10))


def test_optim_config_from_torch_round_trips_and_rejects():
    from w2v2_speaker_amd.optim import OptimConfig
    p = torch.nn.Parameter(torch.zeros(1))
    c = OptimConfig.from_torch(torch.optim.Adam([p], lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-2))
    assert c == OptimConfig("adam", beta2=0.99, eps=1e-6, weight_decay=1e-2)
    c = OptimConfig.from_torch(torch.optim.SGD([p], lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4))
    assert c == OptimConfig("sgd", weight_decay=1e-4, momentum=0.9, dampening=0.0, nesterov=True)
    c = OptimConfig.from_torch(torch.optim.SGD([p], lr=1e-3, momentum=0.5, dampening=0.1))
    assert c == OptimConfig("sgd", momentum=0.5, dampening=0.1, nesterov=False)
    assert OptimConfig.from_torch(torch.optim.SGD([p], lr=1e-3)) == OptimConfig("sgd")
    with pytest.raises(NotImplementedError, match="AdamW"):
        OptimConfig.from_torch(torch.optim.AdamW([p], lr=1e-3))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        OptimConfig.from_torch(torch.optim.Adam([p], lr=1e-3, amsgrad=True))
    with pytest.raises(NotImplementedError, match="maximize"):
        OptimConfig.from_torch(torch.optim.SGD([p], lr=1e-3, maximize=True))
    q = torch.nn.Parameter(torch.zeros(1))
    with pytest.raises(NotImplementedError, match="param_groups"):
        OptimConfig.from_torch(torch.optim.SGD([{"params": [p]}, {"params": [q], "lr": 1.0}], lr=1e-3))
    opt = torch.optim.SGD([p], lr=1e-3, momentum=0.9, nesterov=True)
    opt.param_groups[0]["dampening"] = 0.1               # (the constructor refuses the pair; a config edit can make it)
    with pytest.raises(ValueError, match="dampening"):
        OptimConfig.from_torch(opt)
    with pytest.raises(ValueError, match="algo"):
        OptimConfig("adamw")
