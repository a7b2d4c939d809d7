"""Learning-rate / momentum schedules computed on the host (scalars fed to the fused optimiser kernel).

``OneCycle`` = torch ``OneCycleLR`` with the reference's settings (ref: config/optim/schedule/one_cycle.yaml:3-20,
wired at src/main.py:323-335): cosine anneal, two phases, pct_start 0.3, div_factor 25, final_div 1e4 and
-- torch default ``cycle_momentum=True`` -- Adam's beta1 cycled 0.95 -> 0.85 -> 0.95 (quirk Q11)."""
from __future__ import annotations

import math
from collections import Counter
from dataclasses import dataclass
from typing import Callable, Sequence, Tuple


@dataclass
class OneCycle:
    max_lr: float
    total_steps: int
    pct_start: float = 0.3
    div_factor: float = 25.0
    final_div_factor: float = 1e4
    base_momentum: float = 0.85
    max_momentum: float = 0.95

    def at(self, step: int) -> Tuple[float, float]:
        """(lr, beta1) used by optimiser step number ``step`` (0-based)."""
        if step >= self.total_steps:
            raise ValueError(f"Tried to step {step + 1} times. The specified number of total steps is {self.total_steps}")
        initial_lr = self.max_lr / self.div_factor
        min_lr = initial_lr / self.final_div_factor
        end1 = float(self.pct_start * self.total_steps) - 1
        end2 = self.total_steps - 1

        def cos(a, b, pct):
            return b + (a - b) / 2.0 * (math.cos(math.pi * pct) + 1)

        if step <= end1:
            pct = step / end1
            return cos(initial_lr, self.max_lr, pct), cos(self.max_momentum, self.base_momentum, pct)
        pct = (step - end1) / (end2 - end1)
        return cos(self.max_lr, min_lr, pct), cos(self.base_momentum, self.max_momentum, pct)


@dataclass
class Constant:
    lr: float
    beta1: float = 0.9

    def at(self, step: int) -> Tuple[float, float]:
        return self.lr, self.beta1


class TriStageLearningRateLambdaLRFunction:
    """The reference's tri-stage factor function for ``LambdaLR`` (ref: src/optim/schedule/tri_stage.py,
    config/optim/schedule/tri_stage.yaml): linear warm-up ``initial_lr -> base_lr``, a constant stage at ``base_lr``, an
    exponential decay ``base_lr -> final_lr``; ``__call__(step)`` returns the lr of that step divided by ``base_lr``.
    Same constructor, and the same arithmetic down to its quirks:
      * the three stage lengths are ``floor(max_steps * ratio)``, so they may add up to less than ``max_steps``;
      * the warm-up values are an f32 ``linspace`` table of ``warmup`` points (with two or more of them the last
        warm-up step already sits at ``base_lr``);
      * the constant stage's upper bound is inclusive, so the decay table -- an f32 ``logspace`` of ``decay + 2`` points
        -- is entered at index 1; where the floors lose two or more steps (e.g. max_steps 37 at 0.1 / 0.4 / 0.5) the
        last steps before ``max_steps`` index past the table and raise IndexError, as the reference does;
      * beyond ``max_steps`` the factor is ``final_lr / base_lr``."""

    def __init__(self, max_steps: int, warmup_stage_ratio: float, constant_stage_ratio: float, decay_stage_ratio: float,
                 initial_lr: float, base_lr: float, final_lr: float):
        import torch
        ratios = (warmup_stage_ratio, constant_stage_ratio, decay_stage_ratio)
        if any(not 0 <= r <= 1 for r in ratios):
            raise ValueError(f"stage ratios must lie in [0, 1], got {ratios}")
        if abs(sum(ratios) - 1) >= 1e-9:
            raise ValueError("stage ratio's need to add up to 1")
        if max_steps is None:
            raise ValueError("the tri-stage schedule needs `max_steps`")
        self.max_steps = max_steps
        self.warmup_stage_steps, self.constant_stage_steps, self.decay_stage_steps = (
            math.floor(max_steps * r) for r in ratios)
        self.initial_lr, self.base_lr, self.final_lr = initial_lr, base_lr, final_lr
        self.warmup_stage_space = torch.linspace(initial_lr, base_lr, steps=self.warmup_stage_steps).tolist()
        self.decay_stage_space = torch.logspace(math.log(base_lr), math.log(final_lr), steps=self.decay_stage_steps + 2,
                                                base=math.e).tolist()

    def __call__(self, step_count: int) -> float:
        decay_from = self.warmup_stage_steps + self.constant_stage_steps
        if step_count < self.warmup_stage_steps:
            lr = self.warmup_stage_space[step_count]
        elif step_count <= decay_from:
            lr = self.base_lr
        elif step_count <= self.max_steps:
            lr = self.decay_stage_space[step_count - decay_from]
        else:
            lr = self.final_lr
        return lr / self.base_lr


@dataclass
class LambdaSchedule:
    """torch ``LambdaLR``: lr = base_lr * fn(step); the second value (Adam's beta1 / SGD's momentum) is not cycled."""
    base_lr: float
    fn: Callable[[int], float]
    momentum: float = 0.9

    def at(self, step: int) -> Tuple[float, float]:
        return self.base_lr * self.fn(step), self.momentum


@dataclass
class MultiStep:
    """torch ``MultiStepLR`` (ref: config/optim/schedule/schedule_wav2spk.yaml): the lr is multiplied by ``gamma`` at every
    milestone (a milestone listed n times: by gamma ** n), one factor after the other as torch's chained form does, so the
    values agree with the torch scheduler to the last bit; the second value (Adam's beta1 / SGD's momentum) is not cycled."""
    base_lr: float
    milestones: Sequence[int]
    gamma: float = 0.1
    momentum: float = 0.9

    def at(self, step: int) -> Tuple[float, float]:
        """(lr, beta1) used by optimiser step number ``step`` (0-based)."""
        lr = self.base_lr
        count = Counter(int(m) for m in self.milestones)
        for m in sorted(count):
            if m <= step:
                lr = lr * self.gamma ** count[m]
        return lr, self.momentum


@dataclass
class MarginSchedule:
    """The margin of the classification head as a function of the OPTIMISER step (this project's own definition; the
    trainers write it to ``plan.head.margin`` before each micro-batch):  r = clamp((step - start_step) / (end_step -
    start_step), 0, 1);  "linear": initial + (final - initial) r;  "exp": initial + (final - initial) (1 - 1000^-r) /
    (1 - 1/1000), which has covered half the way at r = 0.1.  ``end_step == start_step`` is a step function at that step.
    Large-margin fine-tuning is the constant schedule ``MarginSchedule(m, initial=m)``."""
    final: float
    initial: float = 0.0
    start_step: int = 0
    end_step: int = 0
    mode: str = "linear"

    def __post_init__(self):
        if self.mode not in ("linear", "exp"):
            raise ValueError(f"margin schedule: mode {self.mode!r} is neither 'linear' nor 'exp'")
        if self.end_step < self.start_step:
            raise ValueError(f"margin schedule: end_step {self.end_step} before start_step {self.start_step}")

    def __call__(self, step: int) -> float:
        span = self.end_step - self.start_step
        r = min(max((step - self.start_step) / span, 0.0), 1.0) if span > 0 else float(step >= self.start_step)
        if self.mode == "exp":
            r = (1.0 - 1000.0 ** -r) / (1.0 - 1.0 / 1000.0)
        return self.initial + (self.final - self.initial) * r


def from_torch_scheduler(sched):
    """A ``torch.optim.lr_scheduler.OneCycleLR`` -> ``OneCycle``, a ``LambdaLR`` -> ``LambdaSchedule``, a ``MultiStepLR`` ->
    ``MultiStep`` (what the reference's config/optim/schedule/{one_cycle,tri_stage,schedule_wav2spk}.yaml instantiate).  ``.at(step)`` of the result is the lr
    and beta1 / momentum the torch scheduler leaves in the param group after ``step`` calls of ``scheduler.step()``.
    Read from the scheduler's attributes and its optimiser's first param group; anything else raises."""
    from torch.optim import lr_scheduler as L
    groups = sched.optimizer.param_groups
    if len(groups) != 1:
        raise NotImplementedError(f"param_groups: {len(groups)} groups; per-group schedules are not supported")
    g = groups[0]
    own = g["betas"][0] if "betas" in g else g.get("momentum", 0.0)
    if isinstance(sched, L.OneCycleLR):
        ph = sched._schedule_phases
        if len(ph) != 2:
            raise NotImplementedError("OneCycleLR three_phase=True is not supported")
        if getattr(sched, "_anneal_func_type", "cos") != "cos":
            raise NotImplementedError("OneCycleLR anneal_strategy='linear' is not supported")
        base, top = (g["base_momentum"], g["max_momentum"]) if sched.cycle_momentum else (own, own)
        return OneCycle(max_lr=g["max_lr"], total_steps=sched.total_steps,
                        pct_start=(float(ph[0]["end_step"]) + 1) / sched.total_steps,
                        div_factor=g["max_lr"] / g["initial_lr"], final_div_factor=g["initial_lr"] / g["min_lr"],
                        base_momentum=base, max_momentum=top)
    if isinstance(sched, L.LambdaLR):
        return LambdaSchedule(sched.base_lrs[0], sched.lr_lambdas[0], own)
    if isinstance(sched, L.MultiStepLR):
        return MultiStep(sched.base_lrs[0], sorted(sched.milestones.elements()), sched.gamma, own)
    raise NotImplementedError(f"scheduler class {type(sched).__name__}: only OneCycleLR, LambdaLR and MultiStepLR are mapped")
