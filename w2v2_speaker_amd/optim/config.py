"""One description of the optimiser, read by every trainer (ref: src/main.py:323-335 builds it with
``instantiate(cfg.optim.algo, params=network.parameters())`` from config/optim/algo/{adam,sgd}.yaml; the paper's
search config/search/lr_and_schedule_search.yaml sweeps ``optim/algo`` and ``optim.algo.weight_decay``).

The learning rate and the cycled second value (Adam's beta1 / SGD's momentum) are NOT here: they come from the
schedule, step by step, like torch's ``OneCycleLR`` writes them into the param group."""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class OptimConfig:
    """algo "adam": torch.optim.Adam (L2 weight decay, not AdamW; ``momentum`` / ``dampening`` / ``nesterov`` unused).
    algo "sgd": torch.optim.SGD (``beta2`` / ``eps`` unused).  The momentum a step runs with is the schedule's second
    value (what torch's ``OneCycleLR`` cycles); ``momentum`` here is the optimiser's own setting, which
    ``schedule.from_torch_scheduler`` hands to a schedule that does not cycle it."""
    algo: str = "adam"
    beta2: float = 0.999
    eps: float = 1e-8
    weight_decay: float = 0.0
    momentum: float = 0.0
    dampening: float = 0.0
    nesterov: bool = False

    def __post_init__(self):
        if self.algo not in ("adam", "sgd"):
            raise ValueError(f"OptimConfig.algo must be 'adam' or 'sgd', got {self.algo!r}")
        if self.weight_decay < 0:
            raise ValueError(f"OptimConfig.weight_decay must be >= 0, got {self.weight_decay}")
        if self.algo == "sgd":
            if self.momentum < 0:
                raise ValueError(f"OptimConfig.momentum must be >= 0, got {self.momentum}")
            if self.nesterov and (self.momentum <= 0 or self.dampening != 0):
                raise ValueError("OptimConfig.nesterov requires a momentum and zero dampening (torch.optim.SGD)")

    @staticmethod
    def from_torch(optimizer) -> "OptimConfig":
        """Read class and ``param_groups[0]`` of a ``torch.optim.Adam`` / ``torch.optim.SGD``.  Whatever the fused step
        does not implement raises and names the field."""
        import torch
        groups = optimizer.param_groups
        if len(groups) != 1:
            raise NotImplementedError(f"param_groups: {len(groups)} groups; per-group hyper-parameters are not supported")
        g = groups[0]
        if g.get("maximize", False):
            raise NotImplementedError("maximize=True is not supported")
        if type(optimizer) is torch.optim.Adam:
            if g.get("amsgrad", False):
                raise NotImplementedError("amsgrad=True is not supported")
            return OptimConfig("adam", beta2=float(g["betas"][1]), eps=float(g["eps"]),
                               weight_decay=float(g["weight_decay"]))
        if type(optimizer) is torch.optim.SGD:
            if g["nesterov"] and g["dampening"] != 0:
                raise ValueError("nesterov=True with dampening != 0 (torch.optim.SGD rejects it as well)")
            return OptimConfig("sgd", weight_decay=float(g["weight_decay"]), momentum=float(g["momentum"]),
                               dampening=float(g["dampening"]), nesterov=bool(g["nesterov"]))
        raise NotImplementedError(f"optimizer class {type(optimizer).__name__}: only torch.optim.Adam and "
                                  "torch.optim.SGD have a fused step")
