"""Host side of the fused optimiser step, shared by ParamStore and EcapaStore: state arenas, the gradient-norm
pair and the choice of entry point; and WindowedTrainer, the step / accumulation-window protocol shared by their trainers.
Everything here only enqueues launches; nothing reads the device."""
from __future__ import annotations

from typing import Optional

import torch

from .. import ops
from .config import OptimConfig

DEFAULT = OptimConfig()


def bind_algo(store, cfg: OptimConfig) -> None:
    """A store steps under one algorithm for its lifetime (the moment arenas mean different things under each)."""
    have = getattr(store, "optim_algo", None)
    if have is not None and have != cfg.algo:
        raise RuntimeError(f"optimiser state of this store belongs to {have!r}; it cannot step (or load a state "
                           f"written) under {cfg.algo!r}")
    store.optim_algo = cfg.algo


def ensure_state(store, cfg: OptimConfig, second: float) -> None:
    """Adam: exp_avg + exp_avg_sq.  SGD: the momentum buffer lives in exp_avg (none at all without momentum);
    exp_avg_sq is never allocated."""
    bind_algo(store, cfg)
    if store.exp_avg is None and (cfg.algo == "adam" or second != 0):
        store.exp_avg = torch.zeros_like(store.grad)
    if store.exp_avg_sq is None and cfg.algo == "adam":
        store.exp_avg_sq = torch.zeros_like(store.grad)


def norm_pass(store, n: int, grad_scale: float, scaler, max_norm: float, grad=None) -> torch.Tensor:
    """store.grad_norm = {norm, clip coefficient} of the first n gradient elements (two launches).  ``grad``: the arena
    to read (None = store.grad)."""
    if getattr(store, "_norm_partials", None) is None:
        store._norm_partials = torch.zeros(ops.grad_norm_partials(store.grad.numel()), dtype=torch.float64,
                                           device=store.grad.device)
    ops.grad_norm(store.grad if grad is None else grad, n, store.grad_norm, store._norm_partials, grad_scale, scaler, max_norm)
    return store.grad_norm


def launch(cfg: OptimConfig, p, g, m, v, pb, n: int, lr: float, second: float, step: int, grad_scale: float,
           scaler=None, skip_slot: int = 0, norm_state: Optional[torch.Tensor] = None) -> None:
    """One optimiser launch over n elements.  ``second``: Adam's beta1 / SGD's momentum of this step.  The default
    optimiser (Adam, no weight decay, no clipping) takes the entry point it always took."""
    if cfg.algo == "adam" and cfg.weight_decay == 0 and norm_state is None:
        ops.adam_step(p, g, m, v, pb, n, lr, second, cfg.beta2, cfg.eps, step, grad_scale, scaler, skip_slot)
        return
    ops.optim_step(cfg.algo, p, g, m, v, pb, n, lr, second, cfg.beta2, cfg.eps, step, grad_scale, scaler, skip_slot,
                   weight_decay=cfg.weight_decay, momentum=second if cfg.algo == "sgd" else 0.0,
                   dampening=cfg.dampening, nesterov=cfg.nesterov, norm_state=norm_state)


def accumulate(store, start: int, end: int) -> None:
    """Add store.grad[start:end] into the open accumulation window (``trainer.accumulate_grad_batches`` > 1): the first
    micro-batch of a window (store.accum_count == 0) overwrites store.grad_acc, so the arena is never zeroed.  The arena
    -- a second gradient arena, 4 B/parameter -- is allocated here, on the first accumulating step.  The caller advances
    store.accum_count once per micro-batch (a micro-batch may accumulate bucket by bucket)."""
    if store.grad_acc is None:
        store.grad_acc = torch.empty_like(store.grad)
    if end > start:
        ops.grad_accumulate(store.grad_acc[start:end], store.grad[start:end], end - start, store.accum_count == 0)


class WindowedTrainer:
    """``accumulate_grad_batches`` = N (PL's ``trainer.accumulate_grad_batches``): at N > 1 one ``train_step`` call is one
    micro-batch whose gradient the trainer adds into ``store.grad_acc``; the N-th call of a window reduces that arena over
    the ranks, steps on the mean over world * N micro-batches and advances the schedule.  ``stepped`` tells which kind
    the last call was, ``flush()`` closes a partial window.  A trainer supplies its ``train_step`` and ``_reduce_window()``,
    the all-reduce of what the open window holds in store.grad_acc (nothing on one rank)."""

    def __init__(self, store, schedule, optimizer: Optional[OptimConfig], gradient_clip_val: float,
                 accumulate_grad_batches: int, world: int):
        if int(accumulate_grad_batches) != accumulate_grad_batches or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches must be an integer >= 1, got {accumulate_grad_batches!r}")
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self.stepped = False               # whether the last train_step / flush call ran the optimiser
        self.store, self.schedule, self.step, self.world = store, schedule, 0, world
        self.optimizer, self.gradient_clip_val = optimizer, float(gradient_clip_val)
        self.margin_schedule = None        # optim.schedule.MarginSchedule (the trainers' ``margin_schedule`` keyword)

    def _apply_margin(self, plan) -> None:
        """``margin_schedule``: write the margin of optimiser step ``self.step`` to the plan's head before a micro-batch.
        The step index moves with the optimiser, so the margin is constant within an accumulation window, and a
        checkpoint that restores the step restores the margin."""
        if self.margin_schedule is not None:
            plan.head.margin = float(self.margin_schedule(self.step))

    def _optimizer_step(self, grad: Optional[torch.Tensor] = None, n_micro: int = 1, head_only: bool = False) -> None:
        """Step on the mean of ``grad`` (None = store.grad), the rank-summed gradient of ``n_micro`` micro-batches per rank,
        with the schedule's values of this step; then advance the schedule."""
        lr, second = self.schedule.at(self.step)           # beta1 under Adam, the momentum under SGD
        self.store.optimizer_step(lr, second, self.optimizer, 1.0 / (self.world * n_micro), self.gradient_clip_val,
                                  head_only=head_only, grad=grad)
        self.step += 1

    def _close_window(self, head_only: bool = False) -> None:
        """Step on the (already reduced) accumulated arena, still divided by world * N when the window is partial -- PL
        divides every micro-batch's loss by N, also those of a short last window."""
        self._optimizer_step(self.store.grad_acc, self.accumulate_grad_batches, head_only)
        self.store.accum_count = 0

    def flush(self) -> None:
        """Close a partial window (the end of an epoch): all-reduce what has been accumulated and step on it.  Nothing
        happens when no window is open."""
        self.stepped = False
        if self.accumulate_grad_batches == 1 or self.store.accum_count == 0:
            return
        self._reduce_window()
        self._close_window()
        self.stepped = True
