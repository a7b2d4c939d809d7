"""``set_optimizer`` / ``set_lr_schedule`` / ``configure_optimizers`` of the reference's ``BaseLightningModule`` (ref:
src/lightning_modules/base_lightning_module.py:58-62,70-75), shared by the three speaker modules.  The reference builds a
torch optimiser and scheduler over ``network.parameters()`` from its configuration and hands them to the module (ref:
src/main.py:323-335); here the two objects are READ -- class and first param group through ``OptimConfig.from_torch``,
the scheduler through ``schedule.from_torch_scheduler`` -- and the fused step runs what they describe.  The torch
optimiser itself is never stepped (manual optimisation, see Wav2vec2FCModule)."""
from __future__ import annotations

from typing import Optional

import torch

from ...optim import OptimConfig
from ...optim.schedule import from_torch_scheduler


class OptimizerSurface:
    optimizer_cfg: Optional[OptimConfig] = None      # None: the fused Adam the modules always ran
    gradient_clip_val: float = 0.0                   # PL ``trainer.gradient_clip_val`` (constructor keyword)
    accumulate_grad_batches: int = 1                 # PL ``trainer.accumulate_grad_batches`` (constructor keyword)
    schedule_step: int = 0                           # optimiser steps taken = position in the learning-rate schedule
    _window_trainer = None                           # the trainer whose calls opened the accumulation window
    _torch_optimizer = None
    _torch_schedule = None

    def set_optimizer(self, optimizer: torch.optim.Optimizer) -> None:
        """A ``torch.optim.Adam`` or ``torch.optim.SGD`` over ``self.parameters()``.  Anything the fused step does not
        implement (another class, amsgrad, maximize, several param groups) raises and names the field."""
        self.optimizer_cfg = OptimConfig.from_torch(optimizer)
        self._torch_optimizer = optimizer
        self._trainers.clear()                       # trainers hold the description they were built with

    def set_lr_schedule(self, schedule) -> None:
        """The reference's schedule dict ``{"scheduler": ..., "interval": "step", ...}`` (config/optim/schedule/*.yaml)
        or the bare torch scheduler: a ``OneCycleLR`` or a ``LambdaLR`` (tri-stage)."""
        sched = schedule["scheduler"] if isinstance(schedule, dict) else schedule
        if isinstance(schedule, dict) and schedule.get("interval", "step") != "step":
            raise NotImplementedError(f"interval: {schedule['interval']!r}; the schedule advances once per optimiser step")
        self.schedule = from_torch_scheduler(sched)
        self._torch_schedule = schedule
        self._trainers.clear()

    def configure_optimizers(self):
        """What was set, in the reference's form ``[optimizer], [schedule]``; None before the ``set_`` calls."""
        if self._torch_optimizer is None:
            return None
        return [self._torch_optimizer], [self._torch_schedule]

    def _trainer_options(self) -> dict:
        return {"optimizer": self.optimizer_cfg, "gradient_clip_val": self.gradient_clip_val,
                "accumulate_grad_batches": self.accumulate_grad_batches}

    def _set_accumulate_grad_batches(self, n) -> None:
        if int(n) != n or n < 1:
            raise ValueError(f"accumulate_grad_batches must be an integer >= 1, got {n!r}")
        self.accumulate_grad_batches = int(n)

    def _after_micro_batch(self, trainer) -> None:
        """``training_step`` bookkeeping: the schedule advances only when the trainer ran the optimiser (every call at
        ``accumulate_grad_batches`` = 1)."""
        if trainer.stepped:
            self.schedule_step += 1
            self._window_trainer = None
        else:
            self._window_trainer = trainer

    def on_train_epoch_end(self) -> None:
        """PL steps on a partial window at the end of an epoch (each micro-batch still divided by N): flush the trainer
        that holds the open window.  Nothing happens without one."""
        tr = self._window_trainer
        if tr is None:
            return
        tr.step = self.schedule_step
        tr.flush()
        self._after_micro_batch(tr)

    def parameters(self, recurse: bool = True):
        """One ``nn.Parameter`` view of the flat arena per parameter (``.grad`` = the matching gradient view), so that
        the reference's ``instantiate(cfg.optim.algo, params=network.parameters())`` has something to hold."""
        if getattr(self, "_param_views", None) is None:
            store = self.store
            # reference registration order where the store knows it (the speaker heads of ParamStore), arena order else
            names = (store.reference_parameter_order() if getattr(store, "head", None) in ("aam", "ce")
                     else list(store.shapes))
            self._param_views = {}
            for n in names:
                p = torch.nn.Parameter(store.p(n), requires_grad=False)
                if store.offsets[n] < store.n_train:
                    p.grad = store.g(n)
                self._param_views[n] = p
        yield from self._param_views.values()
