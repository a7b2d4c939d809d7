"""``set_optimizer`` / ``set_lr_schedule`` / ``configure_optimizers`` of the reference's ``BaseLightningModule`` (ref:
src/lightning_modules/base_lightning_module.py:58-62,70-75), shared by the three speaker modules.  The reference builds a
torch optimiser and scheduler over ``network.parameters()`` from its configuration and hands them to the module (ref:
src/main.py:323-335); here the two objects are READ -- class and first param group through ``OptimConfig.from_torch``,
the scheduler through ``schedule.from_torch_scheduler`` -- and the fused step runs what they describe.  The torch
optimiser itself is never stepped (manual optimisation, see Wav2vec2FCModule).

Next to it the other pieces the modules share: the trainer-per-plan-shape step of ``training_step``, the waveform
input forms, and (EmbeddingEvaluation) the evaluation surface of the two modules that score trials by embeddings."""
from __future__ import annotations

from typing import Callable, List, Optional

import torch

from ...evaluation.speaker.cosine_distance import EmbeddingSample
from ...optim import OptimConfig
from ...optim.schedule import from_torch_scheduler


def prep_waveform_input(input_tensor: torch.Tensor) -> torch.Tensor:
    # ref: wav2vec2_fc.py:414-421 -- [BS,1,N] or [1,N] or [N] -> [BS,N]
    if len(input_tensor.shape) == 3 and input_tensor.shape[1] == 1:
        input_tensor = input_tensor[:, 0, :]
    if len(input_tensor.shape) == 1:
        input_tensor = torch.stack([input_tensor])
    return input_tensor


class OptimizerSurface:
    optimizer_cfg: Optional[OptimConfig] = None      # None: the fused Adam the modules always ran
    gradient_clip_val: float = 0.0                   # PL ``trainer.gradient_clip_val`` (constructor keyword)
    accumulate_grad_batches: int = 1                 # PL ``trainer.accumulate_grad_batches`` (constructor keyword)
    schedule_step: int = 0                           # optimiser steps taken = position in the learning-rate schedule
    _window_trainer = None                           # the trainer whose calls opened the accumulation window
    _torch_optimizer = None
    _torch_schedule = None
    margin_schedule = None                           # optim.schedule.MarginSchedule of the AAM head's margin, or None

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

    def set_margin_schedule(self, schedule) -> None:
        """An ``optim.schedule.MarginSchedule`` (any callable optimiser step -> margin), or None: the trainers write its
        value to the AAM head before each micro-batch.  Derived from the step count: a checkpoint needs nothing new."""
        self.margin_schedule = schedule
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

    def _trainer_step(self, key, build: Callable, run: Callable):
        """One ``training_step`` call on the trainer of plan shape ``key`` (``build()`` makes it on first use; the module
        keeps one per shape over its one store): ``run(trainer)`` at the module's schedule position."""
        tr = self._trainers.get(key)
        if tr is None:
            tr = self._trainers[key] = build()
        tr.step = self.schedule_step
        out = run(tr)
        self._after_micro_batch(tr)
        return out

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

    def _parameter_views(self) -> dict:
        """name -> one ``nn.Parameter`` view of the flat arena per parameter (``.grad`` = the matching gradient view), so
        that the reference's ``instantiate(cfg.optim.algo, params=network.parameters())`` has something to hold."""
        if getattr(self, "_param_views", None) is None:
            store = self.store
            # reference registration order where the store knows it (the speaker heads of ParamStore), arena order else
            names = (store.reference_parameter_order() if getattr(store, "head", None) in ("aam", "ce", "triplet", "triplet_ce")
                     else list(store.shapes))
            self._param_views = {}
            for n in names:
                p = torch.nn.Parameter(store.p(n), requires_grad=False)
                if store.offsets[n] < store.n_train:
                    p.grad = store.g(n)
                self._param_views[n] = p
        return self._param_views

    def parameters(self, recurse: bool = True):
        yield from self._parameter_views().values()


class EmbeddingEvaluation:
    """Validation / test surface of the modules whose trials are scored by the cosine of two speaker embeddings
    (Wav2vec2FCModule, EcapaTdnnModule; ref: speaker_recognition_module.py:451-519) over their
    ``compute_speaker_embedding(s)``, ``evaluator`` and ``validation_pairs`` / ``test_pairs``."""

    def validation_step(self, batch, batch_idx: int = 0):
        emb = self.compute_speaker_embedding(batch.network_input)
        return {"embedding": emb.detach().to("cpu"), "sample_id": batch.keys}

    def test_step(self, batch, batch_idx: int = 0):
        if batch.batch_size != 1:
            raise ValueError("expecting a batch size of 1 for evaluating speaker embeddings")   # ref: :468-469
        return self.validation_step(batch, batch_idx)

    def _evaluate_embeddings(self, outputs: List[dict], pairs, score_norm=None, calibration=None, llr_metrics=False):
        samples = [EmbeddingSample(sample_id=k, embedding=o["embedding"][i]) for o in outputs
                   for i, k in enumerate(o["sample_id"])]
        extra = {} if score_norm is None else {"score_norm": score_norm}
        if calibration is not None or llr_metrics:
            extra.update(calibration=calibration, llr_metrics=llr_metrics)
        return self.evaluator.evaluate(pairs, samples, **extra)

    def validation_epoch_end(self, outputs: List[dict]):
        return self._evaluate_embeddings(outputs, self.validation_pairs)

    def test_epoch_end(self, outputs: List[dict]):
        return self._evaluate_embeddings(outputs, self.test_pairs)

    def evaluate_trials(self, pairs, input_by_key, *, scoring: str = "host", metrics: str = "host", score_norm=None,
                        calibration=None, llr_metrics: bool = False, **batching) -> dict:
        """Score a trial list: every utterance the pairs name (key -> one input of compute_speaker_embeddings in
        ``input_by_key``) is embedded once with compute_speaker_embeddings (``batching``: its keyword arguments) and the
        module's evaluator scores the pairs -- the same dict as test_epoch_end over the batch-size-1 test loop.
        ``scoring="device"``: the embeddings stay on the device as one bank and the evaluator's ``evaluate_bank`` scores
        it there (pooled embeddings only).  ``metrics="device"`` (with ``scoring="device"`` only): EER / minDCF are
        computed on the device as well (``evaluate_bank_metrics(metrics="device")``) and eight doubles come back.
        ``score_norm`` (evaluation.speaker.device_scoring.ScoreNorm): the scores are normalised with its cohort, on the
        device with ``scoring="device"`` and in plain torch on the CPU otherwise.  ``calibration``
        (evaluation.speaker.calibration.ScoreCalibration, fitted) / ``llr_metrics``: the evaluator's keywords of the same
        name -- calibrated llrs go to the metrics and the dict gains cllr, act_dcf, act_p_miss and act_p_fa; on the device
        with ``scoring="device"``, in float64 numpy otherwise."""
        if scoring not in ("host", "device"):
            raise ValueError(f"scoring={scoring!r}: 'host' or 'device'")
        if metrics not in ("host", "device"):
            raise ValueError(f"metrics={metrics!r}: 'host' or 'device'")
        if metrics == "device" and scoring != "device":
            raise ValueError("metrics='device' needs scoring='device': the host path has no scores on the device")
        keys = sorted({k for p in pairs for k in (p.sample1_id, p.sample2_id)})
        embs = self.compute_speaker_embeddings([input_by_key[k] for k in keys], **batching)
        if scoring == "device":
            if embs[0].dim() != 2:
                raise NotImplementedError("scoring='device' takes pooled embeddings; score a no-pooling head's frames with "
                                          "evaluator.evaluate_bank(frame_offsets=)")
            extra = {} if score_norm is None else {"score_norm": score_norm}
            if calibration is not None or llr_metrics:
                extra.update(calibration=calibration, llr_metrics=llr_metrics)
            return self.evaluator.evaluate_bank_metrics(pairs, keys, torch.cat(embs).detach().float(), metrics=metrics, **extra)
        return self._evaluate_embeddings([{"embedding": torch.cat(embs).detach().to("cpu"), "sample_id": keys}], pairs,
                                         score_norm, calibration, llr_metrics)

    @property
    def bucket_plans_built(self) -> int:
        """Plans compute_speaker_embeddings has built for its length buckets."""
        return self._bucket_plans.built
