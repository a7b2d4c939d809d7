"""Mirror of ``src/lightning_modules/speaker/wav2spk.py`` (Wav2SpkModuleConfig :37-45, Wav2SpkModule :48-299) on the HIP
path (w2v2_speaker_amd/wav2spk.py).  Same config field names, same method names and argument meaning."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from ...eval_batching import DEFAULT_MAX_BATCH, DEFAULT_MAX_BATCH_SAMPLES, DEFAULT_QUANTUM, PlanCache, padded_batches
from ...optim.schedule import OneCycle
from ...wav2spk import (Wav2SpkConfig, Wav2SpkHead, Wav2SpkPlan, Wav2SpkStore, Wav2SpkTrainer, wav2spk_min_samples)
from ._optim_surface import EmbeddingEvaluation, OptimizerSurface, prep_waveform_input
from .wav2vec2_fc import SpeakerClassificationDataBatch

MAX_BUCKET_PLANS = 12     # plans of compute_speaker_embeddings' length buckets (LRU, one per bucket shape)


@dataclass
class Wav2SpkModuleConfig:
    """ref: wav2spk.py:37-45 / config/network/wav2spk.yaml."""
    apply_temporal_gating: bool = True
    hidden_fc_layers_out: List[int] = field(default_factory=lambda: [512, 128])
    embedding_layer_idx: int = 0
    stat_pooling_type: str = "mean+std"


class Wav2SpkModule(OptimizerSurface, EmbeddingEvaluation):
    def __init__(self, hyperparameters_to_save, cfg: Wav2SpkModuleConfig, num_speakers: int,
                 loss_fn_constructor: Callable[[], object], validation_pairs=None, test_pairs=None, evaluator=None, *,
                 device="cuda", act_dtype: torch.dtype = torch.float32, max_lr: float = 1e-3,
                 max_steps: int = 100_000, init_seed: int = 20211, gradient_clip_val: float = 0.0,
                 accumulate_grad_batches: int = 1):
        """Positional arguments = ref: wav2spk.py:49-58 (what src/main.py:256-285 passes to every network class).
        ``loss_fn_constructor`` is called once and read for its type: the path runs under ``CrossEntropyLoss``; an AAM loss
        raises the reference's own ValueError (ref :95-96), anything else (triplet, CTC) NotImplementedError.
        ``act_dtype``: f32 only.  The learning-rate schedule is a OneCycle over ``max_lr`` / ``max_steps`` until
        ``set_lr_schedule`` hands over the reference's ``MultiStepLR`` (config/optim/schedule/schedule_wav2spk.yaml)."""
        from ...evaluation.speaker.cosine_distance import CosineDistanceEvaluator
        from ...optim.loss import AngularAdditiveMarginSoftMaxLoss, CrossEntropyLoss
        loss_fn = loss_fn_constructor()
        if isinstance(loss_fn, AngularAdditiveMarginSoftMaxLoss):
            raise ValueError("wav2spk does not support aam softmax")
        if type(loss_fn) is not CrossEntropyLoss:
            raise NotImplementedError(f"loss {type(loss_fn).__name__}: the wav2spk path runs under CrossEntropyLoss")
        del loss_fn
        if act_dtype != torch.float32:
            raise NotImplementedError("wav2spk: act_dtype=torch.float32 only")
        self.hyperparameters_to_save = hyperparameters_to_save
        self.cfg = cfg
        self.num_speakers = num_speakers
        self.model_cfg = Wav2SpkConfig(cfg.apply_temporal_gating, tuple(cfg.hidden_fc_layers_out), cfg.embedding_layer_idx,
                                       cfg.stat_pooling_type)
        self.embedding_size = self.model_cfg.embedding_size(num_speakers)
        self.stat_pool_dimension = self.model_cfg.pool_dim
        self.store = Wav2SpkStore(self.model_cfg, device, act_dtype, num_speakers=num_speakers)
        self.store.init_weights(init_seed)
        self.validation_pairs, self.test_pairs = validation_pairs or [], test_pairs or []
        self.evaluator = evaluator or CosineDistanceEvaluator(False, False, 0)
        self.schedule = OneCycle(max_lr=max_lr, total_steps=max_steps)
        self.gradient_clip_val = float(gradient_clip_val)      # PL ``trainer.gradient_clip_val`` (global norm, 0 = off)
        self._set_accumulate_grad_batches(accumulate_grad_batches)     # PL ``trainer.accumulate_grad_batches``
        self.device = torch.device(device)
        self._plans = PlanCache()                          # one per (batch, samples, train) shape, all kept
        self._trainers: Dict[Tuple, Wav2SpkTrainer] = {}
        self._bucket_plans = PlanCache(MAX_BUCKET_PLANS)
        self._heads = PlanCache()                          # prediction heads, one per batch size
        self.steps = 0              # backward passes (micro-batches)
        self.schedule_step = 0      # optimiser steps = position in the learning-rate schedule

    @classmethod
    def from_config(cls, cfg: Wav2SpkModuleConfig, num_speakers: int, **kw) -> "Wav2SpkModule":
        """Short form for scripts and tests: the cross-entropy loss without a constructor argument."""
        from ...optim.loss import CrossEntropyLoss
        return cls(None, cfg, num_speakers, CrossEntropyLoss, kw.pop("validation_pairs", None),
                   kw.pop("test_pairs", None), kw.pop("evaluator", None), **kw)

    def _plan(self, batch: int, samples: int, train: bool) -> Wav2SpkPlan:
        return self._plans.lookup((batch, samples, train), lambda: Wav2SpkPlan(self.store, batch, samples, train=train))

    def _bucket_plan(self, batch: int, samples: int) -> Wav2SpkPlan:
        return self._bucket_plans.lookup((batch, samples), lambda: Wav2SpkPlan(self.store, batch, samples, train=False))

    def generate_example_input(self, include_batch_dimension: bool, batch_size: Optional[int] = None):
        # ref :219-233
        return torch.rand(size=[batch_size, 1, 16000] if include_batch_dimension else [1, 16000])

    def _prep_waveform(self, input_tensor: torch.Tensor) -> torch.Tensor:
        """[B, 1, N], [B, N] or [N] audio -> [B, N] f32 on the device."""
        x = prep_waveform_input(input_tensor)
        if x.dim() != 2:
            raise ValueError(f"expected [B, 1, N], [B, N] or [N] audio, got {tuple(input_tensor.shape)}")
        return x.to(self.device, torch.float32).contiguous()

    def compute_speaker_embedding(self, input_tensor: torch.Tensor) -> torch.Tensor:
        # ref :269-292
        x = self._prep_waveform(input_tensor)
        return self._plan(x.shape[0], x.shape[1], False).embed(x).clone()

    def compute_speaker_prediction(self, embedding_tensor: torch.Tensor) -> torch.Tensor:
        """ref :294-299 (_fc_head_ops_post_spk_embedding): the fc layers behind ``embedding_layer_idx`` applied to
        embeddings [B, embedding size] -> log-probabilities [B, speakers] (squeezed)."""
        e = embedding_tensor if embedding_tensor.dim() == 2 else embedding_tensor[None]
        e = e.to(self.device, torch.float32)
        idx, n_hidden = self.model_cfg.embedding_layer_idx, len(self.model_cfg.hidden_fc_layers_out)
        if idx >= n_hidden:                                # the embedding is the log-softmax output: nothing is left to run
            return e.clone().squeeze()
        B = e.shape[0]

        def build():
            pooled = torch.empty(B, self.model_cfg.pool_dim, dtype=torch.float32, device=self.device)
            return Wav2SpkHead(self.store, B, pooled, False)
        head = self._heads.lookup(B, build)
        start = max(idx, -1) + 1                           # the first hidden layer that has not run yet
        head.fc.x[start].copy_(e)
        return head.log_probabilities(from_layer=start).clone().squeeze()

    def compute_speaker_embeddings(self, waveforms, *, quantum: int = DEFAULT_QUANTUM,
                                   max_batch_samples: int = DEFAULT_MAX_BATCH_SAMPLES,
                                   max_batch: int = DEFAULT_MAX_BATCH) -> List[torch.Tensor]:
        """Embeddings of many utterances of different lengths, batched: one [1, embedding size] tensor per waveform ([N] or
        [1, N]), in input order, each equal to ``compute_speaker_embedding`` of that utterance alone.  The utterances are
        bucketed by sample count (eval_batching.plan_batches) and each batch runs one variable-length forward
        (Wav2SpkPlan.embed(..., lengths=))."""
        xs = []
        for w in waveforms:
            x = w[0] if (w.dim() == 2 and w.shape[0] == 1) else w
            if x.dim() != 1:
                raise ValueError(f"compute_speaker_embeddings: expected [N] or [1, N] per utterance, got {tuple(w.shape)}")
            xs.append(x)
        out: List[Optional[torch.Tensor]] = [None] * len(xs)
        for idx, wav, lens in padded_batches(xs, quantum, max_batch_samples, max_batch, wav2spk_min_samples(), self.device):
            emb = self._bucket_plan(*wav.shape).embed(wav, lengths=lens)
            for j, i in enumerate(idx):
                out[i] = emb[j:j + 1].clone()
        return out

    def forward(self, input_tensor: torch.Tensor):
        embedding = self.compute_speaker_embedding(input_tensor)
        return embedding, self.compute_speaker_prediction(embedding)

    __call__ = forward

    def training_step(self, batch: SpeakerClassificationDataBatch, batch_idx: int = 0,
                      optimizer_idx: Optional[int] = None):
        x = self._prep_waveform(batch.network_input)
        label = batch.ground_truth.to(self.device)
        key = (x.shape[0], x.shape[1])
        loss, pred = self._trainer_step(
            key, lambda: Wav2SpkTrainer(self.store, self._plan(key[0], key[1], True), self.schedule,
                                        **self._trainer_options()),
            lambda tr: tr.train_step(x, label))
        self.steps += 1
        return {"loss": loss, "prediction": pred}

    def state_dict(self):
        return self.store.state_dict()

    def load_state_dict(self, sd, strict: bool = True):
        self.store.load_state_dict(sd, strict=strict)

    def save_checkpoint(self, path: str) -> None:
        """The weights under the reference's state-dict names and the schedule position, in a PL-style dict."""
        if self.store.accum_count > 0:
            raise RuntimeError("an accumulation window is open: flush it first (on_train_epoch_end())")
        torch.save({"state_dict": self.state_dict(), "global_step": self.schedule_step,
                    "w2v2_amd": {"steps": self.steps}}, path)

    def load_checkpoint(self, path: str, strict: bool = True) -> None:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        self.load_state_dict(ckpt["state_dict"], strict=strict)
        self.schedule_step = int(ckpt.get("global_step", 0))
        self.steps = int((ckpt.get("w2v2_amd") or {}).get("steps", self.schedule_step))
