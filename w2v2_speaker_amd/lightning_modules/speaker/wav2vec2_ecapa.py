"""wav2vec2 encoder + learned layer mix + ECAPA-TDNN back-end as a speaker module (w2v2_speaker_amd/ssl_ecapa.py).

The reference has no such network class; its wav2vec_xvector.py points the same way (a pre-trained front-end into a TDNN
back-end, ``wav2vec_initially_frozen`` / ``num_frozen_steps``).  The surface is that of its neighbours (Wav2vec2FCModule,
EcapaTdnnModule): same config field names where a field is theirs, same method names and argument meaning."""
from __future__ import annotations

import warnings
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from ...config import W2V2Config, Wav2Vec2RegularisationConfig
from ...ecapa import EcapaConfig, EcapaStore, ecapa_min_frames
from ...eval_batching import (DEFAULT_MAX_BATCH, DEFAULT_MAX_BATCH_SAMPLES, DEFAULT_QUANTUM, PlanCache, min_samples,
                              padded_batches)
from ...optim.schedule import OneCycle
from ...params import W2V_PREFIX, ParamStore
from ...ssl_ecapa import LIMITS, SslEcapaPlan, SslEcapaTrainer
from ._optim_surface import EmbeddingEvaluation, OptimizerSurface, prep_waveform_input
from .wav2vec2_fc import SpeakerClassificationDataBatch

MAX_PLANS = 8             # static plans kept per module (LRU)
MAX_BUCKET_PLANS = 12     # plans of compute_speaker_embeddings' length buckets


@dataclass
class Wav2vec2EcapaModuleConfig:
    """The encoder fields of Wav2vec2FCModuleConfig that apply, the fields of EcapaTDNNModuleConfig (its
    ``input_mel_coefficients`` is the encoder's hidden size here and is not a field), and the mix's own."""
    # encoder (ref: wav2vec2_fc.py:48-98)
    wav2vec_hunggingface_id: str = "facebook/wav2vec2-base"
    reset_weights: bool = False
    wav2vec_initially_frozen: bool = True
    num_frozen_steps: Optional[int] = 10000
    completely_freeze_feature_extractor: bool = True
    activation_dropout: float = 0.0
    attention_dropout: float = 0.1
    feat_proj_dropout: float = 0.1
    hidden_dropout: float = 0.1
    layerdrop: float = 0.05
    mask_time_length: int = 10
    mask_time_prob: float = 0.05
    # ECAPA-TDNN (ref: ecapa_tdnn.py:26-48)
    lin_neurons: int = 192
    channels: List[int] = field(default_factory=lambda: [1024, 1024, 1024, 1024, 3072])
    kernel_sizes: List[int] = field(default_factory=lambda: [5, 3, 3, 3, 1])
    dilations: List[int] = field(default_factory=lambda: [1, 2, 3, 4, 1])
    attention_channels: int = 128
    res2net_scale: int = 8
    se_channels: int = 128
    explicit_num_speakers: Optional[int] = None
    # the join
    instance_norm: bool = True
    ssl_lr_factor: float = 1.0


class Wav2vec2EcapaModule(OptimizerSurface, EmbeddingEvaluation):
    def __init__(self, hyperparameters_to_save, cfg: Wav2vec2EcapaModuleConfig, num_speakers: int,
                 loss_fn_constructor: Callable[[], object], validation_pairs=None, test_pairs=None, evaluator=None, *,
                 device="cuda", act_dtype: torch.dtype = torch.bfloat16, ecapa_dtype: torch.dtype = torch.bfloat16,
                 max_lr: float = 1e-3, max_steps: int = 100_000, init_seed: int = 20211, pretrained_state_dict=None,
                 process_group=None, gradient_clip_val: float = 0.0, accumulate_grad_batches: int = 1):
        """Positional arguments: what src/main.py:256-285 passes to every network class.  ``act_dtype`` / ``ecapa_dtype``:
        the encoder's activation format (bf16 or f32; f16 has no training path here) and the ECAPA side's (bf16 or f32).
        ``pretrained_state_dict``: a path or dict of HF wav2vec2 weights for the encoder (Wav2vec2FCModule's keyword).
        The loss is AAM-softmax (or one of its margin heads), as for EcapaTdnnModule."""
        if process_group is not None or accumulate_grad_batches != 1 or gradient_clip_val > 0:
            raise NotImplementedError(LIMITS)
        from ...evaluation.speaker.cosine_distance import CosineDistanceEvaluator
        from ...optim.loss import AngularAdditiveMarginSoftMaxLoss
        loss_fn = loss_fn_constructor()
        if not isinstance(loss_fn, AngularAdditiveMarginSoftMaxLoss):
            raise NotImplementedError(f"loss {type(loss_fn).__name__}: the ECAPA path runs under "
                                      "AngularAdditiveMarginSoftMaxLoss (speechbrain's Classifier + CE is outside it)")
        self.margin, self.scale = float(loss_fn.margin), float(loss_fn.scale)
        sub_centers = int(getattr(loss_fn, "sub_centers", 1))
        self.margin_kw = dict(margin_type=getattr(loss_fn, "margin_type", "arc"),
                              inter_topk=int(getattr(loss_fn, "inter_topk", 0)),
                              inter_margin=float(getattr(loss_fn, "inter_margin", 0.06)))
        del loss_fn
        self.hyperparameters_to_save, self.cfg = hyperparameters_to_save, cfg
        self.encoder_cfg = W2V2Config.from_huggingface_id(cfg.wav2vec_hunggingface_id)
        self.num_speakers = cfg.explicit_num_speakers or num_speakers
        self.embedding_size = cfg.lin_neurons
        self.reg = Wav2Vec2RegularisationConfig(
            activation_dropout=cfg.activation_dropout, attention_dropout=cfg.attention_dropout,
            feat_proj_dropout=cfg.feat_proj_dropout, hidden_dropout=cfg.hidden_dropout, layerdrop=cfg.layerdrop,
            mask_time_length=cfg.mask_time_length, mask_time_prob=cfg.mask_time_prob)
        self.model_cfg = EcapaConfig(self.encoder_cfg.hidden_size, cfg.lin_neurons, tuple(cfg.channels),
                                     tuple(cfg.kernel_sizes), tuple(cfg.dilations), cfg.attention_channels,
                                     cfg.res2net_scale, cfg.se_channels)
        self.enc_store = ParamStore(self.encoder_cfg, device, act_dtype, head=None, num_speakers=1,
                                    freeze_cnn=cfg.completely_freeze_feature_extractor)
        self.enc_store.init_weights(init_seed)
        if pretrained_state_dict is not None:
            sd = (torch.load(pretrained_state_dict, map_location="cpu", weights_only=True)
                  if isinstance(pretrained_state_dict, str) else pretrained_state_dict)
            self.enc_store.load_state_dict(dict(sd), strict=False, prefix_model=True)
        elif not cfg.reset_weights:
            warnings.warn(f"Wav2vec2EcapaModule: reset_weights=False asks for the pretrained {cfg.wav2vec_hunggingface_id!r} "
                          "weights, but none were given (pass pretrained_state_dict=): the encoder starts from a RANDOM "
                          "initialisation", stacklevel=2)
        # ``store`` is the ECAPA-side arena (feature_weight included): what OptimizerSurface's parameter views show
        self.store = EcapaStore(self.model_cfg, device, ecapa_dtype, num_speakers=self.num_speakers, sub_centers=sub_centers,
                                feature_weight=self.encoder_cfg.num_hidden_layers + 1)
        self.store.init_weights(init_seed)
        self.validation_pairs, self.test_pairs = validation_pairs or [], test_pairs or []
        self.evaluator = evaluator or CosineDistanceEvaluator(False, False, 0)
        self.schedule = OneCycle(max_lr=max_lr, total_steps=max_steps)
        self.device = torch.device(device)
        self._trainers: Dict[Tuple, SslEcapaTrainer] = {}
        self._plans = PlanCache(MAX_PLANS, on_evict=lambda key: self._trainers.pop(key, None))
        self._bucket_plans = PlanCache(MAX_BUCKET_PLANS)
        self.steps = 0              # backward passes
        self.schedule_step = 0      # optimiser steps = position in the learning-rate schedule and in the freeze schedule

    @classmethod
    def from_config(cls, cfg: Wav2vec2EcapaModuleConfig, num_speakers: int, aam_margin: float = 0.2, aam_scale: float = 30.0,
                    sub_centers: int = 1, margin_type: str = "arc", inter_topk: int = 0, inter_margin: float = 0.06,
                    **kw) -> "Wav2vec2EcapaModule":
        """Short form for scripts and tests: the AAM loss by its hyper-parameters instead of a constructor."""
        from ...optim.loss import AngularAdditiveMarginSoftMaxLoss, SubCenterMarginSoftMaxLoss
        dev = kw.get("device", "cuda")
        if (sub_centers, margin_type, inter_topk) == (1, "arc", 0):
            ctor = lambda: AngularAdditiveMarginSoftMaxLoss(2, 2, margin=aam_margin, scale=aam_scale, device=dev,
                                                            act_dtype=torch.float32)
        else:      # placeholder sizes, large enough for the loss's own argument check
            ctor = lambda: SubCenterMarginSoftMaxLoss(2, inter_topk + 2, margin=aam_margin, scale=aam_scale,
                                                      sub_centers=sub_centers, margin_type=margin_type, inter_topk=inter_topk,
                                                      inter_margin=inter_margin, device=dev, act_dtype=torch.float32)
        return cls(None, cfg, num_speakers, ctor, kw.pop("validation_pairs", None), kw.pop("test_pairs", None),
                   kw.pop("evaluator", None), **kw)

    # ------------------------------------------------------------------ plans
    def _new_plan(self, batch: int, n: int, train: bool) -> SslEcapaPlan:
        return SslEcapaPlan(self.enc_store, self.store, batch, n, train=train, reg=self.reg,
                            instance_norm=self.cfg.instance_norm, aam_margin=self.margin, aam_scale=self.scale,
                            **self.margin_kw)

    def _plan(self, batch: int, n: int, train: bool) -> SslEcapaPlan:
        return self._plans.lookup((batch, n, train), lambda: self._new_plan(batch, n, train))

    def _new_trainer(self, plan: SslEcapaPlan) -> SslEcapaTrainer:
        return SslEcapaTrainer(plan, self.schedule, ssl_lr_factor=self.cfg.ssl_lr_factor,
                               num_frozen_steps=self.cfg.num_frozen_steps,
                               wav2vec_initially_frozen=self.cfg.wav2vec_initially_frozen, optimizer=self.optimizer_cfg,
                               margin_schedule=self.margin_schedule)

    # ------------------------------------------------------------------ reference surface
    def _prep(self, input_tensor: torch.Tensor) -> torch.Tensor:
        x = prep_waveform_input(input_tensor)
        if x.dim() != 2:
            raise ValueError(f"expected [B, 1, N], [B, N] or [N] audio, got {tuple(input_tensor.shape)}")
        return x.to(self.device, torch.float32).contiguous()

    def min_samples(self) -> int:
        """Fewest samples of an utterance: enough encoder frames for ECAPA's reflect padding."""
        c = self.encoder_cfg
        n = min_samples(c.conv_kernel, c.conv_stride)
        while c.num_frames(n) < ecapa_min_frames(self.model_cfg):
            n += 1
        return n

    def compute_speaker_embedding(self, input_tensor: torch.Tensor) -> torch.Tensor:
        x = self._prep(input_tensor)
        return self._plan(x.shape[0], x.shape[1], False).embed(x).clone()

    def compute_speaker_embeddings(self, waveforms, *, quantum: int = DEFAULT_QUANTUM,
                                   max_batch_samples: int = DEFAULT_MAX_BATCH_SAMPLES,
                                   max_batch: int = DEFAULT_MAX_BATCH) -> List[torch.Tensor]:
        """Embeddings of many utterances of different lengths, batched: one [1, lin_neurons] tensor per waveform ([N] or
        [1, N]), in input order, each equal to ``compute_speaker_embedding`` of that waveform alone.  Bucketed by sample
        count (eval_batching.plan_batches); each batch runs one variable-length forward (SslEcapaPlan.embed(lengths=))."""
        xs = []
        for w in waveforms:
            x = prep_waveform_input(w)
            if x.dim() != 2 or x.shape[0] != 1:
                raise ValueError(f"compute_speaker_embeddings: expected one utterance per waveform, got {tuple(w.shape)}")
            xs.append(x[0])
        out: List[Optional[torch.Tensor]] = [None] * len(xs)
        for idx, wav, lens in padded_batches(xs, quantum, max_batch_samples, max_batch, self.min_samples(), self.device):
            plan = self._bucket_plans.lookup(tuple(wav.shape), lambda: self._new_plan(wav.shape[0], wav.shape[1], False))
            emb = plan.embed(wav, lengths=lens)
            for j, i in enumerate(idx):
                out[i] = emb[j:j + 1].clone()
        return out

    def compute_speaker_prediction(self, embedding_tensor: torch.Tensor) -> torch.Tensor:
        return embedding_tensor.squeeze()                  # under AAM the classifier weight belongs to the loss

    def forward(self, input_tensor: torch.Tensor):
        embedding = self.compute_speaker_embedding(input_tensor)
        return embedding, self.compute_speaker_prediction(embedding)

    __call__ = forward

    def generate_example_input(self, include_batch_dimension: bool, batch_size: Optional[int] = None):
        return torch.rand(size=[batch_size, 16000] if include_batch_dimension else [16000])

    def training_step(self, batch: SpeakerClassificationDataBatch, batch_idx: int = 0, optimizer_idx: Optional[int] = None):
        x, label = self._prep(batch.network_input), batch.ground_truth.to(self.device)
        key = (x.shape[0], x.shape[1])
        loss, pred = self._trainer_step(key, lambda: self._new_trainer(self._plan(key[0], key[1], True)),
                                        lambda tr: tr.train_step(x, label))
        self.steps += 1
        return {"loss": loss, "prediction": pred}

    # ------------------------------------------------------------------ state
    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The encoder under its ``wav2vec.model.*`` names, then the ECAPA arena's: ``feature_extractor.*`` (BatchNorm
        running statistics included), ``feature_weight`` and ``loss_fn.fc_weights``."""
        sd = self.enc_store.state_dict()
        sd.update(self.store.state_dict())
        return sd

    def load_state_dict(self, sd, strict: bool = True) -> None:
        enc = {k: v for k, v in sd.items() if k.startswith(W2V_PREFIX)}
        self.enc_store.load_state_dict(enc, strict=strict, prefix_model=False)
        self.store.load_state_dict({k: v for k, v in sd.items() if k not in enc}, strict=strict)

    def save_checkpoint(self, path: str) -> None:
        torch.save({"state_dict": self.state_dict(), "global_step": self.schedule_step,
                    "w2v2_amd": {"steps": self.steps}}, path)

    def load_checkpoint(self, path: str, strict: bool = True) -> None:
        """Weights, BatchNorm statistics and the schedule / freeze position of save_checkpoint (the optimiser moments
        start afresh)."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        self.load_state_dict(ckpt["state_dict"], strict=strict)
        self.schedule_step = int(ckpt.get("global_step", 0))
        self.steps = int((ckpt.get("w2v2_amd") or {}).get("steps", self.schedule_step))
