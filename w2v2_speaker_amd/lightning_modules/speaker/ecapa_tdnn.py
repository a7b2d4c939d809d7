"""Mirror of ``src/lightning_modules/speaker/ecapa_tdnn.py`` (EcapaTDNNModuleConfig :26-48, EcapaTdnnModule :51-137)
on the HIP path (w2v2_speaker_amd/ecapa.py).  Same config field names, same method names and argument meaning."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from ...ecapa import EcapaConfig, EcapaPlan, EcapaStore, EcapaTrainer, ecapa_min_frames, fbank_frames
from ...eval_batching import (DEFAULT_FRAME_QUANTUM, DEFAULT_MAX_BATCH, DEFAULT_MAX_BATCH_FRAMES, PlanCache,
                              padded_batches)
from ...optim.schedule import OneCycle
from ._optim_surface import EmbeddingEvaluation, OptimizerSurface, prep_waveform_input
from ...ops import FBANK_HOP
from .wav2vec2_fc import SpeakerClassificationDataBatch

MAX_BUCKET_PLANS = 12     # plans of compute_speaker_embeddings' length buckets (LRU, one per bucket shape)


@dataclass
class EcapaTDNNModuleConfig:
    """ref: ecapa_tdnn.py:26-48 / config/network/ecapa_tdnn.yaml."""
    input_mel_coefficients: int = 40
    lin_neurons: int = 192
    channels: List[int] = field(default_factory=lambda: [1024, 1024, 1024, 1024, 3072])
    kernel_sizes: List[int] = field(default_factory=lambda: [5, 3, 3, 3, 1])
    dilations: List[int] = field(default_factory=lambda: [1, 2, 3, 4, 1])
    attention_channels: int = 128
    res2net_scale: int = 8
    se_channels: int = 128
    global_context: bool = True
    pretrained_weights_path: Optional[str] = None
    explicit_stat_pool_embedding_size: Optional[int] = None
    explicit_num_speakers: Optional[int] = None


class FilterbankSpeakerModule(OptimizerSurface, EmbeddingEvaluation):
    """What the modules of the two filterbank models (EcapaTdnnModule, xvector.XVectorModule) share: the input forms, the
    plan caches, the batched variable-length evaluation and ``training_step``.  A module sets ``cfg``, ``model_cfg`` (with
    ``input_mel_coefficients``, ``kernel_sizes``, ``dilations``), ``store``, and supplies ``_new_plan(batch, frames,
    train)`` and ``_new_trainer(plan)``."""

    def _init_runtime(self, device, input_features: str, validation_pairs, test_pairs, evaluator, max_lr: float,
                      max_steps: int, gradient_clip_val: float, accumulate_grad_batches: int, augmenter=None) -> None:
        from ...evaluation.speaker.cosine_distance import CosineDistanceEvaluator
        self.input_features = input_features
        self.augmenter = augmenter                         # data.augment.Augmenter or None: training_step's first stage
        self.validation_pairs, self.test_pairs = validation_pairs or [], test_pairs or []
        self.evaluator = evaluator or CosineDistanceEvaluator(False, False, 0)
        self.schedule = OneCycle(max_lr=max_lr, total_steps=max_steps)
        self.gradient_clip_val = float(gradient_clip_val)      # PL ``trainer.gradient_clip_val`` (global norm, 0 = off)
        self._set_accumulate_grad_batches(accumulate_grad_batches)     # PL ``trainer.accumulate_grad_batches``
        self.device = torch.device(device)
        self._plans = PlanCache()                          # one per (batch, frames, train) shape, all kept
        self._trainers: Dict[Tuple, EcapaTrainer] = {}
        self._bucket_plans = PlanCache(MAX_BUCKET_PLANS)
        self.steps = 0              # backward passes (micro-batches)
        self.schedule_step = 0      # optimiser steps = position in the learning-rate schedule

    @staticmethod
    def _check_input_features(input_features: str) -> None:
        if input_features not in ("fbank", "waveform"):
            raise ValueError(f"input_features: 'fbank' or 'waveform', got {input_features!r}")

    @staticmethod
    def _check_augmenter(augmenter, input_features: str) -> None:
        """The augmenter works on waveforms (the reference's pipeline order: selector -> augmenter -> filterbank)."""
        if augmenter is not None and input_features != "waveform":
            raise ValueError(f"augmenter= needs input_features='waveform' (the augmenter runs in front of the filterbank), "
                             f"got input_features={input_features!r}")
        if augmenter is not None and not hasattr(augmenter, "process_batch"):
            raise ValueError("augmenter= is a data.augment.Augmenter (or None)")

    def _plan(self, batch: int, frames: int, train: bool):
        return self._plans.lookup((batch, frames, train), lambda: self._new_plan(batch, frames, train))

    def generate_example_input(self, include_batch_dimension: bool, batch_size: Optional[int] = None):
        # ref :97-108: [BATCH_SIZE, NUMBER_OF_WINDOWS, NUMBER_OF_MEL_COEFFICIENTS]
        shape = [batch_size, 100, self.model_cfg.input_mel_coefficients] if include_batch_dimension else \
            [100, self.model_cfg.input_mel_coefficients]
        return torch.rand(size=shape)

    def compute_speaker_embedding(self, input_tensor: torch.Tensor) -> torch.Tensor:
        # ref :110-118
        if self.input_features == "waveform":
            x = self._prep_waveform(input_tensor)
            return self._plan(x.shape[0], fbank_frames(x.shape[1]), False).embed_waveform(x).clone()
        x = input_tensor if input_tensor.dim() == 3 else input_tensor[None]
        x = x.to(self.device, torch.float32)
        return self._plan(x.shape[0], x.shape[1], False).embed(x).clone()

    def _prep_waveform(self, input_tensor: torch.Tensor) -> torch.Tensor:
        """[B, 1, N], [B, N] or [N] audio -> [B, N] f32 on the device (Wav2vec2FCModule's input forms)."""
        x = prep_waveform_input(input_tensor)
        if x.dim() != 2:
            raise ValueError(f"expected [B, 1, N], [B, N] or [N] audio, got {tuple(input_tensor.shape)}")
        return x.to(self.device, torch.float32).contiguous()

    def _bucket_plan(self, batch: int, frames: int):
        return self._bucket_plans.lookup((batch, frames), lambda: self._new_plan(batch, frames, False))

    def compute_speaker_embeddings(self, feats, *, quantum: int = DEFAULT_FRAME_QUANTUM,
                                   max_batch_frames: int = DEFAULT_MAX_BATCH_FRAMES,
                                   max_batch: int = DEFAULT_MAX_BATCH) -> List[torch.Tensor]:
        """Embeddings of many utterances of different lengths, batched: one [1, lin_neurons] tensor per filterbank tensor
        ([T, n_mels] or [1, T, n_mels]), in input order, each equal to ``compute_speaker_embedding`` of that utterance
        alone.  The utterances are bucketed by frame count (eval_batching.plan_batches, lengths in frames) and each batch
        runs one variable-length forward (EcapaPlan.embed(..., lengths=)).
        ``input_features="waveform"``: one waveform ([N] or [1, N]) per utterance, bucketed by SAMPLE count with the same
        policy in units of the 160-sample hop (``quantum`` and ``max_batch_frames`` are multiplied by 160), each batch one
        EcapaPlan.embed_waveform(..., lengths=)."""
        if self.input_features == "waveform":
            return self._waveform_embeddings(feats, quantum, max_batch_frames, max_batch)
        F_ = self.model_cfg.input_mel_coefficients
        xs = []
        for f in feats:
            x = f[0] if (f.dim() == 3 and f.shape[0] == 1) else f
            if x.dim() != 2 or x.shape[1] != F_:
                raise ValueError(f"compute_speaker_embeddings: expected [T, {F_}] or [1, T, {F_}] per utterance, got "
                                 f"{tuple(f.shape)}")
            xs.append(x)
        out: List[Optional[torch.Tensor]] = [None] * len(xs)
        fill = ecapa_min_frames(self.model_cfg)
        for idx, feat, lens in padded_batches(xs, quantum, max_batch_frames, max_batch, fill, self.device):
            emb = self._bucket_plan(*feat.shape[:2]).embed(feat, lengths=lens)
            for j, i in enumerate(idx):
                out[i] = emb[j:j + 1].clone()
        return out

    def _waveform_embeddings(self, wavs, quantum: int, max_batch_frames: int, max_batch: int) -> List[torch.Tensor]:
        xs = []
        for w in wavs:
            x = w[0] if (w.dim() == 2 and w.shape[0] == 1) else w
            if x.dim() != 1:
                raise ValueError(f"compute_speaker_embeddings: expected [N] or [1, N] per utterance, got {tuple(w.shape)}")
            xs.append(x)
        out: List[Optional[torch.Tensor]] = [None] * len(xs)
        fill = (ecapa_min_frames(self.model_cfg) - 1) * FBANK_HOP      # fewest samples with the minimum frame count
        for idx, wav, lens in padded_batches(xs, quantum * FBANK_HOP, max_batch_frames * FBANK_HOP, max_batch, fill,
                                             self.device):
            emb = self._bucket_plan(wav.shape[0], fbank_frames(wav.shape[1])).embed_waveform(wav, lengths=lens)
            for j, i in enumerate(idx):
                out[i] = emb[j:j + 1].clone()
        return out

    def forward(self, input_tensor: torch.Tensor):
        embedding = self.compute_speaker_embedding(input_tensor)
        return embedding, self.compute_speaker_prediction(embedding)

    __call__ = forward

    def training_step(self, batch: SpeakerClassificationDataBatch, batch_idx: int = 0,
                      optimizer_idx: Optional[int] = None):
        label = batch.ground_truth.to(self.device)
        if self.input_features == "waveform":
            x = self._prep_waveform(batch.network_input)
            if self.augmenter is not None:                 # [B, N] -> [B', N'] on the device; the plan is built for B', N'
                aug = self.augmenter.process_batch(x, label, keys=getattr(batch, "keys", None))
                x, label = aug.network_input, aug.ground_truth
            key = (x.shape[0], fbank_frames(x.shape[1]))
        else:
            x = batch.network_input.to(self.device, torch.float32)
            key = (x.shape[0], x.shape[1])
        loss, pred = self._trainer_step(
            key, lambda: self._new_trainer(self._plan(key[0], key[1], True)),
            lambda tr: tr.train_step(x, label))
        self.steps += 1
        return {"loss": loss, "prediction": pred}

    def state_dict(self):
        return self.store.state_dict()

    def load_state_dict(self, sd, strict: bool = True):
        self.store.load_state_dict(sd, strict=strict)


class EcapaTdnnModule(FilterbankSpeakerModule):
    def __init__(self, hyperparameters_to_save, cfg: EcapaTDNNModuleConfig, num_speakers: int,
                 loss_fn_constructor: Callable[[], object], validation_pairs=None, test_pairs=None, evaluator=None, *,
                 device="cuda", act_dtype: torch.dtype = torch.bfloat16, max_lr: float = 1e-3,
                 max_steps: int = 100_000, init_seed: int = 20211, gradient_clip_val: float = 0.0,
                 accumulate_grad_batches: int = 1, input_features: str = "fbank", augmenter=None):
        """Positional arguments = ref: ecapa_tdnn.py:51-62 (what src/main.py:256-285 passes to every network class).
        ``loss_fn_constructor`` is called once and read for its type and hyper-parameters: the engine runs the ECAPA
        model under AAM-softmax (``skip_classifier`` of ref :93-95; the paper's configuration,
        config/experiment/speaker_ecapa_tdnn.yaml) -- the cross-entropy + cosine ``Classifier`` variant is not on the
        path.  ``act_dtype=torch.float32`` is the reference's own precision for this model (``precision: 32``).
        ``input_features``: "fbank" -- inputs are [B, T, n_mels] filterbank tensors, the output of the reference's
        ``filterbank`` + ``normalizer`` pipeline stages (data/fbank.py, InputNormalizer2D) -- or "waveform": inputs are
        what the ``selector`` stage delivers ([B, 1, N], [B, N] or [N] audio) and the two stages run on the device
        (EcapaPlan.embed_waveform).  ``augmenter``: a data.augment.Augmenter that ``training_step`` runs on the waveforms
        in front of the filterbank (the reference's `augmenter` pipeline stage); "waveform" inputs only."""
        self._check_input_features(input_features)
        self._check_augmenter(augmenter, input_features)
        from ...optim.loss import AngularAdditiveMarginSoftMaxLoss
        loss_fn = loss_fn_constructor()
        if not isinstance(loss_fn, AngularAdditiveMarginSoftMaxLoss):
            raise NotImplementedError(f"loss {type(loss_fn).__name__}: the ECAPA path runs under "
                                      "AngularAdditiveMarginSoftMaxLoss (speechbrain's Classifier + CE is outside it)")
        aam_margin, aam_scale = float(loss_fn.margin), float(loss_fn.scale)
        # the margin heads (optim.loss.SubCenterMarginSoftMaxLoss); a plain AAM loss has none of the attributes
        sub_centers = int(getattr(loss_fn, "sub_centers", 1))
        self.margin_kw = dict(margin_type=getattr(loss_fn, "margin_type", "arc"),
                              inter_topk=int(getattr(loss_fn, "inter_topk", 0)),
                              inter_margin=float(getattr(loss_fn, "inter_margin", 0.06)))
        del loss_fn
        self.hyperparameters_to_save = hyperparameters_to_save
        if not cfg.global_context:
            raise NotImplementedError("global_context=False (the reference config sets True)")
        self.cfg = cfg
        self.embedding_size = cfg.lin_neurons
        self.num_speakers = cfg.explicit_num_speakers or num_speakers
        self.model_cfg = EcapaConfig(cfg.input_mel_coefficients, cfg.lin_neurons, tuple(cfg.channels),
                                     tuple(cfg.kernel_sizes), tuple(cfg.dilations), cfg.attention_channels,
                                     cfg.res2net_scale, cfg.se_channels)
        self.store = EcapaStore(self.model_cfg, device, act_dtype, num_speakers=self.num_speakers,
                                sub_centers=sub_centers)
        self.store.init_weights(init_seed)
        if cfg.pretrained_weights_path is not None:       # ref :88-91: a bare ECAPA_TDNN state dict
            sd = torch.load(cfg.pretrained_weights_path, map_location="cpu", weights_only=True)
            self.store.load_state_dict(dict(sd), strict=False)    # incl. every BatchNorm running_mean / running_var
        self.margin, self.scale = aam_margin, aam_scale
        self.skip_classifier = True                        # AAM owns the classifier weight (ref :93-95, :129-131)
        self._init_runtime(device, input_features, validation_pairs, test_pairs, evaluator, max_lr, max_steps,
                           gradient_clip_val, accumulate_grad_batches, augmenter)

    @classmethod
    def from_config(cls, cfg: EcapaTDNNModuleConfig, num_speakers: int, aam_margin: float = 0.2,
                    aam_scale: float = 30.0, sub_centers: int = 1, margin_type: str = "arc", inter_topk: int = 0,
                    inter_margin: float = 0.06, **kw) -> "EcapaTdnnModule":
        """Short form for scripts and tests: the AAM loss by its hyper-parameters instead of a constructor (the last
        four: the margin heads of optim.loss.SubCenterMarginSoftMaxLoss)."""
        from ...optim.loss import AngularAdditiveMarginSoftMaxLoss, SubCenterMarginSoftMaxLoss
        dev = kw.get("device", "cuda")
        if (sub_centers, margin_type, inter_topk) == (1, "arc", 0):
            ctor = lambda: AngularAdditiveMarginSoftMaxLoss(2, 2, margin=aam_margin, scale=aam_scale, device=dev,
                                                            act_dtype=torch.float32)
        else:      # placeholder sizes, large enough for the loss's own argument check
            ctor = lambda: SubCenterMarginSoftMaxLoss(2, inter_topk + 2, margin=aam_margin, scale=aam_scale,
                                                      sub_centers=sub_centers, margin_type=margin_type,
                                                      inter_topk=inter_topk, inter_margin=inter_margin, device=dev,
                                                      act_dtype=torch.float32)
        return cls(None, cfg, num_speakers, ctor, kw.pop("validation_pairs", None), kw.pop("test_pairs", None),
                   kw.pop("evaluator", None), **kw)

    def _new_plan(self, batch: int, frames: int, train: bool) -> EcapaPlan:
        return EcapaPlan(self.store, batch, frames, train=train, aam_margin=self.margin, aam_scale=self.scale,
                         **self.margin_kw)

    def _new_trainer(self, plan: EcapaPlan) -> EcapaTrainer:
        return EcapaTrainer(self.store, plan, self.schedule, margin_schedule=self.margin_schedule,
                            **self._trainer_options())

    def compute_speaker_prediction(self, embedding_tensor: torch.Tensor) -> torch.Tensor:
        return embedding_tensor.squeeze()                  # ref :120-122 under AAM
