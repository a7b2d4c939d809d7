"""Mirror of ``src/lightning_modules/speaker/wav2vec2_paired_input.py`` (Wav2vec2PairedSpeakerModuleConfig :27-67,
Wav2vec2PairedSpeakerModule :70-207) + ``paired_speaker_recognition_module.py:60-140`` on the HIP path
(engine.Plan(paired=True), heads.BceHead).

Evaluation (ref: paired_speaker_recognition_module.py:115-248): the step hooks and ``_evaluate`` follow the reference;
``score_trials`` / ``evaluate_trials`` score a whole trial list batched -- every utterance goes through the conv stack once
(Plan.features) into a device feature bank, and the trials, bucketed by their total frames, run through encoder-only plans
(Plan.pair_encoder) that assemble [CLS] left [SEP] right [SEP] from rows of the bank."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from ...config import W2V2Config, Wav2Vec2RegularisationConfig
from ...engine import Plan
from ...eval_batching import (DEFAULT_MAX_BATCH, DEFAULT_MAX_PAIR_BATCH_FRAMES, DEFAULT_PAIR_QUANTUM, DEFAULT_QUANTUM,
                              PlanCache, min_samples, padded_batches, plan_pair_batches)
from ...eval_metrics import calculate_eer, calculate_mdc
from ...optim.schedule import OneCycle
from ._optim_surface import OptimizerSurface
from ...params import ParamStore
from ...trainer import SpeakerTrainer


# plans kept per LRU.  Feature buckets and the variable-length equality plans hold a conv stack (as the bucket plans of
# wav2vec2_fc.py); the encoder-only trial plans are much smaller and their buckets span twice the length range
MAX_BUCKET_PLANS = {"equality": 12, "features": 12, "pairs": 32}
EQUALITY_QUANTUM = DEFAULT_QUANTUM   # compute_speaker_equality at unequal lengths: plan length rounded up to 2 s
DEFAULT_MAX_BANK_BYTES = 8 << 30     # score_trials' feature bank: VoxCeleb1-O in fp16 is about 3 GB of the 288 GB


@dataclass
class Wav2vec2PairedSpeakerModuleConfig:
    """ref: wav2vec2_paired_input.py:27-67 (same field names, incl. the reference's spelling)."""
    wav2vec_hunggingface_id: str = "facebook/wav2vec2-base"
    reset_weights: bool = True
    wav2vec_initially_frozen: bool = False
    num_frozen_steps: Optional[int] = None
    completely_freeze_feature_extractor: bool = True
    completely_freeze_feature_projector: bool = False
    cls_token_constant: float = 1
    sep_token_constant: float = -1
    activation_dropout: float = 0.0
    attention_dropout: float = 0.1
    feat_proj_dropout: float = 0.1
    hidden_dropout: float = 0.1
    layerdrop: float = 0.05
    mask_feature_length: int = 10
    mask_feature_prob: float = 0.0
    mask_time_length: int = 10
    mask_time_prob: float = 0.05
    final_channel_mask_prob: float = 0.0
    final_channel_mask_width: int = 0


@dataclass
class PairedSpeakerClassificationDataBatch:
    """ref: src/data/modules/speaker/training_batch_speaker.py (paired batch): two waveforms per pair + {0,1} label."""
    batch_size: int
    primary_keys: List[str]
    primary_network_input: torch.Tensor
    secondary_keys: List[str]
    secondary_network_input: torch.Tensor
    ground_truth: torch.Tensor


class Wav2vec2PairedSpeakerModule(OptimizerSurface):
    def __init__(self, hyperparameters_to_save, cfg: Wav2vec2PairedSpeakerModuleConfig,
                 loss_fn_constructor: Optional[Callable[[], object]] = None, *, device="cuda",
                 act_dtype: torch.dtype = torch.float16, max_lr: float = 5e-5, max_steps: int = 100_000,
                 process_group=None, init_seed: int = 20211, gradient_clip_val: float = 0.0,
                 accumulate_grad_batches: int = 1):
        """Positional arguments = ref: wav2vec2_paired_input.py:65-71.  ``loss_fn_constructor`` must build the
        reference's ``BinaryCrossEntropyLoss`` (src/optim/loss/binary_cross_entropy.py; the only loss this module is
        configured with, config/optim/loss/binary_cross_entropy.yaml) -- it is called once and checked; the arithmetic
        runs in w2v2_bce_head_fwd_bwd.  Default precision: fp16 operands under the dynamic loss scale, like
        Wav2vec2FCModule (the reference's ``precision: 16``)."""
        if cfg.wav2vec_initially_frozen or cfg.completely_freeze_feature_projector:
            raise NotImplementedError("initially-frozen network / frozen projector for the paired module")
        if loss_fn_constructor is not None:
            from ...optim.loss import BinaryCrossEntropyLoss
            loss_fn = loss_fn_constructor()
            if not isinstance(loss_fn, BinaryCrossEntropyLoss):
                raise NotImplementedError(f"loss {type(loss_fn).__name__}: the paired module trains with "
                                          "BinaryCrossEntropyLoss")
        self.hyperparameters_to_save = hyperparameters_to_save
        self.cfg = cfg
        self.model_cfg = W2V2Config.from_huggingface_id(cfg.wav2vec_hunggingface_id)
        self.reg = Wav2Vec2RegularisationConfig(
            activation_dropout=cfg.activation_dropout, attention_dropout=cfg.attention_dropout,
            feat_proj_dropout=cfg.feat_proj_dropout, hidden_dropout=cfg.hidden_dropout, layerdrop=cfg.layerdrop,
            mask_feature_length=cfg.mask_feature_length, mask_feature_prob=cfg.mask_feature_prob,
            mask_time_length=cfg.mask_time_length, mask_time_prob=cfg.mask_time_prob)
        self.store = ParamStore(self.model_cfg, device, act_dtype, head="bce",
                                freeze_cnn=cfg.completely_freeze_feature_extractor)
        self.store.init_weights(init_seed)
        self.schedule = OneCycle(max_lr=max_lr, total_steps=max_steps)
        self.gradient_clip_val = float(gradient_clip_val)      # PL ``trainer.gradient_clip_val`` (global norm, 0 = off)
        self._set_accumulate_grad_batches(accumulate_grad_batches)     # PL ``trainer.accumulate_grad_batches``
        self.process_group = process_group
        self.device = torch.device(device)
        self._plans = PlanCache()                          # one per (batch, samples, train) shape, all kept
        self._trainers: Dict[Tuple, SpeakerTrainer] = {}
        # evaluation plans, one bounded LRU each: variable-length equality plans (batch, samples), feature plans of
        # score_trials (batch, samples), encoder-only trial plans (batch, frames)
        self._lru: Dict[str, PlanCache] = {k: PlanCache(n) for k, n in MAX_BUCKET_PLANS.items()}
        self.last_bank_bytes = 0
        self.steps = 0              # backward passes (micro-batches)
        self.schedule_step = 0      # optimiser steps = position in the learning-rate schedule

    def _get_wav2vec2_embedding_size(self):
        return self.model_cfg.hidden_size                   # ref :112-118 (768 / 1024)

    def generate_example_input(self, include_batch_dimension: bool, batch_size: Optional[int] = None):
        shape = [batch_size, 16000] if include_batch_dimension else [16000]
        return torch.rand(size=shape), torch.rand(size=shape)

    def _plan(self, batch: int, n: int, train: bool) -> Plan:
        return self._plans.lookup((batch, n, train), lambda: Plan(
            self.store, batch, n, train=train, reg=self.reg, pooling="first", paired=True,
            cls_token_constant=self.cfg.cls_token_constant, sep_token_constant=self.cfg.sep_token_constant))

    @property
    def bucket_plans_built(self) -> int:
        """Plans built by the three evaluation caches together."""
        return sum(c.built for c in self._lru.values())

    @staticmethod
    def _sq(x: torch.Tensor) -> torch.Tensor:
        return x[:, 0, :] if x.dim() == 3 else (x[None] if x.dim() == 1 else x)

    @classmethod
    def _stack(cls, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        a, b = cls._sq(a), cls._sq(b)
        assert a.shape == b.shape                          # ref :166-168
        return torch.cat([a, b], dim=0)

    def _logits(self, emb: torch.Tensor) -> torch.Tensor:
        """ref :205 ``self.linear(cls_token)``: emb [B, H] f32 -> [B, 1]."""
        from ... import ops
        B, H = emb.shape
        out = torch.zeros(B, 4, dtype=torch.float32, device=self.device)          # ldc padded to 4
        ops.gemm(B, 1, H, emb, self.store.p("linear.weight"), out, lda=H, ldb=H, ldc=4, epilogue=ops.EPI_BIAS,
                 bias=self.store.p("linear.bias"))
        return out[:, :1]

    def compute_speaker_equality(self, wav_tensor: torch.Tensor, other_wav_tensor: torch.Tensor,
                                 lengths=None) -> torch.Tensor:
        """ref :163-207 -> equality logits [B, 1] (eval-mode forward).  [B, N] and [B, M] with N != M are accepted, as the
        reference's contract says (paired_speaker_recognition_module.py:51-60): the shorter side is padded and each side's
        full length is its valid length.  ``lengths=(left, right)``: valid samples per pair of a padded batch.  Either way
        each pair is scored over its own frames only (Plan.forward(pair_lengths=)); equal shapes without ``lengths`` run
        the fixed-length forward."""
        a, b = self._sq(wav_tensor), self._sq(other_wav_tensor)
        if lengths is None and a.shape == b.shape:
            wav = torch.cat([a, b], dim=0).to(self.device, torch.float32)
            plan = self._plan(wav.shape[0] // 2, wav.shape[1], False)
            return self._logits(plan.embed(wav))
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"compute_speaker_equality: batches of {a.shape[0]} and {b.shape[0]}")
        B = a.shape[0]
        if lengths is None:
            lengths = ([a.shape[1]] * B, [b.shape[1]] * B)
        n = -(-max(a.shape[1], b.shape[1]) // EQUALITY_QUANTUM) * EQUALITY_QUANTUM
        wav = torch.zeros(2 * B, n, dtype=torch.float32, device=self.device)
        wav[:B, :a.shape[1]].copy_(a)
        wav[B:, :b.shape[1]].copy_(b)
        plan = self._lru["equality"].lookup((B, n), lambda: self._make_plan(B, n))
        return self._logits(plan.embed(wav, pair_lengths=lengths))

    def _make_plan(self, batch: int, n: int, **kw) -> Plan:
        return Plan(self.store, batch, n, train=False, reg=self.reg, pooling="first", paired=True,
                    cls_token_constant=self.cfg.cls_token_constant, sep_token_constant=self.cfg.sep_token_constant, **kw)

    def forward(self, input_tensor: torch.Tensor, other_input_tensor: torch.Tensor):
        return self.compute_speaker_equality(input_tensor, other_input_tensor)

    __call__ = forward

    def training_step(self, batch: PairedSpeakerClassificationDataBatch, batch_idx: int = 0,
                      optimized_idx: Optional[int] = None):
        """ref: paired_speaker_recognition_module.py:68-90: forward, BCE, backward (+ all-reduce), fused Adam."""
        wav = self._stack(batch.primary_network_input, batch.secondary_network_input).to(self.device, torch.float32)
        label = batch.ground_truth.to(self.device).to(torch.int64)
        key = (wav.shape[0] // 2, wav.shape[1])
        loss, pred = self._trainer_step(
            key, lambda: SpeakerTrainer(self.store, self._plan(key[0], key[1], True), self.schedule,
                                        process_group=self.process_group, **self._trainer_options()),
            lambda tr: tr.train_step(wav, label))
        self.steps += 1
        return {"loss": loss, "prediction": pred}

    # ------------------------------------------------------------------ evaluation
    @staticmethod
    def _utterance(w: torch.Tensor) -> torch.Tensor:
        w = w.reshape(-1) if (w.dim() <= 1 or w.numel() == w.shape[-1]) else None
        if w is None:
            raise ValueError("score_trials: one utterance per key ([N] or [1, N])")
        return w.to(torch.float32)

    def score_trials(self, pairs, audio_by_key, *, quantum: int = DEFAULT_PAIR_QUANTUM,
                     max_batch_frames: int = DEFAULT_MAX_PAIR_BATCH_FRAMES, max_batch: int = DEFAULT_MAX_BATCH,
                     max_bank_bytes: int = DEFAULT_MAX_BANK_BYTES, reuse_features: bool = True) -> List[float]:
        """Equality logits of a trial list (``pairs``: EvaluationPair; ``audio_by_key``: key -> waveform [N] or [1, N]), in
        the order of ``pairs``; trial i equals ``compute_speaker_equality`` of its two utterances alone.
        1. Every utterance the pairs name runs through the conv stack + projection ONCE (Plan.features, bucketed by length
           with plan_batches) and its valid frames are copied into one device feature bank [sum of frames, H] in the
           activation dtype.
        2. The trials are bucketed by ta + tb + 3 frames (plan_pair_batches) and every batch runs an encoder-only plan
           (Plan.pair_encoder) that assembles its sequences from rows of the bank; unused rows of a bucket's last batch are
           one-frame dummy pairs.
        ``quantum`` / ``max_batch_frames`` are in encoder frames (20 ms); the utterance buckets of step 1 use the same
        numbers times the conv stack's hop (320 samples).  The bank of VoxCeleb1-O is about 3 GB in fp16; a bank above
        ``max_bank_bytes`` (default 8 GiB) raises ValueError: split the trial list.  ``reuse_features=False`` runs each
        trial's two utterances through step 1 on their own (a measurement aid: the cost without the reuse)."""
        cfg = self.model_cfg
        pairs = list(pairs)
        if not pairs:
            return []
        if reuse_features:
            keys = list(dict.fromkeys(k for p in pairs for k in (p.sample1_id, p.sample2_id)))
            pos = {k: i for i, k in enumerate(keys)}
            sides = [(pos[p.sample1_id], pos[p.sample2_id]) for p in pairs]
        else:
            keys = [k for p in pairs for k in (p.sample1_id, p.sample2_id)]
            sides = [(2 * i, 2 * i + 1) for i in range(len(pairs))]
        wavs = [self._utterance(audio_by_key[k]) for k in keys]
        fill = min_samples(cfg.conv_kernel, cfg.conv_stride)
        for k, w in zip(keys, wavs):
            if w.shape[0] < fill:
                raise ValueError(f"score_trials: utterance {k!r} has {w.shape[0]} samples, one frame needs {fill}")
        frames = [cfg.num_frames(w.shape[0]) for w in wavs]
        offset = [0]
        for f in frames:
            offset.append(offset[-1] + f)
        H, adt = cfg.hidden_size, self.store.act_dtype
        nbytes = offset[-1] * H * torch.empty(0, dtype=adt).element_size()
        if nbytes > max_bank_bytes:
            raise ValueError(f"score_trials: the feature bank of {len(keys)} utterances needs {nbytes} bytes, more than "
                             f"max_bank_bytes={max_bank_bytes}: split the trial list (or raise the limit)")
        bank = torch.empty(offset[-1], H, dtype=adt, device=self.device)
        self.last_bank_bytes = nbytes
        hop = int(np.prod(cfg.conv_stride))
        for idx, wav, lens in padded_batches(wavs, quantum * hop, max_batch_frames * hop, max_batch, fill, self.device):
            batch, n = wav.shape
            plan = self._lru["features"].lookup(
                (batch, n), lambda: Plan(self.store, batch, n, train=False, reg=self.reg, pooling="first"))
            feat, _ = plan.features(wav, lengths=lens)
            for j, i in enumerate(idx):
                bank[offset[i]:offset[i + 1]].copy_(feat[j, :frames[i]])
        lf, rf = [frames[a] for a, _ in sides], [frames[b] for _, b in sides]
        parts = []
        for idx, t, batch in plan_pair_batches(lf, rf, quantum, max_batch_frames, max_batch):
            plan = self._lru["pairs"].lookup((batch, t), lambda: Plan.pair_encoder(
                self.store, batch, t, reg=self.reg, cls_token_constant=self.cfg.cls_token_constant,
                sep_token_constant=self.cfg.sep_token_constant))
            rows = [[0] * batch, [1] * batch, [0] * batch, [1] * batch]      # unused rows: dummy one-frame pairs
            for j, i in enumerate(idx):
                a, b = sides[i]
                rows[0][j], rows[1][j], rows[2][j], rows[3][j] = offset[a], frames[a], offset[b], frames[b]
            parts.append((idx, self._logits(plan.embed_pairs(bank, *rows))[:len(idx), 0]))
        order = [i for idx, _ in parts for i in idx]
        scores = torch.cat([x for _, x in parts]).cpu().tolist()
        out = [0.0] * len(pairs)
        for i, v in zip(order, scores):
            out[i] = v
        return out

    def evaluate_trials(self, pairs, audio_by_key, **batching) -> dict:
        """The ``_evaluate`` dict of a trial list scored with score_trials (``batching``: its keyword arguments) -- what
        test_epoch_end gives over the batch-size-1 test loop."""
        pairs = list(pairs)
        scores = self.score_trials(pairs, audio_by_key, **batching)
        return self._evaluate([{"prediction": scores, "label": [int(p.same_speaker) for p in pairs]}])

    def _eval_step(self, batch: PairedSpeakerClassificationDataBatch) -> dict:
        scores = self.compute_speaker_equality(batch.primary_network_input, batch.secondary_network_input)
        return {"prediction": scores.detach().cpu().numpy().tolist(),
                "label": batch.ground_truth.detach().cpu().numpy().tolist()}

    def validation_step(self, batch: PairedSpeakerClassificationDataBatch, batch_idx: int = 0,
                        dataloader_idx: Optional[int] = None) -> dict:
        """ref: paired_speaker_recognition_module.py:115-137 (without the logging)."""
        return self._eval_step(batch)

    def validation_epoch_end(self, outputs: List[dict]) -> dict:
        return self._evaluate(outputs)                       # ref :139-144 logs its "eer" as val_eer

    def test_step(self, batch: PairedSpeakerClassificationDataBatch, batch_idx: int = 0,
                  dataloader_idx: Optional[int] = None) -> dict:
        """ref :146-166: whole trial utterances, one pair per batch."""
        if batch.batch_size != 1:
            raise ValueError("expecting a batch size of 1 for evaluation")
        return self._eval_step(batch)

    def test_epoch_end(self, outputs: List[dict]) -> dict:
        return self._evaluate(outputs)                       # ref :168-169

    @staticmethod
    def _evaluate(outputs: List[dict]) -> dict:
        """ref :171-248: ``outputs`` = dicts with ``label`` (0 / 1, an int or a list) and ``prediction`` (the raw equality
        logits, a number or a -- possibly nested -- list).  The logits are mapped with clip((s + 1) / 2, 0, 1) like the
        reference, then EER (1 when its threshold is NaN or the computation fails) and minDCF."""
        truth: List[int] = []
        scores: List[float] = []
        for d in outputs:
            truth.extend(int(v) for v in np.asarray(d["label"]).reshape(-1).tolist())
            scores.extend(np.asarray(d["prediction"], dtype=np.float64).reshape(-1).tolist())
        scores = np.clip((np.asarray(scores, dtype=np.float64) + 1) / 2, 0, 1).tolist()
        try:
            eer, eer_threshold = calculate_eer(truth, scores, pos_label=1)
            if np.isnan(eer_threshold):
                eer = 1
        except (ValueError, ZeroDivisionError):              # NaN scores: a very bad score instead of a crash
            eer, eer_threshold = 1, 1337
        try:
            mdc, mdc_threshold = calculate_mdc(truth, scores)
        except (ValueError, ZeroDivisionError):
            mdc, mdc_threshold = 1, 1337
        return {"eer": eer, "eer_threshold": eer_threshold, "mdc": mdc, "mdc_threshold": mdc_threshold}

    def state_dict(self):
        return self.store.state_dict()

    def load_state_dict(self, sd, strict: bool = True):
        self.store.load_state_dict(sd, strict=strict, prefix_model=False)
