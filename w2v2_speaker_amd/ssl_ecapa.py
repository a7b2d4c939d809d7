"""wav2vec2 encoder + ECAPA-TDNN back-end, joined by a learned layer mix on the device.

The strongest published way to use a self-supervised speech encoder for speaker verification: a softmax-weighted sum of
ALL encoder layer outputs (weights learned: ``feature_weight`` [L + 1], zeros at the start = the plain mean), instance
normalised over time, fed to an ECAPA-TDNN, with the encoder frozen for the first steps.  The reference has no such model
(its wav2vec_xvector.py points the same way: ``wav2vec_initially_frozen`` / ``num_frozen_steps``); the definition is this
project's own -- include/w2v2_hip.h "layer mix", DESIGN.md 5 and 7.

Two plans and two arenas that already exist, and three kernels between them (csrc/layer_mix.hip):
    Plan(keep_hidden_states=True).forward  ->  hidden states X[0 .. L]
    ops.layer_mix_fwd                      ->  EcapaPlan.feat (its dtype and row stride), rstd
    EcapaPlan.embed_features, head         ->  loss, d_feat (EcapaPlan(input_grad=True))
    ops.layer_mix_bwd                      ->  dm, gradient of feature_weight
    Plan.backward(dmix=dm, mix_weights=w)  ->  encoder gradients (w_j dm injected at every layer output)
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .config import Wav2Vec2RegularisationConfig
from .ecapa import EcapaPlan, EcapaStore
from .engine import Plan
from .optim import OptimConfig
from .params import ParamStore
from .trainer import SpeakerTrainer

LIMITS = ("the wav2vec2 + ECAPA-TDNN trainer steps one rank, one batch per step, without gradient clipping: "
          "process_group, accumulate_grad_batches > 1 and gradient_clip_val > 0 are not built (DESIGN.md 7)")


def check_stores(enc: ParamStore, ecapa: EcapaStore, train: bool) -> None:
    """What the two arenas of one model must agree on; raised before anything is allocated."""
    cfg = enc.cfg
    J = cfg.num_hidden_layers + 1
    if getattr(cfg, "do_stable_layer_norm", False):
        raise NotImplementedError("do_stable_layer_norm: the layer mix reads the hidden states of the post-LN encoder only")
    if ecapa.feature_weight != J:
        raise ValueError(f"the ECAPA store needs feature_weight = L + 1 = {J} (EcapaStore(feature_weight=)), got "
                         f"{ecapa.feature_weight}")
    if ecapa.cfg.input_mel_coefficients != cfg.hidden_size:
        raise ValueError(f"the ECAPA store needs input_mel_coefficients = hidden_size = {cfg.hidden_size}, got "
                         f"{ecapa.cfg.input_mel_coefficients}")
    if cfg.hidden_size % 8:
        raise ValueError(f"hidden_size {cfg.hidden_size}: the layer mix needs a multiple of 8")
    if train and enc.scaler is not None:
        raise NotImplementedError("f16 encoder training is not supported by this model: the encoder store has a loss scaler "
                                  "and the ECAPA side has none")
    if torch.device(enc.device) != torch.device(ecapa.device):
        raise ValueError("the two stores live on different devices")


class SslEcapaPlan:
    """Static plan of the joined model for a fixed [B, N] waveform batch: owns the encoder plan, the ECAPA plan at the
    encoder's frame count, the pointer table of the hidden states, rstd and dm."""

    def __init__(self, enc_store: ParamStore, ecapa_store: EcapaStore, batch: int, n_samples: int, *, train: bool,
                 reg: Optional[Wav2Vec2RegularisationConfig] = None, instance_norm: bool = True, seed: int = 7,
                 aam_margin: float = 0.2, aam_scale: float = 30.0, sub_centers: Optional[int] = None,
                 margin_type: str = "arc", inter_topk: int = 0, inter_margin: float = 0.06):
        check_stores(enc_store, ecapa_store, train)
        self.enc_store, self.store, self.train, self.instance_norm = enc_store, ecapa_store, train, bool(instance_norm)
        self.enc = Plan(enc_store, batch, n_samples, train=train, reg=reg, keep_hidden_states=True, seed=seed)
        B, T, H = batch, self.enc.T, enc_store.cfg.hidden_size
        self.B, self.T, self.N, self.H, self.J = B, T, n_samples, H, enc_store.cfg.num_hidden_layers + 1
        self.ecapa = EcapaPlan(ecapa_store, B, T, train=train, aam_margin=aam_margin, aam_scale=aam_scale,
                               sub_centers=sub_centers, margin_type=margin_type, inter_topk=inter_topk,
                               inter_margin=inter_margin, input_grad=train)
        self.head = self.ecapa.head                      # (the trainers' margin schedule writes plan.head.margin)
        dev, f32 = ecapa_store.device, torch.float32
        self.table = ops.LayerMixTable(self.enc.X)       # built once: the plan's activations never move
        self.rstd = torch.zeros(B, H, dtype=f32, device=dev)
        self.w = torch.zeros(self.J, dtype=f32, device=dev)
        self.dm = torch.empty(B * T, H, dtype=f32, device=dev) if train else None
        self.ws = ops.layer_mix_workspace(B, T, H, self.J, dev) if train else None
        # beyond the LDS tile the forward stages m in f32: a training plan lends dm (the backward writes it later)
        self.stage = None
        if self.instance_norm and T > ops.LAYER_MIX_LDS_FRAMES:
            self.stage = self.dm if train else torch.empty(B * T, H, dtype=f32, device=dev)
        self.frame_lengths = None

    @property
    def emb(self) -> torch.Tensor:
        return self.ecapa.emb

    def mix(self, lens: Optional[torch.Tensor] = None) -> None:
        """The layer mix of the encoder's hidden states into the ECAPA plan's feature buffer."""
        feat = self.ecapa.feat
        ops.layer_mix_fwd(self.table, self.store.p("feature_weight"), feat, feat.stride(0), self.B, self.T, rstd=self.rstd,
                          lens=lens, w_out=self.w, stage=self.stage, instance_norm=self.instance_norm)

    def embed(self, wav: torch.Tensor, mask: Optional[torch.Tensor] = None, skip_layers: Sequence[int] = (),
              lengths=None, step: int = 0) -> torch.Tensor:
        """wav [B, N] f32 on the device -> speaker embedding [B, lin_neurons] f32.  mask / skip_layers: the encoder's
        SpecAugment time mask and LayerDrop decisions (training plans).  lengths: valid SAMPLES per utterance (evaluation
        plans): the encoder, the mix and the ECAPA stages then see each utterance's own Plan.frames_of(n) frames only, and
        row b equals the utterance alone at its own length."""
        enc = self.enc
        enc.forward(wav, mask, skip_layers, step, lengths=lengths)
        self.frame_lengths = enc.frame_lengths
        if lengths is None:
            self.mix()
            return self.ecapa.embed_features()
        self.mix(enc._len[1])
        return self.ecapa.embed_features(lengths=enc.frame_lengths)

    def head_forward_backward(self, label: torch.Tensor):
        return self.ecapa.head_forward_backward(label)

    def backward(self, encoder: bool = True) -> None:
        """Backward of embed() from the head's gradient: the ECAPA gradients, d_feat, the gradient of feature_weight (ADDED
        into the arena) and dm; with ``encoder`` the encoder's gradients through Plan.backward(dmix=, mix_weights=).
        encoder=False (frozen steps) stops behind the feature_weight gradient: no injection, no encoder launch."""
        assert self.train, "backward needs a training plan"
        ec, feat = self.ecapa, self.ecapa.feat
        ec.backward()
        ops.layer_mix_bwd(self.table, self.store.p("feature_weight"), ec.d_feat, ec.d_feat.stride(0), feat, feat.stride(0),
                          self.rstd, self.dm, self.store.g("feature_weight"), self.ws, self.B, self.T,
                          instance_norm=self.instance_norm)
        if encoder:
            self.enc.backward(dmix=self.dm, mix_weights=self.w)


class SslEcapaTrainer:
    """One training step of the joined model: two arenas under one schedule (ref: speaker_recognition_module.py:207-220 +
    wav2vec2_fc.py:339-361 ``wav2vec_initially_frozen`` / ``num_frozen_steps``).  The encoder's rate is the schedule's
    times ``ssl_lr_factor``.  While frozen only the ECAPA arena (feature_weight included) is stepped: the encoder's
    forward still runs, with its regularisation, and its parameters and optimiser state stay bit-identical."""

    def __init__(self, plan: SslEcapaPlan, schedule, *, ssl_lr_factor: float = 1.0, num_frozen_steps: Optional[int] = 0,
                 wav2vec_initially_frozen: bool = False, optimizer: Optional[OptimConfig] = None, process_group=None,
                 accumulate_grad_batches: int = 1, gradient_clip_val: float = 0.0, margin_schedule=None,
                 layerdrop_seed: int = 1234, mask_seed: int = 7):
        """num_frozen_steps: the encoder is frozen for that many steps; None with ``wav2vec_initially_frozen``: always."""
        if process_group is not None or accumulate_grad_batches != 1 or gradient_clip_val > 0:
            raise NotImplementedError(LIMITS)
        assert plan.train
        self.plan, self.schedule, self.optimizer = plan, schedule, optimizer
        self.ssl_lr_factor = float(ssl_lr_factor)
        if wav2vec_initially_frozen:
            self.num_frozen_steps = None if num_frozen_steps is None else int(num_frozen_steps)
        else:
            self.num_frozen_steps = 0
        self.margin_schedule = margin_schedule
        self.step, self.stepped = 0, False
        # the encoder's regularisation draws are SpeakerTrainer's (one definition): its two sampling methods read the
        # encoder plan and the two host streams off this record
        self._draws = SimpleNamespace(plan=plan.enc, _ld_rng=np.random.RandomState(layerdrop_seed),
                                      _mask_rng=np.random.RandomState(mask_seed))

    def frozen(self) -> bool:
        """Whether the step about to run leaves the encoder alone."""
        return self.num_frozen_steps is None or self.step < self.num_frozen_steps

    def train_step(self, wav: torch.Tensor, label: torch.Tensor, mask: Optional[torch.Tensor] = None,
                   skip_layers: Optional[Sequence[int]] = None):
        """Returns (loss, softmax) as device tensors; no host sync.  mask None / skip_layers None: drawn from the
        regularisation config like SpeakerTrainer; pass () for no LayerDrop."""
        plan = self.plan
        enc_store, store = plan.enc_store, plan.store
        if self.margin_schedule is not None:
            plan.head.margin = float(self.margin_schedule(self.step))
        if skip_layers is None:
            skip_layers = SpeakerTrainer.sample_layerdrop(self._draws)
        if mask is None:
            mask = SpeakerTrainer.sample_time_mask(self._draws)
        frozen = self.frozen()
        store.zero_grad()
        if not frozen:
            enc_store.zero_grad(tuple(skip_layers) if plan.enc.grouped else None)
        plan.embed(wav, mask, skip_layers, step=self.step)
        loss, softmax = plan.head_forward_backward(label)
        plan.backward(encoder=not frozen)
        lr, second = self.schedule.at(self.step)
        store.optimizer_step(lr, second, self.optimizer)
        if not frozen:
            enc_store.optimizer_step(lr * self.ssl_lr_factor, second, self.optimizer)
        self.step += 1
        self.stepped = True
        return loss, softmax
