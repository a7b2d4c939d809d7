"""Mirror of ``src/lightning_modules/speaker/xvector.py`` (XVectorModuleConfig :31-44, XVectorModule :47-122) on the HIP
path (w2v2_speaker_amd/xvector.py).  Same config field names, same method names and argument meaning."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

from ...xvector import XVectorClassifier, XVectorConfig, XVectorPlan, XVectorStore, XVectorTrainer
from ...eval_batching import PlanCache
from .ecapa_tdnn import FilterbankSpeakerModule


@dataclass
class XVectorModuleConfig:
    """ref: xvector.py:31-44 / config/network/xvector.yaml."""
    explicit_stat_pool_embedding_size: Optional[int] = None
    explicit_num_speakers: Optional[int] = None
    tdnn_blocks: int = 5
    tdnn_channels: List[int] = field(default_factory=lambda: [512, 512, 512, 512, 1500])
    tdnn_kernel_sizes: List[int] = field(default_factory=lambda: [5, 3, 3, 1, 1])
    tdnn_dilations: List[int] = field(default_factory=lambda: [1, 2, 3, 1, 1])
    lin_neurons: int = 512
    in_channels: int = 40


class XVectorModule(FilterbankSpeakerModule):
    def __init__(self, hyperparameters_to_save, cfg: XVectorModuleConfig, num_speakers: int,
                 loss_fn_constructor: Callable[[], object], validation_pairs=None, test_pairs=None, evaluator=None, *,
                 device="cuda", act_dtype: torch.dtype = torch.float32, max_lr: float = 1e-3,
                 max_steps: int = 100_000, init_seed: int = 20211, gradient_clip_val: float = 0.0,
                 accumulate_grad_batches: int = 1, input_features: str = "fbank", augmenter=None):
        """Positional arguments = ref: xvector.py:48-57 (what src/main.py:256-285 passes to every network class).
        ``loss_fn_constructor`` is called once and read for its type: the experiment (config/experiment/
        speaker_xvector.yaml) trains under ``CrossEntropyLoss``; an AAM loss raises the reference's own ValueError (ref
        :84-85), anything else NotImplementedError.  ``act_dtype``: f32 only, the reference's ``precision: 32``.
        ``input_features``: as in EcapaTdnnModule -- "fbank" [B, T, n_mels] tensors or "waveform" audio through the device
        front-end.  ``augmenter``: as in EcapaTdnnModule -- a data.augment.Augmenter in front of the filterbank, "waveform"
        inputs only."""
        self._check_input_features(input_features)
        self._check_augmenter(augmenter, input_features)
        from ...optim.loss import AngularAdditiveMarginSoftMaxLoss, CrossEntropyLoss
        loss_fn = loss_fn_constructor()
        if isinstance(loss_fn, AngularAdditiveMarginSoftMaxLoss):
            raise ValueError("xvector does not support aam softmax")
        if type(loss_fn) is not CrossEntropyLoss:
            raise NotImplementedError(f"loss {type(loss_fn).__name__}: the x-vector path runs under CrossEntropyLoss")
        del loss_fn
        if act_dtype != torch.float32:
            raise NotImplementedError("x-vector: act_dtype=torch.float32 only (the reference's precision: 32)")
        if cfg.tdnn_blocks != len(cfg.tdnn_channels) or not (len(cfg.tdnn_channels) == len(cfg.tdnn_kernel_sizes)
                                                              == len(cfg.tdnn_dilations)):
            raise ValueError("tdnn_blocks, tdnn_channels, tdnn_kernel_sizes and tdnn_dilations must agree in length")
        self.hyperparameters_to_save = hyperparameters_to_save
        self.cfg = cfg
        self.embedding_size = cfg.lin_neurons
        self.num_speakers = cfg.explicit_num_speakers or num_speakers
        self.model_cfg = XVectorConfig(cfg.in_channels, cfg.lin_neurons, tuple(cfg.tdnn_channels),
                                       tuple(cfg.tdnn_kernel_sizes), tuple(cfg.tdnn_dilations))
        self.store = XVectorStore(self.model_cfg, device, act_dtype, num_speakers=self.num_speakers)
        self.store.init_weights(init_seed)
        self._classifiers = PlanCache()                    # evaluation classifiers, one per batch size
        self._init_runtime(device, input_features, validation_pairs, test_pairs, evaluator, max_lr, max_steps,
                           gradient_clip_val, accumulate_grad_batches, augmenter)

    @classmethod
    def from_config(cls, cfg: XVectorModuleConfig, num_speakers: int, **kw) -> "XVectorModule":
        """Short form for scripts and tests: the cross-entropy loss without a constructor argument."""
        from ...optim.loss import CrossEntropyLoss
        return cls(None, cfg, num_speakers, CrossEntropyLoss, kw.pop("validation_pairs", None),
                   kw.pop("test_pairs", None), kw.pop("evaluator", None), **kw)

    def _new_plan(self, batch: int, frames: int, train: bool) -> XVectorPlan:
        return XVectorPlan(self.store, batch, frames, train=train)

    def _new_trainer(self, plan: XVectorPlan) -> XVectorTrainer:
        return XVectorTrainer(self.store, plan, self.schedule, **self._trainer_options())

    def compute_speaker_prediction(self, embedding_tensor: torch.Tensor) -> torch.Tensor:
        """ref :117-122: the classifier's log-probabilities [B, speakers] (squeezed) of embeddings [B, lin_neurons], its
        BatchNorm layers on their running statistics."""
        e = embedding_tensor if embedding_tensor.dim() == 2 else embedding_tensor[None]
        B = e.shape[0]

        def build():
            emb = torch.empty(B, self.embedding_size, dtype=torch.float32, device=self.device)
            return XVectorClassifier(self.store, B, emb, False)
        cl = self._classifiers.lookup(B, build)
        cl.emb.copy_(e.to(self.device, torch.float32))
        return cl.log_probabilities().clone().squeeze()
