"""x-vector training step and evaluation on the HIP path (the ``speaker_xvector`` baseline experiment).

ref: src/lightning_modules/speaker/xvector.py:47-122 (``XVectorModule`` -> speechbrain 0.5.x ``Xvector(tdnn_blocks=5,
tdnn_channels=[512]*4+[1500], tdnn_kernel_sizes=[5,3,3,1,1], tdnn_dilations=[1,2,3,1,1], lin_neurons=512,
in_channels=40)`` + ``Classifier``, config/network/xvector.yaml) under cross-entropy.  speechbrain is not part of the
reference tree: the arithmetic is the published definition as recollected ("parity unpinned"),

    five times  Conv1d(bias, "same", reflect, dilation) -> LeakyReLU(0.01) -> BatchNorm1d
    StatisticsPooling over time: cat(mean, unbiased std + 1e-5)  [its Gaussian noise on the mean is left out]
    Linear(2 C5 -> lin_neurons)                                   = the embedding
    classifier: LeakyReLU -> BatchNorm1d -> Linear -> LeakyReLU -> BatchNorm1d -> Linear(-> speakers) -> log-softmax

in f32 (the reference's ``precision: 32``).  The design is ecapa.py's: channels-last activations [B*T, C], a flat f32
parameter arena with the fused optimiser, static buffers and prebuilt GEMM descriptors, hand-written backward.  The TDNN
blocks are ecapa._Tdnn with the LeakyReLU mode of the BatchNorm kernels; the classifier's LeakyReLU -> BatchNorm pairs
are the same two kernels over the B rows of the batch; the last Linear with the loss is heads.ClassifierHead("ce")
(cross-entropy and softmax are idempotent on log-probabilities, so the reference's loss of the log-softmax output equals
the loss of the Linear's output).  The last TDNN layer has 1500 channels: the f32 strip kernels take any multiple of 4
(csrc/tdnn.hip, bn_align), so no tensor is padded and every consumer sees 1500.
"""
from __future__ import annotations

import dataclasses
import math
from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from . import ops
from .ecapa import BN_EPS, BN_MOMENTUM, FE, BnArena, EcapaTrainer, TdnnPlan, _Tdnn, ecapa_min_frames, fbank_frames  # noqa: F401
from .heads import ClassifierHead
from .ops import BN_ACT_LEAKY, EPI_BIAS, Gemm

CLS = "classifier."               # reference attribute name of the speechbrain Classifier (xvector.py:77)


@dataclasses.dataclass
class XVectorConfig:
    """ref: config/network/xvector.yaml:4-9 (XVectorModuleConfig), under the field names of EcapaConfig so that the length
    rules of ecapa.py (ecapa_min_frames, valid_frame_lengths, valid_sample_lengths) read both."""
    input_mel_coefficients: int = 40
    lin_neurons: int = 512
    channels: Tuple[int, ...] = (512, 512, 512, 512, 1500)
    kernel_sizes: Tuple[int, ...] = (5, 3, 3, 1, 1)
    dilations: Tuple[int, ...] = (1, 2, 3, 1, 1)

    @staticmethod
    def tiny() -> "XVectorConfig":
        return XVectorConfig(input_mel_coefficients=8, lin_neurons=16, channels=(16, 16, 16, 16, 44))   # 44 % 8 = 4 = 1500 % 8


def xvector_min_frames(cfg: XVectorConfig) -> int:
    """Fewest frames an utterance may have (reflect padding < length; 4 for the reference configuration: k = 3, dilation 3)."""
    return ecapa_min_frames(cfg)


def xvector_param_shapes(cfg: XVectorConfig, num_speakers: int) -> "OrderedDict[str, Tuple[int, ...]]":
    """speechbrain state-dict names as recollected (not checked against an installed speechbrain): the Xvector's
    ``blocks`` ModuleList holds conv / activation / norm per TDNN layer, then the pooling and the Linear."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    cin = cfg.input_mel_coefficients
    for i, (c, k) in enumerate(zip(cfg.channels, cfg.kernel_sizes)):
        s[FE + f"blocks.{3 * i}.conv.weight"] = (c, cin, k)
        s[FE + f"blocks.{3 * i}.conv.bias"] = (c,)
        s[FE + f"blocks.{3 * i + 2}.norm.weight"] = (c,)
        s[FE + f"blocks.{3 * i + 2}.norm.bias"] = (c,)
        cin = c
    n, L = len(cfg.channels), cfg.lin_neurons
    s[FE + f"blocks.{3 * n + 1}.w.weight"] = (L, 2 * cin)
    s[FE + f"blocks.{3 * n + 1}.w.bias"] = (L,)
    s[CLS + "norm.norm.weight"] = (L,)
    s[CLS + "norm.norm.bias"] = (L,)
    s[CLS + "DNN.block_0.linear.w.weight"] = (L, L)
    s[CLS + "DNN.block_0.linear.w.bias"] = (L,)
    s[CLS + "DNN.block_0.norm.norm.weight"] = (L,)
    s[CLS + "DNN.block_0.norm.norm.bias"] = (L,)
    s[CLS + "out.w.weight"] = (num_speakers, L)
    s[CLS + "out.w.bias"] = (num_speakers,)
    return s


class XVectorStore(BnArena):
    """Parameter arena of the x-vector model and its classifier (f32; the BatchNorm1d buffers beside it)."""

    def __init__(self, cfg: XVectorConfig, device, act_dtype: torch.dtype = torch.float32, num_speakers: int = 5994):
        if act_dtype != torch.float32:
            raise NotImplementedError("x-vector: f32 only (the reference's precision for this experiment)")
        if any(c % 4 for c in cfg.channels) or any(c % 8 for c in (cfg.input_mel_coefficients,) + tuple(cfg.channels[:-1])):
            raise ValueError("x-vector: the input and every convolution's input channels must be multiples of 8 (the "
                             "reflect gather's 16-byte vectors), the last layer's a multiple of 4")
        self.cfg, self.num_speakers = cfg, num_speakers
        self.embed_dim = cfg.lin_neurons
        super().__init__(xvector_param_shapes(cfg, num_speakers), device, act_dtype)

    def init_weights(self, seed: int = 20211) -> None:
        g = torch.Generator(device="cpu").manual_seed(seed)
        for n, s in self.shapes.items():
            if n.endswith("norm.weight"):
                t = torch.ones(s)
            elif n.endswith("bias"):
                t = torch.zeros(s)
            else:                                    # torch Conv1d / Linear default: kaiming-uniform, bound 1/sqrt(fan_in)
                t = (torch.rand(s, generator=g) * 2 - 1) / math.sqrt(math.prod(s[1:]))
            self.p(n).copy_(t.to(self.device))
        self.sync_lowp()


class _ActNorm:
    """LeakyReLU -> BatchNorm1d over the B rows of a [B, L] f32 tensor: the strip BatchNorm kernels in their LeakyReLU mode."""

    def __init__(self, store: XVectorStore, name: str, a: torch.Tensor, B: int, L: int, train: bool):
        dev, f32 = a.device, torch.float32
        self.store, self.a, self.B, self.L, self.train = store, a, B, L, train
        self.n_gamma, self.n_beta = name + "weight", name + "bias"
        self.y = torch.empty(B, L, dtype=f32, device=dev)
        self.mean_rstd = torch.empty(L, 2, dtype=f32, device=dev)
        self.running = store.running(self.n_gamma)
        self.work = ops.bn_workspace(B, L, dev)
        if train:
            self.da = torch.empty(B, L, dtype=f32, device=dev)
            self.cs_part = torch.empty(ops.bn_colsum_rows(B, L), L, dtype=f32, device=dev)

    def forward(self) -> None:
        st = self.store
        ops.bn_fwd(self.a, self.L, self.work, self.mean_rstd, self.running, st.p(self.n_gamma), st.p(self.n_beta), self.y,
                   self.L, self.B, self.L, BN_EPS, BN_MOMENTUM, BN_ACT_LEAKY, self.train)

    def backward(self, dy: torch.Tensor, dbias: torch.Tensor) -> None:
        """dy -> self.da = d(loss)/d(a); the column sums of da -- the bias gradient of the Linear that wrote ``a`` -- are
        added into ``dbias``."""
        st = self.store
        ops.bn_bwd(dy, self.L, self.a, self.L, self.mean_rstd, st.p(self.n_gamma), self.work, st.g(self.n_gamma),
                   st.g(self.n_beta), self.da, self.L, self.B, self.L, BN_ACT_LEAKY, colsum_partial=self.cs_part)
        ops.colsum(self.cs_part, dbias, self.cs_part.shape[0], self.L)


class _Linear:
    """y [B, N] = x [B, K] W^T + b through the exact-f32 GEMM routing, with the two gradient products of its backward."""

    def __init__(self, store: XVectorStore, name: str, x: torch.Tensor, y: torch.Tensor, train: bool):
        B, K = x.shape
        N = y.shape[1]
        self.n_w, self.n_b = name + "weight", name + "bias"
        W = store.p(self.n_w)
        self.forward = Gemm(B, N, K, x, W, y, lda=K, ldb=K, ldc=N, epilogue=EPI_BIAS, bias=store.p(self.n_b))
        if train:
            self.dx = torch.empty(B, K, dtype=torch.float32, device=x.device)
            self._x, self._W, self._dW, self._shape = x, W, store.g(self.n_w), (B, N, K)
            self.dbias = store.g(self.n_b)

    def backward(self, dy: torch.Tensor) -> None:
        """dW += dy^T x (the arena is zeroed per step), self.dx = dy W; the bias gradient is the caller's (_ActNorm)."""
        if getattr(self, "_g_dw", None) is None:
            B, N, K = self._shape
            self._g_dw = Gemm(N, K, B, dy, self._x, self._dW, lda=N, ldb=K, ldc=K, transA=True, transB=True, accumulate=True)
            self._g_dx = Gemm(B, K, N, dy, self._W, self.dx, lda=N, ldb=K, ldc=K, transB=True)
            self._dy = dy
        assert dy.data_ptr() == self._dy.data_ptr()
        self._g_dw()
        self._g_dx()


class XVectorClassifier:
    """speechbrain ``Classifier`` on an embedding buffer [B, lin_neurons]: LeakyReLU -> BN -> Linear -> LeakyReLU -> BN ->
    Linear(-> speakers), the last Linear with the cross-entropy in heads.ClassifierHead("ce")."""

    def __init__(self, store: XVectorStore, batch: int, emb: torch.Tensor, train: bool):
        L = store.cfg.lin_neurons
        self.store, self.B, self.emb, self.train = store, batch, emb, train
        self.norm1 = _ActNorm(store, CLS + "norm.norm.", emb, batch, L, train)
        self.z = torch.empty(batch, L, dtype=torch.float32, device=emb.device)
        self.dnn = _Linear(store, CLS + "DNN.block_0.linear.w.", self.norm1.y, self.z, train)
        self.norm2 = _ActNorm(store, CLS + "DNN.block_0.norm.norm.", self.z, batch, L, train)
        p, g = store.p, store.g
        self.head = ClassifierHead("ce", batch, L, store.num_speakers, w_master=p(CLS + "out.w.weight"),
                                   w_operand=store.w(CLS + "out.w.weight"),
                                   w_grad=g(CLS + "out.w.weight") if train else None, bias=p(CLS + "out.w.bias"),
                                   bias_grad=g(CLS + "out.w.bias") if train else None, emb=self.norm2.y,
                                   act_dtype=torch.float32, train=train)

    def _forward(self) -> None:
        self.norm1.forward()
        self.dnn.forward()
        self.norm2.forward()

    def forward_backward(self, label: torch.Tensor, emb_bias_grad: Optional[torch.Tensor] = None):
        """(loss, softmax [B, speakers]); in training also every classifier gradient into the arena, d(loss)/d(emb) into
        ``self.demb``, and its column sums -- the bias gradient of the embedding Linear -- added into ``emb_bias_grad``."""
        self._forward()
        out = self.head.forward_backward(label)
        if self.train:
            self.norm2.backward(self.head.demb, self.dnn.dbias)
            self.dnn.backward(self.norm2.da)
            self.norm1.backward(self.dnn.dx, emb_bias_grad)
        return out

    @property
    def demb(self) -> torch.Tensor:
        return self.norm1.da

    def log_probabilities(self) -> torch.Tensor:
        """ref: xvector.py:117-122 (compute_speaker_prediction): the Classifier's log-softmax output [B, speakers] for the
        embedding buffer.  The stack and the logits run on the kernels; the log-softmax of the [B, speakers] logits is
        one torch call (an evaluation-time convenience, not part of a training step)."""
        self._forward()
        self.head._forward_logits()
        return torch.log_softmax(self.head.logits[:, :self.head.C], dim=1)


class XVectorPlan(TdnnPlan):
    """Static plan of one x-vector forward (+ backward) for a fixed [B, T, n_mels] input."""

    def __init__(self, store: XVectorStore, batch: int, frames: int, *, train: bool):
        super().__init__(store, batch, frames, train)
        cfg = store.cfg
        B, T, M, dev, f32 = batch, frames, batch * frames, self.dev, torch.float32
        if T < 2:
            raise ValueError("x-vector: the unbiased standard deviation of the statistics pooling needs 2 frames")
        C = cfg.channels
        self.tdnns: List[_Tdnn] = []
        x, ldx, cin = self.feat, cfg.input_mel_coefficients, cfg.input_mel_coefficients
        for i, (c, k, d) in enumerate(zip(C, cfg.kernel_sizes, cfg.dilations)):
            y = self.buf(M, c)
            self.tdnns.append(_Tdnn(self, "blocks.", x, ldx, cin, c, k, d, y, c, act=BN_ACT_LEAKY, conv=f"{3 * i}.conv.",
                                    norm=f"{3 * i + 2}.norm."))
            x, ldx, cin = y, c, c
        self.CL, L = C[-1], cfg.lin_neurons
        self.pooled = torch.empty(B, 2 * self.CL, dtype=f32, device=dev)
        self.pool_stats = torch.empty(B, 2 * self.CL, dtype=f32, device=dev) if train else None
        self.emb = torch.empty(B, L, dtype=f32, device=dev)
        self.linear = _Linear(store, FE + f"blocks.{3 * len(C) + 1}.w.", self.pooled, self.emb, train)
        if train:
            self.classifier = XVectorClassifier(store, B, self.emb, True)
            self.d_x = [torch.empty(M, c, dtype=f32, device=dev) for c in C]       # d(loss)/d(output of block i)

    def _tdnns(self) -> List[_Tdnn]:
        return self.tdnns

    def _embed_features(self) -> torch.Tensor:
        """The forward from the plan's feature buffer on: ref xvector.py:103-115.  With lengths (evaluation) every stage
        that reaches across frames -- the reflect gathers and the pooling -- sees each utterance's own frames only; the
        k = 1 blocks and the BatchNorm on running statistics work row by row."""
        for t in self.tdnns:
            t.forward()
        ops.stat_pool_fwd(self.tdnns[-1].y, self.CL, self.pooled, self.pool_stats, self.B, self.T, self.CL, lens=self._len)
        self.linear.forward()
        return self.emb

    def head_forward_backward(self, label: torch.Tensor):
        assert self.train, "the classifier of an evaluation plan is XVectorClassifier.log_probabilities"
        return self.classifier.forward_backward(label, self.linear.dbias)

    def backward(self) -> None:
        """Backward of embed() from the classifier's d(loss)/d(emb): every parameter gradient into store.grad."""
        assert self.train
        C = self.cfg.channels
        self.linear.backward(self.classifier.demb)
        n = len(self.tdnns)
        ops.stat_pool_bwd(self.tdnns[-1].y, self.CL, self.pool_stats, self.linear.dx, self.d_x[-1], self.CL, self.B, self.T,
                          self.CL)
        for i in range(n - 1, -1, -1):
            dx, ld = (self.d_x[i - 1], C[i - 1]) if i > 0 else (None, 0)
            self.tdnns[i].backward(self.d_x[i], C[i], dx, ld, False)


class XVectorTrainer(EcapaTrainer):
    """One training step: forward, classifier + cross-entropy, backward, fused optimiser step (ref:
    speaker_recognition_module.py:207-220).  The step, the accumulation window and the data-parallel all-reduce of the flat
    gradient arena are EcapaTrainer's (a fused.WindowedTrainer): both plans have the same four entry points."""
