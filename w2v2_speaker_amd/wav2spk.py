"""wav2spk training step and evaluation on the HIP path (the reference's waveform-to-embedding baseline).

ref: src/lightning_modules/speaker/wav2spk.py:116-299 (``Wav2SpkModule``), src/layers/temporal_gating.py (``TemporalGate``),
config/network/wav2spk.yaml.  Input is raw audio [B, N]:

    encoder     five times  Conv1d(bias, zero padding, stride) -> InstanceNorm1d(no affine, eps 1e-5) -> ReLU
    gate        y = sigmoid(W x + b) * x per frame                         [if apply_temporal_gating]
    aggregator  four times  Conv1d(512, 512, k = 3, stride 1, padding 1, bias) -> ReLU
    pooling     cat(std unbiased, mean) over time ("mean+std") or the mean ("mean")
    head        the fc_list: hidden Linear + ReLU layers, then Linear(-> speakers) + log-softmax, under cross-entropy

in f32 (like the x-vector: the reference's ``precision: 32``).  The design is xvector.py's: channels-last activations
[B*T, C], a flat f32 parameter arena with the fused optimiser, static buffers and prebuilt GEMM descriptors, a hand-written
backward.  Layer 0 (one input channel) runs straight from the waveform (w2v2_conv1d_first); the other eight convolutions are
a zero-padded gather (w2v2_im2col_zero) + the exact-f32 GEMM against the packed [Cout][k][Cin] weight, as ECAPA does with
its reflect gather; InstanceNorm + ReLU, the gate and the fold of the partial products are csrc/wav2spk.hip; the pooling is w2v2_pool_fwd mode
0 / 1, the hidden layers heads.FcStack, the last Linear with the loss heads.ClassifierHead("ce") (cross-entropy and softmax
are idempotent on log-probabilities, the argument of xvector.py).

The five encoder conv biases have NO gradient: an InstanceNorm without affine removes any per-channel constant, so
d(loss)/d(bias) is zero in exact arithmetic (the reference's autograd returns 1e-16 .. 1e-19 of rounding noise, on which its
Adam random-walks the biases without the output seeing it).  Here the gradient is exact zeros -- the arena is zeroed per step
and nothing writes those five ranges -- so the biases keep their values; they stay in the arena and the state dict, and the
forward still adds them, so checkpoints round-trip and stage outputs stay comparable.
"""
from __future__ import annotations

import dataclasses
import math
from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from . import ops
from .ecapa import BnArena, EcapaTrainer, f32_dw_split
from .heads import ClassifierHead, FcStack
from .ops import EPI_ADD, EPI_BIAS, Gemm, conv_out_frames

# (Cin, Cout, kernel, stride, padding): fixed by the reference (wav2spk.py:138-152, :175-186), not configuration
ENCODER = ((1, 40, 10, 5, 4), (40, 200, 5, 4, 2), (200, 300, 5, 2, 2), (300, 512, 3, 2, 1), (512, 512, 3, 2, 1))
AGGREGATOR = ((512, 512, 3, 1, 1),) * 4
FEATURES = 512
MIN_FRAMES = 2          # per layer: torch's InstanceNorm1d refuses one frame in training, the pooled std needs two
POOLINGS = ("mean", "mean+std")


@dataclasses.dataclass
class Wav2SpkConfig:
    """ref: wav2spk.py:37-45 / config/network/wav2spk.yaml (Wav2SpkModuleConfig)."""
    apply_temporal_gating: bool = True
    hidden_fc_layers_out: Tuple[int, ...] = (512, 128)
    embedding_layer_idx: int = 0
    stat_pooling_type: str = "mean+std"

    def __post_init__(self):
        self.hidden_fc_layers_out = tuple(int(h) for h in self.hidden_fc_layers_out)
        if self.stat_pooling_type not in POOLINGS:
            raise ValueError(f"unknown value cfg.stat_pooling_type={self.stat_pooling_type!r}, should be one of "
                             f"['mean', 'mean+std']")
        if self.embedding_layer_idx > len(self.hidden_fc_layers_out):         # (any negative index: the pooled vector)
            raise ValueError("could not determine size of speaker embeddings")

    @property
    def pool_dim(self) -> int:
        return FEATURES * (2 if self.stat_pooling_type == "mean+std" else 1)

    def embedding_size(self, num_speakers: int) -> int:
        """ref: wav2spk.py:98-106 (_determine_embedding_size)."""
        i, hid = self.embedding_layer_idx, self.hidden_fc_layers_out
        return self.pool_dim if i < 0 else hid[i] if i < len(hid) else num_speakers


def wav2spk_frames(n: int) -> Tuple[int, ...]:
    """Frames after each of the five encoder layers over n samples: L' = (L + 2p - k) // s + 1 (3200 -> 640, 160, 80, 40,
    20).  The aggregator keeps the last count."""
    out = []
    for _, _, k, s, p in ENCODER:
        n = conv_out_frames(int(n), k, s, p)
        out.append(n)
    return tuple(out)


def wav2spk_min_samples() -> int:
    """Fewest samples with MIN_FRAMES frames behind every encoder layer (162)."""
    n = MIN_FRAMES
    for _, _, k, s, p in reversed(ENCODER):
        n = (n - 1) * s + k - 2 * p
    return n


def wav2spk_param_shapes(cfg: Wav2SpkConfig, num_speakers: int) -> "OrderedDict[str, Tuple[int, ...]]":
    """The reference's state-dict names in its registration order (encoder, temporal_gate, aggregator, fc_list; the gate is
    a member whether it is applied or not, wav2spk.py:87).  InstanceNorm1d(affine=False) owns nothing."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    for i, (cin, cout, k, _, _) in enumerate(ENCODER):
        s[f"encoder.{i}.0.weight"] = (cout, cin, k)
        s[f"encoder.{i}.0.bias"] = (cout,)
    s["temporal_gate.W"] = (FEATURES, FEATURES)
    s["temporal_gate.b"] = (FEATURES, 1)
    for i, (cin, cout, k, _, _) in enumerate(AGGREGATOR):
        s[f"aggregator.{i}.0.weight"] = (cout, cin, k)
        s[f"aggregator.{i}.0.bias"] = (cout,)
    dims = (cfg.pool_dim,) + cfg.hidden_fc_layers_out + (num_speakers,)
    for i in range(len(dims) - 1):
        s[f"fc_list.{i}.0.weight"] = (dims[i + 1], dims[i])
        s[f"fc_list.{i}.0.bias"] = (dims[i + 1],)
    return s


class Wav2SpkStore(BnArena):
    """Parameter arena of the wav2spk model (f32; no norm layer owns a parameter or a buffer)."""
    PREFIX = ""

    def __init__(self, cfg: Wav2SpkConfig, device, act_dtype: torch.dtype = torch.float32, num_speakers: int = 5994):
        if act_dtype != torch.float32:
            raise NotImplementedError("wav2spk: f32 only (the reference's precision for this experiment)")
        self.cfg, self.num_speakers = cfg, num_speakers
        self.embed_dim = cfg.embedding_size(num_speakers)
        super().__init__(wav2spk_param_shapes(cfg, num_speakers), device, act_dtype)

    def init_weights(self, seed: int = 20211) -> None:
        """torch's defaults: Conv1d / Linear kaiming-uniform(a = sqrt 5) = U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and
        bias; the gate's W and b ``xavier_normal_`` (temporal_gating.py:24-29)."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        fan_in = 1
        for n, s in self.shapes.items():
            if n.startswith("temporal_gate."):
                t = torch.randn(s, generator=g) * math.sqrt(2.0 / (s[0] + s[1]))
            else:
                if n.endswith("weight"):
                    fan_in = math.prod(s[1:])                      # (the bias follows its weight in the arena)
                t = (torch.rand(s, generator=g) * 2 - 1) / math.sqrt(fan_in)
            self.p(n).copy_(t.to(self.device))
        self.sync_lowp()


def valid_sample_lengths(lengths, batch: int, samples: int) -> List[int]:
    """Per-utterance sample counts of a padded [batch, samples] input as Python ints; ValueError unless there is one per row,
    none exceeds ``samples`` and each gives MIN_FRAMES frames behind every encoder layer."""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda or lengths.is_floating_point() or lengths.is_complex():
            raise ValueError("lengths must be Python ints or a CPU integer tensor")
        lengths = lengths.reshape(-1).tolist()
    lens = [int(n) for n in lengths]
    if len(lens) != batch:
        raise ValueError(f"lengths: {len(lens)} values for a batch of {batch}")
    lo = wav2spk_min_samples()
    for n in lens:
        if n > samples:
            raise ValueError(f"lengths: {n} samples is longer than the batch's {samples}")
        if n < lo:
            raise ValueError(f"lengths: {n} samples is shorter than the {lo} the encoder needs for {MIN_FRAMES} frames per layer")
    return lens


K_CHUNK = 128           # longest f32 accumulation chain of a forward convolution product (see _Conv)


def k_chunk(K: int) -> int:
    """The largest divisor of K that is a multiple of 4 (whole 16-byte vectors) and at most K_CHUNK (K itself if none)."""
    return max((d for d in range(4, min(K, K_CHUNK) + 1, 4) if K % d == 0), default=K)


class _Conv:
    """Zero-padded strided Conv1d + bias of one [B*Tin, Cin] activation: w2v2_im2col_zero + the exact-f32 GEMM against the
    packed weight, with the three products and the adjoint gather of its backward.

    The exact-f32 GEMM accumulates each output as ONE k-ordered fma chain, whose rounding error grows with the square root
    of its length: over K = 1536 it loses 2.6 times what torch's blocked f32 sum loses (4.9e-7 against 1.9e-7 rel-L2), which
    put the whole chain outside twice torch-f32's own error.  So the K range is cut into S chunks of k_chunk(K) <= 128 -- one
    batched product into ``parts`` [S, M, Cout] -- which w2v2_sum_bias_act_rows adds in a fixed order, in double, with the
    bias (and the aggregator's ReLU); a K of at most 128 would stay one product with the bias epilogue.

    Evaluation plans hand the GEMM a SEGMENTED A operand (one segment per utterance: the same addresses): the routing
    then keeps the product on the register-staged kernel whatever the number of rows, so that a row of a padded batch and
    the utterance alone go through the same arithmetic (the LDS-DMA kernel, which takes plain operands with more than 64
    rows, orders its sums differently)."""

    def __init__(self, plan: "Wav2SpkPlan", name: str, x: torch.Tensor, Tin: int, geom):
        cin, cout, k, s, p = geom
        st, B, dev, f32 = plan.store, plan.B, plan.dev, torch.float32
        self.plan, self.x, self.Tin, self.geom = plan, x, Tin, geom
        self.Tout = conv_out_frames(Tin, k, s, p)
        self.M, self.K, self.cin, self.cout = B * self.Tout, k * cin, cin, cout
        self.n_w, self.n_b = name + "weight", name + "bias"
        self.wp = torch.empty(cout, self.K, dtype=f32, device=dev)           # packed [cout][tap][cin] operand
        self.col = torch.empty(self.M, self.K, dtype=f32, device=dev)
        self.z = torch.empty(self.M, cout, dtype=f32, device=dev)
        self.Kc = k_chunk(self.K)
        self.S = self.K // self.Kc
        seg = (0, 0) if plan.train else (self.Tout, self.Tout * self.K)
        if self.S == 1:
            self.parts = None
            self.g_fwd = Gemm(self.M, cout, self.K, self.col, self.wp, self.z, lda=self.K, ldb=self.K, ldc=cout,
                              epilogue=EPI_BIAS, bias=st.p(self.n_b), a_seg=seg)
        else:
            self.parts = torch.empty(self.S, self.M, cout, dtype=f32, device=dev)
            self.g_fwd = Gemm(self.M, cout, self.Kc, self.col, self.wp, self.parts, lda=self.K, ldb=self.K, ldc=cout,
                              batch=self.S, batch_inner=self.S, a_strides=(0, self.Kc), b_strides=(0, self.Kc),
                              c_strides=(0, self.M * cout), a_seg=seg)
        if plan.train:
            M, K = self.M, self.K
            self.dz = torch.empty(M, cout, dtype=f32, device=dev)
            self.dwp = torch.zeros(cout, K, dtype=f32, device=dev)
            self.dcol = torch.empty(M, K, dtype=f32, device=dev)
            # the token dimension of the weight-gradient product split over the idle workgroup slots (ecapa.f32_dw_split)
            sk = f32_dw_split(cout, K, M)
            self._ztab = torch.tensor([[0, cout * K]], dtype=torch.int64, device=dev) if sk > 1 else None
            self.g_dw = Gemm(cout, K, M, self.dz, self.col, self.dwp, lda=cout, ldb=K, ldc=K, transA=True, transB=True,
                             split_k=sk, accumulate=sk > 1)
            self.g_dx = Gemm(M, K, cout, self.dz, self.wp, self.dcol, lda=cout, ldb=K, ldc=K, transB=True)

    def refresh(self) -> None:
        ops.pack_conv_weight(self.plan.store.p(self.n_w), self.wp)

    def forward(self, relu: bool = False, lens: Optional[torch.Tensor] = None) -> None:
        """self.z = act(conv(x) + bias); lens (with ``relu``: the aggregator): zeros in the rows past each utterance's frames."""
        cin, cout, k, s, p = self.geom
        ops.im2col_zero(self.x, cin, self.col, self.plan.B, self.Tin, cin, k, s, p)
        self.g_fwd()
        if self.parts is not None:
            ops.sum_bias_act_rows(self.parts, self.plan.store.p(self.n_b), self.z, self.plan.B, self.Tout, cout, relu, lens)
        elif relu or lens is not None:
            ops.sum_bias_act_rows(self.z[None], None, self.z, self.plan.B, self.Tout, cout, relu, lens)

    def backward(self, dx: Optional[torch.Tensor], bias_grad: bool) -> None:
        """From self.dz: dW (and, with ``bias_grad``, db) added into the arena, dx [B*Tin, Cin] written (None: not needed)."""
        st = self.plan.store
        cin, cout, k, s, p = self.geom
        if bias_grad:
            ops.colsum(self.dz, st.g(self.n_b), self.M, cout)
        if self._ztab is not None:
            ops.zero_ranges(self.dwp.view(-1), self._ztab, blocks_per_range=64)
        self.g_dw()
        ops.unpack_conv_grad(self.dwp.view(cout, k, cin), st.g(self.n_w))
        if dx is not None:
            self.g_dx()
            ops.col2im_zero(self.dcol, dx, cin, self.plan.B, self.Tin, cin, k, s, p)


class _EncoderLayer:
    """Conv1d -> InstanceNorm1d -> ReLU.  Layer 0 has no _Conv: w2v2_conv1d_first reads the plan's waveform."""

    def __init__(self, plan: "Wav2SpkPlan", idx: int, x: Optional[torch.Tensor], Tin: int):
        self.plan, self.idx, self.geom = plan, idx, ENCODER[idx]
        cin, cout, k, s, p = self.geom
        B, dev, f32 = plan.B, plan.dev, torch.float32
        self.name = f"encoder.{idx}.0."
        self.T = conv_out_frames(Tin, k, s, p)
        self.M, self.C = B * self.T, cout
        self.conv = _Conv(plan, self.name, x, Tin, self.geom) if idx > 0 else None
        self.z = self.conv.z if self.conv else torch.empty(self.M, cout, dtype=f32, device=dev)
        self.y = torch.empty(self.M, cout, dtype=f32, device=dev)
        self.mean_rstd = torch.empty(B, cout, 2, dtype=f32, device=dev)
        self.work = ops.instnorm_workspace(B, self.T, cout, dev)
        if plan.train:
            self.dz = self.conv.dz if self.conv else torch.empty(self.M, cout, dtype=f32, device=dev)
            if self.conv is None:
                self.dw_work = ops.conv1d_first_bwd_workspace(self.M, cout, k, dev)

    def forward(self) -> None:
        pl, st = self.plan, self.plan.store
        _, _, k, s, p = self.geom
        if self.conv is None:
            ops.conv1d_first(pl.wav, st.p(self.name + "weight"), st.p(self.name + "bias"), self.z, self.C, k, s, p,
                             lens=pl.lens(0))
        else:
            self.conv.forward()
        ops.instnorm_relu_fwd(self.z, self.C, self.work, self.mean_rstd, self.y, self.C, pl.B, self.T, self.C,
                              lens=pl.lens(self.idx + 1))

    def backward(self, dy: torch.Tensor, dx: Optional[torch.Tensor]) -> None:
        """dy = d(loss)/d(y) -> dW into the arena, dx written.  The bias gradient is exact zero (module docstring)."""
        pl, st = self.plan, self.plan.store
        _, _, k, s, p = self.geom
        ops.instnorm_relu_bwd(dy, self.C, self.z, self.C, self.y, self.C, self.mean_rstd, self.work, self.dz, self.C, pl.B,
                              self.T, self.C)
        if self.conv is None:
            ops.conv1d_first_bwd(pl.wav, self.dz, self.C, self.dw_work, st.g(self.name + "weight"), k, s, p)
        else:
            self.conv.backward(dx, bias_grad=False)


class _Gate:
    """TemporalGate: y = sigmoid(x W^T + b) * x over the [M, 512] rows."""

    def __init__(self, plan: "Wav2SpkPlan", x: torch.Tensor, M: int):
        st, dev, f32, F = plan.store, plan.dev, torch.float32, FEATURES
        self.plan, self.x, self.M = plan, x, M
        self.W, self.b = st.p("temporal_gate.W"), st.p("temporal_gate.b").view(F)
        self.P = torch.empty(M, F, dtype=f32, device=dev)
        self.y = torch.empty(M, F, dtype=f32, device=dev)
        seg = (0, 0) if plan.train else (plan.T, plan.T * F)          # evaluation: one kernel whatever M is (see _Conv)
        self.g_fwd = Gemm(M, F, F, x, self.W, self.P, lda=F, ldb=F, ldc=F, epilogue=EPI_BIAS, bias=self.b, a_seg=seg)
        if plan.train:
            self.dP = torch.empty(M, F, dtype=f32, device=dev)
            sk = f32_dw_split(F, F, M)
            self.g_dw = Gemm(F, F, M, self.dP, x, st.g("temporal_gate.W"), lda=F, ldb=F, ldc=F, transA=True, transB=True,
                             split_k=sk, accumulate=True)
            self._g_dx = {}

    def forward(self) -> None:
        self.g_fwd()
        ops.gate_fwd(self.P, self.x, self.y)

    def backward(self, dy: torch.Tensor, dx: torch.Tensor) -> None:
        """dx = dy * s + dP W (written); dW, db added into the arena."""
        st, F = self.plan.store, FEATURES
        ops.gate_bwd(dy, self.P, self.x, self.dP, dx)
        ops.colsum(self.dP, st.g("temporal_gate.b").view(F), self.M, F)
        self.g_dw()
        key = dx.data_ptr()
        if key not in self._g_dx:
            self._g_dx[key] = Gemm(self.M, F, F, self.dP, self.W, dx, lda=F, ldb=F, ldc=F, transB=True, epilogue=EPI_ADD,
                                   aux=dx, ldaux=F)
        self._g_dx[key]()


class _AggLayer:
    """Conv1d(512, 512, 3, 1, 1, bias) -> ReLU: _Conv, whose fold of the partial products adds the bias and applies the ReLU."""

    def __init__(self, plan: "Wav2SpkPlan", idx: int, x: torch.Tensor, T: int):
        self.plan, self.T = plan, T
        self.conv = _Conv(plan, f"aggregator.{idx}.0.", x, T, AGGREGATOR[idx])
        self.y = self.conv.z                                               # post-ReLU

    def forward(self) -> None:
        pl = self.plan
        self.conv.forward(relu=True, lens=pl.lens(len(ENCODER)))

    def backward(self, dy: torch.Tensor, dx: torch.Tensor) -> None:
        ops.act_bwd(dy, self.y, self.conv.dz, 0)
        self.conv.backward(dx, bias_grad=True)


class Wav2SpkHead:
    """The fc_list over a pooled buffer [B, pool_dim]: heads.FcStack (hidden Linear + ReLU) and ClassifierHead("ce") (the last
    Linear with the loss).  Also the prediction path of an embedding taken at ``embedding_layer_idx``."""

    def __init__(self, store: Wav2SpkStore, batch: int, pooled: torch.Tensor, train: bool):
        cfg = store.cfg
        hid = cfg.hidden_fc_layers_out
        self.store, self.B, self.train, self.n_hidden = store, batch, train, len(hid)
        self.fc = FcStack(store, batch, cfg.pool_dim, hid, pooled, train)
        last = f"fc_list.{len(hid)}.0."
        p, g = store.p, store.g
        self.head = ClassifierHead("ce", batch, self.fc.dims[-1], store.num_speakers, w_master=p(last + "weight"),
                                   w_operand=store.w(last + "weight"), w_grad=g(last + "weight") if train else None,
                                   bias=p(last + "bias"), bias_grad=g(last + "bias") if train else None, emb=self.fc.x[-1],
                                   act_dtype=torch.float32, train=train)

    def forward_backward(self, label: torch.Tensor):
        """(loss, softmax [B, speakers]); in training every fc_list gradient into the arena and d(loss)/d(pooled) into
        ``self.dpooled``."""
        self.fc.forward()
        out = self.head.forward_backward(label)
        if self.train:
            self.dpooled = self.fc.backward(self.head.demb)
        return out

    def log_probabilities(self, from_layer: int = 0) -> torch.Tensor:
        """Log-softmax output [B, speakers] of the stack run from hidden layer ``from_layer`` on (its input already in
        ``self.fc.x[from_layer]``).  The log-softmax of the [B, speakers] logits is one torch call, as in xvector.py."""
        for i in range(from_layer, self.n_hidden):
            ops.skinny_linear_fwd(self.fc.x[i], self.fc.w[i], self.fc.b[i], self.fc.x[i + 1], ops.ACT_RELU)
        self.head._forward_logits()
        return torch.log_softmax(self.head.logits[:, :self.head.C], dim=1)


class Wav2SpkPlan:
    """Static plan of one wav2spk forward (+ backward) for a fixed [B, N] waveform input."""

    def __init__(self, store: Wav2SpkStore, batch: int, samples: int, *, train: bool):
        cfg = store.cfg
        self.store, self.cfg, self.B, self.N, self.train = store, cfg, batch, samples, train
        self.dev = dev = store.device
        f32 = torch.float32
        self.frames = wav2spk_frames(samples)
        if samples < wav2spk_min_samples():
            raise ValueError(f"wav2spk: {samples} samples give {self.frames} frames per encoder layer; every layer needs "
                             f"{MIN_FRAMES} (at least {wav2spk_min_samples()} samples)")
        self.T = self.frames[-1]
        B, M, F = batch, batch * self.T, FEATURES
        self.wav = torch.empty(B, samples, dtype=f32, device=dev)
        # variable-length evaluation: device int32 [6, B] = samples, then frames behind each encoder layer; one upload
        self._len_dev, self._len_on = None, False
        self.sample_lengths: Optional[List[int]] = None
        self.encoder: List[_EncoderLayer] = []
        x, Tin = None, samples
        for i in range(len(ENCODER)):
            self.encoder.append(_EncoderLayer(self, i, x, Tin))
            x, Tin = self.encoder[-1].y, self.encoder[-1].T
        self.gate = _Gate(self, x, M) if cfg.apply_temporal_gating else None
        x = self.gate.y if self.gate else x
        self.aggregator: List[_AggLayer] = []
        for i in range(len(AGGREGATOR)):
            self.aggregator.append(_AggLayer(self, i, x, self.T))
            x = self.aggregator[-1].y
        self.pool_mode = ops.POOL_MODES[cfg.stat_pooling_type]
        self.pooled = torch.empty(B, cfg.pool_dim, dtype=f32, device=dev)
        self.head = Wav2SpkHead(store, B, self.pooled, train)
        if train:
            # d(loss)/d(stage output): one buffer per encoder layer, one for the gate's output, one per aggregator layer
            self.d_enc = [torch.empty(l.M, l.C, dtype=f32, device=dev) for l in self.encoder]
            self.d_gate = torch.empty(M, F, dtype=f32, device=dev) if self.gate else None
            self.d_agg = [torch.empty(M, F, dtype=f32, device=dev) for _ in self.aggregator]
        self._version = -1

    def _convs(self) -> List[_Conv]:
        return [l.conv for l in self.encoder if l.conv is not None] + [l.conv for l in self.aggregator]

    def _refresh(self) -> None:
        if self._version != self.store.version:
            for c in self._convs():
                c.refresh()
            self._version = self.store.version

    def lens(self, level: int) -> Optional[torch.Tensor]:
        """Device lengths at ``level`` (0: samples, i: frames behind encoder layer i - 1) of a variable-length forward."""
        return self._len_dev[level] if self._len_on else None

    def _set_lengths(self, lengths) -> None:
        if self.train:
            raise NotImplementedError("lengths: evaluation plans only (the backward has no variable-length form)")
        ns = valid_sample_lengths(lengths, self.B, self.N)
        if self._len_dev is None:
            self._len_dev = torch.empty(1 + len(ENCODER), self.B, dtype=torch.int32, device=self.dev)
        table = [ns] + [list(col) for col in zip(*(wav2spk_frames(n) for n in ns))]
        self._len_dev.copy_(torch.tensor(table, dtype=torch.int32))
        self._len_on, self.sample_lengths = True, ns

    def forward(self, wav: torch.Tensor, lengths=None) -> torch.Tensor:
        """ref: wav2spk.py:269-292 up to the pooling: wav [B, N] f32 on the device -> the pooled vector [B, pool_dim].
        lengths: valid SAMPLES per utterance (ints or a CPU integer tensor, wav2spk_min_samples() <= n <= N; evaluation
        plans).  Samples past an utterance's own count never enter the arithmetic, every stage writes zeros into the rows
        past its own frame count, and row b equals the utterance alone in a (1, n) plan."""
        if wav.dim() != 2 or tuple(wav.shape) != (self.B, self.N):
            raise ValueError(f"wav2spk: a plan of {self.B} x {self.N} samples got {tuple(wav.shape)}")
        assert wav.is_cuda and wav.dtype == torch.float32
        self._len_on, self.sample_lengths = False, None
        if lengths is not None:
            self._set_lengths(lengths)
        self._refresh()
        self.wav.copy_(wav)
        for l in self.encoder:
            l.forward()
        if self.gate:
            self.gate.forward()
        for l in self.aggregator:
            l.forward()
        x = self.aggregator[-1].y.view(self.B, self.T, FEATURES)
        if self._len_on:
            ops.pool_fwd_len(x, self.pooled, self.lens(len(ENCODER)), self.pool_mode)
        else:
            ops.pool_fwd(x, self.pooled, self.pool_mode)
        return self.pooled

    def speaker_embedding(self, embedding_layer_idx: Optional[int] = None) -> torch.Tensor:
        """ref: wav2spk.py:235-252 (_fc_head_ops_pre_spk_embedding) behind forward(): -1 the pooled vector, i the
        post-ReLU output of hidden layer i, len(hidden) the log-probabilities."""
        i = self.cfg.embedding_layer_idx if embedding_layer_idx is None else embedding_layer_idx
        if i < 0:
            return self.pooled
        if i < self.head.n_hidden:
            return self.head.fc.forward(upto=i)
        if i == self.head.n_hidden:
            return self.head.log_probabilities()
        raise ValueError("could not determine size of speaker embeddings")

    def embed(self, wav: torch.Tensor, lengths=None, embedding_layer_idx: Optional[int] = None) -> torch.Tensor:
        """ref: wav2spk.py:269-292 (compute_speaker_embedding): wav [B, N] -> [B, embedding size] f32."""
        self.forward(wav, lengths)
        return self.speaker_embedding(embedding_layer_idx)

    def head_forward_backward(self, label: torch.Tensor):
        return self.head.forward_backward(label)

    def backward(self) -> None:
        """Backward of forward() from the head's d(loss)/d(pooled): every parameter gradient into store.grad."""
        assert self.train
        agg, enc = self.aggregator, self.encoder
        x = agg[-1].y.view(self.B, self.T, FEATURES)
        ops.pool_bwd(x, self.pooled, self.head.dpooled, self.d_agg[-1], self.pool_mode)
        below = self.d_gate if self.gate else self.d_enc[-1]
        for i in range(len(agg) - 1, -1, -1):
            agg[i].backward(self.d_agg[i], self.d_agg[i - 1] if i > 0 else below)
        if self.gate:
            self.gate.backward(self.d_gate, self.d_enc[-1])
        for i in range(len(enc) - 1, -1, -1):
            enc[i].backward(self.d_enc[i], self.d_enc[i - 1] if i > 0 else None)


class Wav2SpkTrainer(EcapaTrainer):
    """One training step: forward, fc head + cross-entropy, backward, fused optimiser step (ref:
    speaker_recognition_module.py:207-220).  The step, gradient clipping, the accumulation window and the data-parallel
    all-reduce of the flat gradient arena are EcapaTrainer's (a fused.WindowedTrainer): the plan has the same entry points."""

    def _embed(self, x: torch.Tensor) -> None:
        self.plan.forward(x)
