"""Static execution plans for the wav2vec2 speaker path on one MI355X.

A ``Plan`` is built once per (batch, samples, mode): it allocates every activation / saved-for-backward
buffer out of HBM up front (the whole base model at B=66 needs ~3 GB of 288 GB) and pre-builds every
GEMM descriptor over those fixed buffers, so a training step is a flat sequence of C-ABI launches on
one HIP stream with no allocation, no autograd graph and no host<->device sync.  Forward and the
hand-written backward follow SURVEY.md 3.2 / 8(a) rows a2-a14 (HF:382-726 +
ref: src/layers/pooling.py, src/optim/loss/aam_softmax.py, src/optim/loss/cross_entropy.py).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import ops
from .config import W2V2Config, Wav2Vec2RegularisationConfig
from .ops import (EPI_ADD, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_GRAD, EPI_GELU_BWD, EPI_MUL, EPI_NONE, EPI_SCALE_RC, Gemm,
                  POOL_MODES,
                  WgradGroup)
from .params import W2V_PREFIX, ParamStore

_SITE = {"featproj": 1, "prologue": 2, "attn": 3, "post_attn": 4, "ffn": 5, "act": 6, "final": 7}


def _splitk(m_tiles: int, n_tiles: int, k: int, batch: int = 1) -> int:
    """Split K of the weight-gradient GEMMs (K = tokens) until ~2 workgroups per CU are in flight."""
    blocks = max(1, m_tiles * n_tiles * batch)
    s = max(1, min(16, 512 // blocks))
    while s > 1 and k // s < 256:
        s -= 1
    return s


def _tiles(n: int, t: int = 128) -> int:
    return (n + t - 1) // t


def _pad64(n: int) -> int:
    """n rounded up to a multiple of 64: the padded token rows of a K-major weight-gradient operand (csrc/wgrad.hip)."""
    return (n + 63) // 64 * 64


def _wb(name: str):
    return name + ".weight", name + ".bias"


@dataclass(frozen=True)
class PlanSwitches:
    """The environment switches of a plan, read ONCE when it is constructed (like W2v2Switches on the C side): descriptors,
    buffers and the backward schedule are all built from the same record, whatever the environment does afterwards."""
    wgrad_group: int = 0              # W2V2_WGRAD_GROUP: blocks per grouped weight-gradient launch, 1 / 2 / 4 (0: the plan decides)
    no_wgrad_pairs: bool = False      # W2V2_NO_WGRAD_PAIRS: one weight-gradient launch per block
    no_ln_fold: bool = False          # W2V2_NO_LN_FOLD: one gamma / beta fold launch per LayerNorm
    no_posconv_direct: bool = False   # W2V2_NO_POSCONV_DIRECT: positional convolution through the implicit GEMM
    pos_dw_gemm: bool = False         # W2V2_POS_DW_GEMM: its weight gradient through the transposing GEMM

    @classmethod
    def from_env(cls) -> "PlanSwitches":
        env = os.environ.get
        group = env("W2V2_WGRAD_GROUP")
        return cls(max(1, min(4, int(group))) if group else 0, bool(env("W2V2_NO_WGRAD_PAIRS")),
                   bool(env("W2V2_NO_LN_FOLD")), bool(env("W2V2_NO_POSCONV_DIRECT")), bool(env("W2V2_POS_DW_GEMM")))


def encoder_backward_schedule(num_layers: int, skip: Sequence[int], pair_uppers: Sequence[int], grouped: bool = True,
                              group: int = 2):
    """Order of the encoder part of one backward pass, as plain data (no device work): a list of events
        ("body", l)        data-gradient chain of layer l up to and including the attention backward; its LayerNorm
                           gamma/beta partials are parked in the fold group; without the grouped weight-gradient
                           kernel (f32 mode) it also writes the layer's weight gradients
        ("wgrad", layers)  one grouped weight-gradient launch writing dW / dbias of `layers` (one layer, or a pair
                           (upper, upper - 1) whose dY buffers live in the two alternating scratch sets)
        ("dx", l)          G += DQKV Wqkv of layer l
        ("fold",)          gamma/beta of every LayerNorm parked since the last fold are added to the gradients
        ("notify", l)      gradient bucket "layer l" is final (LayerDrop-skipped layers: zero gradient, final at once)
    `pair_uppers` = upper layers of the weight-gradient pairs (Plan.g_wgrad_pair); `skip` = this step's LayerDrop
    decisions.  Plan.backward executes exactly this list; tests/test_host_cpu.py checks its invariants (every bucket
    is notified once, in descending order, after its last writer) for every skip pattern."""
    if grouped and group > 2:
        # Groups of `group` NON-SKIPPED layers, counted down from the top (round 6: wav2vec2-large, whose 192 tiles of
        # 256 x 256 per layer fill 256 CUs badly in ones -- 0.75 -- and in pairs -- 1.5 rounds -- but well in fours: 3.0).
        # Every layer has its OWN dY scratch set in this mode (3.5 GB of the 288 at wav2vec2-large), so a group may span
        # LayerDrop-skipped layers and its launch may come after the data-gradient products of its last member.  Buckets
        # are notified once, in descending order, after their last writer: a skipped layer inside an open group waits for
        # the group's launch.
        ev, held, skip, pending_top = [], [], set(skip), num_layers - 1

        def flush(down_to):
            nonlocal held, pending_top
            if held:
                ev.extend([("wgrad", tuple(held)), ("fold",)])
            ev.extend(("notify", h) for h in range(pending_top, down_to - 1, -1))
            held, pending_top = [], down_to - 1
        for l in reversed(range(num_layers)):
            if l in skip:
                if not held:
                    flush(l)                      # nothing open: the zero-gradient bucket is final at once
                continue
            ev.append(("body", l))
            held.append(l)
            ev.append(("dx", l))
            if len(held) == group:
                flush(l)
        flush(0)
        return ev
    ev, held, Ltop, skip, pair_uppers = [], None, num_layers - 1, set(skip), set(pair_uppers)
    for l in reversed(range(num_layers)):
        upper = grouped and (Ltop - l) % 2 == 0 and l > 0 and l in pair_uppers      # l pairs with l - 1
        if l in skip:
            if held is not None:          # partner skipped by LayerDrop: the held layer goes alone
                ev += [("wgrad", (held,)), ("fold",), ("notify", held)]
                held = None
            ev.append(("notify", l))
            continue
        ev.append(("body", l))
        if grouped:
            if held is not None:
                ev.append(("wgrad", (held, l)))
            elif not upper:
                ev.append(("wgrad", (l,)))
        ev.append(("dx", l))
        if grouped and held is None and upper:
            held = l                      # wait for layer l - 1 (its dY's live in the other buffer set)
            continue
        ev.append(("fold",))
        if held is not None:
            ev.append(("notify", held))
            held = None
        ev.append(("notify", l))
    assert held is None
    return ev


def mix_injection_points(events, num_layers: int):
    """Where Plan.backward(dmix=, mix_weights=) adds w_j * dm into the running activation gradient G, derived from the event
    list of encoder_backward_schedule (plain data, no device work): a list of (index, lo, hi, overwrite) -- before event
    `index` (len(events): behind the last one, in front of the prologue backward) G = (0 if overwrite else G) +
    (w_lo + ... + w_hi) dm.  G must hold the full gradient of X[l + 1] when the data-gradient chain ("body") of layer l
    starts, and it passes through a LayerDrop-skipped layer unchanged: the states above a body that have not been added
    yet go in as ONE add in front of it, the first add (which holds j = L) overwrites instead of the pool backward, and
    what is left (j = 0 at least) goes in behind the last event."""
    points, hi = [], num_layers
    for i, ev in enumerate(events):
        if ev[0] == "body":
            l = ev[1]
            points.append((i, l + 1, hi, hi == num_layers))
            hi = l
    points.append((len(events), 0, hi, hi == num_layers))
    return points


def mix_backward_check(*, train: bool, stable: bool, scaler, B: int, T: int, H: int, L: int, dmix, mix_weights,
                       demb=None, dhidden=None) -> None:
    """The argument rules of Plan.backward(dmix=, mix_weights=), checked before any device work."""
    if (dmix is None) != (mix_weights is None):
        raise ValueError("backward: dmix and mix_weights come together (the gradient of the layer mix and its J = L + 1 "
                         "softmax weights)")
    if dmix is None:
        return
    if demb is not None or dhidden is not None:
        raise ValueError("backward: dmix replaces demb / dhidden (the mix's gradient arrives at every layer output)")
    if not train:
        raise ValueError("backward: dmix needs a training plan")
    if stable:
        raise NotImplementedError("do_stable_layer_norm: the layer-mix backward (dmix) is built for the post-LN encoder only")
    if scaler is not None:
        raise NotImplementedError("backward(dmix=): f16 encoder training is not supported here -- the store has a loss "
                                  "scaler and the ECAPA side that produces dmix has none")
    if not isinstance(dmix, torch.Tensor) or dmix.numel() != B * T * H or dmix.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"backward: dmix is [B, T, H] = [{B}, {T}, {H}] in float32 or bfloat16")
    if not dmix.is_contiguous():
        raise ValueError("backward: dmix must be contiguous")
    if (not isinstance(mix_weights, torch.Tensor) or mix_weights.dtype != torch.float32 or mix_weights.dim() != 1
            or mix_weights.numel() != L + 1):
        raise ValueError(f"backward: mix_weights is a float32 vector of J = L + 1 = {L + 1} softmax weights on the device")


def valid_lengths(cfg: W2V2Config, lengths, batch: int, n_samples: int) -> List[int]:
    """Per-utterance valid sample counts of a variable-length forward as Python ints, checked against the plan: one per
    row, at most the plan's N, and long enough for one encoder frame (400 samples for the standard conv stack)."""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda or lengths.is_floating_point() or lengths.is_complex():
            raise ValueError("lengths must be Python ints or a CPU integer tensor")
        lengths = lengths.reshape(-1).tolist()
    lens = [int(n) for n in lengths]
    if len(lens) != batch:
        raise ValueError(f"lengths: {len(lens)} values for a batch of {batch}")
    for n in lens:
        if n > n_samples:
            raise ValueError(f"lengths: {n} samples is longer than the plan's {n_samples}")
        if min(cfg.conv_lengths(n)) < 1:
            raise ValueError(f"lengths: {n} samples is too short for one encoder frame")
    return lens


@dataclass
class LayerBufs:
    qkv: torch.Tensor
    ctx: torch.Tensor
    a: torch.Tensor        # out-proj output, overwritten with s1 = x + drop(a)
    x1: torch.Tensor
    hpre: torch.Tensor     # gelu'(FFN pre-activation), written by the FFN1 epilogue (training plans)
    h: torch.Tensor
    f: torch.Tensor        # FFN output, overwritten with s2
    mean1: torch.Tensor
    rstd1: torch.Tensor
    mean2: torch.Tensor
    rstd2: torch.Tensor
    lse: Optional[torch.Tensor] = None      # fused attention
    p: Optional[torch.Tensor] = None        # unfused attention probabilities
    pd: Optional[torch.Tensor] = None       # ... after dropout


class Plan:
    def __init__(self, store: ParamStore, batch: int, n_samples: int, *, train: bool,
                 reg: Optional[Wav2Vec2RegularisationConfig] = None, pooling: str = "mean+std",
                 insert_cls_token: bool = False, cls_token_constant: float = 1.0,
                 aam_margin: float = 0.2, aam_scale: float = 30.0, fused_attention: Optional[bool] = None,
                 seed: int = 7, keep_hidden_states: bool = False, paired: bool = False,
                 sep_token_constant: float = -1.0, encoder_frames: Optional[int] = None,
                 triplet_margin: float = 1.0, triplet_coef: float = 1.0, final_dropout: float = 0.0,
                 max_target: int = ops.CTC_LONG_MAX_TARGET, sub_centers: Optional[int] = None,
                 margin_type: str = "arc", inter_topk: int = 0, inter_margin: float = 0.06):
        cfg = store.cfg
        # the margin heads (heads.ClassifierHead): the sub-centre count is the store's (it shapes loss_fn.fc_weights)
        K = getattr(store, "sub_centers", 1)
        if sub_centers is not None and int(sub_centers) != K:
            raise ValueError(f"plan: sub_centers {sub_centers}, but the parameter store was built with {K}")
        self.margin_kw = dict(sub_centers=K, margin_type=margin_type, inter_topk=int(inter_topk),
                              inter_margin=float(inter_margin))
        # the letter head (store.head "letter"): dropout in front of its Linear, the longest transcript it holds
        self.final_dropout, self.max_target = float(final_dropout), int(max_target)
        self.triplet_margin, self.triplet_coef = float(triplet_margin), float(triplet_coef)
        self.store, self.cfg, self.B, self.N, self.train = store, cfg, batch, n_samples, train
        # paired input (ref: wav2vec2_paired_input.py:163-207): the conv stack and projection run on 2B waveforms (first
        # B = left, last B = right utterance of each pair); the encoder sees B sequences [CLS] left [SEP] right [SEP]
        self.paired, self.sep_c = paired, sep_token_constant
        self.Bc = 2 * batch if paired else batch
        assert not (paired and insert_cls_token)
        self.reg = reg if reg is not None else Wav2Vec2RegularisationConfig()
        # "random" (IndexPool1D, ref: src/layers/pooling.py:125-126,150-154): one frame index per forward call, drawn on
        # the host with random.randint like the reference.  "none" (NoPooling, :160-166): no pooling, every frame is an
        # embedding -- the head then sees B * T rows and the label of an utterance repeated for each of its frames
        # (ref: speaker_recognition_module.py:246-267 _train_step_ce_loss_no_pooling)
        pooling = pooling.lower() if pooling.lower() == "none" else pooling
        self.pooling, self.pool_mode = pooling, POOL_MODES.get(pooling, -1)
        assert pooling in ("attentive", "random", "none") or pooling in POOL_MODES, pooling
        self.no_pool = pooling == "none"
        if train and store.head == "ctc" and not self.no_pool:
            raise ValueError(f"a training plan of a \"ctc\" store needs pooling=\"none\" (got {pooling!r}): the CTC loss acts "
                             "on the logits of every frame (ref: config/experiment/speaker_wav2vec2_ctc.yaml "
                             "stat_pooling_type: none)")
        if store.head == "letter" and not self.no_pool:
            raise ValueError(f"a plan of a \"letter\" store needs pooling=\"none\" (got {pooling!r}): the letter head "
                             "predicts the vocabulary on every frame (ref: config/experiment/speech_wav2vec2_ctc.yaml)")
        self._rand_idx = 0
        self.cls, self.cls_c = insert_cls_token, cls_token_constant
        self.margin, self.scale = aam_margin, aam_scale
        self.seed = seed
        # eval plans normally ping-pong two activation buffers; keeping all L+1 of them gives HF's
        # ``output_hidden_states`` (ref: wav2vec2_fc.py:440-463 ensemble of layers)
        self.all_x = train or keep_hidden_states
        self.dev, self.adt = store.device, store.act_dtype
        # encoder-only paired plan (Plan.pair_encoder): sequences of exactly `encoder_frames` frames assembled from a feature
        # matrix the caller holds (embed_pairs); no conv stack, no projection, none of their buffers
        self.enc_only = encoder_frames is not None
        if self.enc_only and (not paired or train or n_samples != 0 or encoder_frames < 5):
            raise ValueError("encoder_frames: an evaluation plan with paired=True, n_samples=0 and at least 5 frames "
                             "([CLS] l [SEP] r [SEP]); build it with Plan.pair_encoder")
        self.lens = [0] * len(cfg.conv_dim) if self.enc_only else cfg.conv_lengths(n_samples)
        self.T0 = self.lens[-1]                       # frames out of the CNN
        if self.enc_only:
            self.T = int(encoder_frames)
        else:
            self.T = 2 * self.T0 + 3 if paired else self.T0 + (1 if insert_cls_token else 0)
        self.M0, self.M = self.Bc * self.T0, batch * self.T
        H, d = cfg.hidden_size, cfg.head_dim
        if fused_attention is None:
            fused_attention = ops.is16(self.adt) and d == 64        # any T (tiled kernels beyond 160 frames)
        self.fused = fused_attention
        # checkpoint families (config.W2V2Config): pre-LN encoder ("stable layer norm", HF:611-654,729-802) and LayerNorm
        # convolutions with bias (HF:275-299) -- the "-lv60" / xlsr models the reference can be pointed at by id
        self.stable = bool(cfg.do_stable_layer_norm)
        self.ln_conv = cfg.feat_extract_norm == "layer"
        if cfg.feat_extract_norm not in ("group", "layer"):
            raise ValueError(f"feat_extract_norm must be 'group' or 'layer', got {cfg.feat_extract_norm!r}")
        if not self.ln_conv and cfg.conv_bias and train and not store.freeze_cnn:
            raise NotImplementedError("feat_extract_norm='group' with conv_bias=True (no published checkpoint has it) has a "
                                      "forward path only: train it with the feature extractor frozen "
                                      "(completely_freeze_feature_extractor: true, the reference's default)")
        if self.stable and (insert_cls_token or paired or keep_hidden_states):
            raise NotImplementedError("do_stable_layer_norm: the CLS-token, paired-input and hidden-state-ensemble paths are "
                                      "built for the post-LN encoder only")
        self.embed_dim = H * (2 if pooling == "attentive" else ops.POOL_WIDTH.get(self.pool_mode, 1))
        self._pack_version = -1
        self._cnn_version = -1
        self._asp = {}
        self.sw = PlanSwitches.from_env()
        # 16-bit training: the weight gradients of a block (or of several) are ONE grouped, atomic-free launch
        self.grouped = train and store.flat_lp_t is not None
        self.wg_group = self._wgrad_group_size() if train else 2
        self.g_wgrad_pair, self._wgrad_cache = {}, {}
        self.head, self.fc, self._lnfold, self.triplet = None, None, None, None
        # variable-length evaluation (forward(..., lengths=)): device int32 table [conv-0 frames | encoder frames] of the
        # current forward, or None on the fixed-length path
        self._len_dev, self._len = None, None
        self.frame_lengths: Optional[List[int]] = None
        # paired variable-length evaluation: device int32 [4, B] = left row | left frames | right row | right frames of the
        # feature matrix the sequences are assembled from (ops.pair_assemble)
        self._pair_dev = None
        self._alloc()
        self._build_gemms()

    @classmethod
    def pair_encoder(cls, store: ParamStore, batch: int, frames: int, **kw) -> "Plan":
        """Encoder-only paired evaluation plan: `batch` sequences [CLS] left [SEP] right [SEP] of at most `frames` frames
        (T = frames exactly), assembled by embed_pairs from rows of a projected-feature matrix (Plan.features).  It holds
        no conv-stack or projection buffer."""
        return cls(store, batch, 0, train=False, pooling="first", paired=True, encoder_frames=frames, **kw)

    def _wgrad_group_size(self) -> int:
        """How many consecutive blocks share one grouped weight-gradient launch: 2 (pairs, since round 3) unless FOUR fill
        the chip's rounds of 256 x 256 tiles strictly better (wav2vec2-large: 192 tiles per block -> pairs 384 = 1.5
        rounds, fours 768 = 3.0).  W2V2_WGRAD_GROUP forces 1 / 2 / 4 (tests, A/B)."""
        if self.sw.wgrad_group:
            return self.sw.wgrad_group
        cfg = self.cfg
        H, I = cfg.hidden_size, cfg.intermediate_size
        c = lambda n: -(-n // 256)
        tiles = c(H) * c(I) * 2 + c(H) * c(H) + c(3 * H) * c(H)
        ncu = torch.cuda.get_device_properties(self.dev).multi_processor_count if self.dev.type == "cuda" else 256
        cost = {k: -(-k * tiles // ncu) / k for k in (2, 4)}
        return 4 if (cfg.num_hidden_layers >= 4 and cost[4] < cost[2] - 1e-9) else 2

    def _wgrad_for(self, layers):
        """The grouped weight-gradient launch covering `layers` (a tuple from encoder_backward_schedule): prebuilt for
        single blocks and for the regular pairs, built on first use (and kept) for every other subset."""
        if len(layers) == 1:
            return self.g_layer[layers[0]]["wgrad"]
        if len(layers) == 2 and layers[0] in self.g_wgrad_pair and layers[1] == layers[0] - 1:
            return self.g_wgrad_pair[layers[0]]
        if layers not in self._wgrad_cache:
            if len(self._wgrad_cache) >= 256:          # LayerDrop patterns: bounded (descriptors only, a few KB each)
                self._wgrad_cache.clear()
            probs = []
            for l in layers:
                probs += self.g_layer[l]["wgrad_problems"]
            self._wgrad_cache[layers] = WgradGroup(probs, self.M, _pad64(self.M))
        return self._wgrad_cache[layers]

    def _x(self, l: int) -> torch.Tensor:
        """Activation buffer of index l: input of block l, output of block l - 1 (all kept, or two in ping-pong)."""
        return self.X[l if self.all_x else l % 2]

    # ------------------------------------------------------------------------------------------ buffers
    def _e(self, *shape, dtype=None) -> torch.Tensor:
        return torch.empty(*shape, dtype=dtype or self.adt, device=self.dev)

    def _ep(self, rows: int, cols: int, pad_rows: int = 0) -> torch.Tensor:
        """[rows, cols] activation whose storage is padded with ZERO rows up to a multiple of 64 (at least
        ``pad_rows``): it can be the K-major operand of the grouped weight-gradient GEMM (csrc/wgrad.hip contract)."""
        rp = max(_pad64(rows), pad_rows)
        full = torch.zeros(rp, cols, dtype=self.adt, device=self.dev)
        v = full[:rows]
        v._w2v2_padded = full
        return v

    def _alloc(self) -> None:
        cfg, B, T, M, H, I = self.cfg, self.B, self.T, self.M, self.cfg.hidden_size, self.cfg.intermediate_size
        f32 = torch.float32
        C = cfg.conv_dim
        Bc = self.Bc
        if self.enc_only:
            self.cnn_train = False
            self.hx = self._e(M, H)                                # encoder input, written by the assemble kernel
            self._alloc_encoder()
            return
        self.stats0 = ops.conv0_workspace(Bc, self.N, C[0], cfg.conv_kernel[0], cfg.conv_stride[0], self.dev)
        self.conv = [self._e(Bc, L, c) for L, c in zip(self.lens, C)]
        cins = (1,) + tuple(C[:-1])
        self.convw = [None] + [self._e(C[i], cfg.conv_kernel[i] * cins[i]) for i in range(1, len(C))]
        self.zero_bias = torch.zeros(max(max(C), H), dtype=f32, device=self.dev)
        self.cnn_train = self.train and not self.store.freeze_cnn
        if self.cnn_train:      # unfrozen feature extractor: pre-activations saved, gradient + im2col scratch
            self.conv_pre = [None] + [self._e(Bc, L, c) for L, c in zip(self.lens[1:], C[1:])]
            self.dconv = [self._e(Bc, L, c) for L, c in zip(self.lens[:-1], C[:-1])]      # d(conv[i] output), i < last
            self.col = self._e(max(Bc * self.lens[i] * cfg.conv_kernel[i] * cins[i] for i in range(1, len(C))))
            self.dwp = torch.zeros(max(C[i] * cfg.conv_kernel[i] * cins[i] for i in range(1, len(C))), dtype=f32,
                                   device=self.dev)
            self.sums0 = self._e(Bc, C[0], 2, dtype=f32)
            if self.ln_conv:        # per-workgroup column partials of the two LayerNorm-GELU backward kernels
                self.lng_ws = self._e(max(ops.lib().w2v2_layernorm_gelu_bwd_workspace_floats(Bc * L, c)
                                          for L, c in zip(self.lens[1:], C[1:])), dtype=f32)
                self.c0l_ws = ops.conv0_layernorm_gelu_bwd_workspace(Bc, self.N, C[0], cfg.conv_kernel[0],
                                                                     cfg.conv_stride[0], self.dev)
        # The projection's weight gradient is ONE small problem (768 x 512 outputs = 12 tiles) over all M0 tokens: alone
        # in a grouped launch it ran on 12 CUs for 144 us.  Its token dimension is cut into PROJ_SLICES slices of
        # proj_slice_len rows (a multiple of 64), each a problem of its own writing its own partial (96 workgroups),
        # summed in a fixed order afterwards -- which needs the two operands zero-padded up to slices * slice_len rows
        self.proj_slices = 8
        self.proj_slice_len = -(-self.M0 // (self.proj_slices * 64)) * 64
        proj_pad = self.proj_slices * self.proj_slice_len
        self.ln_feat = self._ep(self.M0, C[-1], proj_pad)
        self.mean_f, self.rstd_f = self._e(self.M0, dtype=f32), self._e(self.M0, dtype=f32)
        self.h0 = self._e(self.M0, H)                          # projection output (pre-CLS)
        self.hx = self._e(M, H) if (self.cls or self.paired) else self.h0       # encoder input
        self._alloc_encoder(proj_pad)

    def _alloc_encoder(self, proj_pad: int = 0) -> None:
        """Everything from the positional convolution on (the part an encoder-only plan has too)."""
        cfg, B, T, M, H, I = self.cfg, self.B, self.T, self.M, self.cfg.hidden_size, self.cfg.intermediate_size
        f32 = torch.float32
        C = cfg.conv_dim
        G, K = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings
        self.Cg, self.Tp = H // G, T + K - 1
        # the direct convolution kernel is built for 48 (w2v2-base) and 64 (wav2vec2-large, round 6) channels per group at
        # 128 taps; everything else (the tiny test geometry, the exact-f32 mode) runs the implicit GEMM
        self.pos_direct = (ops.is16(self.adt) and self.Cg in (48, 64) and K == 128 and not self.sw.no_posconv_direct)
        self.xg = self._e(B, G, self.Tp, self.Cg)
        self.posw_f, self.posw_b = self._e(G, self.Cg, K * self.Cg), self._e(G, self.Cg, K * self.Cg)
        self.pos_sumsq = ops.weightnorm_scratch(H, G, K, self.dev)
        self.pos = self._e(M, H)                               # GELU(posconv) -> overwritten with s0
        self.pos_pre = self._e(M, H) if self.train else None
        self.mean0, self.rstd0 = self._e(M, dtype=f32), self._e(M, dtype=f32)
        L = cfg.num_hidden_layers
        nset = L if self.train else 1
        self.X = [self._ep(M, H) for _ in range(L + 1 if self.all_x else 2)]
        heads = cfg.num_attention_heads
        self.Tl = (T + 7) // 8 * 8
        self.lb: List[LayerBufs] = []
        for _ in range(nset):
            lb = LayerBufs(qkv=self._e(M, 3 * H), ctx=self._ep(M, H), a=self._e(M, H), x1=self._ep(M, H),
                           hpre=self._e(M, I) if self.train else None, h=self._ep(M, I), f=self._e(M, H),
                           mean1=self._e(M, dtype=f32), rstd1=self._e(M, dtype=f32),
                           mean2=self._e(M, dtype=f32), rstd2=self._e(M, dtype=f32))
            if self.fused:
                lb.lse = self._e(B * heads * T, dtype=f32)
            else:
                lb.p = torch.zeros(B * heads * T, self.Tl, dtype=self.adt, device=self.dev)
                lb.pd = (torch.zeros(B * heads * T, self.Tl, dtype=self.adt, device=self.dev)
                         if (self.train and self.reg.attention_dropout > 0) else lb.p)
            self.lb.append(lb)
        if not self.fused:
            self.S = torch.zeros(B * heads * T, self.Tl, dtype=f32, device=self.dev)   # scores / dP scratch
        E = self.embed_dim
        self.head_rows = B * T if self.no_pool else B          # rows the head sees
        self.emb = self._e(self.head_rows, E, dtype=f32)
        st = self.store
        if st.head == "bce":
            from .heads import BceHead
            self.head = BceHead(self.head_rows, E, w=st.p("linear.weight"), b=st.p("linear.bias"),
                                w_grad=st.g("linear.weight") if self.train else None,
                                b_grad=st.g("linear.bias") if self.train else None, emb=self.emb, train=self.train,
                                loss_scale=st.scaler)
        elif st.head == "ctc" and not self.no_pool:
            pass      # an evaluation plan under test_stat_pooling_type (mean+std in the experiment): embeddings, no loss
        elif st.head == "ctc":
            # ref: config/experiment/speaker_wav2vec2_ctc.yaml (stat_pooling_type: none, optim/loss: ctc) +
            # speaker_recognition_module.py:222-244: one label per utterance over the logits of all its T frames
            from .heads import CtcHead, FcStack
            nh = len(st.hidden_fc)
            self.fc = FcStack(st, self.head_rows, E, st.hidden_fc, self.emb, self.train) if nh else None
            self.head = CtcHead(B, T, st.head_in_dim, st.num_speakers + 1,
                                w_master=st.p(f"fc_list.{nh}.0.weight"), w_operand=st.w(f"fc_list.{nh}.0.weight"),
                                w_grad=st.g(f"fc_list.{nh}.0.weight") if self.train else None,
                                bias=st.p(f"fc_list.{nh}.0.bias"),
                                bias_grad=st.g(f"fc_list.{nh}.0.bias") if self.train else None,
                                emb=self.fc.x[-1] if self.fc is not None else self.emb, act_dtype=self.adt,
                                train=self.train, loss_scale=st.scaler)
        elif st.head == "letter":
            # ref: config/experiment/speech_wav2vec2_ctc.yaml + wav2vec2_fc_letter.py:65-86: dropout + lm_head on every
            # frame, the CTC loss against the transcript
            from .heads import LetterHead
            W, Bn = "speech_recognition_head.lm_head.weight", "speech_recognition_head.lm_head.bias"
            self.head = LetterHead(B, T, st.head_in_dim, st.vocab_size, max_target=self.max_target,
                                   final_dropout=self.final_dropout, w_master=st.p(W), w_operand=st.w(W),
                                   w_grad=st.g(W) if self.train else None, bias=st.p(Bn),
                                   bias_grad=st.g(Bn) if self.train else None, emb=self.emb, act_dtype=self.adt,
                                   train=self.train, loss_scale=st.scaler)
        elif st.head is not None and st.head != "triplet":
            from .heads import ClassifierHead, FcStack
            aam = st.head == "aam"
            nh = len(st.hidden_fc)
            # hidden Linear+ReLU layers between the pooled embedding and the head (ref: wav2vec2_fc.py:185-228)
            self.fc = FcStack(st, self.head_rows, E, st.hidden_fc, self.emb, self.train) if nh else None
            head_in = self.fc.x[-1] if self.fc is not None else self.emb
            wname = "loss_fn.fc_weights" if aam else f"fc_list.{nh}.0.weight"
            bname = f"fc_list.{nh}.0.bias"
            self.head = ClassifierHead("aam" if aam else "ce", self.head_rows, st.head_in_dim, st.num_speakers,
                                       w_master=st.p(wname), w_operand=st.w(wname), w_grad=st.g(wname) if self.train else None,
                                       bias=None if aam else st.p(bname),
                                       bias_grad=None if (aam or not self.train) else st.g(bname),
                                       emb=head_in, act_dtype=self.adt, train=self.train, margin=self.margin,
                                       scale=self.scale, loss_scale=st.scaler, **(self.margin_kw if aam else {}))
        if self.train:
            self.demb = (self.head.demb if (self.head is not None and self.fc is None)
                         else self._e(self.head_rows, E, dtype=f32))
            self.G = self._ep(M, H, 0 if (self.cls or self.paired) else proj_pad)           # running activation gradient
            # Gradient scratch of one layer's backward: Gd = df (after the dropout mask of the FFN residual branch),
            # Gd1 = da (attention residual branch), DH, DQKV.  TWO sets, used by alternating layers: the grouped
            # weight-gradient launch then covers a PAIR of layers (8 problems = 216 tiles of 256x256, one full round
            # of the chip instead of two 216-tile rounds of 256x128), see _build_gemms / backward.
            # two alternating sets for single / paired launches; groups of four get one set PER LAYER (they may span
            # LayerDrop-skipped layers: encoder_backward_schedule)
            self._gsets = [dict(Gd=self._ep(M, H), Gd1=self._ep(M, H), DH=self._ep(M, I), DQKV=self._ep(M, 3 * H))
                           for _ in range(cfg.num_hidden_layers if self.wg_group > 2 else 2)]
            self.DC = self._e(M, H)
            self.P1 = self._e(M, H)
            self.GR = self._e(M, H) if self.stable else None        # pre-LN: gradient of the un-normalised residual stream
            self.dyg = self._e(B, G, self.Tp, self.Cg)
            self.dwf = self._e(G, K * self.Cg, self.Cg, dtype=f32)
            self.pos_dot = ops.weightnorm_scratch(H, G, K, self.dev)
            self.dn = self._e(self.M0, C[-1])
            self.G0 = self._ep(self.M0, H, proj_pad) if (self.cls or self.paired) else None
            if self.fused:
                self.delta = self._e(B * heads * T, dtype=f32)
            else:
                self.dS = torch.zeros(B * heads * T, self.Tl, dtype=self.adt, device=self.dev)
            self._lnfold = ops.LnFoldGroup(H, self.dev)
        if st.head in ("triplet", "triplet_ce"):
            # ref: speaker_recognition_module.py:85-93,269-294: the triplet term acts on the pooled embedding; alone it
            # writes self.demb, next to the CE head it is added to the gradient the CE path has left there
            if self.no_pool:
                raise ValueError("triplet loss does not support no_pooling")
            from .heads import TripletHead
            self.triplet = TripletHead(self.head_rows, E, emb=self.emb, margin=self.triplet_margin,
                                       coef=self.triplet_coef, train=self.train, loss_scale=st.scaler,
                                       demb=self.demb if self.train else None,
                                       accumulate=self.train and st.head == "triplet_ce")
            if st.head == "triplet":
                self.head = self.triplet

    # ------------------------------------------------------------------------------------------ descriptors
    def _build_gemms(self) -> None:
        cfg, st, B, T, M, H, I = self.cfg, self.store, self.B, self.T, self.M, self.cfg.hidden_size, self.cfg.intermediate_size
        C = cfg.conv_dim
        cins = (1,) + tuple(C[:-1])
        # conv layers 1..6: implicit GEMM over the channels-last activation of the previous layer
        self.g_conv = []
        for i in range(1, len(C) if not self.enc_only else 0):
            k, s, ci, co = cfg.conv_kernel[i], cfg.conv_stride[i], cins[i], C[i]
            cbias = st.mp(f"feature_extractor.conv_layers.{i}.conv.bias") if cfg.conv_bias else self.zero_bias
            # layer-norm family: the product only adds the bias; LayerNorm + GELU follow (_cnn_forward) -- in place, or, with
            # the feature extractor unfrozen, from the pre-norm z the product leaves in conv_pre[i] for the backward
            ln_train = self.ln_conv and self.cnn_train
            self.g_conv.append(Gemm(self.Bc * self.lens[i], co, k * ci, self.conv[i - 1], self.convw[i],
                                    self.conv_pre[i] if ln_train else self.conv[i],
                                    lda=s * ci, ldb=k * ci, ldc=co, a_seg=(self.lens[i], self.lens[i - 1] * ci),
                                    epilogue=EPI_BIAS if self.ln_conv else EPI_BIAS_GELU, bias=cbias,
                                    aux=self.conv_pre[i] if (self.cnn_train and not self.ln_conv) else None, ldaux=co))
        if self.cnn_train:
            # conv layer i backward: dW (packed layout, f32 scratch) and the im2col-space data gradient
            self.g_conv_dw, self.g_conv_dx = [None], [None]
            for i in range(1, len(C)):
                k, sd, ci, co = cfg.conv_kernel[i], cfg.conv_stride[i], cins[i], C[i]
                Mi = self.Bc * self.lens[i]
                gout = self.dn if i == len(C) - 1 else self.dconv[i]          # d(conv[i] output) -> dpre in place
                self.g_conv_dw.append(Gemm(co, k * ci, Mi, gout, self.conv[i - 1], self.dwp, lda=co, ldb=sd * ci,
                                           ldc=k * ci, transA=True, transB=True,
                                           b_seg=(self.lens[i], self.lens[i - 1] * ci),
                                           split_k=_splitk(_tiles(co), _tiles(k * ci), Mi), accumulate=True))
                self.g_conv_dx.append(Gemm(Mi, k * ci, co, gout, self.convw[i], self.col, lda=co, ldb=k * ci,
                                           ldc=k * ci, transB=True))
        mw, mp = st.mw, st.mp
        self.g_proj = None if self.enc_only else Gemm(
            self.M0, H, C[-1], self.ln_feat, mw("feature_projection.projection.weight"), self.h0,
            lda=C[-1], ldb=C[-1], ldc=H, epilogue=EPI_BIAS, bias=mp("feature_projection.projection.bias"))
        G, K, Cg, Tp = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings, self.Cg, self.Tp
        self.g_pos = Gemm(M, Cg, K * Cg, self.xg, self.posw_f, self.pos, lda=Cg, ldb=K * Cg, ldc=H,
                          a_seg=(T, G * Tp * Cg), batch=G, batch_inner=G, a_strides=(0, Tp * Cg),
                          b_strides=(0, Cg * K * Cg), c_strides=(0, Cg), epilogue=EPI_BIAS_GELU,
                          bias=mp("encoder.pos_conv_embed.conv.bias"), bias_stride1=Cg,
                          aux=self.pos_pre, ldaux=H, aux_strides=(0, Cg))
        heads, d = cfg.num_attention_heads, cfg.head_dim
        L = cfg.num_hidden_layers
        self.g_layer: List[Dict[str, Gemm]] = []
        for l in range(L):
            lb = self.lb[l if self.train else 0]
            xin = self._x(l)
            pre = f"encoder.layers.{l}."
            gl: Dict[str, Gemm] = {}
            # fp16: the value and output projections run with two-term weights (W = hi + lo planes, 2 x K steps on
            # those columns): their rounding is the largest single term of the embedding error (DESIGN "precision")
            two = st.two_term and H % 64 == 0
            gl["qkv"] = Gemm(M, 3 * H, H, xin, st.qkv(l, "w"), lb.qkv, lda=H, ldb=H, ldc=3 * H, epilogue=EPI_BIAS,
                             bias=st.qkv(l, "p", "bias"), b_lo=st.qkv_lo(l) if two else None, n_ext_from=2 * H)
            if not self.fused:
                qkv = lb.qkv.view(-1)
                sc = (heads * T * self.Tl, T * self.Tl)
                gl["scores"] = Gemm(T, T, d, qkv, qkv[H:], self.S, lda=3 * H, ldb=3 * H, ldc=self.Tl,
                                    batch=B * heads, batch_inner=heads, a_strides=(T * 3 * H, d),
                                    b_strides=(T * 3 * H, d), c_strides=sc, alpha=d ** -0.5)
                gl["ctx"] = Gemm(T, d, T, lb.pd, qkv[2 * H:], lb.ctx, lda=self.Tl, ldb=3 * H, ldc=H, transB=True,
                                 batch=B * heads, batch_inner=heads, a_strides=sc, b_strides=(T * 3 * H, d),
                                 c_strides=(T * H, d))
            gl["out"] = Gemm(M, H, H, lb.ctx, mw(pre + "attention.out_proj.weight"), lb.a, lda=H, ldb=H, ldc=H,
                             epilogue=EPI_BIAS, bias=mp(pre + "attention.out_proj.bias"),
                             b_lo=st.w_lo(W2V_PREFIX + pre + "attention.out_proj.weight") if two else None)
            # training: the epilogue leaves gelu'(pre) in lb.hpre (the f32 pre-activation is in registers there), the
            # backward product "dh" just multiplies by it (w2v2_hip.h, W2V2_EPI_BIAS_GELU_GRAD / W2V2_EPI_MUL)
            gl["ffn1"] = Gemm(M, I, H, lb.x1, mw(pre + "feed_forward.intermediate_dense.weight"), lb.h, lda=H, ldb=H,
                              ldc=I, epilogue=EPI_BIAS_GELU_GRAD if lb.hpre is not None else EPI_BIAS_GELU,
                              bias=mp(pre + "feed_forward.intermediate_dense.bias"), aux=lb.hpre, ldaux=I)
            gl["ffn2"] = Gemm(M, H, I, lb.h, mw(pre + "feed_forward.output_dense.weight"), lb.f, lda=I, ldb=I, ldc=H,
                              epilogue=EPI_BIAS, bias=mp(pre + "feed_forward.output_dense.bias"))
            if self.train:
                mg = st.mg
                sk = lambda m, n: _splitk(_tiles(m), _tiles(n), M)
                W2, W1, Wo = (mw(pre + "feed_forward.output_dense.weight"), mw(pre + "feed_forward.intermediate_dense.weight"),
                              mw(pre + "attention.out_proj.weight"))
                Wqkv = st.qkv(l, "w")
                # data-gradient products: with the pre-transposed bf16 weight copies they are plain
                # K-contiguous GEMMs (LDS-DMA kernel); the f32 parity mode reads W as a K-major operand
                gs = self._gsets[l % len(self._gsets)]
                tb = st.flat_lp_t is None
                if not tb:
                    W2, W1, Wo = (st.wt("wav2vec.model." + pre + "feed_forward.output_dense.weight"),
                                  st.wt("wav2vec.model." + pre + "feed_forward.intermediate_dense.weight"),
                                  st.wt("wav2vec.model." + pre + "attention.out_proj.weight"))
                    Wqkv = st.qkv_t(l)
                if self.grouped:
                    pad = lambda t: t._w2v2_padded
                    gl["wgrad_problems"] = [
                        (pad(gs["Gd"]), pad(lb.h), mg(pre + "feed_forward.output_dense.weight"),
                         mg(pre + "feed_forward.output_dense.bias")),
                        (pad(gs["DH"]), pad(lb.x1), mg(pre + "feed_forward.intermediate_dense.weight"),
                         mg(pre + "feed_forward.intermediate_dense.bias")),
                        (pad(gs["Gd1"]), pad(lb.ctx), mg(pre + "attention.out_proj.weight"),
                         mg(pre + "attention.out_proj.bias")),
                        (pad(gs["DQKV"]), pad(xin), st.qkv(l, "g"), st.qkv(l, "g", "bias"))]
                    gl["wgrad"] = WgradGroup(gl["wgrad_problems"], M, _pad64(M))
                gl["dW2"] = Gemm(H, I, M, gs["Gd"], lb.h, mg(pre + "feed_forward.output_dense.weight"), lda=H, ldb=I,
                                 ldc=I, transA=True, transB=True, split_k=sk(H, I), accumulate=True)
                gl["dh"] = Gemm(M, I, H, gs["Gd"], W2, gs["DH"], lda=H, ldb=I if tb else H, ldc=I, transB=tb,
                                epilogue=EPI_MUL, aux=lb.hpre, ldaux=I)
                gl["dW1"] = Gemm(I, H, M, gs["DH"], lb.x1, mg(pre + "feed_forward.intermediate_dense.weight"), lda=I,
                                 ldb=H, ldc=H, transA=True, transB=True, split_k=sk(I, H), accumulate=True)
                # post-LN: G = DH @ W1 + G (the residual path rides in G); pre-LN: G = DH @ W1 alone (the residual
                # gradient lives in self.GR, _backward_encoder_stable); likewise "dx" below
                into_g = {} if self.stable else dict(epilogue=EPI_ADD, aux=self.G, ldaux=H)
                gl["dx1"] = Gemm(M, H, I, gs["DH"], W1, self.G, lda=I, ldb=H if tb else I, ldc=H, transB=tb, **into_g)
                gl["dWo"] = Gemm(H, H, M, gs["Gd1"], lb.ctx, mg(pre + "attention.out_proj.weight"), lda=H, ldb=H, ldc=H,
                                 transA=True, transB=True, split_k=sk(H, H), accumulate=True)
                gl["dctx"] = Gemm(M, H, H, gs["Gd1"], Wo, self.DC, lda=H, ldb=H, ldc=H, transB=tb)
                if not self.fused:
                    qkv = lb.qkv.view(-1)
                    dq = gs["DQKV"].view(-1)
                    sc = (heads * T * self.Tl, T * self.Tl)
                    hs = (T * 3 * H, d)
                    gl["dP"] = Gemm(T, T, d, self.DC, qkv[2 * H:], self.S, lda=H, ldb=3 * H, ldc=self.Tl,
                                    batch=B * heads, batch_inner=heads, a_strides=(T * H, d), b_strides=hs, c_strides=sc)
                    gl["dq"] = Gemm(T, d, T, self.dS, qkv[H:], dq, lda=self.Tl, ldb=3 * H, ldc=3 * H, transB=True,
                                    batch=B * heads, batch_inner=heads, a_strides=sc, b_strides=hs, c_strides=hs,
                                    alpha=d ** -0.5)
                    gl["dk"] = Gemm(T, d, T, self.dS, qkv, dq[H:], lda=self.Tl, ldb=3 * H, ldc=3 * H, transA=True,
                                    transB=True, batch=B * heads, batch_inner=heads, a_strides=sc, b_strides=hs,
                                    c_strides=hs, alpha=d ** -0.5)
                    gl["dv"] = Gemm(T, d, T, lb.pd, self.DC, dq[2 * H:], lda=self.Tl, ldb=H, ldc=3 * H, transA=True,
                                    transB=True, batch=B * heads, batch_inner=heads, a_strides=sc,
                                    b_strides=(T * H, d), c_strides=hs)
                gl["dWqkv"] = Gemm(3 * H, H, M, gs["DQKV"], xin, st.qkv(l, "g"), lda=3 * H, ldb=H, ldc=H, transA=True,
                                   transB=True, split_k=sk(3 * H, H), accumulate=True)
                gl["dx"] = Gemm(M, H, 3 * H, gs["DQKV"], Wqkv, self.G, lda=3 * H, ldb=H if tb else 3 * H, ldc=H,
                                transB=tb, **into_g)
            self.g_layer.append(gl)
        # weight gradients of two consecutive layers (l, l-1; l counted down from the top) in one launch
        if self.grouped and not self.sw.no_wgrad_pairs:
            for l in range(L - 1, 0, -2):
                self.g_wgrad_pair[l] = WgradGroup(self.g_layer[l]["wgrad_problems"] +
                                                  self.g_layer[l - 1]["wgrad_problems"], M, _pad64(M))
        if self.train:
            mg = st.mg
            # pos-conv backward: weight gradient (packed layout) and data gradient (flipped weights)
            # weight gradient with the LARGE dimension (tap, ci) = 6144 as M and the 48 output channels of the
            # group as N (narrow 128x64 tiles, 75 % full) instead of M = 48 on 128-row tiles (37 % full)
            self.g_pos_dw = Gemm(K * Cg, Cg, M, self.xg, self.P1, self.dwf, lda=Cg, ldb=H, ldc=Cg, transA=True,
                                 transB=True, a_seg=(T, G * Tp * Cg), batch=G, batch_inner=G, a_strides=(0, Tp * Cg),
                                 b_strides=(0, Cg), c_strides=(0, K * Cg * Cg))
            self.g_pos_dx = Gemm(M, Cg, K * Cg, self.dyg, self.posw_b, self.G, lda=Cg, ldb=K * Cg, ldc=H,
                                 a_seg=(T, G * Tp * Cg), batch=G, batch_inner=G, a_strides=(0, Tp * Cg),
                                 b_strides=(0, Cg * K * Cg), c_strides=(0, Cg), epilogue=EPI_ADD, aux=self.G, ldaux=H,
                                 aux_strides=(0, Cg))
            g0 = self.G0 if (self.cls or self.paired) else self.G
            if st.flat_lp_t is not None:
                S, Ls, Cf = self.proj_slices, self.proj_slice_len, C[-1]
                self.proj_parts = torch.zeros(S, H * Cf + H, dtype=torch.float32, device=self.dev)   # [slice][dW | db]
                g0p, lnp = g0._w2v2_padded, self.ln_feat._w2v2_padded
                assert g0p.shape[0] >= S * Ls and lnp.shape[0] >= S * Ls
                self.g_proj_dw = WgradGroup([(g0p[i * Ls:], lnp[i * Ls:], self.proj_parts[i, :H * Cf].view(H, Cf),
                                              self.proj_parts[i, H * Cf:]) for i in range(S)], Ls, Ls)
            else:
                self.g_proj_dw = Gemm(H, C[-1], self.M0, g0, self.ln_feat, mg("feature_projection.projection.weight"),
                                      lda=H, ldb=C[-1], ldc=C[-1], transA=True, transB=True,
                                      split_k=_splitk(_tiles(H), _tiles(C[-1]), self.M0), accumulate=True)
            tbp = st.flat_lp_t is None
            Wp = (mw("feature_projection.projection.weight") if tbp
                  else st.wt("wav2vec.model.feature_projection.projection.weight"))
            self.g_proj_dn = Gemm(self.M0, C[-1], H, g0, Wp, self.dn, lda=H, ldb=C[-1] if tbp else H, ldc=C[-1],
                                  transB=tbp)

    # ------------------------------------------------------------------------------------------ derived weights
    def _refresh_packs(self) -> None:
        st, cfg = self.store, self.cfg
        if self._cnn_version != st.cnn_version and not self.enc_only:
            for i in range(1, len(cfg.conv_dim)):
                ops.pack_conv_weight(st.mp(f"feature_extractor.conv_layers.{i}.conv.weight"), self.convw[i])
            self._cnn_version = st.cnn_version
        if self._pack_version != st.version:
            ops.weightnorm_pack(st.mp("encoder.pos_conv_embed.conv.parametrizations.weight.original0"),
                                st.mp("encoder.pos_conv_embed.conv.parametrizations.weight.original1"),
                                self.pos_sumsq, self.posw_f, self.posw_b, cfg.hidden_size,
                                cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings)
            self._pack_version = st.version

    def _sd(self, site: str, layer: int, step: int) -> int:
        """Dropout stream key for (site, layer, step)."""
        return (self.seed * 1000003 + step) * 4096 + layer * 8 + _SITE[site]

    # ------------------------------------------------------------------------------------------ forward
    def _set_lengths(self, lengths) -> None:
        """Validate per-utterance sample counts and upload the frame counts of every length-aware stage (conv-0 frames,
        encoder frames incl. the CLS token) in one host-to-device copy."""
        if self.train:
            raise NotImplementedError("lengths: evaluation plans only (there is no backward for variable lengths)")
        if self.paired:
            raise NotImplementedError("lengths: a paired plan takes the two sides' sample counts as pair_lengths=(left, right)")
        if self.pooling in ("random", "none"):
            raise NotImplementedError(f"lengths: pooling {self.pooling!r} has no variable-length form "
                                      "(supported: mean+std, mean, max, first, first+cls, last, middle, quantile, attentive)")
        lens = valid_lengths(self.cfg, lengths, self.B, self.N)
        f0 = [self.cfg.conv_lengths(n)[0] for n in lens]
        te = [self.cfg.num_frames(n) + (1 if self.cls else 0) for n in lens]
        if self._len_dev is None:
            self._len_dev = torch.empty(2, self.B, dtype=torch.int32, device=self.dev)
        self._len_dev.copy_(torch.tensor([f0, te], dtype=torch.int32))
        self._len = self._len_dev
        self.frame_lengths = te

    def _set_pair_lengths(self, pair_lengths) -> None:
        """Validate the two sides' per-pair sample counts; upload the conv-0 frame counts of the 2B conv rows (left
        utterances, then right) and keep the rows of self.h0 each pair is assembled from (the pair's encoder frames are
        uploaded by _assemble_pairs)."""
        if not self.paired or self.enc_only:
            raise ValueError("pair_lengths: a plan built with paired=True over waveforms (an encoder-only plan takes "
                             "embed_pairs; other plans take lengths=)")
        if self.train:
            raise NotImplementedError("pair_lengths: evaluation plans only (there is no backward for variable lengths)")
        if self.pooling != "first":
            raise NotImplementedError("pair_lengths: the paired model reads token 0 (pooling='first')")
        try:
            left, right = pair_lengths
        except (TypeError, ValueError):
            raise ValueError("pair_lengths: a pair (left, right) of per-pair sample counts") from None
        B, T0 = self.B, self.T0
        lens = valid_lengths(self.cfg, left, B, self.N) + valid_lengths(self.cfg, right, B, self.N)
        if self._len_dev is None:
            self._len_dev = torch.empty(3 * B, dtype=torch.int32, device=self.dev)   # conv-0 frames [2B] | encoder frames [B]
        self._len_dev[:2 * B].copy_(torch.tensor([self.cfg.conv_lengths(n)[0] for n in lens], dtype=torch.int32))
        self._len = (self._len_dev[:2 * B], self._len_dev[2 * B:])
        fr = [self.cfg.num_frames(n) for n in lens]
        self._pair_rows = ([b * T0 for b in range(B)], fr[:B], [(B + b) * T0 for b in range(B)], fr[B:])

    def _assemble_pairs(self, feat: torch.Tensor, left_row, left_frames, right_row, right_frames) -> None:
        """self.hx = [CLS] left [SEP] right [SEP] 0... of each pair from rows of feat [R, H] (tables: host values, checked
        in ops.pair_assemble); the encoder frames te = ta + tb + 3 become the length table of every stage after it."""
        B, T, H = self.B, self.T, self.cfg.hidden_size
        if self._pair_dev is None:
            self._pair_dev = torch.empty(4, B, dtype=torch.int32, device=self.dev)
        if self.enc_only:                              # no conv rows: the table holds the encoder frames alone
            if self._len_dev is None:
                self._len_dev = torch.empty(B, dtype=torch.int32, device=self.dev)
            self._len = (None, self._len_dev)
        host = ops.pair_assemble(feat, self.hx.view(B, T, H), left_row, left_frames, right_row, right_frames, self.cls_c,
                                 self.sep_c, table=self._pair_dev)
        te = host[1] + host[3] + 3
        self._len[1].copy_(te)
        self.frame_lengths = te.tolist()

    def embed_pairs(self, feat: torch.Tensor, left_row, left_frames, right_row, right_frames) -> torch.Tensor:
        """Encoder-only paired plan (Plan.pair_encoder): pair b = rows [left_row[b], + left_frames[b]) and [right_row[b],
        + right_frames[b]) of feat [R, H] (projected features in the activation dtype, e.g. Plan.features of each
        utterance; rows may be shared between pairs) -> token 0 of each pair's encoder output [B, H] f32.  The tables are
        host values; ta + tb + 3 <= the plan's frames.  Same code as forward(pair_lengths=) from the assembly on."""
        if not self.enc_only:
            raise ValueError("embed_pairs: an encoder-only paired plan (Plan.pair_encoder)")
        assert feat.is_cuda and feat.dtype == self.adt and feat.dim() == 2 and feat.is_contiguous()
        self._refresh_packs()
        self._step, self._skip, self._mask, self._fmask = 0, (), None, None
        self._assemble_pairs(feat, left_row, left_frames, right_row, right_frames)
        self._pool_fwd(self._encode(0))
        return self.emb

    def features(self, wav: torch.Tensor, lengths=None):
        """Conv stack + LayerNorm + projection alone (evaluation, non-paired plans; HF:382-419,1287 without dropout) ->
        (projected frames [B, T0, H] in the activation dtype -- the plan's own buffer, valid until its next call --,
        frames per row).  With lengths, row b's first frames[b] frames equal the utterance alone at its own length."""
        if self.train or self.paired or self.cls:
            raise NotImplementedError("features: non-paired evaluation plans without a CLS token")
        cfg = self.cfg
        if wav.dim() == 3:
            wav = wav[:, 0, :]
        wav = wav.contiguous()
        assert wav.shape == (self.Bc, self.N) and wav.dtype == torch.float32 and wav.is_cuda
        self._len, self.frame_lengths = None, None
        frames = [self.T0] * self.B
        if lengths is not None:
            lens = valid_lengths(cfg, lengths, self.B, self.N)
            if self._len_dev is None:
                self._len_dev = torch.empty(2, self.B, dtype=torch.int32, device=self.dev)
            frames = [cfg.num_frames(n) for n in lens]
            self._len_dev.copy_(torch.tensor([[cfg.conv_lengths(n)[0] for n in lens], frames], dtype=torch.int32))
            self._len = self._len_dev
        self._refresh_packs()
        self._wav = wav
        self._project(wav)
        return self.h0.view(self.B, self.T0, cfg.hidden_size), frames

    def _project(self, wav: torch.Tensor) -> None:
        """wav -> self.h0: conv stack, LayerNorm, projection (before the projection's dropout)."""
        mp = self.store.mp
        self._cnn_forward(wav)
        ops.layernorm_fwd(self.conv[-1].view(self.M0, -1), None, mp("feature_projection.layer_norm.weight"),
                          mp("feature_projection.layer_norm.bias"), self.ln_feat, self.mean_f, self.rstd_f,
                          self.cfg.layer_norm_eps)
        self.g_proj()

    def forward(self, wav: torch.Tensor, mask: Optional[torch.Tensor] = None, skip_layers: Sequence[int] = (),
                step: int = 0, feature_mask: Optional[torch.Tensor] = None, lengths=None,
                pair_lengths=None) -> torch.Tensor:
        """wav [B,N] (or [B,1,N]) f32 on the GPU -> last_hidden_state [B,T,H] (act dtype).
        mask: [B,T0] uint8/bool SpecAugment time mask, feature_mask: [B,H] uint8/bool SpecAugment feature mask
        (HF:1294-1304; training only).  Dropout is active iff the plan was built with train=True and the
        regularisation probabilities are > 0.
        lengths: valid samples per utterance (ints or a CPU integer tensor; evaluation plans).  Every cross-frame
        reduction (conv-0 GroupNorm statistics, positional-conv padding, attention, pooling) then sees each utterance's own
        frames only, so row b equals the utterance alone at its own length; padded samples may hold any finite values.
        ``frame_lengths`` gives the encoder frames of each row; rows of the output past them are unspecified.
        pair_lengths: (left, right) valid samples of each pair's two utterances (paired evaluation plans; wav [2B,N] =
        left utterances, then right).  Pair b is then [CLS] left [SEP] right [SEP] over its own ta + tb + 3 frames
        (``frame_lengths``), equal to the pair alone at its own lengths."""
        cfg, st, reg = self.cfg, self.store, self.reg
        if self.enc_only:
            raise ValueError("forward: an encoder-only plan has no conv stack (embed_pairs)")
        B, T, M, H = self.B, self.T, self.M, cfg.hidden_size
        if wav.dim() == 3:
            wav = wav[:, 0, :]
        wav = wav.contiguous()
        assert wav.shape == (self.Bc, self.N) and wav.dtype == torch.float32 and wav.is_cuda
        self._len, self.frame_lengths = None, None
        if lengths is not None:
            self._set_lengths(lengths)
        if pair_lengths is not None:
            self._set_pair_lengths(pair_lengths)
        self._refresh_packs()
        self._wav = wav
        tr = self.train
        self._step, self._skip, self._mask, self._fmask = step, tuple(skip_layers), None, None
        mp = st.mp
        self._project(wav)
        if tr and reg.feat_proj_dropout > 0:
            ops.dropout_(self.h0, reg.feat_proj_dropout, self._sd("featproj", 0, step))
        if self.cls:
            ops.prepend_token(self.h0.view(B, self.T0, H), self.hx.view(B, T, H), self.cls_c)
        elif pair_lengths is not None:
            assert mask is None and feature_mask is None
            self._assemble_pairs(self.h0, *self._pair_rows)
        elif self.paired:
            # [CLS] left [SEP] right [SEP] (constant tokens; no SpecAugment on this path) -- buffer plumbing only
            assert mask is None
            T0, hx, h0 = self.T0, self.hx.view(B, T, H), self.h0.view(2, B, self.T0, H)
            hx[:, 0].fill_(self.cls_c)
            hx[:, 1:1 + T0].copy_(h0[0])
            hx[:, 1 + T0].fill_(self.sep_c)
            hx[:, 2 + T0:2 + 2 * T0].copy_(h0[1])
            hx[:, 2 + 2 * T0].fill_(self.sep_c)
        elif mask is not None:
            self._mask = mask.to(torch.uint8).contiguous().view(-1)
            ops.mask_fill(self.h0, self._mask, mp("masked_spec_embed"))
        if feature_mask is not None:          # after the time mask, like HF's _mask_hidden_states
            assert not (self.cls or self.paired)
            self._fmask = feature_mask.to(torch.uint8).contiguous().view(-1)
            ops.mask_feature(self.h0, self._fmask, B, self.T0)
        return self._encode(step)

    def _encode(self, step: int) -> torch.Tensor:
        """self.hx (encoder input) -> last_hidden_state: positional convolution and the transformer encoder."""
        cfg, mp = self.cfg, self.store.mp
        B, T, H = self.B, self.T, cfg.hidden_size
        G, K = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings
        if self._len is not None:
            ops.posconv_regroup_len(self.hx, self.xg, self._len[1], B, T, H, G, K, K // 2)
        else:
            ops.posconv_regroup(self.hx, self.xg, B, T, H, G, K, K // 2)
        if self.pos_direct:      # image-resident direct convolution (csrc/posconv_direct.hip), bit-equal to the GEMM
            ops.posconv_direct(self.xg, self.posw_f, self.pos, self.pos_pre, mp("encoder.pos_conv_embed.conv.bias"), B, T, G,
                               self.Cg, K, H, 0)
        else:
            self.g_pos()
        return self._encoder_forward(step)

    def _attention(self, l: int, lb: LayerBufs, gl, pa: float, step: int) -> None:
        """Self-attention of block l from lb.qkv into lb.ctx: fused (16-bit, head dim 64) or scores GEMM + softmax +
        context GEMM; the length-aware kernels when the forward has lengths."""
        B, T, heads, d = self.B, self.T, self.cfg.num_attention_heads, self.cfg.head_dim
        lens = None if self._len is None else self._len[1]
        if self.fused:
            if lens is not None:
                ops.attention_fwd_len(lb.qkv, lb.ctx, lb.lse, lens, B, T, heads, d, d ** -0.5)
            else:
                ops.attention_fwd(lb.qkv, lb.ctx, lb.lse, B, T, heads, d, d ** -0.5, pa, self._sd("attn", l, step))
            return
        gl["scores"]()
        if lens is not None:
            ops.softmax_fwd_len(self.S, lb.p, lens, B, heads, T, self.Tl)
        else:
            ops.softmax_fwd(self.S, lb.p, lb.pd if pa > 0 else None, B * heads * T, T, self.Tl, pa,
                            self._sd("attn", l, step))
        gl["ctx"]()

    def _ln_params_for_input_of(self, l: int):
        """Pre-LN encoder: the LayerNorm that produces X[l], the normalised input of block l (its ``layer_norm``), or -- for
        l = number of blocks -- the encoder's final ``layer_norm`` (HF:791)."""
        n = f"encoder.layers.{l}.layer_norm" if l < self.cfg.num_hidden_layers else "encoder.layer_norm"
        return _wb(n)

    def _encoder_forward(self, step: int) -> torch.Tensor:
        """The transformer encoder, hx (projection output) and pos (positional embedding) -> self.out.  Both checkpoint families
        run ONE block (_block_forward: same buffers, GEMM descriptors and fused residual + dropout + LayerNorm kernel), re-wired:
        Post-LN (HF:382-726):
            X[0] = drop(LN(hx + pos))
            block l:  a = out_proj(attn(qkv(X[l])))                lb.x1 = LN1_l(X[l] + drop(a))        [s1 -> lb.a]
                      f = ffn2(gelu(ffn1(lb.x1)))                  X[l+1] = LN2_l(lb.x1 + drop(f))      [s2 -> lb.f]
            a LayerDrop-skipped block is the identity: X[l+1] = X[l].
        Pre-LN (do_stable_layer_norm, HF:611-654,729-802):
            x_0 = drop(hx + pos)                                   X[0] = LN1_0(x_0)
            block l:  a = out_proj(attn(qkv(X[l])))                s1 = x_l + drop(a)     -> lb.a,   lb.x1 = LN2_l(s1)
                      f = ffn2(gelu(ffn1(lb.x1)))                  x_{l+1} = s1 + drop(f) -> lb.f,   X[l+1] = LN1_{l+1}(x_{l+1})
            (the last X is the encoder's final LayerNorm).  The un-normalised residual stream x_l lives in the tensor the
            fused kernel writes its pre-norm sum into (`res` below); a LayerDrop-skipped block passes it on and only
            re-normalises it for the next block (self._res_src[l] remembers which tensor that was, for the backward)."""
        cfg, mp, eps = self.cfg, self.store.mp, self.cfg.layer_norm_eps
        H, L = cfg.hidden_size, cfg.num_hidden_layers
        ph = self.reg.hidden_dropout if self.train else 0.0
        if self.stable:
            ops.add(self.hx, self.pos, self.pos)                  # x_0 (before dropout) replaces the positional embedding
            if ph > 0:
                ops.dropout_(self.pos, ph, self._sd("prologue", 0, step))
            res = self.pos
            w0, b0 = self._ln_params_for_input_of(0)
            ops.layernorm_fwd(res, None, mp(w0), mp(b0), self._x(0), self.mean0, self.rstd0, eps)
            self._res_src = {}
        else:
            ops.layernorm_fwd(self.hx, self.pos, mp("encoder.layer_norm.weight"), mp("encoder.layer_norm.bias"), self._x(0),
                              self.mean0, self.rstd0, eps)
            if ph > 0:
                ops.dropout_(self._x(0), ph, self._sd("prologue", 0, step))
        for l in range(L):
            xin, xout, lb = self._x(l), self._x(l + 1), self.lb[l if self.train else 0]
            pre = f"encoder.layers.{l}."
            if self.stable:
                ln_next = self._ln_params_for_input_of(l + 1)
                if l in self._skip:                 # LayerDrop: x_{l+1} = x_l, re-normalised for the next block
                    ops.layernorm_fwd(res, None, mp(ln_next[0]), mp(ln_next[1]), xout, lb.mean2, lb.rstd2, eps)
                    self._res_src[l] = res
                    continue
                self._block_forward(l, step, res, _wb(pre + "final_layer_norm"), lb.a, ln_next, xout)
                res = lb.f                          # lb.a <- s1, lb.f <- x_{l+1}
            elif l in self._skip:                   # LayerDrop (HF:698-709): the layer is the identity
                ops.copy_strided(xin, H, xout, H, xin.shape[0], H)
            else:
                self._block_forward(l, step, xin, _wb(pre + "layer_norm"), lb.x1, _wb(pre + "final_layer_norm"), xout)
        self.out = self._x(L).view(self.B, self.T, H)
        return self.out

    def _block_forward(self, l: int, step: int, res1: torch.Tensor, ln1, res2: torch.Tensor, ln2, xout: torch.Tensor) -> None:
        """Transformer block l of either family (wiring: _encoder_forward): attention of X[l], lb.x1 = LN(res1 + drop(a))
        with the parameters named ln1, FFN of lb.x1, xout = LN(res2 + drop(f)) with the parameters named ln2.  The fused
        kernel leaves the two pre-norm sums in lb.a and lb.f."""
        reg, tr, mp, eps = self.reg, self.train, self.store.mp, self.cfg.layer_norm_eps
        lb, gl = self.lb[l if tr else 0], self.g_layer[l]
        ph = reg.hidden_dropout if tr else 0.0
        gl["qkv"]()
        self._attention(l, lb, gl, reg.attention_dropout if tr else 0.0, step)
        gl["out"]()
        ops.layernorm_fwd(res1, lb.a, mp(ln1[0]), mp(ln1[1]), lb.x1, lb.mean1, lb.rstd1, eps, ph,
                          self._sd("post_attn", l, step))
        gl["ffn1"]()
        if tr and reg.activation_dropout > 0:
            # HF:566-569 intermediate_dropout.  The SAME keep decisions (same stream key, same element index) are
            # applied to the saved gelu'(pre): the backward product "dh" multiplies by it, which is then exactly
            # d(dropout(gelu(pre))) / d(pre) -- no separate dropout backward, no mask tensor
            ops.dropout_(lb.h, reg.activation_dropout, self._sd("act", l, step))
            ops.dropout_(lb.hpre, reg.activation_dropout, self._sd("act", l, step))
        gl["ffn2"]()
        ops.layernorm_fwd(res2, lb.f, mp(ln2[0]), mp(ln2[1]), xout, lb.mean2, lb.rstd2, eps, ph, self._sd("ffn", l, step))

    def conv_features(self, wav: torch.Tensor) -> torch.Tensor:
        """The conv feature extractor alone (HF:382-419; ref: src/models/wav2vec2.py:163-169,
        ``Wav2vecLiteWrapperModule.forward``): wav [B,N] f32 -> [B, L, 512] (act dtype, channels-last; the reference
        returns the transpose).  Same kernels as the first stage of forward()."""
        cfg, st = self.cfg, self.store
        if wav.dim() == 3:
            wav = wav[:, 0, :]
        wav = wav.contiguous()
        assert wav.shape == (self.Bc, self.N) and wav.dtype == torch.float32 and wav.is_cuda
        self._refresh_packs()
        self._wav = wav
        self._len = None
        self._cnn_forward(wav)
        return self.conv[-1]

    def _cnn_forward(self, wav: torch.Tensor) -> None:
        """The seven convolution layers (HF:382-419) into self.conv[i] ([Bc, L_i, C_i], channels-last).  Group-norm family
        (wav2vec2-base / -large): layer 0 = conv + GroupNorm + GELU in one kernel pair, layers 1-6 = implicit GEMM with
        a bias + GELU epilogue (HF:254-272,302-323; a layer-0 conv bias would be cancelled by the GroupNorm's mean over time
        and is not read).  Layer-norm family ("-lv60" / xlsr, HF:275-299): every layer is conv (+ bias) -> LayerNorm over
        the channels -> GELU; layer 0 in one kernel, layers 1-6 as GEMM (bias epilogue) + an in-place LayerNorm-GELU pass."""
        cfg, mp = self.cfg, self.store.mp
        fe = "feature_extractor.conv_layers."
        if not self.ln_conv and self._len is not None:     # GroupNorm statistics over each utterance's own frames
            ops.conv0_groupnorm_gelu_len(wav, mp(fe + "0.conv.weight"), mp(fe + "0.layer_norm.weight"),
                                         mp(fe + "0.layer_norm.bias"), self.conv[0], self.stats0, self._len[0],
                                         cfg.conv_kernel[0], cfg.conv_stride[0])
            for g in self.g_conv:
                g()
            return
        if not self.ln_conv:
            ops.conv0_groupnorm_gelu(wav, mp(fe + "0.conv.weight"), mp(fe + "0.layer_norm.weight"), mp(fe + "0.layer_norm.bias"),
                                     self.conv[0], self.stats0, cfg.conv_kernel[0], cfg.conv_stride[0])
            for g in self.g_conv:
                g()
            return
        ops.conv0_layernorm_gelu(wav, mp(fe + "0.conv.weight"), mp(fe + "0.conv.bias") if cfg.conv_bias else None,
                                 mp(fe + "0.layer_norm.weight"), mp(fe + "0.layer_norm.bias"), self.conv[0],
                                 cfg.conv_kernel[0], cfg.conv_stride[0])
        for i, g in enumerate(self.g_conv, start=1):
            g()
            y = self.conv[i].view(-1, cfg.conv_dim[i])
            z = self.conv_pre[i].view(-1, cfg.conv_dim[i]) if self.cnn_train else y      # (kept for _backward_cnn)
            ops.layernorm_gelu_fwd(z, mp(fe + f"{i}.layer_norm.weight"), mp(fe + f"{i}.layer_norm.bias"), y, 1e-5)

    def conv_backward(self, dfeat: torch.Tensor) -> None:
        """Backward of conv_features(): dfeat [B, L, 512] = d(loss)/d(features); the gradients of the seven conv layers
        and their normalisations are ACCUMULATED in the arena.  Needs a plan built with train=True over a store with
        ``freeze_cnn=False``."""
        if not self.train or self.store.freeze_cnn:
            raise RuntimeError("conv_backward needs Plan(train=True) over ParamStore(freeze_cnn=False)")
        self.dn.view(-1).copy_(dfeat.to(self.adt).contiguous().view(-1))
        self._backward_cnn()

    def embed(self, wav, mask=None, skip_layers=(), step: int = 0, feature_mask=None, lengths=None,
              pair_lengths=None) -> torch.Tensor:
        """ref: src/lightning_modules/speaker/wav2vec2_fc.py:414-431 -> pooled embedding [B,E] f32.  lengths: see
        forward(); each row is then pooled over its own frames."""
        out = self.forward(wav, mask, skip_layers, step, feature_mask, lengths=lengths, pair_lengths=pair_lengths)
        if self.pooling == "attentive":       # (the encoder frame counts are the table the pooling needs)
            return self._asp_for(out).forward(None if self._len is None else self._len[1])
        self._pool_fwd(out)
        return self.emb

    def _pool_fwd(self, out: torch.Tensor) -> None:
        B, T, H = out.shape
        if self._len is not None:
            ops.pool_fwd_len(out, self.emb, self._len[1], self.pool_mode)
        elif self.no_pool:
            ops.pool_fwd(out.view(B * T, 1, H), self.emb, POOL_MODES["first"])      # f32 copy of every frame
        elif self.pooling == "random":
            import random
            self._rand_idx = random.randint(0, T - 1)                             # ref: pooling.py:150-154
            ops.pool_fwd(out, self.emb, ops.POOL_INDEX_BASE + self._rand_idx)
        else:
            ops.pool_fwd(out, self.emb, self.pool_mode)

    def hidden_states(self) -> List[torch.Tensor]:
        """HF ``output_hidden_states`` of the last forward: [prologue output, layer 1, ..., layer L], each [B,T,H]."""
        assert self.all_x, "build the plan with keep_hidden_states=True"
        return [x.view(self.B, self.T, self.cfg.hidden_size) for x in self.X]

    def ensemble_embeddings(self, wav, num_ensembles: int) -> List[torch.Tensor]:
        """ref: src/lightning_modules/speaker/wav2vec2_fc.py:440-463 (compute_ensemble_embedding): the pooled
        embedding of each of the last ``num_ensembles`` hidden states (hidden_states[L+1-n : L+1])."""
        assert self.pooling != "attentive", "ensemble pooling shares one stat-pooling layer: use a stateless pool"
        self.forward(wav, None, (), 0)          # (fixed length: the hidden-state ensemble has no variable-length form)
        hs = self.hidden_states()
        out = []
        for h in hs[len(hs) - num_ensembles:]:
            e = torch.empty_like(self.emb)
            ops.pool_fwd(h, e, self.pool_mode)
            out.append(e)
        return out

    def _asp_for(self, out: torch.Tensor):
        """Attentive statistics pooling over the buffer the encoder just wrote (built once per buffer)."""
        from .asp import AttentivePool
        key = out.data_ptr()
        if key not in self._asp:
            B, T, H = out.shape
            x2 = out.view(B * T, H)
            src = next((x for x in self.X if x.data_ptr() == key), None)
            if src is not None and hasattr(src, "_w2v2_padded"):
                x2._w2v2_padded = src._w2v2_padded
            self._asp[key] = AttentivePool(self.store, x2, self.emb, self.G if self.train else None, B, T, self.train)
        self._asp_cur = self._asp[key]
        return self._asp_cur

    # ------------------------------------------------------------------------------------------ head
    def frames_of(self, sample_counts) -> List[int]:
        """Encoder frames of utterances of the given sample counts (ref: wav2vec2_fc_letter.py:146
        ``floor((n - 80) / 320)``, which is the conv stack's output length), on the host."""
        return [int(math.floor((int(n) - 80) / 320)) for n in sample_counts]

    def head_forward_backward(self, label: torch.Tensor, triplets=None, transcript=None):
        """Loss head on self.emb (hidden FC layers, then heads.ClassifierHead): returns (loss scalar tensor,
        softmax [B,C]); a training plan also leaves d(loss)/d(pooled embedding) in self.demb and the head gradients
        in the flat buffer.  Triplet heads: ``triplets`` = (pos, neg) row indices of every anchor row (None: heads.TripletHead
        draws them from ``label.tolist()``, a host synchronisation); "triplet" returns (loss, None), "triplet_ce" returns
        (CE + triplet_coef * triplet, softmax) with the sum taken on the device.  The "letter" head: ``transcript`` =
        (targets [B, width], target lengths [B], sample counts [B]) still on the host (heads.LetterHead uploads them without
        waiting; ``label`` is not used) -> (loss, None)."""
        if triplets is not None and self.triplet is None:
            raise ValueError(f"triplets were given, but the head is {self.store.head!r}")
        if (transcript is not None) != (self.store.head == "letter"):
            raise ValueError(f"a transcript is what the \"letter\" head takes, and all it takes; the head is "
                             f"{self.store.head!r}")
        if transcript is not None:
            # (targets [B, width], target lengths [B], sample counts [B]) on the host: one upload, no wait
            targets, target_lengths, sample_counts = transcript
            self.head.set_batch(targets, target_lengths, self.frames_of(sample_counts))
            return self.head.forward_backward(seed=self._sd("final", 0, self._step))
        if self.store.head == "triplet":
            return self.triplet.forward_backward(label, triplets)
        if self.no_pool and self.store.head != "ctc":    # one prediction per frame: the utterance label for each of its
            label = torch.repeat_interleave(label, self.T)   # T frames (CTC: one label per utterance, passed through)
        if self.fc is not None:
            self.fc.forward()
        out = self.head.forward_backward(label)
        if self.fc is not None and self.train:
            self.demb.copy_(self.fc.backward(self.head.demb))
        if self.triplet is not None:     # "triplet_ce": the triplet term is added to the gradient the CE path has left
            tl, _ = self.triplet.forward_backward(label, triplets)
            return torch.add(out[0], tl, alpha=self.triplet_coef), out[1]
        return out

    def speaker_embedding(self, embedding_layer_idx: int = -1) -> torch.Tensor:
        """ref: wav2vec2_fc.py:363-398 (_fc_head_ops_pre_spk_embedding) after embed(): the pooled embedding
        (idx < 0), the output of hidden layer idx, or (idx == number of hidden layers, CE head) the logits."""
        if embedding_layer_idx < 0:
            return self.emb
        nh = len(self.store.hidden_fc)
        if embedding_layer_idx < nh:
            return self.fc.forward(upto=embedding_layer_idx)
        if embedding_layer_idx == nh and self.store.head in ("ce", "triplet_ce"):
            if self.fc is not None:
                self.fc.forward()
            h = self.head
            if h.emb_lp is not h.emb:
                ops.cast(h.emb, h.emb_lp)
            h.g_fwd()
            return h.logits[:, :h.C]
        raise ValueError("could not determine the speaker embedding layer")

    # ------------------------------------------------------------------------------------------ backward
    def backward(self, demb: Optional[torch.Tensor] = None,
                 on_bucket_ready: Optional[Callable[[str], None]] = None,
                 dhidden: Optional[torch.Tensor] = None, dmix: Optional[torch.Tensor] = None,
                 mix_weights: Optional[torch.Tensor] = None) -> None:
        """Backward of embed(): demb [B,E] f32 (default self.demb from the head) -> parameter gradients
        accumulated into store.grad.  on_bucket_ready(name) fires as soon as a gradient bucket
        ('head', 'layer11', ..., 'layer0', 'prologue', 'projection') is final, for the overlapped all-reduce.
        dmix [B,T,H] (f32 or bf16) with mix_weights [L + 1] f32 on the device: the gradient of a softmax-weighted sum of
        ALL hidden states (include/w2v2_hip.h, "layer mix") -- d loss / d X[j] receives w_j * dmix in addition to what
        flows down from above, at the points mix_injection_points derives from the event list; the host never reads the
        weights.  Post-LN encoder, no loss scaler; a store with head=None has no head bucket to notify."""
        cfg, st, reg = self.cfg, self.store, self.reg
        B, T, M, H = self.B, self.T, self.M, cfg.hidden_size
        mix_backward_check(train=self.train, stable=self.stable, scaler=st.scaler, B=B, T=T, H=H, L=cfg.num_hidden_layers,
                           dmix=dmix, mix_weights=mix_weights, demb=demb, dhidden=dhidden)
        assert self.train, "backward needs a training plan"
        mp, mg = st.mp, st.mg
        step = self._step
        notify = on_bucket_ready or (lambda name: None)
        events = () if self.stable else encoder_backward_schedule(cfg.num_hidden_layers, self._skip, self.g_wgrad_pair,
                                                                  self.grouped,
                                                                  1 if self.sw.no_wgrad_pairs else self.wg_group)
        inject = {}
        if dmix is not None:
            inject = {i: (lo, hi, ow) for i, lo, hi, ow in mix_injection_points(events, cfg.num_hidden_layers)}
            dmix = dmix.view(-1)
        if dmix is not None:
            pass                          # G starts as w_L * dmix: the first injection overwrites it
        elif dhidden is not None:         # gradient wrt last_hidden_state given directly (module surface)
            self.G.view(B, T, H).copy_(dhidden)
        else:
            if demb is None:
                demb = self.demb
            if self.pooling == "attentive":   # its parameters share the head's gradient bucket
                self._asp_cur.backward(demb)
            elif self.no_pool:
                ops.pool_bwd(self.out.view(B * T, 1, H), self.emb, demb, self.G.view(B * T, 1, H), POOL_MODES["first"])
            elif self.pooling == "random":
                ops.pool_bwd(self.out, self.emb, demb, self.G.view(B, T, H), ops.POOL_INDEX_BASE + self._rand_idx)
            else:
                ops.pool_bwd(self.out, self.emb, demb, self.G.view(B, T, H), self.pool_mode)
        if not (dmix is not None and st.head is None and not st.attentive_pool):
            notify("head")
        lnfold = None if self.sw.no_ln_fold else self._lnfold
        if self.stable:
            self._backward_encoder_stable(notify)               # leaves d(loss)/d(hx + pos) in self.G
        for i, ev in enumerate(events):
            if i in inject:                                     # G holds the full gradient of X[l + 1] before body l
                ops.scale_add(self.G, dmix, mix_weights, *inject[i])
            kind = ev[0]
            if kind == "body":
                self._layer_backward_body(ev[1], lnfold)
            elif kind == "wgrad":
                layers = ev[1]
                self._wgrad_for(tuple(layers))()
            elif kind == "dx":
                self.g_layer[ev[1]]["dx"]()                     # G = DQKV @ Wqkv + G
            elif kind == "fold":
                if lnfold is not None:
                    lnfold.fold()                               # gamma / beta of the bucket's LayerNorms: one launch
            else:
                notify(f"layer{ev[1]}")
        if len(events) in inject:                               # X[0] (and the states of skipped layers right above it)
            ops.scale_add(self.G, dmix, mix_weights, *inject[len(events)])
        # encoder prologue: x0 = drop(LN(hx + pos)), pos = GELU(posconv(hx) + b)
        ph = reg.hidden_dropout
        if not self.stable:
            if ph > 0:
                ops.dropout_(self.G, ph, self._sd("prologue", 0, step))
            ops.layernorm_bwd(self.G, self.pos, self.mean0, self.rstd0, mp("encoder.layer_norm.weight"), self.G, None,
                              mg("encoder.layer_norm.weight"), mg("encoder.layer_norm.bias"))
        if H % 8 == 0:
            ops.gelu_bwd_colsum(self.G, self.pos_pre, self.P1, mg("encoder.pos_conv_embed.conv.bias"), M, H)
        else:
            ops.gelu_bwd(self.G, self.pos_pre, self.P1)
            ops.colsum(self.P1, mg("encoder.pos_conv_embed.conv.bias"), M, H)
        G_, K = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings
        if ops.is16(self.P1.dtype) and not self.sw.pos_dw_gemm:
            ops.posconv_wgrad(self.P1, self.xg, self.dwf, B, T, H, G_, K)      # correlation kernel (posconv_wgrad.hip)
        else:
            self.g_pos_dw()                                                    # exact-f32 mode: implicit GEMM
        ops.weightnorm_bwd(mp("encoder.pos_conv_embed.conv.parametrizations.weight.original0"),
                           mp("encoder.pos_conv_embed.conv.parametrizations.weight.original1"), self.pos_sumsq,
                           self.dwf, self.pos_dot, mg("encoder.pos_conv_embed.conv.parametrizations.weight.original0"),
                           mg("encoder.pos_conv_embed.conv.parametrizations.weight.original1"), H, G_, K)
        notify("prologue")            # encoder LayerNorm, pos-conv bias and weight-norm pair are final (params.grad_buckets)
        ops.posconv_regroup(self.P1, self.dyg, B, T, H, G_, K, K - 1 - K // 2)
        if self.pos_direct:
            ops.posconv_direct(self.dyg, self.posw_b, self.G, self.G, None, B, T, G_, self.Cg, K, H, 1)
        else:
            self.g_pos_dx()                                     # G = conv^T(P1) + G
        if self.cls:
            self.G0.view(B, self.T0, H).copy_(self.G.view(B, T, H)[:, 1:, :])    # the CLS row has no input
            g0 = self.G0
        elif self.paired:                     # the three constant tokens have no input
            T0, G3, G0 = self.T0, self.G.view(B, T, H), self.G0.view(2, B, self.T0, H)
            G0[0].copy_(G3[:, 1:1 + T0])
            G0[1].copy_(G3[:, 2 + T0:2 + 2 * T0])
            g0 = self.G0
        else:
            g0 = self.G
            if self._fmask is not None:
                ops.mask_feature(g0, self._fmask, B, self.T0)
            if self._mask is not None:
                ops.mask_fill_bwd(g0, self._mask, mg("masked_spec_embed"))
        if reg.feat_proj_dropout > 0:
            ops.dropout_(g0, reg.feat_proj_dropout, self._sd("featproj", 0, step))
        self.g_proj_dw()
        if st.flat_lp_t is None:
            ops.colsum(g0, mg("feature_projection.projection.bias"), self.M0, H)
        else:          # fixed-order sum of the slices' partials (one writer per column: no atomics race, reproducible)
            S, Cf = self.proj_slices, cfg.conv_dim[-1]
            ld = H * Cf + H
            ops.colsum(self.proj_parts, mg("feature_projection.projection.weight").view(-1), S, H * Cf, ld)
            ops.colsum(self.proj_parts[:, H * Cf:], mg("feature_projection.projection.bias"), S, H, ld)
        self.g_proj_dn()
        ops.layernorm_bwd(self.dn, self.conv[-1].view(self.M0, -1), self.mean_f, self.rstd_f,
                          mp("feature_projection.layer_norm.weight"), self.dn, None,
                          mg("feature_projection.layer_norm.weight"), mg("feature_projection.layer_norm.bias"))
        notify("projection")
        if not st.freeze_cnn:
            if not st.cnn_runtime_frozen:         # feature_extractor.requires_grad_(False) at run time: zero gradient
                self._backward_cnn()
            notify("cnn")

    def _backward_encoder_stable(self, notify) -> None:
        """Backward of the pre-LN wiring of _encoder_forward.  Two running gradients: self.G = d(loss)/dX[l+1] (the NORMALISED
        input of the block above: what its QKV data-gradient product wrote) and self.GR = d(loss)/dx_{l+1} (the un-normalised
        residual stream, accumulated over every block above).  Per block, top down:
            GR += LN_bwd(G)  [the LayerNorm that fed X[l+1]]      df = drop(GR)  -> FFN backward -> G = d(LN2_l output)
            GR += LN_bwd(G)  [final_layer_norm of block l]         da = drop(GR)  -> attention backward -> G = dX[l]
        A LayerDrop-skipped block only passes its re-normalisation back.  One weight-gradient launch per block (the
        grouped kernel in the 16-bit modes), LayerNorm gamma / beta folded at once; the gradient of a block's FIRST
        LayerNorm is produced by the block BELOW it (or the prologue), so the layer buckets are notified at the end."""
        # (follow-up, not done here: reuse encoder_backward_schedule and the LayerNorm fold group -- the open finding on this function in ADVICE.md)
        mp, mg = self.store.mp, self.store.mg
        step, ph, L = self._step, self.reg.hidden_dropout, self.cfg.num_hidden_layers
        G, GR = self.G, self.GR
        GR.zero_()
        for l in reversed(range(L)):
            lb, gs = self.lb[l], self._gsets[l % len(self._gsets)]
            wn, bn = self._ln_params_for_input_of(l + 1)
            if l in self._skip:
                ops.layernorm_bwd(G, self._res_src[l], lb.mean2, lb.rstd2, mp(wn), G, None, mg(wn), mg(bn))
                ops.add(GR, G, GR)
                G.zero_()                       # X[l] fed a skipped block: nothing flows into it
                continue
            w2, b2 = _wb(f"encoder.layers.{l}.final_layer_norm")
            ops.layernorm_bwd(G, lb.f, lb.mean2, lb.rstd2, mp(wn), G, None, mg(wn), mg(bn))
            ops.add(GR, G, GR)                                  # GR = d x_{l+1}
            gs["Gd"].copy_(GR)
            if ph > 0:
                ops.dropout_(gs["Gd"], ph, self._sd("ffn", l, step))
            self._ffn_backward(l)                               # G = DH @ W1 = d(LN2_l output)
            ops.layernorm_bwd(G, lb.a, lb.mean1, lb.rstd1, mp(w2), G, None, mg(w2), mg(b2))
            ops.add(GR, G, GR)                                  # GR = d s1 = d x_l (residual part)
            gs["Gd1"].copy_(GR)
            if ph > 0:
                ops.dropout_(gs["Gd1"], ph, self._sd("post_attn", l, step))
            self._attention_backward(l)
            if self.grouped:
                self.g_layer[l]["wgrad"]()
            else:
                self._qkv_wgrad_ungrouped(l)
            self.g_layer[l]["dx"]()                             # G = DQKV @ Wqkv = dX[l]
        w0, b0 = self._ln_params_for_input_of(0)
        ops.layernorm_bwd(G, self.pos, self.mean0, self.rstd0, mp(w0), G, None, mg(w0), mg(b0))
        ops.add(GR, G, GR)                                      # d x_0
        if ph > 0:
            ops.dropout_(GR, ph, self._sd("prologue", 0, step))
        G.copy_(GR)                                             # = d(hx + pos): the shared prologue backward continues
        for l in reversed(range(L)):
            notify(f"layer{l}")

    def _layer_backward_body(self, l: int, lnfold) -> None:
        """("body", l) of encoder_backward_schedule: the data-gradient chain of one post-LN transformer block."""
        mp, mg = self.store.mp, self.store.mg
        step, ph = self._step, self.reg.hidden_dropout
        lb, gs = self.lb[l], self._gsets[l % len(self._gsets)]
        w1, b1 = _wb(f"encoder.layers.{l}.layer_norm")
        w2, b2 = _wb(f"encoder.layers.{l}.final_layer_norm")
        # x2 = LN2(x1 + drop(f)):  G <- ds2 (residual path), Gd <- df = ds2 * dropmask
        ops.layernorm_bwd(self.G, lb.f, lb.mean2, lb.rstd2, mp(w2), self.G, gs["Gd"], mg(w2), mg(b2), ph,
                          self._sd("ffn", l, step), defer_to=lnfold)
        self._ffn_backward(l)                               # G = DH @ W1 + G
        # x1 = LN1(x + drop(a)):  G <- ds1, Gd1 <- da
        ops.layernorm_bwd(self.G, lb.a, lb.mean1, lb.rstd1, mp(w1), self.G, gs["Gd1"], mg(w1), mg(b1), ph,
                          self._sd("post_attn", l, step), defer_to=lnfold)
        self._attention_backward(l)
        if not self.grouped:
            self._qkv_wgrad_ungrouped(l)

    def _ffn_backward(self, l: int) -> None:
        """Shared by the two bodies above.  From df in Gd: [dW2, db2], DH = (df @ W2) * gelu'(pre) (lb.hpre holds gelu'(pre)),
        [dW1, db1], G = DH @ W1 (+ G in the post-LN wiring, where the residual path rides in G).  [...]: only without the
        grouped weight-gradient kernel (exact-f32 mode), each right after the dY it reads is final."""
        mg, M, H, I = self.store.mg, self.M, self.cfg.hidden_size, self.cfg.intermediate_size
        gl, gs = self.g_layer[l], self._gsets[l % len(self._gsets)]
        pre = f"encoder.layers.{l}.feed_forward."
        if not self.grouped:
            gl["dW2"]()
            ops.colsum(gs["Gd"], mg(pre + "output_dense.bias"), M, H)
        gl["dh"]()
        if not self.grouped:
            gl["dW1"]()
            ops.colsum(gs["DH"], mg(pre + "intermediate_dense.bias"), M, I)
        gl["dx1"]()

    def _attention_backward(self, l: int) -> None:
        """Shared likewise.  From da in Gd1: [dWo, dbo], DC = da @ Wo, attention backward into DQKV (fused, or dP, softmax, dq, dk, dv)."""
        cfg, B, T = self.cfg, self.B, self.T
        heads, d, pa = cfg.num_attention_heads, cfg.head_dim, self.reg.attention_dropout
        lb, gl, gs = self.lb[l], self.g_layer[l], self._gsets[l % len(self._gsets)]
        if not self.grouped:
            gl["dWo"]()
            ops.colsum(gs["Gd1"], self.store.mg(f"encoder.layers.{l}.attention.out_proj.bias"), self.M, cfg.hidden_size)
        gl["dctx"]()
        if self.fused:
            ops.attention_bwd(lb.qkv, lb.ctx, self.DC, lb.lse, gs["DQKV"], self.delta, B, T, heads, d, d ** -0.5,
                              pa, self._sd("attn", l, self._step))
        else:
            gl["dP"]()
            ops.softmax_bwd(self.S, lb.p, self.dS, B * heads * T, T, self.Tl, pa, self._sd("attn", l, self._step))
            gl["dq"]()
            gl["dk"]()
            gl["dv"]()

    def _qkv_wgrad_ungrouped(self, l: int) -> None:
        """dWqkv, dbqkv of block l from DQKV (exact-f32 mode: the 16-bit modes have them in the grouped launch)."""
        self.g_layer[l]["dWqkv"]()
        ops.colsum(self._gsets[l % len(self._gsets)]["DQKV"], self.store.qkv(l, "g", "bias"), self.M, 3 * self.cfg.hidden_size)

    def _conv_layer_grads(self, i: int) -> None:
        """Conv layer i >= 1 of the feature extractor, from d(pre-activation) in place of its output gradient: the weight
        gradient (dW GEMM into dwp, unpacked into the HF layout and added) and the data gradient (dX GEMM into col,
        folded into dconv[i - 1] by the adjoint of the tap gather)."""
        cfg = self.cfg
        self.dwp.zero_()
        self.g_conv_dw[i]()
        ops.unpack_conv_grad(self.dwp, self.store.mg(f"feature_extractor.conv_layers.{i}.conv.weight"))
        self.g_conv_dx[i]()
        ops.col2im(self.col, self.dconv[i - 1], self.Bc, self.lens[i - 1], self.lens[i], cfg.conv_dim[i - 1],
                   cfg.conv_kernel[i], cfg.conv_stride[i])

    def _backward_cnn(self) -> None:
        """Backward of the 7-layer conv feature extractor (HF:382-419) -- the reference's
        ``completely_freeze_feature_extractor: false`` ablation.  self.dn holds d(conv[6] output)."""
        cfg, st = self.cfg, self.store
        C = cfg.conv_dim
        mg = st.mg
        if self.ln_conv:
            self._backward_cnn_layer_norm()
            return
        for i in reversed(range(1, len(C))):
            gv = (self.dn if i == len(C) - 1 else self.dconv[i]).view(-1, C[i])
            ops.gelu_bwd(gv, self.conv_pre[i].view(-1, C[i]), gv)          # d(pre-activation), in place
            self._conv_layer_grads(i)
        ops.conv0_bwd(self._wav, st.mp("feature_extractor.conv_layers.0.conv.weight"), self.stats0,
                      st.mp("feature_extractor.conv_layers.0.layer_norm.weight"),
                      st.mp("feature_extractor.conv_layers.0.layer_norm.bias"), self.dconv[0], self.sums0,
                      mg("feature_extractor.conv_layers.0.conv.weight"),
                      mg("feature_extractor.conv_layers.0.layer_norm.weight"),
                      mg("feature_extractor.conv_layers.0.layer_norm.bias"), cfg.conv_kernel[0], cfg.conv_stride[0])


    def _backward_cnn_layer_norm(self) -> None:
        """_backward_cnn for the layer-norm family (HF:275-299, "-lv60" / xlsr): every layer is conv (+ bias) -> LayerNorm
        over the channels -> GELU.  Layers 6 .. 1: LayerNorm-GELU backward from the saved pre-norm z (in place on the
        incoming gradient; it also yields the LayerNorm's and the conv bias's gradients), then the same weight- and
        data-gradient products as the group-norm family.  Layer 0 recomputes its convolution from the waveform."""
        cfg, st = self.cfg, self.store
        C = cfg.conv_dim
        mp, mg = st.mp, st.mg
        fe = "feature_extractor.conv_layers."
        for i in reversed(range(1, len(C))):
            gv = (self.dn if i == len(C) - 1 else self.dconv[i]).view(-1, C[i])
            ops.layernorm_gelu_bwd(gv, self.conv_pre[i].view(-1, C[i]), mp(fe + f"{i}.layer_norm.weight"),
                                   mp(fe + f"{i}.layer_norm.bias"), gv, mg(fe + f"{i}.layer_norm.weight"),
                                   mg(fe + f"{i}.layer_norm.bias"), mg(fe + f"{i}.conv.bias") if cfg.conv_bias else None,
                                   self.lng_ws)
            self._conv_layer_grads(i)
        ops.conv0_layernorm_gelu_bwd(self._wav, mp(fe + "0.conv.weight"), mp(fe + "0.conv.bias") if cfg.conv_bias else None,
                                     mp(fe + "0.layer_norm.weight"), mp(fe + "0.layer_norm.bias"), self.dconv[0],
                                     mg(fe + "0.conv.weight"), mg(fe + "0.conv.bias") if cfg.conv_bias else None,
                                     mg(fe + "0.layer_norm.weight"), mg(fe + "0.layer_norm.bias"), self.c0l_ws,
                                     cfg.conv_kernel[0], cfg.conv_stride[0])
