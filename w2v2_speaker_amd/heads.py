"""Speaker classification heads on the HIP kernels: AAM-softmax (ref: src/optim/loss/aam_softmax.py:21-74)
and Linear + cross-entropy (ref: src/lightning_modules/speaker/wav2vec2_fc.py:199-210,
src/optim/loss/cross_entropy.py:15-33).  One object = fixed buffers + prebuilt GEMM descriptors for a
given (batch, embedding dim, classes); used by engine.Plan and by the nn.Module surface."""
from __future__ import annotations

import random
from collections import Counter
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from .ops import EPI_BIAS, EPI_SCALE_RC, Gemm


class ClassifierHead:
    def __init__(self, kind: str, batch: int, embed_dim: int, classes: int, *, w_master: torch.Tensor,
                 w_operand: torch.Tensor, w_grad: Optional[torch.Tensor], bias: Optional[torch.Tensor] = None,
                 bias_grad: Optional[torch.Tensor] = None, emb: torch.Tensor, act_dtype: torch.dtype,
                 train: bool, margin: float = 0.2, scale: float = 30.0, loss_scale: Optional[torch.Tensor] = None,
                 easy_margin: bool = False, sub_centers: int = 1, margin_type: str = "arc", inter_topk: int = 0,
                 inter_margin: float = 0.06):
        assert kind in ("aam", "ce", "ctc")      # "ctc" (CtcHead): the Linear of "ce" under another row kernel
        # the margin heads (include/w2v2_hip.h "margin heads"): K sub-centres per class, "arc" / "cos" margin, inter-top-k.
        # With all four at their defaults the head is the single-centre AAM head, launch for launch; anything else goes
        # through w2v2_margin_softmax_fwd_bwd, and every product below runs over classes * K rows or columns.
        self.K, self.margin_type = int(sub_centers), margin_type
        self.inter_topk, self.inter_margin = int(inter_topk), float(inter_margin)
        ops.check_margin_head(classes, self.K, self.inter_topk, self.inter_margin, margin_type)
        self.margin_head = (self.K, margin_type, self.inter_topk) != (1, "arc", 0)
        if self.margin_head and kind != "aam":
            raise ValueError(f"sub-centres, the cosine margin and inter-top-k belong to the 'aam' head, not to {kind!r}")
        self.loss_scale = loss_scale          # device record of the dynamic loss scale (fp16 activations) or None
        self.kind, self.B, self.E, self.C, self.train = kind, batch, embed_dim, classes, train
        self.margin, self.scale, self.easy_margin = margin, scale, bool(easy_margin)
        self.w_master, self.w_grad, self.bias, self.bias_grad, self.emb = w_master, w_grad, bias, bias_grad, emb
        dev, f32 = emb.device, torch.float32
        B, E, Cn = batch, embed_dim, classes * self.K
        self.Cn = Cn                          # weight rows = logit columns; self.C stays the number of classes
        self.ldc = (Cn + 7) // 8 * 8
        self.ldp = (classes + 7) // 8 * 8     # row stride of the softmax over the classes (= ldc without sub-centres)
        self.emb_lp = torch.empty(B, E, dtype=act_dtype, device=dev) if act_dtype != f32 else emb
        self.logits = torch.zeros(B, self.ldc, dtype=f32, device=dev)
        self.softmax = torch.zeros(B, self.ldp, dtype=f32, device=dev) if kind != "ctc" else None
        self.loss_rows = torch.empty(B, dtype=f32, device=dev)
        self.correct = torch.zeros(B, dtype=f32, device=dev)      # 1 where argmax(prediction) == label (train_acc)
        aam = kind == "aam"
        if aam:
            self.inv_x, self.inv_w = torch.empty(B, dtype=f32, device=dev), torch.empty(Cn, dtype=f32, device=dev)
            self.g_fwd = Gemm(B, Cn, E, self.emb_lp, w_operand, self.logits, lda=E, ldb=E, ldc=self.ldc,
                              epilogue=EPI_SCALE_RC, row_scale=self.inv_x, col_scale=self.inv_w)
        else:
            self.g_fwd = Gemm(B, Cn, E, self.emb_lp, w_operand, self.logits, lda=E, ldb=E, ldc=self.ldc,
                              epilogue=EPI_BIAS, bias=bias)
        if train:
            self.dcos_w = torch.zeros(B, self.ldc, dtype=act_dtype, device=dev)
            self.dcos_x = torch.zeros(B, self.ldc, dtype=act_dtype, device=dev) if aam else self.dcos_w
            self.rowdot = torch.empty(B, dtype=f32, device=dev)
            # the two accumulators of a step (column dots of the AAM normalisation, d(emb) partial sums) share one
            # buffer so that ONE zero_ranges launch clears both
            self._zbuf = torch.empty(Cn + B * E, dtype=f32, device=dev)
            self._ztab = torch.tensor([[0, Cn + B * E]], dtype=torch.int64, device=dev)
            self.coldot = self._zbuf[:Cn]
            self.G1 = self._zbuf[Cn:].view(B, E)
            # per-element g * cos of the AAM normalisation backward; folded over the batch in a fixed order (colsum with
            # <= 128 rows has one writer per column): the class-weight gradient is bitwise reproducible
            self.colprod = torch.empty(B, Cn, dtype=f32, device=dev) if aam else None
            self.demb = torch.empty(B, E, dtype=f32, device=dev)
            # d emb = dcos_w [B, C] . W [C, E]: 66 rows = ONE row of tiles, so the class dimension is cut into S chunks
            # (one batched launch + the ragged rest) whose f32 partials are then summed in a fixed order -- the single
            # launch walked all 5994 classes on 12 workgroups (144 us)
            S = max(1, min(16, Cn // 256))
            Kc = (Cn // S) // 8 * 8 if S > 1 else Cn
            rest = Cn - S * Kc
            self.dx_parts = torch.empty(S + (1 if rest else 0), B, E, dtype=f32, device=dev)
            self.g_dx = [Gemm(B, E, Kc, self.dcos_w, w_operand, self.dx_parts, lda=self.ldc, ldb=E, ldc=E, transB=True,
                              batch=S, batch_inner=S, a_strides=(0, Kc), b_strides=(0, Kc * E), c_strides=(0, B * E))]
            if rest:
                self.g_dx.append(Gemm(B, E, rest, self.dcos_w.view(-1)[S * Kc:], w_operand.view(-1)[S * Kc * E:],
                                      self.dx_parts[S], lda=self.ldc, ldb=E, ldc=E, transB=True))
            # AAM class-weight gradient: product, column dots and the F.normalize backward in ONE launch (csrc/heads.hip
            # aam_dw_kernel) when E % 8 == 0; other embeddings keep the three-launch GEMM path
            self.fused_dw = aam and E % 8 == 0
            if aam and not self.fused_dw:
                self.H1 = torch.empty(Cn, E, dtype=f32, device=dev)
                self.g_dw = Gemm(Cn, E, B, self.dcos_x, self.emb_lp, self.H1, lda=self.ldc, ldb=E, ldc=E,
                                 transA=True, transB=True)
            elif not aam:
                self.g_dw = Gemm(Cn, E, B, self.dcos_x, self.emb_lp, w_grad, lda=self.ldc, ldb=E, ldc=E,
                                 transA=True, transB=True, accumulate=True)

    def forward_backward(self, label: torch.Tensor):
        """(loss, softmax[B,C]); in training also d(loss)/d(emb) -> self.demb and the head gradients
        (dW written for AAM, accumulated for CE; dbias accumulated) into the tensors given at build."""
        B, Cn = self.B, self.C
        assert label.dtype == torch.int64 and label.is_cuda and label.shape == (B,)
        aam, tr = self.kind == "aam", self.train
        self._forward_logits()
        if self.margin_head:
            ops.margin_softmax_fwd_bwd(self.logits, label, self.softmax, self.loss_rows, self.dcos_w if tr else None,
                                       self.dcos_x if tr else None, self.inv_x, self.inv_w, self.rowdot if tr else None,
                                       self.colprod if tr else None, B, Cn, self.K, self.ldc, self.ldp, self.margin,
                                       self.scale, self.loss_scale if tr else None, self.correct,
                                       easy_margin=self.easy_margin, margin_type=self.margin_type, n_top=self.inter_topk,
                                       inter_margin=self.inter_margin)
        else:
            ops.aam_softmax_fwd_bwd(self.logits, label, self.softmax, self.loss_rows,
                                    self.dcos_w if tr else None, (self.dcos_x if aam else None) if tr else None,
                                    self.inv_x if aam else None, self.inv_w if aam else None,
                                    self.rowdot if (tr and aam) else None, self.colprod if (tr and aam) else None,
                                    B, Cn, self.ldc, self.margin if aam else -1.0, self.scale,
                                    self.loss_scale if tr else None, self.correct, easy_margin=self.easy_margin)
        loss = torch.empty((), dtype=torch.float32, device=self.loss_rows.device)     # (allocator only: no kernel)
        ops.mean(self.loss_rows, loss)
        if tr:
            self._backward_from_dlogits()
        return loss, self.softmax[:, :Cn]

    def _forward_logits(self) -> None:
        """The launches in front of the row kernel: operand cast, (AAM) row norms, the logit GEMM, the accumulators' zeroing."""
        B, E, Cn = self.B, self.E, self.Cn
        aam, tr = self.kind == "aam", self.train
        if self.emb_lp is not self.emb:
            ops.cast(self.emb, self.emb_lp)
        if aam:
            ops.row_invnorm(self.emb, self.inv_x, B, E)
            ops.row_invnorm(self.w_master, self.inv_w, Cn, E)
        self.g_fwd()
        if tr:
            ops.zero_ranges(self._zbuf, self._ztab, blocks_per_range=16)

    def _backward_from_dlogits(self) -> None:
        """The launches behind the row kernel: d(emb) and the head's parameter gradients from dcos_w / dcos_x."""
        B, E, Cn = self.B, self.E, self.Cn
        aam = self.kind == "aam"
        for g in self.g_dx:
            g()
        ops.colsum(self.dx_parts, self.G1.view(-1), self.dx_parts.shape[0], B * E)    # <= 128 rows: one writer
        if aam:
            ops.normalize_bwd(self.G1, self.emb, self.inv_x, self.rowdot, self.demb, B, E)
            if self.fused_dw:
                ops.aam_dw(self.dcos_x, self.emb_lp, self.colprod, self.w_master, self.inv_w, self.w_grad, B, Cn, E,
                           self.ldc)
            else:
                self.g_dw()
                ops.colsum(self.colprod, self.coldot, B, Cn)
                ops.normalize_bwd(self.H1, self.w_master, self.inv_w, self.coldot, self.w_grad, Cn, E)
        else:
            self.demb.copy_(self.G1)
            self.g_dw()
            ops.colsum(self.dcos_w, self.bias_grad, B, Cn, self.ldc)


class CtcHead(ClassifierHead):
    """ref: src/lightning_modules/speaker/speaker_recognition_module.py:222-244 (_train_step_ctc_loss) +
    src/optim/loss/ctc_loss.py:36-58: per-frame Linear (``classes`` = speakers + 1 outputs, class 0 the blank) and the CTC
    loss of ONE label per utterance over all ``frames`` frames.  ClassifierHead("ce")'s forward GEMM and gradient GEMMs over
    the ``batch * frames`` rows of the no-pooling embedding, with w2v2_ctc_fwd_bwd in the row kernel's place.  The
    reference adds 1 to the batch's label tensor in place; here the label stays as it is and the kernel adds
    ``target_offset``.  The length tensors (``frames`` and 1 per utterance) are built once: a step uploads nothing and
    synchronises nothing.  Returns (loss, None): no softmax and no accuracy in this mode (ref: :458)."""

    def __init__(self, batch: int, frames: int, embed_dim: int, classes: int, *, blank: int = 0, target_offset: int = 1,
                 **kw):
        super().__init__("ctc", batch * frames, embed_dim, classes, **kw)
        dev = self.emb.device
        self.U, self.T, self.blank, self.target_offset = batch, frames, int(blank), int(target_offset)
        self.loss_rows = torch.empty(batch, dtype=torch.float32, device=dev)
        self.correct = None
        self.in_len = torch.full((batch,), frames, dtype=torch.int32, device=dev)
        self.tgt_len = torch.ones(batch, dtype=torch.int32, device=dev)
        self.workspace = torch.empty(ops.ctc_workspace_floats(batch, frames, 1), dtype=torch.float32, device=dev)

    def forward_backward(self, label: torch.Tensor):
        """label [batch] int64 speaker indices in [0, classes - 1) -> (loss, None)."""
        assert label.dtype == torch.int64 and label.is_cuda and label.shape == (self.U,) and label.is_contiguous()
        tr = self.train
        self._forward_logits()
        ops.ctc_fwd_bwd(self.logits, label, self.in_len, self.tgt_len, self.loss_rows, self.dcos_w if tr else None,
                        self.workspace, self.U, self.T, self.C, self.ldc, target_width=1, target_stride=1,
                        target_offset=self.target_offset, blank=self.blank, loss_scale=self.loss_scale if tr else None)
        loss = torch.empty((), dtype=torch.float32, device=self.loss_rows.device)
        ops.mean(self.loss_rows, loss)
        if tr:
            self._backward_from_dlogits()
        return loss, None


class LetterHead(ClassifierHead):
    """ref: src/lightning_modules/speech/wav2vec2_fc_letter.py:65-86 (SpeechRecognitionHead: dropout + ``lm_head``) +
    speech_recognition_module.py:100-116 (the CTC loss against the transcript): CtcHead's sibling over the ``batch *
    frames`` rows of the no-pooling embedding, with ``classes`` = the vocabulary size, class 0 the blank and the labels
    taken as they are (``target_offset`` 0).  Transcripts of up to ``max_target`` <= 1023 letters: the kernels of
    csrc/ctc_long.hip where the step's transcript tensor is wider than 31, the short ones below (the rule of
    ``CtcLoss(long_targets=True)``).

    A step's transcript [batch, width] int64, its target lengths and the input lengths IN FRAMES travel in one upload
    through two pinned staging buffers used in turn, the way TripletHead uploads its indices: the host never waits for
    the step it enqueues.  ``final_dropout`` > 0 in training: the library's dropout kernel in front of the Linear, the
    same keep-mask (same seed) on d(emb) behind it; 0 launches nothing.  ``decode()`` runs the greedy decoder on the logits
    the step just produced.  Returns (loss, None)."""

    def __init__(self, batch: int, frames: int, embed_dim: int, classes: int, *, blank: int = 0,
                 max_target: int = ops.CTC_LONG_MAX_TARGET, final_dropout: float = 0.0, **kw):
        if not 1 <= max_target <= ops.CTC_LONG_MAX_TARGET:
            raise ValueError(f"letter head: max_target {max_target} outside [1, {ops.CTC_LONG_MAX_TARGET}]")
        self.emb_in = kw["emb"]
        self.p_drop = float(final_dropout) if kw["train"] else 0.0
        if self.p_drop > 0:
            kw["emb"] = torch.empty_like(self.emb_in)           # dropout(emb): what the Linear and its weight gradient read
        super().__init__("ctc", batch * frames, embed_dim, classes, **kw)
        dev = self.emb.device
        self.U, self.T, self.blank, self.Wmax, self.width = batch, frames, int(blank), int(max_target), 0
        self.loss_rows = torch.empty(batch, dtype=torch.float32, device=dev)
        self.correct = None
        floats = max(ops.ctc_long_workspace_floats(batch, frames, self.Wmax),
                     ops.ctc_workspace_floats(batch, frames, min(self.Wmax, ops.CTC_MAX_TARGET)))
        self.workspace = torch.empty(floats, dtype=torch.float32, device=dev)
        # one byte image {transcript int64 [U, Wmax] | input lengths int32 [U] | target lengths int32 [U]} on the device
        # and in two pinned staging buffers: one copy per step
        nb = batch * self.Wmax * 8
        self._raw = torch.zeros(nb + 8 * batch, dtype=torch.uint8, device=dev)
        self.targets, self.in_len, self.tgt_len = self._views(self._raw)
        self._stage = [torch.zeros(nb + 8 * batch, dtype=torch.uint8, pin_memory=dev.type == "cuda") for _ in range(2)]
        self._copied = [None, None]
        self._turn = 0
        # decoder output {tokens int32 [U, T] | counts int32 [U]}: one buffer, one copy to the host per batch
        self._dec = torch.zeros(batch * frames + batch, dtype=torch.int32, device=dev)
        self.tokens, self.counts = self._dec[:batch * frames].view(batch, frames), self._dec[batch * frames:]

    def _views(self, raw: torch.Tensor):
        U, nb = self.U, self.U * self.Wmax * 8
        return (raw[:nb].view(torch.int64).view(U, self.Wmax), raw[nb:nb + 4 * U].view(torch.int32),
                raw[nb + 4 * U:].view(torch.int32))

    def set_batch(self, transcript: torch.Tensor, target_lengths, input_frames) -> None:
        """transcript [U, width] integer host tensor (right-padded), target_lengths [U] and input_frames [U] (frames of
        each utterance, at most ``frames``) host sequences or tensors.  Validated here, on the host."""
        U = self.U
        transcript = torch.as_tensor(transcript).to("cpu", torch.int64)
        if transcript.dim() == 1:
            transcript = transcript[None]
        tl = [int(v) for v in (target_lengths.tolist() if hasattr(target_lengths, "tolist") else target_lengths)]
        fl = [int(v) for v in (input_frames.tolist() if hasattr(input_frames, "tolist") else input_frames)]
        if transcript.dim() != 2 or transcript.shape[0] != U or len(tl) != U or len(fl) != U:
            raise ValueError(f"letter head: a transcript [{U}, width] with {U} target and {U} input lengths is needed, got "
                             f"{tuple(transcript.shape)}, {len(tl)} and {len(fl)}")
        width = int(transcript.shape[1])
        if max(tl) > self.Wmax:
            raise ValueError(f"letter head: a transcript of {max(tl)} labels; at most {self.Wmax} per utterance are built")
        width = min(width, self.Wmax)                      # (columns past the longest transcript are padding)
        if min(tl) < 0 or max(tl) > width:
            raise ValueError(f"letter head: target lengths must lie in [0, {width}]")
        if min(fl) < 0 or max(fl) > self.T:
            raise ValueError(f"letter head: input lengths must lie in [0, {self.T}] frames")
        t = self._turn
        self._turn = 1 - t
        if self._copied[t] is not None:
            self._copied[t].synchronize()     # the upload of two steps ago has left this staging buffer
        tg, il, tgl = self._views(self._stage[t])
        tg[:, :width] = transcript[:, :width]
        il.copy_(torch.tensor(fl, dtype=torch.int32))
        tgl.copy_(torch.tensor(tl, dtype=torch.int32))
        self._raw.copy_(self._stage[t], non_blocking=True)
        if self._stage[t].is_pinned():
            self._copied[t] = torch.cuda.Event()
            self._copied[t].record()
        self.width = width

    def forward_backward(self, label: Optional[torch.Tensor] = None, seed: int = 0):
        """On what ``set_batch`` uploaded (``label`` is not used) -> (loss, None).  ``seed``: the dropout stream key."""
        tr = self.train
        if self.p_drop > 0:
            ops.dropout(self.emb_in, self.emb, self.p_drop, seed)
        self._forward_logits()
        long = self.width > ops.CTC_MAX_TARGET
        (ops.ctc_long_fwd_bwd if long else ops.ctc_fwd_bwd)(
            self.logits, self.targets if self.width else None, self.in_len, self.tgt_len, self.loss_rows,
            self.dcos_w if tr else None, self.workspace, self.U, self.T, self.C, self.ldc, target_width=self.width,
            target_stride=self.Wmax, target_offset=0, blank=self.blank, loss_scale=self.loss_scale if tr else None)
        loss = torch.empty((), dtype=torch.float32, device=self.loss_rows.device)
        ops.mean(self.loss_rows, loss)
        if tr:
            self._backward_from_dlogits()
            if self.p_drop > 0:
                ops.dropout_(self.demb, self.p_drop, seed)
        return loss, None

    def forward_only(self, input_frames) -> None:
        """The logits of the current embedding without a loss (test_step): uploads the input lengths for ``decode()``."""
        self.set_batch(torch.zeros(self.U, 0, dtype=torch.int64), [0] * self.U, input_frames)
        if self.p_drop > 0:
            raise RuntimeError("letter head: forward_only is the evaluation path; a training head with final_dropout "
                               "draws its mask in forward_backward")
        self._forward_logits()

    def decode(self):
        """Greedy decoding of the current logits over each utterance's input length -> (tokens int32 [U, T], counts int32
        [U]) on the device: views of ONE buffer, ``decoded()`` copies it to the host once."""
        ops.ctc_greedy_decode(self.logits, self.in_len, self.tokens, self.counts, self.U, self.T, self.C, self.ldc,
                              blank=self.blank)
        return self.tokens, self.counts

    def decoded(self):
        """decode() and the one device-to-host copy of the batch -> (tokens [U, T], counts [U]) host tensors."""
        self.decode()
        host = self._dec.cpu()
        return host[:self.U * self.T].view(self.U, self.T), host[self.U * self.T:]


class BceHead:
    """ref: wav2vec2_paired_input.py:200-206 + binary_cross_entropy.py:24-40: Linear(H -> 1) on the CLS token,
    BCE-with-logits (mean over pairs), prediction = sigmoid(logit).  Same interface as ClassifierHead."""

    def __init__(self, batch: int, embed_dim: int, *, w: torch.Tensor, b: torch.Tensor,
                 w_grad: Optional[torch.Tensor], b_grad: Optional[torch.Tensor], emb: torch.Tensor, train: bool,
                 loss_scale: Optional[torch.Tensor] = None):
        dev, f32 = emb.device, torch.float32
        self.loss_scale = loss_scale
        self.B, self.E, self.w, self.b, self.w_grad, self.b_grad, self.emb, self.train = (batch, embed_dim, w, b, w_grad,
                                                                                          b_grad, emb, train)
        self.prob = torch.empty(batch, dtype=f32, device=dev)
        self.loss_rows = torch.empty(batch, dtype=f32, device=dev)
        self.dlogit = torch.empty(batch, dtype=f32, device=dev) if train else None
        self.demb = torch.empty(batch, embed_dim, dtype=f32, device=dev) if train else None

    def forward_backward(self, label: torch.Tensor):
        """label [B] int64 in {0, 1} (1 = same speaker) -> (loss, prediction [B])."""
        assert label.dtype == torch.int64 and label.is_cuda and label.shape == (self.B,)
        tr = self.train
        ops.bce_head_fwd_bwd(self.emb, self.w.view(-1), self.b, label, self.prob, self.loss_rows,
                             self.dlogit if tr else None, self.demb if tr else None,
                             self.w_grad.view(-1) if tr else None, self.b_grad if tr else None, self.B, self.E,
                             self.loss_scale if tr else None)
        loss = torch.empty((), dtype=torch.float32, device=self.loss_rows.device)
        ops.mean(self.loss_rows, loss)
        return loss, self.prob


def sample_triplets(labels: Sequence[int], rng=random) -> Tuple[List[int], List[int]]:
    """(pos, neg): for every batch row the row of its positive (another row with the same label) and of its negative
    (a row with another label), drawn like ref: src/optim/loss/triplet_loss.py:45-99 -- row by row, the positive then
    the negative, each ``rng.choice`` over the candidate rows in ascending order -- so the same ``random.seed`` gives
    the reference's triplets.  ValueError when a label occurs once (the reference's ``verify_labels`` assertion) or when
    the batch holds one speaker (no negative exists)."""
    labels = [int(l) for l in labels]
    count = Counter(labels)
    single = sorted(l for l, c in count.items() if c < 2)
    if single:
        raise ValueError(f"triplet loss: every label of a batch must occur at least twice, labels {single} occur once")
    if len(count) < 2:
        raise ValueError("triplet loss: a batch with a single speaker has no negative")
    pos, neg = [], []
    for i, l in enumerate(labels):
        pos.append(rng.choice([j for j, m in enumerate(labels) if m == l and j != i]))
        neg.append(rng.choice([j for j, m in enumerate(labels) if m != l]))
    return pos, neg


class TripletHead:
    """ref: src/optim/loss/triplet_loss.py (F.triplet_margin_loss over one sampled triplet per batch row) on
    w2v2_triplet_fwd_bwd: two launches + the mean.  The host never waits for the step it enqueues: the index upload goes
    through two pinned staging buffers used in turn, and the only wait is for the upload of two steps ago.  ``emb`` [B, E] f32 is read in place;
    ``demb`` (given, or allocated) is written, or added to with ``accumulate`` (the triplet + CE head, whose CE part has
    filled it).  ``coef`` weighs the gradient (``c_triplet``); ``loss_rows`` and the returned loss stay unweighted."""

    def __init__(self, batch: int, embed_dim: int, emb: torch.Tensor, margin: float = 1.0, coef: float = 1.0,
                 train: bool = True, loss_scale: Optional[torch.Tensor] = None, demb: Optional[torch.Tensor] = None,
                 accumulate: bool = False):
        dev, f32 = emb.device, torch.float32
        assert emb.dtype == f32 and emb.shape == (batch, embed_dim) and emb.stride(1) == 1
        assert not accumulate or demb is not None, "accumulate adds to a gradient somebody else wrote"
        self.B, self.E, self.emb, self.train = batch, embed_dim, emb, train
        self.margin, self.coef, self.loss_scale, self.accumulate = float(margin), float(coef), loss_scale, accumulate
        self.d_ap = torch.empty(batch, dtype=f32, device=dev)
        self.d_an = torch.empty(batch, dtype=f32, device=dev)
        self.loss_rows = torch.empty(batch, dtype=f32, device=dev)
        self.demb = (demb if demb is not None else torch.empty(batch, embed_dim, dtype=f32, device=dev)) if train else None
        # fixed device index buffers [2, B], fed from a pinned staging buffer by one non-blocking copy per step
        self._idx = torch.zeros(2, batch, dtype=torch.int64, device=dev)
        # two pinned staging buffers, used in turn: before one is rewritten the host waits for the upload that read it
        # TWO steps ago (an event that has long fired), so the host may run one whole step ahead of the device
        self._stage = [torch.zeros(2, batch, dtype=torch.int64, pin_memory=dev.type == "cuda") for _ in range(2)]
        self._copied = [None, None]
        self._turn = 0

    def set_triplets(self, pos: Sequence[int], neg: Sequence[int]) -> None:
        B = self.B
        pos, neg = [int(v) for v in pos], [int(v) for v in neg]
        if len(pos) != B or len(neg) != B:
            raise ValueError(f"triplets: {len(pos)} positives and {len(neg)} negatives for a batch of {B}")
        if min(pos + neg) < 0 or max(pos + neg) >= B:
            raise ValueError(f"triplets: row indices must lie in [0, {B})")
        t = self._turn
        self._turn = 1 - t
        if self._copied[t] is not None:
            self._copied[t].synchronize()     # the upload of two steps ago has left this staging buffer
        self._stage[t].copy_(torch.tensor([pos, neg], dtype=torch.int64))
        self._idx.copy_(self._stage[t], non_blocking=True)
        if self._stage[t].is_pinned():
            self._copied[t] = torch.cuda.Event()
            self._copied[t].record()

    def forward_backward(self, label: Optional[torch.Tensor] = None, triplets=None):
        """-> (loss, None).  ``triplets`` = (pos, neg) row indices (validated on the host); None draws them with
        ``sample_triplets`` from ``label.tolist()`` -- a host synchronisation when the label is on the device."""
        if triplets is None:
            triplets = sample_triplets(label.tolist())
        self.set_triplets(*triplets)
        tr = self.train
        ops.triplet_fwd_bwd(self.emb, self._idx[0], self._idx[1], self.d_ap, self.d_an, self.loss_rows,
                            self.demb if tr else None, self.B, self.E, self.margin, self.coef, self.accumulate and tr,
                            self.loss_scale if tr else None, ld=self.emb.stride(0))
        loss = torch.empty((), dtype=torch.float32, device=self.loss_rows.device)
        ops.mean(self.loss_rows, loss)
        return loss, None


class FcStack:
    """Hidden ``nn.Sequential(nn.Linear, nn.ReLU)`` layers between the pooled embedding and the loss head
    (ref: src/lightning_modules/speaker/wav2vec2_fc.py:185-228 ``fc_list``, :363-412 pre/post speaker-embedding ops).
    f32 throughout (B x a few hundred features: negligible work, exact arithmetic) on the skinny linear kernels
    (csrc/skinny.hip): one launch per layer forward (bias + ReLU fused), two per layer backward (ReLU' fused)."""

    def __init__(self, store, batch: int, in_dim: int, hidden, x0: torch.Tensor, train: bool):
        dev, f32 = x0.device, torch.float32
        self.B, self.dims, self.train = batch, [in_dim] + list(hidden), train
        self.x = [x0] + [torch.empty(batch, h, dtype=f32, device=dev) for h in hidden]
        self.w = [store.p(f"fc_list.{i}.0.weight") for i in range(len(hidden))]
        self.b = [store.p(f"fc_list.{i}.0.bias") for i in range(len(hidden))]
        if train:
            self.dw = [store.g(f"fc_list.{i}.0.weight") for i in range(len(hidden))]
            self.db = [store.g(f"fc_list.{i}.0.bias") for i in range(len(hidden))]
            self.dx = [torch.empty(batch, d, dtype=f32, device=dev) for d in self.dims]      # d(loss)/d(x[i])

    def forward(self, upto: Optional[int] = None) -> torch.Tensor:
        """Run layers 0 .. upto (all by default); returns the output of the last one run."""
        n = len(self.w) if upto is None else upto + 1
        for i in range(n):
            ops.skinny_linear_fwd(self.x[i], self.w[i], self.b[i], self.x[i + 1], ops.ACT_RELU)
        return self.x[n]

    def backward(self, dout: torch.Tensor) -> torch.Tensor:
        """dout = d(loss)/d(output of the last layer) -> d(loss)/d(x0); parameter gradients accumulated."""
        n = len(self.w)
        self.dx[n].copy_(dout)
        for i in reversed(range(n)):
            ops.skinny_linear_bwd_w(self.dx[i + 1], self.x[i + 1], self.x[i], self.dw[i], self.db[i], ops.ACT_RELU, True)
            ops.skinny_linear_bwd_x(self.dx[i + 1], self.x[i + 1], self.w[i], self.dx[i], ops.ACT_RELU)
        return self.dx[0]
