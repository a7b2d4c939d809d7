"""The CTC loss of ref: src/optim/loss/ctc_loss.py on the device (``w2v2_ctc_fwd_bwd``, csrc/ctc.hip).  The reference
transposes the logits, takes ``log_softmax`` and copies the whole [T, B, C] tensor to the host for torch's CPU
``F.ctc_loss`` (ref: :36-58); here the logits stay where they are: row statistics, the lattice recursion and the dense
gradient are three launches, and nothing waits for the host.  Same surface as the reference's class:
``CtcLoss(blank_idx=0)``, ``forward(predictions [B, T, C], prediction_lengths [B], ground_truths, ground_truth_lengths
[B])`` -> the mean over the batch of nll / max(target length, 1), infinite losses counted as 0 (``zero_infinity=True``).
``ground_truths``: [B, Lmax] or the concatenated 1-D layout of ``F.ctc_loss``; at most 31 labels per utterance (longer
targets: ValueError from the width of the tensor; a 1-D row that is longer than 31 gives a NaN loss).  Lengths that are
already int32 device tensors cost no upload.  ``CtcLoss(long_targets=True)`` is the speech form (ref:
src/lightning_modules/speech/speech_recognition_module.py:100-116): up to 1023 labels per utterance in both layouts, the
kernels of csrc/ctc_long.hip (``w2v2_ctc_long_fwd_bwd``) where the rows are wider than 31 and the short ones below."""
from __future__ import annotations

import torch

from ... import ops


class _CtcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predictions, in_len, targets, tgt_len, blank):
        B, T, C = predictions.shape
        f32, dev = torch.float32, predictions.device
        logits = predictions.detach().to(f32).contiguous().view(B * T, C)
        rows = torch.empty(B, dtype=f32, device=dev)
        dlogits = torch.empty(B * T, C, dtype=f32, device=dev) if predictions.requires_grad else None
        width = 0 if targets is None else targets.shape[1]
        # (the width decides: the short form refuses what it cannot hold, and pad_targets let it through only on request)
        long = width > ops.CTC_MAX_TARGET
        ws_floats, fwd_bwd = (ops.ctc_long_workspace_floats, ops.ctc_long_fwd_bwd) if long else (ops.ctc_workspace_floats,
                                                                                                 ops.ctc_fwd_bwd)
        ws = torch.empty(ws_floats(B, T, width), dtype=f32, device=dev)
        fwd_bwd(logits, targets, in_len, tgt_len, rows, dlogits, ws, B, T, C, C, target_width=width, target_offset=0,
                blank=blank)
        loss = torch.empty((), dtype=f32, device=dev)
        ops.mean(rows, loss)
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.dtype = (B, T, C), predictions.dtype
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        return (dlogits.view(ctx.shape) * dloss).to(ctx.dtype), None, None, None, None


def pad_targets(ground_truths: torch.Tensor, tgt_len: torch.Tensor, batch: int, long_targets: bool = False):
    """[B, Lmax] int64 rows for the kernel, on the device and without a synchronisation; None when there is no label."""
    if long_targets:
        return _pad_long_targets(ground_truths, tgt_len, batch)
    t = ground_truths.to(torch.int64)
    if t.dim() == 2:
        if t.shape[0] != batch:
            raise ValueError(f"ctc: {t.shape[0]} target rows for a batch of {batch}")
        if t.shape[1] > ops.CTC_MAX_TARGET:
            raise ValueError(f"ctc: targets of width {t.shape[1]}; at most {ops.CTC_MAX_TARGET} labels per utterance are "
                             "built (the lattice of one utterance is one wavefront)")
        return t.contiguous() if t.shape[1] else None
    if t.dim() != 1:
        raise ValueError(f"ctc: targets must be [B, Lmax] or concatenated 1-D, got {tuple(t.shape)}")
    n = t.numel()
    if n > ops.CTC_MAX_TARGET * batch:
        raise ValueError(f"ctc: {n} concatenated labels for {batch} utterances; at most {ops.CTC_MAX_TARGET} per "
                         "utterance are built")
    if n == 0:
        return None
    width = min(n, ops.CTC_MAX_TARGET)
    start = torch.cumsum(tgt_len.to(torch.int64), 0) - tgt_len
    idx = (start[:, None] + torch.arange(width, device=t.device)).clamp_(0, n - 1)
    return t[idx]          # (columns past a row's length hold its neighbours' labels: never read)


def _pad_long_targets(ground_truths: torch.Tensor, tgt_len: torch.Tensor, batch: int):
    cap = ops.CTC_LONG_MAX_TARGET
    t = ground_truths.to(torch.int64)
    if t.dim() == 2:
        if t.shape[0] != batch:
            raise ValueError(f"ctc: {t.shape[0]} target rows for a batch of {batch}")
        if t.shape[1] > cap:
            raise ValueError(f"ctc: targets of width {t.shape[1]}; at most {cap} labels per utterance are built (the "
                             "lattice of one utterance is one workgroup)")
        return t.contiguous() if t.shape[1] else None
    if t.dim() != 1:
        raise ValueError(f"ctc: targets must be [B, Lmax] or concatenated 1-D, got {tuple(t.shape)}")
    n = t.numel()
    if n > cap * batch:
        raise ValueError(f"ctc: {n} concatenated labels for {batch} utterances; at most {cap} per utterance are built")
    if n == 0:
        return None
    width = min(n, cap)        # (no synchronisation for the longest row: a row longer than this gives a NaN loss)
    start = torch.cumsum(tgt_len.to(torch.int64), 0) - tgt_len
    idx = (start[:, None] + torch.arange(width, device=t.device)).clamp_(0, n - 1)
    return t[idx]


class CtcLoss(torch.nn.Module):
    def __init__(self, blank_idx: int = 0, long_targets: bool = False):
        super().__init__()
        self.blank_idx = blank_idx
        self.long_targets = bool(long_targets)

    def forward(self, predictions: torch.Tensor, prediction_lengths: torch.Tensor, ground_truths: torch.Tensor,
                ground_truth_lengths: torch.Tensor) -> torch.Tensor:
        if predictions.dim() != 3:
            raise ValueError(f"ctc: predictions must be [B, T, C], got {tuple(predictions.shape)}")
        if predictions.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"ctc: predictions must be f32, f16 or bf16, got {predictions.dtype}")
        dev, B = predictions.device, predictions.shape[0]
        in_len = prediction_lengths.to(dev, torch.int32).contiguous()
        tgt_len = ground_truth_lengths.to(dev, torch.int32).contiguous()
        if in_len.shape != (B,) or tgt_len.shape != (B,):
            raise ValueError(f"ctc: the length tensors must be [{B}]")
        targets = pad_targets(ground_truths.to(dev), tgt_len, B, self.long_targets)
        return _CtcFn.apply(predictions, in_len, targets, tgt_len, int(self.blank_idx)).to(predictions.dtype)
