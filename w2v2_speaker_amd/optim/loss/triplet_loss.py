"""The triplet margin loss of ref: src/optim/loss/triplet_loss.py on the HIP triplet head (``w2v2_triplet_fwd_bwd``):
one (anchor, positive, negative) triplet per batch row, drawn on the host with the reference's calls of the global
``random`` module (heads.sample_triplets), named by row index -- nothing is gathered or stacked on the device.
Same surface as the reference's class: ``TripletLoss(margin=1)``, ``.margin``, ``forward(embeddings, label_indexes)``
-> loss, the static ``verify_labels`` (AssertionError when a label occurs once)."""
from __future__ import annotations

from collections import Counter
from typing import Optional, Sequence

import torch

from ... import ops
from ...heads import sample_triplets


class _TripletFn(torch.autograd.Function):
    """loss = c_ce * ce + c_triplet * mean_i max(margin + d(a_i, p_i) - d(a_i, n_i), 0); ``ce`` is an optional scalar
    (the cross-entropy term of TripletCrossEntropyLoss) whose gradient is passed through with its weight."""

    @staticmethod
    def forward(ctx, emb, idx, margin, c_triplet, ce, c_ce):
        B, E = emb.shape
        f32, dev = torch.float32, emb.device
        d_ap, d_an, rows = (torch.empty(B, dtype=f32, device=dev) for _ in range(3))
        demb = torch.empty(B, E, dtype=f32, device=dev)
        ops.triplet_fwd_bwd(emb, idx[0], idx[1], d_ap, d_an, rows, demb, B, E, margin, c_triplet)
        loss = torch.empty((), dtype=f32, device=dev)
        ops.mean(rows, loss)
        ctx.save_for_backward(demb)                     # already weighted by c_triplet
        ctx.c_ce = c_ce
        return loss * c_triplet if ce is None else ce * c_ce + loss * c_triplet

    @staticmethod
    def backward(ctx, dloss):
        (demb,) = ctx.saved_tensors
        return demb * dloss, None, None, None, (dloss * ctx.c_ce if ctx.needs_input_grad[4] else None), None


class TripletLoss(torch.nn.Module):
    def __init__(self, margin: float = 1):
        super().__init__()
        self.margin = margin

    @staticmethod
    def verify_labels(label_list: Sequence[int]) -> None:
        lonely = [label for label, n in Counter(label_list).items() if n < 2]
        assert not lonely, f"labels {lonely} occur once in the batch: no positive for them"

    def _weighted(self, embeddings: torch.Tensor, label_indexes: torch.Tensor, c_triplet: float = 1.0,
                  ce: Optional[torch.Tensor] = None, c_ce: float = 1.0) -> torch.Tensor:
        """c_ce * ce + c_triplet * triplet(embeddings).  The labels come to the host, as in the reference (a
        synchronisation): that is where the triplets are drawn."""
        labels = label_indexes.detach().cpu().tolist()
        self.verify_labels(labels)
        idx = torch.tensor(sample_triplets(labels), dtype=torch.int64).to(embeddings.device)
        out = _TripletFn.apply(embeddings.float().contiguous(), idx, float(self.margin), float(c_triplet), ce,
                               float(c_ce))
        return out.to(embeddings.dtype)

    def forward(self, embeddings: torch.Tensor, label_indexes: torch.Tensor):
        return self._weighted(embeddings, label_indexes)
