"""The weighted sum of cross-entropy and triplet loss of ref: src/optim/loss/triplet_ce_loss.py:
``TripletCrossEntropyLoss(c_ce=1, c_triplet=1)``, ``forward(embeddings, logits, label_indexes)`` ->
(c_ce * CE(logits) + c_triplet * triplet(embeddings), CE softmax prediction); a weight below 1 is a ValueError.
Both terms run on the HIP head kernels; one autograd function forms the sum (triplet_loss._TripletFn)."""
from __future__ import annotations

import torch

from .cross_entropy import CrossEntropyLoss
from .triplet_loss import TripletLoss


class TripletCrossEntropyLoss(TripletLoss, CrossEntropyLoss):
    def __init__(self, c_ce: float = 1, c_triplet: float = 1):
        super().__init__()              # (the triplet term runs at the default margin, as in the reference)
        if min(c_ce, c_triplet) < 1:
            raise ValueError(f"the loss weights must be at least 1, got {c_ce=}, {c_triplet=}")
        self.c_ce, self.c_triplet = c_ce, c_triplet

    def forward(self, embeddings: torch.Tensor, logits: torch.Tensor, label_indexes: torch.Tensor):
        ce, prediction = CrossEntropyLoss.forward(self, logits, label_indexes)
        return self._weighted(embeddings, label_indexes, self.c_triplet, ce, self.c_ce), prediction
