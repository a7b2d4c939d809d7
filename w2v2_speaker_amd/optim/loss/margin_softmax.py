"""``SubCenterMarginSoftMaxLoss``: the margin heads of include/w2v2_hip.h ("margin heads") behind the interface of
``AngularAdditiveMarginSoftMaxLoss`` -- ``sub_centers`` weight rows per class (the class cosine is the largest of them),
``margin_type`` "arc" (additive angular) or "cos" (additive cosine: AM-softmax / CosFace), and ``inter_topk`` hardest
negative classes pushed ``inter_margin`` radians towards the embedding.  No reference file has such a loss: the semantics are this
project's own.  It IS an ``AngularAdditiveMarginSoftMaxLoss`` (the modules' isinstance checks accept it); with
``sub_centers=1, margin_type="arc", inter_topk=0`` it runs that class's kernel, launch for launch."""
from __future__ import annotations

import torch

from ... import ops
from .aam_softmax import AngularAdditiveMarginSoftMaxLoss


class SubCenterMarginSoftMaxLoss(AngularAdditiveMarginSoftMaxLoss):
    def __init__(self, input_features, output_features, margin=0.2, scale=30, easy_margin=False, *, sub_centers=1,
                 margin_type="arc", inter_topk=0, inter_margin=0.06, device="cuda",
                 act_dtype: torch.dtype = torch.bfloat16):
        """``fc_weights`` is [output_features * sub_centers, input_features] (xavier-normal over that shape), sub-centre k
        of class c in row c * sub_centers + k; ``forward(x, label) -> (loss, prediction [B, output_features])``."""
        ops.check_margin_head(int(output_features), sub_centers, inter_topk, inter_margin, margin_type)
        super().__init__(input_features, int(output_features) * int(sub_centers), margin=margin, scale=scale,
                         easy_margin=easy_margin, device=device, act_dtype=act_dtype)
        self.output_features = int(output_features)
        self.sub_centers, self.margin_type = int(sub_centers), margin_type
        self.inter_topk, self.inter_margin = int(inter_topk), float(inter_margin)

    def _margin_kw(self) -> dict:
        return dict(sub_centers=self.sub_centers, margin_type=self.margin_type, inter_topk=self.inter_topk,
                    inter_margin=self.inter_margin)
