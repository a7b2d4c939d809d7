"""Golden vectors for the CTC loss: runs the REFERENCE's CtcLoss (authoring container only; needs /root/reference) on the
CPU in float64 and records logits, labels, loss and the autograd gradient for the 2-D and the concatenated 1-D target
layout, and for the speaker training step.  The step is restated here from ref:
src/lightning_modules/speaker/speaker_recognition_module.py:222-244 (``_train_step_ctc_loss``) and the bias
initialisation from ref: src/lightning_modules/speaker/wav2vec2_fc.py:226-233; the loss class is the reference's own.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ctc_goldens.py
"""
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "src", "optim", "loss"))
from ctc_loss import CtcLoss  # noqa: E402  (the module alone: the package's __init__ pulls in the whole training stack)

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64
out, meta = {}, {}


def run(name, logits, in_len, targets, tgt_len):
    x = logits.clone().requires_grad_(True)
    loss = CtcLoss()(x, in_len, targets, tgt_len)
    loss.backward()
    out[name + "_loss"], out[name + "_grad"] = loss.detach().numpy(), x.grad.numpy()


# ---- the generic forward: mixed input and target lengths, a repeated label, an empty target, an infeasible utterance
g = torch.Generator().manual_seed(2207)
B, T, C = 5, 9, 7
logits = torch.randn(B, T, C, generator=g, dtype=F64) * 2.0
targets = torch.tensor([[1, 2, 2, 5], [3, 3, 1, 1], [6, 1, 1, 1], [1, 1, 1, 1], [4, 4, 4, 1]])
tgt_len = torch.tensor([4, 3, 1, 0, 3], dtype=torch.int32)
in_len = torch.tensor([9, 7, 9, 4, 4], dtype=torch.int32)       # the last needs 5 frames for 4, 4, 4 and has 4
out["generic_logits"], out["generic_targets"] = logits.numpy(), targets.numpy()
out["generic_in_len"], out["generic_tgt_len"] = in_len.numpy(), tgt_len.numpy()
run("generic_2d", logits, in_len, targets, tgt_len)
flat = torch.cat([targets[b, :int(tgt_len[b])] for b in range(B)])
out["generic_targets_1d"] = flat.numpy()
run("generic_1d", logits, in_len, flat, tgt_len)

# ---- the speaker step (ref: speaker_recognition_module.py:222-244), on the logits of a Linear with the reference's bias
B, T, H, speakers = 4, 11, 12, 9
num_speakers = speakers + 1                                     # ref: :104-107 ``self.num_speakers += 1``
final_out = torch.nn.Linear(H, num_speakers).double()
torch.manual_seed(5)
torch.nn.init.uniform_(final_out.weight, -H ** -0.5, H ** -0.5)
new_bias = torch.zeros(final_out.bias.shape, dtype=F64)         # ref: wav2vec2_fc.py:226-233
new_bias[0] = 100
final_out.bias = torch.nn.Parameter(new_bias)
embedding = torch.randn(B, T, H, generator=g, dtype=F64)
label = torch.tensor([0, 8, 3, 3])
spk_label = label.clone()
spk_label += 1                                                  # ref: :228 (in place, on the batch's tensor)
logits_prediction = final_out(embedding).detach().requires_grad_(True)
pred_length = (torch.ones((B)) * logits_prediction.shape[1]).to(torch.int32)
gt_length = torch.ones((B)).to(torch.int32)
loss = CtcLoss()(logits_prediction, pred_length, spk_label, gt_length)
loss.backward()
out["step_embedding"], out["step_weight"] = embedding.numpy(), final_out.weight.detach().numpy()
out["step_bias"], out["step_label"] = final_out.bias.detach().numpy(), label.numpy()
out["step_logits"], out["step_loss"] = logits_prediction.detach().numpy(), loss.detach().numpy()
out["step_grad"] = logits_prediction.grad.numpy()
meta = {"blank": 0, "speakers": speakers, "classes": num_speakers, "label_after_step": spk_label.tolist(),
        "generic_infeasible": [4], "torch": torch.__version__}

np.savez_compressed(os.path.join(HERE, "g22_ctc.npz"), **out)
with open(os.path.join(HERE, "g22_ctc.json"), "w") as f:
    json.dump(meta, f, indent=1)
print({k: v.shape for k, v in out.items()}, meta)
