"""Golden vectors for the triplet losses and the triplet batch processor: runs the REFERENCE's TripletLoss,
TripletCrossEntropyLoss and TripletSpeakerBatchProcessor (authoring container only; needs /root/reference) on the CPU in
float64 and records, per seed of the ``random`` module, the triplets it drew (``random.choice`` is wrapped, no reference
code is edited), its losses and its autograd gradients; and the keys of every batch of the batch processor.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_triplet_goldens.py
"""
import json
import os
import random
import sys
import types
import warnings

import numpy as np
import torch

REF = "/root/reference"
sys.path.insert(0, REF)
torch.cuda.Device = torch.device
pl = types.ModuleType("pytorch_lightning")
pl.LightningModule, pl.LightningDataModule, pl.Trainer = torch.nn.Module, object, object
sys.modules["pytorch_lightning"] = pl
for n in ("hurry", "hurry.filesize", "torchaudio", "webdataset", "seaborn", "yaspin", "dotenv", "omegaconf", "hydra",
          "hydra.utils"):
    sys.modules.setdefault(n, types.ModuleType(n))
sys.modules["hurry.filesize"].size = lambda *a, **k: ""
sys.modules["omegaconf"].DictConfig = dict
sys.modules["omegaconf"].OmegaConf = object
sys.modules["omegaconf"].MISSING = None

from src.optim.loss import TripletCrossEntropyLoss, TripletLoss  # noqa: E402
from src.data.modules.speaker.voxceleb import TripletSpeakerBatchProcessor  # noqa: E402
from src.data.modules.speaker.training_batch_speaker import (  # noqa: E402
    SpeakerClassificationDataBatch, SpeakerClassificationDataSample)

HERE = os.path.dirname(os.path.abspath(__file__))
MARGINS = (1.0, 0.3)
COEFS = ((1, 1), (1, 2))
CLASSES = 5
# seed of ``random`` -> (labels, embedding width, embedding scale)
CASES = {3: ([0, 0, 1, 1, 2, 2, 0, 1], 16, 0.25),
         11: ([4, 1, 3, 0, 1, 4, 0, 3, 3, 0, 4, 1], 40, 0.125),
         29: ([2, 0, 0, 2, 2, 0], 7, 0.5)}

drawn = []
_choice = random.choice


def recording_choice(seq):
    v = _choice(seq)
    drawn.append(int(v))
    return v


random.choice = recording_choice


def run(seed, fn):
    """fn() under random.seed(seed) -> (its result, the pos / neg rows drawn: pos[0], neg[0], pos[1], ...)"""
    del drawn[:]
    random.seed(seed)
    out = fn()
    return out, drawn[0::2], drawn[1::2]


arrays, meta = {}, {"margins": list(MARGINS), "coefs": [list(c) for c in COEFS], "classes": CLASSES, "seeds": []}
for seed, (labels, E, scale) in CASES.items():
    B = len(labels)
    g = torch.Generator().manual_seed(1000 + seed)
    emb = (torch.randn(B, E, generator=g) * scale).double()          # f32-representable values, float64 arithmetic
    logits = torch.randn(B, CLASSES, generator=g).double()
    label = torch.tensor(labels, dtype=torch.int64)
    pre = f"s{seed}_"
    arrays[pre + "label"], arrays[pre + "emb"], arrays[pre + "logits"] = label.numpy(), emb.numpy(), logits.numpy()
    triplets = None
    for m in MARGINS:
        x = emb.clone().requires_grad_(True)
        loss, pos, neg = run(seed, lambda: TripletLoss(margin=m)(x, label))
        loss.backward()
        assert triplets in (None, (pos, neg))
        triplets = (list(pos), list(neg))
        d_ap = (emb - emb[pos] + 1e-6).norm(dim=1)
        d_an = (emb - emb[neg] + 1e-6).norm(dim=1)
        assert float((m + d_ap - d_an).abs().min()) > 1e-3, (seed, m)     # no hinge an f32 evaluation could flip
        arrays[pre + f"loss_m{m}"], arrays[pre + f"demb_m{m}"] = loss.detach().numpy(), x.grad.numpy()
        print(seed, m, float(loss), "active rows", int((m + d_ap - d_an > 0).sum()), "of", B)
    for c_ce, c_t in COEFS:
        x, z = emb.clone().requires_grad_(True), logits.clone().requires_grad_(True)
        (loss, pred), pos, neg = run(seed, lambda: TripletCrossEntropyLoss(c_ce, c_t)(x, z, label))
        loss.backward()
        assert triplets == (list(pos), list(neg))
        arrays[pre + f"loss_ce{c_ce}{c_t}"], arrays[pre + f"demb_ce{c_ce}{c_t}"] = loss.detach().numpy(), x.grad.numpy()
        arrays[pre + f"dlogits_ce{c_ce}{c_t}"], arrays[pre + f"pred_ce{c_ce}{c_t}"] = z.grad.numpy(), pred.detach().numpy()
    arrays[pre + "pos"], arrays[pre + "neg"] = np.array(triplets[0], np.int64), np.array(triplets[1], np.int64)
    meta["seeds"].append(seed)
random.choice = _choice


sys.path.insert(0, os.path.dirname(HERE))
from triplet_cases import sample_stream  # noqa: E402  (the stream of make_data_goldens.py, one copy for maker and test)


def stream(*a):
    return sample_stream(SpeakerClassificationDataSample, *a)


meta["batch_processor"] = []
for case in [dict(max_batch_size=8, max_queue_size=32, n_speakers=12, per_speaker=6, seq=2, seed=11, ensure=False),
             dict(max_batch_size=12, max_queue_size=24, n_speakers=20, per_speaker=4, seq=4, seed=5, ensure=False),
             dict(max_batch_size=6, max_queue_size=64, n_speakers=14, per_speaker=3, seq=3, seed=3, ensure=True)]:
    def batches(ensure):
        random.seed(case["seed"])
        bp = TripletSpeakerBatchProcessor(case["max_batch_size"], case["max_queue_size"],
                                          SpeakerClassificationDataBatch.default_collate_fn, ensure)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)        # random.sample over a set (Python 3.10)
            return [list(b.keys) for b in bp(stream(case["n_speakers"], case["per_speaker"], case["seq"], case["seed"]))]
    got = batches(case["ensure"])
    if case["ensure"]:                 # this case ends through the ensure_all_samples_seen drain
        assert len(got) > len(batches(False)) and sum(map(len, got)) == case["n_speakers"] * case["per_speaker"]
    meta["batch_processor"].append({**case, "batches": got})
    print("batch processor", case["seed"], [len(b) for b in got])

np.savez(os.path.join(HERE, "g21_triplet.npz"), **arrays)
with open(os.path.join(HERE, "g21_triplet.json"), "w") as f:
    json.dump(meta, f, indent=0)
print("wrote g21_triplet.npz / .json")
