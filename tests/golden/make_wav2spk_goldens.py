"""Golden vectors for the wav2spk model (authoring container only; needs /root/reference): float64 autograd on the CPU over
the reference's layer list -- restated from ref: src/lightning_modules/speaker/wav2spk.py:116-217, :235-292 with torch's
own nn.Conv1d / nn.InstanceNorm1d / nn.ReLU / nn.Linear / nn.LogSoftmax and the reference's OWN TemporalGate
(src/layers/temporal_gating.py) and MeanStdStatPool1D / MeanStatPool1D (src/layers/pooling.py), loaded by path: the
speakers package __init__ drags in pytorch_lightning internals, fairseq and torchmetrics (the approach of
make_ctc_goldens.py).  Weights are tests/wav2spk_cases.make_state_dict (synth_weight by name), inputs its synth_batch, so
neither is stored.  Recorded per (case, gating, pooling): every stage output and every large gradient as norm + a strided
sample, every small gradient whole, the loss, and the embeddings of embedding_layer_idx -1, 0, 2.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_wav2spk_goldens.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import wav2spk_cases as K  # noqa: E402

sb = "speechbrain.lobes.models.ECAPA_TDNN"           # pooling.py imports AttentiveStatisticsPooling from it (make_goldens.py)
parts = sb.split(".")
for i in range(1, 5):
    sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
sys.modules[sb].AttentiveStatisticsPooling = object


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TemporalGate = load("ref_temporal_gating", "src/layers/temporal_gating.py").TemporalGate
pooling = load("ref_pooling", "src/layers/pooling.py")


class Wav2Spk(nn.Module):
    """ref: wav2spk.py:71-93 (members), :116-217 (layer lists), :235-292 (forward)."""

    def __init__(self, gating, stat_pooling_type, hidden, speakers):
        super().__init__()
        self.gating = gating
        self.stat_pooling = (pooling.MeanStatPool1D if stat_pooling_type == "mean" else pooling.MeanStdStatPool1D)(dim_to_reduce=2)
        enc = lambda ci, co, k, s, p: nn.Sequential(nn.Conv1d(ci, co, (k,), (s,), (p,)), nn.InstanceNorm1d(co), nn.ReLU())
        agg = lambda ci, co, k, s, p: nn.Sequential(nn.Conv1d(ci, co, (k,), (s,), (p,)), nn.ReLU())
        self.encoder = nn.ModuleList([enc(*g) for g in K.ENCODER])
        self.temporal_gate = TemporalGate(512)
        self.aggregator = nn.ModuleList([agg(*g) for g in K.AGGREGATOR])
        dims = [K.pool_dim(stat_pooling_type)] + list(hidden)
        self.fc_list = nn.ModuleList([nn.Sequential(nn.Linear(dims[i], dims[i + 1]), nn.ReLU()) for i in range(len(hidden))])
        self.fc_list.append(nn.Sequential(nn.Linear(dims[-1], speakers), nn.LogSoftmax(dim=1)))

    def forward(self, x):
        """-> (stage outputs by name [B, C, T] / [B, F], embeddings by embedding_layer_idx)."""
        stages, emb = {}, {}
        for i, conv in enumerate(self.encoder):
            stages[f"encoder.{i}"] = x = conv(x)
        if self.gating:
            stages["temporal_gate"] = x = self.temporal_gate(x)
        for i, conv in enumerate(self.aggregator):
            stages[f"aggregator.{i}"] = x = conv(x)
        stages["pooled"] = emb[-1] = x = self.stat_pooling(x)
        for i, fc in enumerate(self.fc_list):
            x = fc(x)
            emb[i] = x
            stages[f"fc.{i}" if i < len(self.fc_list) - 1 else "logprob"] = x
        return stages, emb


out, meta = {}, {"cases": [], "torch": torch.__version__, "seed": K.SEED, "speakers": K.SPEAKERS, "hidden": list(K.HIDDEN),
                 "sample": K.SAMPLE}
for B, N in K.STEP_CASES:
    wav, label = K.synth_batch(B, N)
    for gating in K.GATINGS:
        for pool in K.POOLINGS:
            tag = f"b{B}n{N}_{'gate' if gating else 'nogate'}_{pool.replace('+', '')}"
            net = Wav2Spk(gating, pool, K.HIDDEN, K.SPEAKERS).double()
            sd = K.make_state_dict(pooling=pool)
            assert list(sd) == [n for n, _ in net.named_parameters()], "state-dict names / registration order"
            assert sum(p.numel() for p in net.parameters()) == (K.PARAMETERS if pool == "mean+std" else K.PARAMETERS - 512 * 512)
            net.load_state_dict({n: v.double() for n, v in sd.items()}, strict=True)
            stages, emb = net(wav.double()[:, None, :])
            loss = nn.functional.nll_loss(emb[len(K.HIDDEN)], label)       # CE on log-probabilities = NLL of them
            loss.backward()
            out[f"{tag}.loss"] = loss.detach().numpy()
            for n, t in stages.items():
                t = t.detach()
                t = t.transpose(1, 2).reshape(-1, t.shape[1]) if t.dim() == 3 else t       # channels last [B*T, C]
                out[f"{tag}.stage.{n}.norm"] = t.norm().numpy()
                out[f"{tag}.stage.{n}.sample"] = K.strided(t).numpy()
            for i in K.EMBEDDING_LAYERS:
                out[f"{tag}.emb.{i}"] = K.strided(emb[i].detach(), 1024).numpy()
            for n, p in net.named_parameters():
                g = torch.zeros_like(p) if p.grad is None else p.grad
                if g.numel() <= 512:
                    out[f"{tag}.grad.{n}"] = g.numpy()
                else:
                    out[f"{tag}.grad.{n}.norm"] = g.norm().numpy()
                    out[f"{tag}.grad.{n}.sample"] = K.strided(g).numpy()
            meta["cases"].append({"tag": tag, "batch": B, "samples": N, "gating": gating, "pooling": pool,
                                  "loss": float(loss)})

np.savez_compressed(os.path.join(HERE, "g23_wav2spk.npz"), **out)
with open(os.path.join(HERE, "g23_wav2spk.json"), "w") as f:
    json.dump(meta, f, indent=1)
print(len(out), "arrays", os.path.getsize(os.path.join(HERE, "g23_wav2spk.npz")), "bytes", meta["cases"])
