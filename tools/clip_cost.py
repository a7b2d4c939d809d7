#!/usr/bin/env python3
"""What gradient-norm clipping (and the other optimiser options) cost inside a real training step: the flagship
workload of bench.py (w2v2-base, fp16, B = 66, 3 s, regularisation on), stepped by ONE trainer whose optimiser options
are switched between timed windows, alternating (off, on, off, on, ...) in one process on one box.
    python tools/clip_cost.py [--rounds 4] [--steps 20]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synth_batch
from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
from w2v2_speaker_amd.engine import Plan
from w2v2_speaker_amd.optim import OptimConfig
from w2v2_speaker_amd.optim.schedule import Constant
from w2v2_speaker_amd.params import ParamStore
from w2v2_speaker_amd.trainer import SpeakerTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--clip", type=float, default=1.0)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
store = ParamStore(W2V2Config.from_huggingface_id("facebook/wav2vec2-base"), dev, torch.float16, head="aam",
                   num_speakers=5994)
store.init_weights(seed=20211)
plan = Plan(store, 66, 48000, train=True, reg=Wav2Vec2RegularisationConfig(), seed=7)
tr = SpeakerTrainer(store, plan, Constant(1e-6, 0.9))        # (a tiny lr: the windows compare like with like)
wav, label = synth_batch(66, 48000, 5994, seed=42133724, device=dev)
modes = [("adam (default step)", OptimConfig(), 0.0), (f"adam + clip {args.clip:g}", OptimConfig(), args.clip),
         ("adam + weight decay 1e-2 + clip", OptimConfig(weight_decay=1e-2), args.clip)]


def window(cfg, clip):
    tr.optimizer, tr.gradient_clip_val = cfg, clip
    for _ in range(3):
        tr.train_step(wav, label)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        tr.train_step(wav, label)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


for _ in range(5):
    tr.train_step(wav, label)
res = {m[0]: [] for m in modes}
for _ in range(args.rounds):
    for name, cfg, clip in modes:
        res[name].append(window(cfg, clip))
base = float(np.median(res[modes[0][0]]))
for name, ts in res.items():
    print(f"{name:34s} median {np.median(ts):7.3f} ms/step  ({100 * (np.median(ts) / base - 1):+5.2f} %)  windows {['%.3f' % t for t in ts]}")
print(f"last norm {float(store.grad_norm[0]):.4f}  coefficient {float(store.grad_norm[1]):.4f}  loss scale {float(store.scaler[0]):g}")
