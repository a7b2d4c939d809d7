#!/usr/bin/env python3
"""What gradient accumulation costs.
  * default: w2v2_grad_accumulate in both modes (first: acc = g, 8 B/parameter; add: acc += g, 12 B/parameter) over the
    w2v2-base (99.4 M) and wav2vec2-large (323.5 M) arenas, each next to a device copy of the same number of bytes moved
    (the stream ceiling of the box on the day; ACCUM_N overrides the sizes);
  * --instep: the flagship workload of bench.py (w2v2-base, fp16, B = 66, 3 s, regularisation on) stepped at
    accumulate_grad_batches N in {1, 2, 4} over ONE store, the windows interleaved in one process on one box:
    ms per micro-batch and per utterance.
    python tools/accum_bench.py [--instep [--rounds 4] [--steps 16]]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from w2v2_speaker_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--instep", action="store_true")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=16, help="micro-batches per timed window (a multiple of 4)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def timed(fn, reps=10, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(rounds):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0 / reps)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]           # median, min, max in us


def row(name, nbytes, t):
    med, lo, hi = t
    print(f"  {name:40s} {med:8.1f} us  [{lo:7.1f} .. {hi:7.1f}]  {nbytes / med / 1e6:5.2f} TB/s")
    return med


def kernel_bench():
    sizes = ([("custom", int(os.environ["ACCUM_N"]))] if os.environ.get("ACCUM_N")
             else [("w2v2-base", 99_400_000), ("wav2vec2-large", 323_500_000)])
    for label, n in sizes:
        n = n // 64 * 64
        acc, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 1e-3
        # a copy of k floats moves 8 k bytes: k = n for the 8 B/parameter mode, 1.5 n for the 12 B/parameter mode
        src, dst = torch.randn(n + n // 2, device=dev), torch.empty(n + n // 2, device=dev)
        print(f"{label}: n = {n}")
        c8 = row("device copy of n floats (8 B/param)", 8.0 * n, timed(lambda: dst[:n].copy_(src[:n])))
        f = row("grad_accumulate first (8 B/param)", 8.0 * n, timed(lambda: ops.grad_accumulate(acc, g, n, True)))
        c12 = row("device copy of 1.5 n floats (12 B/param)", 12.0 * n, timed(lambda: dst.copy_(src)))
        a = row("grad_accumulate add (12 B/param)", 12.0 * n, timed(lambda: ops.grad_accumulate(acc, g, n, False)))
        print(f"  first = {c8 / f:.2f} of its copy, add = {c12 / a:.2f} of its copy")
        del acc, g, src, dst
        torch.cuda.empty_cache()


def instep_bench():
    from bench import synth_batch
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    B = 66
    store = ParamStore(W2V2Config.from_huggingface_id("facebook/wav2vec2-base"), dev, torch.float16, head="aam",
                       num_speakers=5994)
    store.init_weights(seed=20211)
    plan = Plan(store, B, 48000, train=True, reg=Wav2Vec2RegularisationConfig(), seed=7)
    trs = {N: SpeakerTrainer(store, plan, Constant(1e-6, 0.9), accumulate_grad_batches=N) for N in (1, 2, 4)}
    wav, label = synth_batch(B, 48000, 5994, seed=42133724, device=dev)

    def window(tr):
        for _ in range(4):
            tr.train_step(wav, label)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            tr.train_step(wav, label)
        e1.record()
        torch.cuda.synchronize()
        assert store.accum_count == 0
        return e0.elapsed_time(e1) / args.steps

    for _ in range(4):
        trs[1].train_step(wav, label)
    res = {N: [] for N in trs}
    for _ in range(args.rounds):
        for N, tr in trs.items():
            res[N].append(window(tr))
    base = float(np.median(res[1]))
    for N, ts in res.items():
        med = float(np.median(ts))
        print(f"N = {N}: median {med:7.3f} ms/micro-batch  {1e3 * med / B:7.1f} us/utterance  ({100 * (med / base - 1):+5.2f} %)  "
              f"windows {['%.3f' % t for t in ts]}")
    print(f"loss scale {float(store.scaler[0]):g}  skipped steps {int(store.scaler[3])}")


if args.instep:
    assert args.steps % 4 == 0
    instep_bench()
else:
    kernel_bench()
