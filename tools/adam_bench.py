#!/usr/bin/env python3
"""Time the fused optimiser launches over the w2v2-base (99.4 M) and wav2vec2-large (323 M) trainable arenas with an fp16
operand copy, next to a device copy of the same arena (the stream ceiling of the box on the day):
  * fused Adam (w2v2_adam_step), 30 B/parameter of algorithmic HBM traffic;
  * the gradient-norm pair (w2v2_grad_norm, two launches), 4 B/parameter, next to w2v2_grad_scaler_check over the same
    bytes in the same process -- both are read-only passes;
  * Adam with weight decay / clipping (w2v2_optim_step), 30 B/parameter;
  * --algo sgd: the SGD step, 22 B/parameter with momentum, 14 without.
Knobs of the plain Adam kernel: W2V2_ADAM_U, W2V2_ADAM_BLOCKS (csrc/optim.hip).  ADAM_N overrides the arena sizes."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from w2v2_speaker_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--algo", choices=("adam", "sgd"), default="adam")
ap.add_argument("--weight-decay", type=float, default=0.0)
ap.add_argument("--clip", type=float, default=0.0, help="gradient_clip_val (> 0: norm pair + coefficient folded into the step)")
ap.add_argument("--momentum", type=float, default=0.9)
args = ap.parse_args()
dev = "cuda"


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
    print(f"  {name:34s} {med:8.1f} us  [{lo:7.1f} .. {hi:7.1f}]  {nbytes / med / 1e6:5.2f} TB/s")


sizes = ([("custom", int(os.environ["ADAM_N"]))] if os.environ.get("ADAM_N")
         else [("w2v2-base", 99_400_000), ("wav2vec2-large", 323_000_000)])
for label, n in sizes:
    n = n // 64 * 64
    p, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 1e-3
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    pb = torch.empty(n, dtype=torch.float16, device=dev)
    sc = torch.tensor([16384.0, 0, 0, 0, 0, 0, 0, 0], device=dev)
    norm = torch.zeros(2, device=dev)
    partials = torch.zeros(ops.grad_norm_partials(n), dtype=torch.float64, device=dev)
    dst = torch.empty_like(p)
    print(f"{label}: n = {n}  (algo {args.algo}, weight decay {args.weight_decay}, clip {args.clip})")
    row("device copy (8 B/param)", 8.0 * n, timed(lambda: dst.copy_(p)))
    row("adam_step (30 B/param)", 30.0 * n, timed(lambda: ops.adam_step(p, g, m, v, pb, n, 1e-5, 0.9, 0.999, 1e-8, 10, 1.0, sc)))
    row("grad_scaler_check (4 B/param)", 4.0 * n, timed(lambda: ops.grad_scaler_check(g, n, sc)))
    row("grad_norm pair (4 B/param)", 4.0 * n, timed(lambda: ops.grad_norm(g, n, norm, partials, 1.0, sc, args.clip)))
    ns = norm if args.clip > 0 else None
    if args.algo == "adam":
        if args.weight_decay or args.clip > 0:
            row("optim_step adam wd/clip (30 B/param)", 30.0 * n, timed(lambda: ops.optim_step(
                "adam", p, g, m, v, pb, n, 1e-5, 0.9, 0.999, 1e-8, 10, 1.0, sc, weight_decay=args.weight_decay, norm_state=ns)))
    else:
        mom = args.momentum
        bpp = 22.0 if mom else 14.0
        row(f"optim_step sgd ({bpp:.0f} B/param)", bpp * n, timed(lambda: ops.optim_step(
            "sgd", p, g, m if mom else None, None, pb, n, 1e-5, step=10, grad_scale=1.0, scaler=sc,
            weight_decay=args.weight_decay, momentum=mom, nesterov=bool(mom), norm_state=ns)))
    del p, g, m, v, pb, dst
    torch.cuda.empty_cache()
