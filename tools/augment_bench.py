"""Timing of the device augmentation stage (csrc/augment.hip, data/augment.py) at the size of one x-vector training
step: the reference's xvector_all_augment pipeline without reverb (time dropout 0..5 x <= 0.25 s, frequency dropout
0..5 bands, speed 0.95 / 1 / 1.05, uniform noise at 15 / 20 / 100 dB; unaugmented row kept) over 66 chunks of 3 s, i.e.
[66, 48000] -> [330, 50527].  With HIP events:
  the whole stage   Augmenter.process_batch: the host's share (draws, filter design, table, enqueue; wall clock; it runs ahead
                    of the device, which is busy with the training step) and the sum of its kernels
  per kernel        every ops.aug_* launch of the stage, summed per kind
  FIR, worst case   all 66 rows under the cap of 2,561 taps, against the f32 vector rate
and next to them a float32 numpy implementation of the same definitions on the host, fed the same draws (one pass).
No time target is asserted; the file records what came out.
    python tools/augment_bench.py [--reps 5] [--out profiles/augment_bench.txt]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from w2v2_speaker_amd import ops
from w2v2_speaker_amd.data import augment as A

dev = "cuda"
B, N, SR = 66, 48000, 16000
F32_VECTOR_TFLOPS = 157.3       # the f32 vector peak of the MI355X (packed fma on every SIMD)
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def augmenters():
    return [A.TimeDropoutAugment(SR, 0.25, 0, 5), A.FrequencyDropoutAugment(SR, 0, 5, 1),
            A.ChoiceSpeedAugment(SR, [0.95, 1, 1.05]), A.ChoiceRandomNoiseAugment(SR, [15, 20, 100])]


class KernelTimes:
    """Wraps the ops.aug_* entries with event pairs, summed per entry over a pass."""
    NAMES = ("aug_resample", "aug_time_dropout", "aug_fir", "aug_mix_uniform", "aug_mix_bank")

    def __init__(self):
        self.orig = {n: getattr(ops, n) for n in self.NAMES}
        self.pairs = {n: [] for n in self.NAMES}
        self.on = False
        for n in self.NAMES:
            setattr(ops, n, self._wrap(n))

    def _wrap(self, n):
        def run(*a, **k):
            if not self.on:
                return self.orig[n](*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.orig[n](*a, **k)
            e1.record()
            self.pairs[n].append((e0, e1))
        return run

    def ms(self):
        torch.cuda.synchronize()
        out = {n: (sum(a.elapsed_time(b) for a, b in p), len(p)) for n, p in self.pairs.items()}
        self.pairs = {n: [] for n in self.NAMES}
        return out


def host_f32(x, draws, seed):
    """The same definitions in float32 numpy, row by row: what a host stage would do per step."""
    outs = []
    rng = np.random.RandomState(seed)
    for b in range(x.shape[0]):
        d_drop, d_band, d_speed, d_noise = draws[b]
        y = x[b].copy()
        for s, l in d_drop.spans:
            y[s:s + l] = 0
        outs.append(y)
        h = d_band.taps.astype(np.float32)
        outs.append(np.convolve(x[b], h)[(h.size - 1) // 2:][:N] if h.size > 1 else x[b] * h[0])
        U, D = d_speed.U, d_speed.D
        if U == D:
            outs.append(x[b].copy())
        else:
            p = A.resample_prototype(U, D).astype(np.float32)
            half = (p.size - 1) // 2
            n_out = A.resampled_length(N, U, D)
            c = np.arange(n_out, dtype=np.int64) * D + half
            y = np.zeros(n_out, np.float32)
            for ph in range(U):                           # polyphase: the outputs of one phase share a tap subset
                m = np.nonzero(c % U == ph)[0]
                full = np.convolve(x[b], p[ph::U])
                q = c[m] // U
                ok = q < full.size
                y[m[ok]] = U * full[q[ok]]
            outs.append(y)
        cf = np.float32(d_noise.coef)
        outs.append(cf * x[b] + (np.float32(1) - cf) * rng.random_sample(N).astype(np.float32))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "augment_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    say(f"tools/augment_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}; HIP events, one warm-up pass, median / min / "
        f"max of {a.reps} passes")
    g = torch.Generator(device=dev).manual_seed(1)
    wav = 0.1 * torch.randn(B, N, device=dev, generator=g)
    label = torch.arange(B, device=dev)
    aug = A.Augmenter(augmenters(), stack_augmentations=False, yield_intermediate_augmentations=True, yield_unaugmented=True)
    Bo, No = aug.output_shape(B, N)
    say(f"--- the stage: [{B}, {N}] -> [{Bo}, {No}] ({Bo * No * 4 / 1e6:.0f} MB written), {len(aug.augmenters)} augmenters + the "
        f"unaugmented row")
    kt = KernelTimes()
    whole, wall, per = [], [], {n: [] for n in kt.NAMES}
    counts, draws, out = {}, None, None
    for rep in range(a.reps + 1):
        np.random.seed(100 + rep)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = aug.process_batch(wav, label)
        e1.record()
        t_host = time.perf_counter() - t0                  # the host returns here: nothing waited for the device
        torch.cuda.synchronize()
        t_all = time.perf_counter() - t0
        kt.on = True                                       # the same draws again, every launch between its own events
        np.random.seed(100 + rep)
        aug.process_batch(wav, label)
        kt.on = False
        ms = kt.ms()
        if rep:
            whole.append(e0.elapsed_time(e1)); wall.append((t_host * 1e3, t_all * 1e3))
            for n in kt.NAMES:
                per[n].append(ms[n][0])
                counts[n] = ms[n][1]
        draws = out.draws
    m = statistics.median
    say(f"{'process_batch, host returns after':46s} median {m([w[0] for w in wall]):9.3f} ms  (draws, filter design in numpy, table, "
        f"enqueue; no wait for the device)")
    say(f"{'process_batch, until the device is done':46s} median {m([w[1] for w in wall]):9.3f} ms")
    say(f"{'process_batch, first event to last (host-bound)':46s} median {m(whole):9.3f} ms  min {min(whole):9.3f}  max {max(whole):9.3f}")
    dev_ms = sum(m(per[n]) for n in kt.NAMES if counts.get(n))
    say(f"{'the kernels of the stage, summed':46s} median {dev_ms:9.3f} ms")
    for n in kt.NAMES:
        if counts.get(n):
            say(f"{'  ops.' + n + f' x {counts[n]}':46s} median {m(per[n]):9.3f} ms  min {min(per[n]):9.3f}  max {max(per[n]):9.3f}")
    taps = [d[1].taps.size for d in draws]
    say(f"  (last pass: composed filters of {min(taps)}..{max(taps)} taps, mean {sum(taps) / len(taps):.0f}; "
        f"speed ratios {sorted({(d[2].U, d[2].D) for d in draws})})")

    # ---- the FIR at the cap
    K = ops.AUG_MAX_TAPS
    taps_d = torch.randn(B, K + 3, device=dev, generator=g) * 0.01
    ntaps, rows = torch.full((B,), K, dtype=torch.int32, device=dev), torch.arange(B, dtype=torch.int32, device=dev)
    dst = torch.empty(B, N, device=dev)
    ts = []
    for rep in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.aug_fir(wav, dst, rows, rows, taps_d, ntaps)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ts.append(e0.elapsed_time(e1))
    flop = 2.0 * B * N * K
    say(f"--- w2v2_aug_fir at the cap: {B} rows x {N} samples x {K} taps = {flop / 1e9:.1f} GFLOP")
    say(f"{'ops.aug_fir':46s} median {m(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}   {flop / m(ts) / 1e9:6.1f} TFLOP/s = "
        f"{100 * flop / m(ts) / 1e9 / F32_VECTOR_TFLOPS:.0f} % of the f32 vector rate ({F32_VECTOR_TFLOPS} TFLOP/s)")

    # ---- the host, one pass on the last draws
    x = wav.cpu().numpy()
    t0 = time.perf_counter()
    outs = host_f32(x, draws, 0)
    t_host = time.perf_counter() - t0
    say(f"--- float32 numpy on the host, the same draws, one pass over {B} chunks ({len(outs)} augmented rows)")
    say(f"{'host stage':46s} {t_host * 1e3:12.1f} ms = {t_host * 1e3 / dev_ms:.0f} x the kernels of the stage, "
        f"{t_host / statistics.median([w[0] for w in wall]) * 1e3:.1f} x the host share of process_batch")
    got = out.network_input.cpu().numpy()
    worst = 0.0
    for b in range(B):                                     # the two agree (dropout, FIR, speed rows; the noise streams differ)
        for k in range(3):
            h = outs[4 * b + k]
            worst = max(worst, float(np.abs(got[5 * b + 1 + k, :h.size] - h).max()))
    say(f"device vs host f32 on the dropout / FIR / speed rows: max |difference| {worst:.2e}")
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
