"""Timing of the device augmentation stage (csrc/augment.hip, csrc/reverb.hip, data/augment.py) at the size of one
x-vector training step: the reference's xvector_all_augment pipeline (time dropout 0..5 x <= 0.25 s, frequency dropout
0..5 bands, speed 0.95 / 1 / 1.05, reverb 50 50 <room scale 0..100>, uniform noise at 15 / 20 / 100 dB; unaugmented row
kept) over 66 chunks of 3 s, i.e. [66, 48000] -> [396, 50527], and the same stage without the reverb.  With HIP events:
  the whole stage   Augmenter.process_batch: the host's share (draws, filter design, table, enqueue; wall clock; it runs ahead
                    of the device, which is busy with the training step) and the sum of its kernels
  per kernel        every ops.aug_* launch of the stage, summed per kind
  FIR, worst case   all 66 rows under the cap of 2,561 taps, against the f32 vector rate
  reverb            one launch over the 66 rows at room scale 0 (the shortest delays: the longest chain of block steps) and
                    100, next to a device copy of the same rows (the HBM floor) and to block-vectorised float32 numpy on the host.
                    One workgroup per row: 66 rows occupy 66 of the 256 CUs.
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


def augmenters(reverb):
    """The list of xvector_all_augment, in its order; without the reverb it is the stage this file timed before."""
    np.random.seed(7)                                      # (the reverb's three draws, once, at construction)
    rev = [A.ReverbAugment(SR, room_scale_min=0, room_scale_max=100, on_device=True)] if reverb else []
    return [A.TimeDropoutAugment(SR, 0.25, 0, 5), A.FrequencyDropoutAugment(SR, 0, 5, 1),
            A.ChoiceSpeedAugment(SR, [0.95, 1, 1.05])] + rev + [A.ChoiceRandomNoiseAugment(SR, [15, 20, 100])]


class KernelTimes:
    """Wraps the ops.aug_* entries with event pairs, summed per entry over a pass."""
    NAMES = ("aug_resample", "aug_time_dropout", "aug_fir", "aug_reverb", "aug_mix_uniform", "aug_mix_bank")

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


def host_reverb_f32(x, d):
    """w2v2_aug_reverb's definition in float32 numpy over all rows [B, N] at once (one parameter set, as the reference
    draws it once): every filter in blocks of its delay, the comb's one-pole low-pass of a block by scipy's lfilter with
    the carried state."""
    from scipy.signal import lfilter
    f = np.float32
    n_rows, n = x.shape
    wet = []
    for w in range(2):
        acc = np.zeros_like(x)
        for i in range(7, -1, -1):
            D = int(d.comb_delays[w, i])
            line, zi, out = np.zeros((n_rows, D), f), np.zeros((n_rows, 1), f), np.empty_like(x)
            num, den = np.asarray([1 - d.damp], f), np.asarray([1, -d.damp], f)
            for n0 in range(0, n, D):
                m = min(D, n - n0)
                out[:, n0:n0 + m] = line[:, :m]
                st, zi = lfilter(num, den, line[:, :m], axis=1, zi=zi)
                line[:, :m] = x[:, n0:n0 + m] + st.astype(f) * d.feedback
            acc += out
        for j in range(3, -1, -1):
            D = int(d.allpass_delays[w, j])
            line, out = np.zeros((n_rows, D), f), np.empty_like(x)
            for n0 in range(0, n, D):
                m = min(D, n - n0)
                o = line[:, :m].copy()
                line[:, :m] = acc[:, n0:n0 + m] + f(0.5) * o
                out[:, n0:n0 + m] = o - acc[:, n0:n0 + m]
            acc = out
        wet.append(acc * d.wet_gain)
    return f(0.5) * ((d.dry_gain * x + wet[0]) + (d.dry_gain * x + wet[1]))


def host_f32(x, draws, seed):
    """The same definitions in float32 numpy, row by row (the reverb over all rows at once): what a host stage would do
    per step.  -> the augmented rows per input row, in the stage's order."""
    outs = []
    rng = np.random.RandomState(seed)
    with_reverb = len(draws[0]) == 5
    rev = host_reverb_f32(x, draws[0][3]) if with_reverb else None
    for b in range(x.shape[0]):
        d_drop, d_band, d_speed, d_noise = draws[b][0], draws[b][1], draws[b][2], draws[b][-1]
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
        if with_reverb:
            outs.append(rev[b])
        cf = np.float32(d_noise.coef)
        outs.append(cf * x[b] + (np.float32(1) - cf) * rng.random_sample(N).astype(np.float32))
    return outs


def stage(kt, wav, label, reps, reverb):
    """Times Augmenter.process_batch and its kernels -> (kernels ms, host share ms, the last pass's draws, its output)."""
    aug = A.Augmenter(augmenters(reverb), stack_augmentations=False, yield_intermediate_augmentations=True, yield_unaugmented=True)
    Bo, No = aug.output_shape(B, N)
    say(f"--- the stage{'' if reverb else ' without the reverb'}: [{B}, {N}] -> [{Bo}, {No}] ({Bo * No * 4 / 1e6:.0f} MB written), "
        f"{len(aug.augmenters)} augmenters + the unaugmented row")
    whole, wall, per = [], [], {n: [] for n in kt.NAMES}
    counts, draws, out = {}, None, None
    for rep in range(reps + 1):
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
        f"speed ratios {sorted({(d[2].U, d[2].D) for d in draws})}" + (f"; room scale {aug.augmenters[3].room_scale}" if reverb else "") + ")")
    return dev_ms, m([w[0] for w in wall]), draws, out


def reverb_section(wav, reps, g):
    """One w2v2_aug_reverb launch over the 66 rows at the reference's reverberance and damping, room scale 0 and 100, a device
    copy of the same rows, and the host's float32 numpy on the same rows."""
    m = statistics.median
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    dst = torch.empty(B, N, device=dev)
    x = wav.cpu().numpy()

    def timed(fn, inner=20):                               # `inner` launches between one pair of events
        ts = []
        for rep in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ts.append(e0.elapsed_time(e1) / inner)
        return ts

    say(f"--- w2v2_aug_reverb: {B} rows x {N} samples, one workgroup per row ({B} of 256 CUs), chunks of {ops.AUG_REVERB_CHUNK} samples; "
        f"20 launches per event pair")
    ts = timed(lambda: dst.copy_(wav))
    byt = 2.0 * B * N * 4
    say(f"{'device copy of the same rows (the HBM floor)':46s} median {m(ts):9.4f} ms  min {min(ts):9.4f}  max {max(ts):9.4f}   "
        f"{byt / m(ts) / 1e9:6.2f} TB/s")
    for room in (0, 100):
        d = A.reverb_parameters(SR, 50, 50, room)
        table = torch.from_numpy(np.tile(d.row(), (B, 1))).to(dev)
        ts = timed(lambda: ops.aug_reverb(wav, dst, rows, rows, table))
        got = dst.cpu().numpy()
        t0 = time.perf_counter()
        host = host_reverb_f32(x, d)
        t_host = time.perf_counter() - t0
        say(f"{f'ops.aug_reverb, room scale {room}':46s} median {m(ts):9.4f} ms  min {min(ts):9.4f}  max {max(ts):9.4f}   "
            f"comb delays {int(d.comb_delays.min())}..{int(d.comb_delays.max())}; {N * B / m(ts) / 1e6:.1f} G samples/s")
        say(f"{f'  float32 numpy on the host, room scale {room}':46s} {t_host * 1e3:12.1f} ms = {t_host * 1e3 / m(ts):.0f} x the launch; "
            f"max |device - host f32| {float(np.abs(got - host).max()):.2e}")


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
    kt = KernelTimes()
    m = statistics.median
    stage(kt, wav, label, a.reps, reverb=False)
    dev_ms, host_ms, draws, out = stage(kt, wav, label, a.reps, reverb=True)

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

    reverb_section(wav, a.reps, g)

    # ---- the host, one pass on the last draws
    x = wav.cpu().numpy()
    t0 = time.perf_counter()
    outs = host_f32(x, draws, 0)
    t_host = time.perf_counter() - t0
    say(f"--- float32 numpy on the host, the same draws as the stage with the reverb, one pass over {B} chunks ({len(outs)} augmented rows)")
    say(f"{'host stage':46s} {t_host * 1e3:12.1f} ms = {t_host * 1e3 / dev_ms:.0f} x the kernels of the stage, "
        f"{t_host * 1e3 / host_ms:.1f} x the host share of process_batch")
    got = out.network_input.cpu().numpy()
    worst = 0.0
    for b in range(B):                                     # the two agree (dropout, FIR, speed, reverb rows; the noise streams differ)
        for k in range(4):
            h = outs[5 * b + k]
            worst = max(worst, float(np.abs(got[6 * b + 1 + k, :h.size] - h).max()))
    say(f"device vs host f32 on the dropout / FIR / speed / reverb rows: max |difference| {worst:.2e}")
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
