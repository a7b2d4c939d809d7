"""Timing of trial scoring on the device (csrc/score.hip) next to the host evaluator's _compute_prediction_scores on the
same box, at the sizes of real trial lists:
  score_pairs       37,611 trials over 4,708 rows (VoxCeleb1-O) and 579,818 trials over 145,160 rows (VoxCeleb1-E), D = 1536,
                    plain and with centring + length norm;
  embed_stats       145,160 x 1536;
  score_frame_sets  37,611 trials x (50 + 50) frames x 768 over a 4,708 x 149-frame bank.
Device: HIP events around single calls, median / p10 / p90 of --reps runs after a warm-up, with the bytes each call has
to move and the rate that makes.  Host: wall clock of CosineDistanceEvaluator._compute_prediction_scores over the
EmbeddingSample pairs (the objects are built outside the timed region), median of --host-reps runs, in full at the
smaller size; on the first 500 trials for frame sets, reported per trial; left out at the larger size, where the two
stacked [P, D] tensors alone are the figure printed.  No threshold is asserted: these are first measurements.
    python tools/scoring_bench.py [--reps 50] [--host-reps 3]"""
import argparse, os, random, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from w2v2_speaker_amd import ops
from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EmbeddingSample

dev = "cuda"
D = 1536


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def gpu_times(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def line(what, us, nbytes):
    med = statistics.median(us)
    print(f"{what:58s} median {med:9.1f} us  p10 {pct(us, 0.1):9.1f}  p90 {pct(us, 0.9):9.1f}   {nbytes / 1e6:9.1f} MB  "
          f"{nbytes / med / 1e3:7.1f} GB/s")
    return med


def host_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def pairs_bench(N, P, reps, host_reps):
    g = torch.Generator(device=dev).manual_seed(N)
    bank = torch.randn(N, D, device=dev, generator=g) + 0.5
    pairs = torch.randint(0, N, (P, 2), device=dev, generator=g, dtype=torch.int32)
    cos, score = torch.empty(P, device=dev), torch.empty(P, device=dev)
    mean, std = ops.embed_stats(bank)
    nbytes = P * (2 * D * 4 + 8 + 8)
    print(f"--- score_pairs, {P:,} trials over {N:,} rows, D = {D} (bank {N * D * 4 / 1e6:.0f} MB)")
    for tag, kw in (("plain", {}), ("centring + length norm", dict(mean=mean, std=std, length_norm=True))):
        dev_us = line(f"device, {tag}", gpu_times(lambda: ops.score_pairs(bank, pairs, cos_out=cos, score_out=score, **kw),
                                                   reps), nbytes)
        if host_reps and P <= 100000:
            cpu = bank.cpu()
            rows = [EmbeddingSample(str(i), cpu[i]) for i in range(N)]
            pp = [(rows[i], rows[j]) for i, j in pairs.cpu().tolist()]
            ev = CosineDistanceEvaluator(bool(kw), bool(kw), 0)
            if kw:
                ev.mean, ev.std = mean.cpu(), std.cpu()
            ref = np.array(ev._compute_prediction_scores(pp))
            err = float(np.abs(ref - cos.cpu().numpy()).max())
            t = host_time(lambda: ev._compute_prediction_scores(pp), host_reps)
            print(f"{'host _compute_prediction_scores, ' + tag:58s} median {t * 1e6:9.0f} us  ({t * 1e6 / dev_us:.0f} x the "
                  f"device call; max |cos difference| {err:.1e}; bank -> host copy not included)")
    if P > 100000:
        print(f"host run left out: its two stacked [P, D] f32 tensors are 2 x {P:,} x {D} x 4 B = {2 * P * D * 4 / 1e9:.2f} GB")


def stats_bench(N, reps, host_reps):
    g = torch.Generator(device=dev).manual_seed(7)
    bank = torch.randn(N, D, device=dev, generator=g) + 0.5
    mean, std, work = torch.empty(D, device=dev), torch.empty(D, device=dev), ops.embed_stats_workspace(N, D, dev)
    print(f"--- embed_stats, {N:,} x {D}")
    dev_us = line("device (2 launches)", gpu_times(lambda: ops.embed_stats(bank, mean, std, work), reps), N * D * 4)
    if host_reps:
        cpu = bank.cpu()
        t = host_time(lambda: torch.std_mean(cpu, dim=0), host_reps)
        print(f"{'host torch.std_mean on the stacked bank':58s} median {t * 1e6:9.0f} us  ({t * 1e6 / dev_us:.0f} x the device call; "
              f"the stack of N tensors not included)")


def frames_bench(U, T, P, reps, host_reps):
    Df, cap = 768, 50
    g = torch.Generator(device=dev).manual_seed(11)
    frames = torch.randn(U * T, Df, device=dev, generator=g)
    rng = np.random.default_rng(0)
    utt = rng.integers(0, U, (P, 2))
    sel = np.stack([np.stack([u * T + rng.permutation(T)[:cap] for u in row]) for row in utt]).astype(np.int32)
    counts = np.full((P, 2), cap, dtype=np.int32)
    sel_d, counts_d = torch.from_numpy(sel).to(dev), torch.from_numpy(counts).to(dev)
    cos, score = torch.empty(P, device=dev), torch.empty(P, device=dev)
    print(f"--- score_frame_sets, {P:,} trials x ({cap} + {cap}) frames x {Df} over {U:,} utterances of {T} frames "
          f"(frame bank {U * T * Df * 4 / 1e9:.2f} GB)")
    nbytes = P * 2 * cap * Df * 4
    dev_us = line("device (each row read twice; bytes = one read of each)",
                  gpu_times(lambda: ops.score_frame_sets(frames, sel_d, counts_d, cos, score), reps), nbytes)
    if host_reps:
        n = 500
        cpu = [frames[u * T:(u + 1) * T].cpu() for u in range(U)]
        pp = [(EmbeddingSample("l", cpu[a]), EmbeddingSample("r", cpu[b])) for a, b in utt[:n]]
        ev = CosineDistanceEvaluator()
        random.seed(0)
        t = host_time(lambda: ev._compute_prediction_scores(pp), host_reps)
        print(f"{'host non-pooled scoring, first 500 trials':58s} median {t / n * 1e6:9.1f} us per trial  (device: "
              f"{dev_us / P:.3f} us per trial; the whole list at the host's rate: {t / n * P:.1f} s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    print(f"device: {torch.cuda.get_device_name(0)}; host threads: {torch.get_num_threads()}")
    pairs_bench(4708, 37611, a.reps, a.host_reps)
    pairs_bench(145160, 579818, a.reps, a.host_reps)
    stats_bench(145160, a.reps, a.host_reps)
    frames_bench(4708, 149, 37611, a.reps, a.host_reps)


if __name__ == "__main__":
    main()
