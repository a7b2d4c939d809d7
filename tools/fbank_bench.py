"""Timing of the device log-mel front-end (csrc/fbank.hip: w2v2_fbank_db + w2v2_fbank_normalize) next to the host stage
it replaces (data/fbank.py Fbank + the channel-wise InputNormalizer2D, one utterance at a time):
  (a) one training batch, B = 66, N = 48000 (3 s), and (b) one 145 s evaluation utterance;
  device: HIP-event timings of single calls after a warm-up, median / p10 / p90;
  host: wall-clock time of the same inputs through Fbank() + normalize (thread count stated);
  upload: host-to-device copy of the [B, T, 40] f32 features against the [B, N] f32 waveforms (pinned memory);
  and the algorithmic FMA count and bytes of the device path against the vector and HBM peaks.
    python tools/fbank_bench.py [--reps 50] [--host-reps 5]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from w2v2_speaker_amd import ops
from w2v2_speaker_amd.data.fbank import Fbank
from w2v2_speaker_amd.data.pipeline import InputNormalizer2D

VECTOR_FMA_PEAK = 157.3e12 / 2          # f32 vector FMA / s (157.3 TFLOPS)
HBM_PEAK = 8.0e12                       # bytes / s
dev = "cuda"


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def stats(xs):
    return f"median {statistics.median(xs):9.1f} us  p10 {pct(xs, 0.1):9.1f}  p90 {pct(xs, 0.9):9.1f}"


def gpu_times(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    fb, n_mels = Fbank(), 40
    window, fbank = fb.window.to(dev), fb.fbank.to(dev)
    print(f"device: {torch.cuda.get_device_name(0)}; host threads: {torch.get_num_threads()}; {a.reps} timed calls each")
    for name, B, N in (("training batch", 66, 48000), ("145 s utterance", 1, 145 * 16000)):
        T = 1 + N // ops.FBANK_HOP
        wav = torch.randn(B, N, generator=torch.Generator().manual_seed(1))
        wav = (wav - wav.mean(dim=1, keepdim=True)) / (wav.std(dim=1, keepdim=True) + 1e-5)
        wav_d = wav.to(dev)
        db = torch.empty(B, T, n_mels, device=dev)
        pmax = ops.fbank_partial_max(B, T, dev)
        print(f"--- {name}: B = {B}, N = {N}, T = {T}")
        for dtype in (torch.float32, torch.bfloat16):
            out = torch.empty(B * T, n_mels, dtype=dtype, device=dev)
            t_db = gpu_times(lambda: ops.fbank_db(wav_d, None, window, fbank, db, pmax), a.reps)
            t_nm = gpu_times(lambda: ops.fbank_normalize(db, pmax, None, out, n_mels), a.reps)
            t_all = gpu_times(lambda: (ops.fbank_db(wav_d, None, window, fbank, db, pmax),
                                       ops.fbank_normalize(db, pmax, None, out, n_mels)), a.reps)
            print(f"device {str(dtype)[6:]:9s} fbank_db        {stats(t_db)}")
            print(f"device {str(dtype)[6:]:9s} fbank_normalize {stats(t_nm)}")
            print(f"device {str(dtype)[6:]:9s} both            {stats(t_all)}")
        # what the arithmetic and the traffic of the device path cost at the peaks
        fma = B * T * (400 * 201 * 2 + 201 * n_mels)
        byts = B * N * 4 + 2 * B * T * n_mels * 4 + 3 * B * T * n_mels * 4 + B * T * n_mels * 4
        med = statistics.median(t_all) * 1e-6                # (the bf16 output: the benchmark's ECAPA precision)
        print(f"algorithmic: {fma / 1e9:.2f} G FMA = {fma / VECTOR_FMA_PEAK * 1e6:.1f} us at the f32 vector peak "
              f"({100 * fma / VECTOR_FMA_PEAK / med:.1f} % of it reached); {byts / 1e6:.1f} MB = "
              f"{byts / HBM_PEAK * 1e6:.1f} us at the HBM peak")
        host = []
        for _ in range(a.host_reps + 1):
            t0 = time.perf_counter()
            feats = torch.stack([InputNormalizer2D.normalize(fb(w), True)[0] for w in wav])
            host.append((time.perf_counter() - t0) * 1e6)
        host = host[1:]
        print(f"host ({torch.get_num_threads()} threads) Fbank + normalize  {stats(host)}")
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        host1 = []
        for _ in range(a.host_reps + 1):
            t0 = time.perf_counter()
            torch.stack([InputNormalizer2D.normalize(fb(w), True)[0] for w in wav])
            host1.append((time.perf_counter() - t0) * 1e6)
        torch.set_num_threads(threads)
        print(f"host (1 thread) Fbank + normalize   {stats(host1[1:])}")
        f_pin, w_pin = feats.contiguous().pin_memory(), wav.pin_memory()
        f_dev, w_dev = torch.empty_like(feats, device=dev), torch.empty_like(wav, device=dev)
        t_f = gpu_times(lambda: f_dev.copy_(f_pin, non_blocking=True), a.reps)
        t_w = gpu_times(lambda: w_dev.copy_(w_pin, non_blocking=True), a.reps)
        print(f"upload features {feats.numel() * 4 / 1e6:6.2f} MB  {stats(t_f)}")
        print(f"upload waveform {wav.numel() * 4 / 1e6:6.2f} MB  {stats(t_w)}")
        print(f"per batch: host front-end + feature upload {statistics.median(host) + statistics.median(t_f):.0f} us; "
              f"waveform upload + device front-end {statistics.median(t_w) + statistics.median(t_all):.0f} us")


if __name__ == "__main__":
    main()
