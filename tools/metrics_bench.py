"""Timing of the trial metrics on the device (csrc/metrics.hip) next to the host metrics of eval_metrics.py on the same
box, at the sizes of real trial lists (37,611 trials = VoxCeleb1-O, 579,818 = VoxCeleb1-E):
  sort_f32_index   the stable argsort alone (order and sorted keys);
  trial_metrics    sort, scans, ROC / EER / minDCF -> eight doubles, plus their copy to the host;
  host             what evaluate_bank does behind the scores today: the copy of P floats, .tolist(), calculate_eer and
                   calculate_mdc (wall clock, median of --host-reps runs);
  evaluate_bank    end to end both ways over a 4,708 x 1536 bank at 37,611 trials (wall clock, synchronised).
Device: HIP events around single calls, median / p10 / p90 of --reps runs after 5 warm-up calls.  Scores are drawn as the
test generator draws them (two overlapping classes at 100,000 levels: ties exist).  No threshold is asserted.
    python tools/metrics_bench.py [--reps 50] [--host-reps 3]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from w2v2_speaker_amd import ops
from w2v2_speaker_amd.eval_metrics import calculate_eer, calculate_mdc
from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EvaluationPair
from scoring_bench import gpu_times, host_time, pct

dev = "cuda"


def line(what, us):
    med = statistics.median(us)
    print(f"{what:58s} median {med:9.1f} us  p10 {pct(us, 0.1):9.1f}  p90 {pct(us, 0.9):9.1f}")
    return med


def draw(P, seed):
    rng = np.random.default_rng(seed)
    gt = (rng.random(P) < 0.1).astype(np.uint8)
    s = np.clip(0.3 * gt + rng.normal(0.4, 0.25, P), 0, 1)
    return gt, (np.round(s * 99999) / 99999).astype(np.float32)


def metrics_bench(P, reps, host_reps):
    gt, s = draw(P, P)
    scores, labels = torch.from_numpy(s).to(dev), torch.from_numpy(gt).to(dev)
    order, skeys = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, device=dev)
    sort_ws, ws = ops.sort_f32_index_workspace(P, dev), ops.trial_metrics_workspace(P, dev)
    out = torch.empty(8, dtype=torch.float64, device=dev)
    print(f"--- {P:,} trials ({int(gt.sum()):,} targets; workspace {ws.numel() / 1e6:.1f} MB)")
    line("device sort_f32_index", gpu_times(lambda: ops.sort_f32_index(scores, order, skeys, sort_ws), reps))
    assert np.array_equal(order.cpu().numpy(), np.argsort(s, kind="stable"))
    dev_us = line("device trial_metrics", gpu_times(lambda: ops.trial_metrics(scores, labels, out=out, workspace=ws), reps))
    t_dev = host_time(lambda: ops.trial_metrics(scores, labels, out=out, workspace=ws).cpu().tolist(), max(host_reps, 5))
    print(f"{'device trial_metrics + copy of 8 doubles (wall clock)':58s} median {t_dev * 1e6:9.1f} us")
    glist = gt.tolist()
    res = {}

    def host():
        lst = scores.cpu().numpy().astype(np.float64).tolist()
        res["copy"] = time.perf_counter()
        res["eer"] = calculate_eer(glist, lst)
        res["t_eer"] = time.perf_counter()
        res["mdc"] = calculate_mdc(glist, lst)
    parts = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        host()
        t1 = time.perf_counter()
        parts.append((t1 - t0, res["copy"] - t0, res["t_eer"] - res["copy"], t1 - res["t_eer"]))
    tot, cp, te, tm = (statistics.median(p[i] for p in parts) for i in range(4))
    print(f"{'host copy + tolist + calculate_eer + calculate_mdc':58s} median {tot * 1e6:9.0f} us  (copy + tolist {cp * 1e6:.0f}, "
          f"eer {te * 1e6:.0f}, mdc {tm * 1e6:.0f}; {tot * 1e6 / dev_us:.0f} x the device call, {tot / t_dev:.0f} x with its copy)")
    got = dict(zip(ops.TRIAL_METRICS_FIELDS, out.cpu().tolist()))
    print(f"device eer {got['eer']:.12f} mdc {got['mdc']:.12f}; host eer {res['eer'][0]:.12f} mdc {res['mdc'][0]:.12f}; "
          f"|eer difference| {abs(got['eer'] - res['eer'][0]):.1e}, {int(got['n_thresholds']):,} thresholds")


def bank_bench(N, P, host_reps):
    D = 1536
    g = torch.Generator(device=dev).manual_seed(N)
    spk = torch.randint(0, 40, (N,), device=dev, generator=g)
    bank = torch.randn(40, D, device=dev, generator=g)[spk] + 2.0 * torch.randn(N, D, device=dev, generator=g)
    idx = torch.randint(0, N, (P, 2), generator=torch.Generator().manual_seed(1)).tolist()
    spk_h = spk.cpu().tolist()
    keys = [f"u{i}" for i in range(N)]
    pairs = [EvaluationPair(spk_h[i] == spk_h[j], keys[i], keys[j]) for i, j in idx]
    ev = CosineDistanceEvaluator()
    print(f"--- evaluate_bank end to end, {P:,} trials over {N:,} x {D} (wall clock; the trial table is built in both)")
    out = {}
    for metrics in ("host", "device"):
        def run():
            out[metrics] = ev.evaluate_bank_metrics(pairs, keys, bank, metrics=metrics)
            torch.cuda.synchronize()
        run()
        t = host_time(run, host_reps)
        print(f"{'evaluate_bank_metrics(metrics=' + repr(metrics) + ')':58s} median {t * 1e6:9.0f} us  (floats to the host: "
              f"{ev.last_bank_scoring.host_copy_floats:,}; eer {out[metrics]['eer']:.6f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    print(f"device: {torch.cuda.get_device_name(0)}; host threads: {torch.get_num_threads()}")
    metrics_bench(37611, a.reps, a.host_reps)
    metrics_bench(579818, a.reps, a.host_reps)
    bank_bench(4708, 37611, a.host_reps)


if __name__ == "__main__":
    main()
