"""Timing of the score calibration on the device (csrc/calibration.hip) next to the same Newton iteration written in torch
float64 on the same device (one host synchronisation per round, to read the decrement) and next to the float64 numpy path
on the host, at the sizes of real trial lists (579,818 trials = VoxCeleb1-E, K = 1 and K = 4) and at 10,000 trials, where
the launches dominate:
  fit, max_iter = 32      the whole fit as it is enqueued: two moment passes, then 32 rounds of two launches each;
  fit, max_iter = rounds  the same fit cut at the round in which it converged: what the rounds behind the convergence cost
                          is the difference, per round (an idle round is two launches that return at once);
  active round            the slope of the fit's time over max_iter = 1 .. rounds (statistics launch + fold / solve launch);
  apply, llr_metrics      one call each.
Device: HIP events around single calls, median / p10 / p90 of --reps runs after 5 warm-up calls.  The statistics kernel's
bandwidth is stated against K * P * 4 + P bytes per round over the active round's time (an upper bound on the kernel's own
time: it includes the fold / solve launch and the boundary between the two); ``--only-fit`` runs the fits alone, for a
kernel trace in a run of its own.  No threshold is asserted.
    python tools/calibration_bench.py [--reps 50] [--host-reps 3] [--only-fit]"""
import argparse, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from w2v2_speaker_amd import ops
from w2v2_speaker_amd.evaluation.speaker.calibration import effective_prior, fit_numpy
from scoring_bench import gpu_times, host_time, pct

dev = "cuda"


def line(what, us, extra=""):
    med = statistics.median(us)
    print(f"{what:58s} median {med:9.1f} us  p10 {pct(us, 0.1):9.1f}  p90 {pct(us, 0.9):9.1f}{extra}")
    return med


def draw(P, K, seed):
    rng = np.random.default_rng(seed)
    y = (rng.random(P) < 0.1).astype(np.uint8)
    S = rng.standard_normal((K, P)) + 1.5 * y * (0.5 + 0.5 * rng.random((K, 1)))
    return S.astype(np.float32), y


def torch_newton(S, y, pi, max_iter=32):
    """The definition in torch float64 on the device, as one would write it without the kernels: every round ends in a
    host read of the decrement (and of J, for the step halving)."""
    S = S.double()
    P = S.shape[1]
    m = S.mean(dim=1, keepdim=True)
    X = torch.cat([torch.ones(P, 1, dtype=torch.float64, device=S.device), ((S - m) / S.std(dim=1, keepdim=True)).T], dim=1)
    t = y.bool()
    c = torch.where(t, pi / t.sum(), (1 - pi) / (~t).sum())
    tau = math.log(pi / (1 - pi))
    sign = torch.where(t, -1.0, 1.0).double()

    def stats(w):
        z = X @ w + tau
        J = (c * torch.nn.functional.softplus(sign * z)).sum()
        p = torch.sigmoid(z)
        return J, X.T @ (c * (p - t.double())), (X * (c * p * (1 - p))[:, None]).T @ X
    w = torch.zeros(X.shape[1], dtype=torch.float64, device=S.device)
    J, g, H = stats(w)
    for rounds in range(1, max_iter + 1):
        d = torch.cholesky_solve(g[:, None], torch.linalg.cholesky(H))[:, 0]
        if float(g @ d) / 2 < 1e-12:                        # the synchronisation of the round
            return w, rounds
        step = 1.0
        while True:
            Jn, gn, Hn = stats(w - step * d)
            if float(Jn) <= float(J) or step < 2.0 ** -20:
                break
            step *= 0.5
        w, J, g, H = w - step * d, Jn, gn, Hn
    return w, max_iter


def bench(P, K, reps, host_reps, only_fit):
    S, y = draw(P, K, P + K)
    scores, labels = torch.from_numpy(S).to(dev), torch.from_numpy(y).to(dev)
    rec = torch.empty(ops.CALIB_RECORD_DOUBLES, dtype=torch.float64, device=dev)
    ws = ops.calib_workspace(P, dev)
    f = ops.calib_record_fields(ops.calib_fit(scores, labels, record=rec, workspace=ws))
    rounds = f["rounds"]
    nbytes = K * P * 4 + P
    print(f"--- {P:,} trials, K = {K} ({int(y.sum()):,} targets): status {f['status']} after {rounds} rounds, workspace "
          f"{ws.numel() / 1e3:.1f} kB, {nbytes / 1e6:.2f} MB per statistics pass")
    t32 = line("device fit, max_iter = 32 (68 launches)", gpu_times(lambda: ops.calib_fit(scores, labels, record=rec, workspace=ws), reps))
    if only_fit:
        return
    meds = []
    for r in range(1, rounds + 1):
        meds.append(statistics.median(gpu_times(lambda: ops.calib_fit(scores, labels, max_iter=r, record=rec, workspace=ws), reps)))
    tr = meds[-1]
    print(f"{'device fit, max_iter = rounds (' + str(4 + 2 * rounds) + ' launches)':58s} median {tr:9.1f} us")
    slope = float(np.polyfit(np.arange(1, rounds + 1), np.array(meds), 1)[0]) if rounds > 1 else meds[0]
    print(f"{'active round (slope over max_iter = 1 .. rounds)':58s}        {slope:9.1f} us   statistics pass >= "
          f"{nbytes / slope / 1e3:7.1f} GB/s; moment passes + first round {meds[0]:.1f} us")
    print(f"{'idle round behind the convergence':58s}        {(t32 - tr) / (32 - rounds):9.1f} us   ({32 - rounds} of them: "
          f"{t32 - tr:.1f} us = {100 * (t32 - tr) / t32:.0f} % of the fit)")
    out = torch.empty(P, device=dev)
    line("device apply", gpu_times(lambda: ops.calib_apply(scores, rec, out), reps),
         f"   {(nbytes - P + 4 * P) / 1e6:6.2f} MB")
    m8 = torch.empty(8, dtype=torch.float64, device=dev)
    line("device llr_metrics", gpu_times(lambda: ops.llr_metrics(out, labels, out=m8, workspace=ws), reps))
    t_dev = host_time(lambda: ops.calib_record_fields(ops.calib_fit(scores, labels, record=rec, workspace=ws)), max(host_reps, 5))
    print(f"{'device fit + copy of the record (wall clock)':58s} median {t_dev * 1e6:9.1f} us")
    pi = effective_prior(1, 1, 0.05)
    w_t, r_t = torch_newton(scores, labels, pi)
    torch.cuda.synchronize()

    def run_torch():
        torch_newton(scores, labels, pi)
        torch.cuda.synchronize()
    t_torch = host_time(run_torch, max(host_reps, 5))
    print(f"{'torch float64 Newton on the device (wall clock)':58s} median {t_torch * 1e6:9.1f} us  ({r_t} rounds, one "
          f"synchronisation each; {t_torch / t_dev:.1f} x the device fit with its copy)")
    t_np = host_time(lambda: fit_numpy(S, y), host_reps)
    print(f"{'float64 numpy on the host (wall clock, scores there)':58s} median {t_np * 1e6:9.1f} us  ({t_np / t_dev:.1f} x)")
    fn = fit_numpy(S, y)
    print(f"weights: device {np.array2string(np.array(f['a']), precision=6)}, numpy {np.array2string(np.array(fn['a']), precision=6)}, "
          f"torch slope ratio {float(w_t[1]) / f['w'][1]:.9f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only-fit", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    print(f"device: {torch.cuda.get_device_name(0)}; host threads: {torch.get_num_threads()}")
    for P, K in ((579818, 1), (579818, 4), (10000, 1), (10000, 4)):
        bench(P, K, a.reps, a.host_reps, a.only_fit)


if __name__ == "__main__":
    main()
