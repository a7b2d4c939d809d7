"""Timing of the triplet head (csrc/heads.hip: w2v2_triplet_fwd_bwd + the mean) at the real head's size, B = 66 rows of
E = 1536, forward + backward, next to the same arithmetic done the reference's way on the same device
(index_select x 3 + F.triplet_margin_loss + autograd; without the reference's host copy of the labels and its B
Python-level draws), and of a full "triplet_ce" training step next to a "ce" step of the same build (wav2vec2-base,
B = 66, 3 s, fp16, default regularisation), the two alternating in one process.
  head: HIP-event timings of blocks of 20 back-to-back calls after a warm-up, per call: median / p10 / p90;
  step: host clock around blocks of steps that end in a device synchronise, per step.
    python tools/triplet_bench.py [--reps 50] [--steps 10] [--rounds 4]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch
import torch.nn.functional as F
from w2v2_speaker_amd import ops

dev = "cuda"
INNER = 20


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def stats(xs):
    return f"median {statistics.median(xs):8.1f} us  p10 {pct(xs, 0.1):8.1f}  p90 {pct(xs, 0.9):8.1f}"


def gpu_times(fn, reps, warmup=3):
    for _ in range(warmup * INNER):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / INNER)
    return out


def head_timings(reps):
    import triplet_cases as TC
    B, E = 66, 1536
    emb, pos, neg = TC.shape_case(B, E)
    x = emb.to(dev)
    idx = torch.tensor([pos, neg], dtype=torch.int64, device=dev)
    d_ap, d_an, rows = (torch.empty(B, device=dev) for _ in range(3))
    demb, loss = torch.empty(B, E, device=dev), torch.empty((), device=dev)

    def ours():
        ops.triplet_fwd_bwd(x, idx[0], idx[1], d_ap, d_an, rows, demb, B, E, 1.0)
        ops.mean(rows, loss)

    xr = x.clone().requires_grad_(True)

    def torch_way():
        xr.grad = None
        l = F.triplet_margin_loss(xr, xr.index_select(0, idx[0]), xr.index_select(0, idx[1]), margin=1.0)
        l.backward()
        return l

    ours()
    l = torch_way()
    torch.cuda.synchronize()
    err = float((demb - xr.grad).norm() / xr.grad.norm())
    print(f"--- head, B = {B}, E = {E} ({B * E * 4 / 1e3:.0f} KB of input), forward + backward, {reps} x {INNER} calls")
    print(f"same result: loss {float(loss):.6f} vs {float(l):.6f}, gradient rel-L2 difference {err:.1e}")
    print(f"triplet_fwd_bwd + mean (3 launches)                {stats(gpu_times(ours, reps))}")
    print(f"index_select x 3 + triplet_margin_loss + autograd  {stats(gpu_times(torch_way, reps))}")


def step_timings(steps, rounds):
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import OneCycle
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    cfg = W2V2Config.from_huggingface_id("facebook/wav2vec2-base")
    B, N, C = 66, 48000, 5994
    g = torch.Generator().manual_seed(1)
    wav = torch.randn(B, N, generator=g)
    wav = ((wav - wav.mean(dim=1, keepdim=True)) / (wav.std(dim=1, keepdim=True) + 1e-5)).to(dev)
    labels = [i // 3 for i in range(B)]                      # 22 speakers of three utterances
    label = torch.tensor(labels, dtype=torch.int64, device=dev)
    from w2v2_speaker_amd.heads import sample_triplets
    import random
    triplets = sample_triplets(labels, rng=random.Random(0))
    trainers = {}
    for head in ("ce", "triplet_ce"):
        st = ParamStore(cfg, dev, torch.float16, head=head, num_speakers=C)
        st.init_weights(seed=20211)
        plan = Plan(st, B, N, train=True, reg=Wav2Vec2RegularisationConfig())
        tr = SpeakerTrainer(st, plan, OneCycle(max_lr=5e-5, total_steps=10 + 2 * (rounds + 1) * steps))
        kw = {"triplets": triplets} if head == "triplet_ce" else {}
        trainers[head] = (lambda tr=tr, kw=kw: tr.train_step(wav, label, **kw))
    times = {h: [] for h in trainers}
    for r in range(rounds + 1):                              # round 0 is the warm-up
        for head, step in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            if r:
                times[head].append((time.perf_counter() - t0) / steps * 1e3)
    print(f"--- training step, wav2vec2-base, B = {B}, 3 s, fp16, {C} speakers: {rounds} alternating blocks of {steps} steps")
    for head, ts in times.items():
        print(f"{head:10s} step  median {statistics.median(ts):7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}   "
              f"({B / statistics.median(ts) * 1e3:.0f} utterances/s)")
    d = statistics.median(times["triplet_ce"]) - statistics.median(times["ce"])
    spread = max(max(ts) - min(ts) for ts in times.values())
    print(f"triplet_ce - ce: {d * 1e3:+.0f} us per step; block-to-block spread of one head: {spread * 1e3:.0f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    print(f"device: {torch.cuda.get_device_name(0)}")
    head_timings(a.reps)
    step_timings(a.steps, a.rounds)


if __name__ == "__main__":
    main()
