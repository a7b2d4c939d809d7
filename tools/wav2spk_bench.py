"""wav2spk training step at batch 32 x 3 s of 16 kHz audio x 5994 speakers, f32 (config/network/wav2spk.yaml: temporal
gating, mean+std pooling, hidden layers 512 and 128): the HIP path beside the same step in torch eager on the same device, in
one process.

    python tools/wav2spk_bench.py [--batch 32 --samples 48000 --steps 50 --warmup 10 --out profiles/wav2spk_bench.txt]

Each step is timed with a pair of HIP events on the launch stream (forward, loss, backward, Adam); the two paths are timed
in alternating blocks of steps so that what else runs on the host meets both.  Reported per path: median / p10 / p90 of the
step time and utterances per second at the median; then the ratio.  No gate: the file says which path was faster.

Then the HIP step once more in four parts (forward to the pooled vector, fc head + loss with its backward, backward, zeroing +
optimiser), each between its own pair of events: which launches dominate.

The eager twin is the model from torch's own modules -- nn.Conv1d, InstanceNorm1d, ReLU, the gate as sigmoid(W x + b) * x,
torch.std_mean, Linear, F.cross_entropy of the log-softmax output -- under torch.optim.Adam, f32, no autocast."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F


class EagerWav2Spk(torch.nn.Module):
    def __init__(self, cfg, speakers):
        super().__init__()
        from w2v2_speaker_amd.wav2spk import AGGREGATOR, ENCODER, FEATURES
        nn = torch.nn
        self.encoder = nn.Sequential(*[nn.Sequential(nn.Conv1d(ci, co, k, s, p), nn.InstanceNorm1d(co), nn.ReLU())
                                       for ci, co, k, s, p in ENCODER])
        self.W = nn.Parameter(nn.init.xavier_normal_(torch.ones(FEATURES, FEATURES)))
        self.b = nn.Parameter(nn.init.xavier_normal_(torch.ones(FEATURES, 1)))
        self.aggregator = nn.Sequential(*[nn.Sequential(nn.Conv1d(ci, co, k, s, p), nn.ReLU()) for ci, co, k, s, p in AGGREGATOR])
        dims = [cfg.pool_dim] + list(cfg.hidden_fc_layers_out)
        self.fc = nn.Sequential(*[nn.Sequential(nn.Linear(dims[i], dims[i + 1]), nn.ReLU()) for i in range(len(dims) - 1)],
                                nn.Linear(dims[-1], speakers))
        self.gating = cfg.apply_temporal_gating

    def forward(self, wav, label):
        x = self.encoder(wav[:, None, :])
        if self.gating:
            x = torch.sigmoid(self.W.matmul(x) + self.b) * x
        x = self.aggregator(x)
        return F.cross_entropy(torch.log_softmax(self.fc(torch.cat(torch.std_mean(x, dim=2), 1)), 1), label)


def _stats(ms):
    t = torch.tensor(sorted(ms), dtype=torch.float64)
    q = lambda p: float(t[min(len(ms) - 1, int(round(p * (len(ms) - 1))))])
    return q(0.5), q(0.1), q(0.9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=10, help="steps of one path before the other takes its turn")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wav2spk_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wav2spk_bench: needs the GPU (a step time is not measured anywhere else)")
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.wav2spk import Wav2SpkConfig, Wav2SpkPlan, Wav2SpkStore, Wav2SpkTrainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg, speakers = Wav2SpkConfig(), 5994
    st = Wav2SpkStore(cfg, dev, num_speakers=speakers)
    st.init_weights(1)
    plan = Wav2SpkPlan(st, a.batch, a.samples, train=True)
    tr = Wav2SpkTrainer(st, plan, Constant(1e-3, 0.9))
    eager = EagerWav2Spk(cfg, speakers).to(dev).train()
    opt = torch.optim.Adam(eager.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(0)
    NB = 8                                       # distinct minibatches, round-robin: one fixed batch is memorised
    feats = torch.randn(NB, a.batch, a.samples, generator=g).to(dev)
    labels = torch.randint(0, speakers, (NB, a.batch), generator=g).to(dev)
    last = {}

    def hip_step(i):
        last["hip"] = tr.train_step(feats[i % NB], labels[i % NB])[0]

    def eager_step(i):
        opt.zero_grad(set_to_none=True)
        loss = eager(feats[i % NB], labels[i % NB])
        loss.backward()
        opt.step()
        last["eager"] = loss.detach()

    paths = {"hip": hip_step, "eager": eager_step}
    for fn in paths.values():
        for i in range(a.warmup):
            fn(i)
    torch.cuda.synchronize()
    events = {n: [] for n in paths}
    done = 0
    while done < a.steps:
        n = min(a.block, a.steps - done)
        for name, fn in paths.items():
            for i in range(done, done + n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(i)
                e1.record()
                events[name].append((e0, e1))
            torch.cuda.synchronize()
        done += n
    ms = {n: [e0.elapsed_time(e1) for e0, e1 in ev] for n, ev in events.items()}
    med = {n: _stats(v) for n, v in ms.items()}
    ratio = med["eager"][0] / med["hip"][0]
    # the HIP step in four parts, each between its own events (the sum is a little more than a step: three more event pairs)
    parts = {"forward (encoder, gate, aggregator, pooling)": lambda i: plan.forward(feats[i % NB]),
             "fc head + cross-entropy + its backward": lambda i: plan.head_forward_backward(labels[i % NB]),
             "backward (pooling .. encoder layer 0)": lambda i: plan.backward(),
             "zeroing + Adam": lambda i: (tr._optimizer_step(), st.zero_grad())}
    part_ev = {n: [] for n in parts}
    st.zero_grad()
    for i in range(min(a.steps, 20)):
        for name, fn in parts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(i)
            e1.record()
            part_ev[name].append((e0, e1))
    torch.cuda.synchronize()
    lines = [f"wav2spk training step, {torch.cuda.get_device_name(dev)}, f32, batch {a.batch} x {a.samples} samples, gating, "
             f"mean+std, {speakers} speakers, forward + cross-entropy + backward + Adam",
             f"HIP events around each step, {a.steps} steps per path after {a.warmup} warm-up steps, the two paths in "
             f"alternating blocks of {a.block} steps, {NB} synthetic minibatches round-robin"]
    for n, label in (("hip", "HIP path (Wav2SpkTrainer)   "), ("eager", "torch eager (same device)   ")):
        m, lo, hi = med[n]
        lines.append(f"{label}: median {m:8.3f} ms  p10 {lo:8.3f}  p90 {hi:8.3f}   {a.batch / m * 1e3:9.1f} utt/s at the median"
                     f"   last loss {float(last[n]):.4f}")
    lines.append(f"ratio eager / HIP at the median: {ratio:.2f}x -- " +
                 ("the HIP step is the faster one" if ratio > 1 else "the HIP step is NOT the faster one"))
    for name, ev in part_ev.items():
        m, lo, hi = _stats([e0.elapsed_time(e1) for e0, e1 in ev])
        lines.append(f"  HIP step part: {name:48s} median {m:8.3f} ms  p10 {lo:8.3f}  p90 {hi:8.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
