"""x-vector training step at the reference's shape (config/experiment/speaker_xvector.yaml: batch 32, 300 frames x 40 mel
channels, 5994 speakers, f32): the HIP path beside the same step in torch eager on the same device, in one process.

    python tools/xvector_bench.py [--batch 32 --frames 300 --steps 50 --warmup 10 --out profiles/xvector_bench.txt]

Each step is timed with a pair of HIP events on the launch stream (forward, loss, backward, Adam); the two paths are timed
in alternating blocks of steps so that what else runs on the host meets both.  Reported per path: median / p10 / p90 of the
step time and utterances per second at the median; then the ratio.  No gate: the file says which path was faster.

The eager twin is the model from torch's own modules -- nn.Conv1d(padding_mode="reflect"), LeakyReLU, BatchNorm1d,
torch.std_mean, Linear, F.cross_entropy of the log-softmax output -- under torch.optim.Adam, f32, no autocast."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

SURVEY_UTT_PER_S = 1080        # SURVEY.md section 6.2, xvector/run.log: batch 32 on the reference's hardware


class EagerXVector(torch.nn.Module):
    def __init__(self, cfg, speakers):
        super().__init__()
        blocks, cin = [], cfg.input_mel_coefficients
        for c, k, d in zip(cfg.channels, cfg.kernel_sizes, cfg.dilations):
            blocks += [torch.nn.Conv1d(cin, c, k, dilation=d, padding=d * (k - 1) // 2, padding_mode="reflect"),
                       torch.nn.LeakyReLU(0.01), torch.nn.BatchNorm1d(c)]
            cin = c
        self.blocks = torch.nn.Sequential(*blocks)
        L = cfg.lin_neurons
        self.linear = torch.nn.Linear(2 * cin, L)
        self.classifier = torch.nn.Sequential(torch.nn.LeakyReLU(0.01), torch.nn.BatchNorm1d(L), torch.nn.Linear(L, L),
                                              torch.nn.LeakyReLU(0.01), torch.nn.BatchNorm1d(L), torch.nn.Linear(L, speakers))

    def forward(self, feat, label):
        x = self.blocks(feat.transpose(1, 2))
        std, mean = torch.std_mean(x, dim=2)
        emb = self.linear(torch.cat([mean, std + 1e-5], 1))
        return F.cross_entropy(torch.log_softmax(self.classifier(emb), 1), label)


def _stats(ms):
    t = torch.tensor(sorted(ms), dtype=torch.float64)
    q = lambda p: float(t[min(len(ms) - 1, int(round(p * (len(ms) - 1))))])
    return q(0.5), q(0.1), q(0.9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=10, help="steps of one path before the other takes its turn")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xvector_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xvector_bench: needs the GPU (a step time is not measured anywhere else)")
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.xvector import XVectorConfig, XVectorPlan, XVectorStore, XVectorTrainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg, speakers = XVectorConfig(), 5994
    st = XVectorStore(cfg, dev, num_speakers=speakers)
    st.init_weights(1)
    tr = XVectorTrainer(st, XVectorPlan(st, a.batch, a.frames, train=True), Constant(1e-3, 0.9))
    eager = EagerXVector(cfg, speakers).to(dev).train()
    opt = torch.optim.Adam(eager.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(0)
    NB = 8                                       # distinct minibatches, round-robin: one fixed batch is memorised
    feats = torch.randn(NB, a.batch, a.frames, cfg.input_mel_coefficients, generator=g).to(dev)
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
    lines = [f"x-vector training step, {torch.cuda.get_device_name(dev)}, f32, batch {a.batch} x {a.frames} frames x "
             f"{cfg.input_mel_coefficients} mels, {speakers} speakers, forward + cross-entropy + backward + Adam",
             f"HIP events around each step, {a.steps} steps per path after {a.warmup} warm-up steps, the two paths in "
             f"alternating blocks of {a.block} steps, {NB} synthetic minibatches round-robin"]
    for n, label in (("hip", "HIP path (XVectorTrainer)   "), ("eager", "torch eager (same device)   ")):
        m, lo, hi = med[n]
        lines.append(f"{label}: median {m:8.3f} ms  p10 {lo:8.3f}  p90 {hi:8.3f}   {a.batch / m * 1e3:9.1f} utt/s at the median"
                     f"   last loss {float(last[n]):.4f}")
    lines.append(f"ratio eager / HIP at the median: {ratio:.2f}x -- " +
                 ("the HIP step is the faster one" if ratio > 1 else "the HIP step is NOT the faster one"))
    lines.append(f"SURVEY 6.2 (reference's own run.log, other hardware, indicative only): about {SURVEY_UTT_PER_S} utt/s at batch 32")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
