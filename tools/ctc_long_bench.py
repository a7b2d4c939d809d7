"""Timing of the speech recognition path's device pieces (csrc/ctc_long.hip) at a LibriSpeech-like shape: 8 utterances x 800
frames x 32 letters, transcripts of 100 ... 400 letters (seeded; the widest sets the target width), fp16 gradient operand:
  - the three launches of w2v2_ctc_long_fwd_bwd (row statistics + lattice + dense gradient) and the forward two, beside
    (a) torch on the device: log_softmax + F.ctc_loss + autograd on the same logits, and
    (b) the reference's route (ref: src/optim/loss/ctc_loss.py:36-58): device log_softmax, copy to the host, CPU
        F.ctc_loss, the gradient back through the copy;
  - the greedy decoder (w2v2_ctc_greedy_decode + ONE copy of tokens and counts to the host) beside the reference's loop
    (ref: speech_recognition_module.py:233-248): an argmax and a copy to the host per utterance;
  - one full letter-head training step (wav2vec2-base, B = 8, 800 frames = 16 s, fp16, default regularisation) beside a
    no-pooling "ce" step of the same shape and class count, the two alternating in one process.
Kernels: HIP-event timings of blocks of back-to-back calls after a warm-up, per call: median / p10 / p90; the candidates
of a comparison alternate block by block.  What ends in a host synchronisation is timed with the host clock.
    python tools/ctc_long_bench.py [--reps 30] [--steps 4] [--rounds 3] [--host-reps 5] [--out profiles/ctc_long_bench.txt]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
from ctc_bench import interleaved, stats
from w2v2_speaker_amd import ops

dev = "cuda"
B, T, C, E = 8, 800, 32, 768
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def host_timed(fn, reps):
    ts = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i:
            ts.append((time.perf_counter() - t0) * 1e6)
    return ts


def batch(g):
    tgt_len = torch.randint(100, 401, (B,), generator=g)
    tgt_len[0] = 400
    W = int(tgt_len.max())
    targets = torch.randint(1, C, (B, W), generator=g)
    in_len = torch.randint(700, T + 1, (B,), generator=g)
    in_len[0] = T
    return targets, tgt_len.to(torch.int32), in_len.to(torch.int32), W


def loss_timings(reps, host_reps):
    g = torch.Generator().manual_seed(24)
    targets, tgt_len, in_len, W = batch(g)
    logits = (torch.randn(B * T, C, generator=g) * 1.5).to(dev)
    tg, tl, il = targets.to(dev), tgt_len.to(dev), in_len.to(dev)
    rows, loss = torch.empty(B, device=dev), torch.empty((), device=dev)
    dl = torch.empty(B * T, C, dtype=torch.float16, device=dev)
    floats = ops.ctc_long_workspace_floats(B, T, W)
    ws = torch.empty(floats, device=dev)

    def ours(grad=True):
        ops.ctc_long_fwd_bwd(logits, tg, il, tl, rows, dl if grad else None, ws, B, T, C, C, target_width=W)

    xr = logits.view(B, T, C).clone().requires_grad_(True)

    def torch_device():
        xr.grad = None
        l = F.ctc_loss(F.log_softmax(xr, 2).transpose(0, 1), tg, il.long(), tl.long(), blank=0, zero_infinity=True)
        l.backward()
        return l

    def reference_route():
        xr.grad = None
        lp = F.log_softmax(xr.transpose(0, 1), dim=2)
        l = F.ctc_loss(lp.to("cpu"), tg.to("cpu"), il.to("cpu"), tl.to("cpu"), blank=0, zero_infinity=True).to(dev)
        l.backward()
        return l

    ours()
    ops.mean(rows, loss)
    l = torch_device().detach()
    torch.cuda.synchronize()
    err = float((dl.float().view(B, T, C) - xr.grad).norm() / xr.grad.norm())
    say(f"--- CTC at {B} x {T} x {C}, transcripts of {sorted(tgt_len.tolist())} letters (target width {W}), input lengths "
        f"{sorted(in_len.tolist())}")
    say(f"workspace: {floats * 4 / 1e6:.1f} MB (the short form's layout at this width would take "
        f"{(4 * B + B * T * (4 + 2 * (W + 1) + 4 * (2 * W + 1))) * 4 / 1e6:.1f} MB)")
    say(f"same result as torch on the device: loss {float(loss):.5f} vs {float(l):.5f}, fp16 gradient rel-L2 difference {err:.1e}")
    times = interleaved({"row statistics + lattice + gradient (3 launches)": ours,
                         "row statistics + lattice (forward only)": lambda: ours(False),
                         "(a) torch device: log_softmax + F.ctc_loss + autograd": torch_device}, reps, inner=4)
    for n, ts in times.items():
        say(f"{n:56s} {stats(ts)}")
    ts = host_timed(reference_route, host_reps)
    say(f"{'(b) reference route: log_softmax, to host, CPU F.ctc_loss, back':56s} {stats(ts)}   ({host_reps} calls, host clock)")
    # the decoder: both routes end on the host, host clock for both
    tokens = torch.zeros(B * T + B, dtype=torch.int32, device=dev)

    def ours_decode():
        ops.ctc_greedy_decode(logits, il, tokens[:B * T].view(B, T), tokens[B * T:], B, T, C, C)
        return tokens.cpu()

    lengths = in_len.tolist()
    z3 = logits.view(B, T, C)

    def reference_decode():
        return [torch.argmax(z3[b, :lengths[b]], dim=1).cpu() for b in range(B)]

    a = host_timed(ours_decode, host_reps * 4)
    b = host_timed(reference_decode, host_reps * 4)
    say(f"{'greedy decoder: one launch + one copy to the host':56s} {stats(a)}   ({host_reps * 4} calls, host clock)")
    say(f"{'reference loop: argmax + copy to the host per utterance':56s} {stats(b)}   (the collapse on the host not counted)")
    t = interleaved({"greedy decoder, the launch alone": lambda: ops.ctc_greedy_decode(
        logits, il, tokens[:B * T].view(B, T), tokens[B * T:], B, T, C, C)}, reps)
    for n, ts in t.items():
        say(f"{n:56s} {stats(ts)}")


def step_timings(steps, rounds):
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import OneCycle
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    cfg = W2V2Config.from_huggingface_id("facebook/wav2vec2-base")
    N = T * 320 + 80
    g = torch.Generator().manual_seed(1)
    wav = torch.randn(B, N, generator=g)
    wav = ((wav - wav.mean(dim=1, keepdim=True)) / (wav.std(dim=1, keepdim=True) + 1e-5)).to(dev)
    targets, tgt_len, in_len, W = batch(g)
    samples = [int(n) * 320 + 80 for n in in_len]
    label = torch.randint(0, C, (B,), generator=g).to(dev)
    trainers = {}
    for head in ("ce", "letter"):
        kw = dict(head="letter", vocab_size=C) if head == "letter" else dict(head="ce", num_speakers=C, embed_dim=cfg.hidden_size)
        st = ParamStore(cfg, dev, torch.float16, **kw)
        st.init_weights(seed=20211)
        plan = Plan(st, B, N, train=True, reg=Wav2Vec2RegularisationConfig(), pooling="none", max_target=W)
        assert plan.T == T
        tr = SpeakerTrainer(st, plan, OneCycle(max_lr=5e-5, total_steps=10 + 2 * (rounds + 1) * steps))
        if head == "letter":
            trainers[head] = (lambda tr=tr: tr.train_step(wav, None, transcript=(targets, tgt_len, samples)))
        else:
            trainers[head] = (lambda tr=tr: tr.train_step(wav, label))
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
    say(f"--- training step, wav2vec2-base, B = {B}, {N / 16000:.0f} s ({T} frames), fp16, no pooling, {C} classes: {rounds} "
        f"alternating blocks of {steps} steps")
    for head, ts in times.items():
        say(f"{head:7s} step  median {statistics.median(ts):7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}   "
            f"({B / statistics.median(ts) * 1e3:.0f} utterances/s)")
    d = statistics.median(times["letter"]) - statistics.median(times["ce"])
    spread = max(max(ts) - min(ts) for ts in times.values())
    say(f"letter - ce (no pooling): {d * 1e3:+.0f} us per step; block-to-block spread of one head: {spread * 1e3:.0f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "ctc_long_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    say(f"device: {torch.cuda.get_device_name(0)}")
    loss_timings(a.reps, a.host_reps)
    step_timings(a.steps, a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
