"""Timing of the CTC loss (csrc/ctc.hip: w2v2_ctc_fwd_bwd) at the paper's batch, 66 utterances x 149 frames x 5995 classes
(5994 speakers + the blank), one label per utterance, fp16 gradient operand:
  - the CTC-specific launches (row statistics + lattice + dense gradient), forward only (row statistics + lattice), and
    the lattice alone (the same batch over 8 classes, where the row passes are nothing);
  - the whole head, heads.CtcHead.forward_backward (cast, logit GEMM, the three launches, mean, the gradient GEMMs);
  - (a) torch on the device: log_softmax + F.ctc_loss + autograd on the same logits;
  - (b) the reference's route (ref: src/optim/loss/ctc_loss.py:36-58): device log_softmax, copy to the host, CPU
    F.ctc_loss, the gradient back through the copy;
  - a "ctc" training step next to a no-pooling "ce" step of the same build (wav2vec2-base, B = 66, 3 s, fp16, default
    regularisation), the two alternating in one process.
Kernels: HIP-event timings of blocks of back-to-back calls after a warm-up, per call: median / p10 / p90; the candidates
of a comparison alternate block by block.  Steps: host clock around blocks of steps that end in a device synchronise.
    python tools/ctc_bench.py [--reps 30] [--steps 6] [--rounds 3] [--host-reps 3]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from w2v2_speaker_amd import ops

dev = "cuda"
INNER = 10
B, T, C, E = 66, 149, 5995, 768


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def stats(xs):
    return f"median {statistics.median(xs):9.1f} us  p10 {pct(xs, 0.1):9.1f}  p90 {pct(xs, 0.9):9.1f}"


def interleaved(fns, reps, inner=INNER, warmup=2):
    """{name: [us per call]}: the candidates take turns, block by block (same clocks, same neighbours for all)."""
    for fn in fns.values():
        for _ in range(warmup * inner):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[n].append(e0.elapsed_time(e1) * 1e3 / inner)
    return out


def head_timings(reps, host_reps):
    from w2v2_speaker_amd.heads import CtcHead
    g = torch.Generator().manual_seed(3)
    ldc = (C + 7) // 8 * 8
    logits = torch.zeros(B * T, ldc)
    logits[:, :C] = torch.randn(B * T, C, generator=g) * 1.5
    logits[:, 0] += 100.0                                        # the reference's blank bias
    logits = logits.to(dev)
    label = torch.randint(0, C - 1, (B,), generator=g).to(dev)
    in_len = torch.full((B,), T, dtype=torch.int32, device=dev)
    tgt_len = torch.ones(B, dtype=torch.int32, device=dev)
    rows, loss = torch.empty(B, device=dev), torch.empty((), device=dev)
    dl = torch.empty(B * T, ldc, dtype=torch.float16, device=dev)
    ws = torch.empty(ops.ctc_workspace_floats(B, T, 1), device=dev)
    small = torch.randn(B * T, 8, generator=g).to(dev)
    small_label = torch.randint(0, 7, (B,), generator=g).to(dev)

    def ours(grad=True, z=logits, lab=label, c=C, ld=ldc):
        ops.ctc_fwd_bwd(z, lab, in_len, tgt_len, rows, dl if grad else None, ws, B, T, c, ld, target_width=1, target_stride=1,
                        target_offset=1)

    fns = {"row statistics + lattice + gradient (3 launches)": ours,
           "row statistics + lattice (forward only)": lambda: ours(False),
           "lattice alone (8 classes, forward only)": lambda: ours(False, small, small_label, 8, 8)}
    xr = logits[:, :C].reshape(B, T, C).clone().requires_grad_(True)
    tg = (label + 1)[:, None]

    def torch_device():
        xr.grad = None
        l = F.ctc_loss(F.log_softmax(xr, 2).transpose(0, 1), tg, in_len.long(), tgt_len.long(), blank=0, zero_infinity=True)
        l.backward()
        return l

    def reference_route():
        xr.grad = None
        lp = F.log_softmax(xr.transpose(0, 1), dim=2)
        l = F.ctc_loss(lp.to("cpu"), tg.to("cpu"), in_len.to("cpu"), tgt_len.to("cpu"), blank=0, zero_infinity=True).to(dev)
        l.backward()
        return l

    ours()
    ops.mean(rows, loss)
    l = torch_device().detach()
    torch.cuda.synchronize()
    err = float((dl.float().view(B, T, ldc)[..., :C] - xr.grad).norm() / xr.grad.norm())
    print(f"--- CTC at {B} x {T} x {C} (logits {B * T * C * 4 / 1e6:.0f} MB f32), blank bias 100, one label per utterance")
    print(f"same result as torch on the device: loss {float(loss):.5f} vs {float(l):.5f}, fp16 gradient rel-L2 difference {err:.1e}")
    fns["(a) torch device: log_softmax + F.ctc_loss + autograd"] = torch_device
    times = interleaved(fns, reps)
    for n, ts in times.items():
        print(f"{n:56s} {stats(ts)}")
    t3 = statistics.median(times["row statistics + lattice + gradient (3 launches)"])
    t2 = statistics.median(times["row statistics + lattice (forward only)"])
    t1 = statistics.median(times["lattice alone (8 classes, forward only)"])
    byt = B * T * C * 4
    print(f"dense gradient pass   ~ {t3 - t2:7.1f} us: {byt / 1e6:.0f} MB read + {byt / 2e6:.0f} MB written = "
          f"{1.5 * byt / (t3 - t2) / 1e6:.2f} TB/s")
    print(f"row statistics pass   ~ {t2 - t1:7.1f} us: {byt / 1e6:.0f} MB read (twice, the second time from cache) = "
          f"{byt / max(t2 - t1, 1e-9) / 1e6:.2f} TB/s of HBM traffic")
    # (b) includes a host synchronisation: host clock, a few repetitions
    ts = []
    for i in range(host_reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reference_route()
        torch.cuda.synchronize()
        if i:
            ts.append((time.perf_counter() - t0) * 1e6)
    print(f"{'(b) reference route: log_softmax, to host, CPU F.ctc_loss, back':56s} {stats(ts)}   ({host_reps} calls, host clock)")
    # the whole head
    emb = torch.randn(B * T, E, generator=g).to(dev)
    W, b = (torch.randn(C, E, generator=g) / E ** 0.5).to(dev), torch.zeros(C)
    b[0] = 100.0
    b = b.to(dev)
    head = CtcHead(B, T, E, C, w_master=W, w_operand=W.half(), w_grad=torch.zeros_like(W), bias=b, bias_grad=torch.zeros_like(b),
                   emb=emb, act_dtype=torch.float16, train=True, loss_scale=torch.tensor([1024.0, 0, 0, 0], device=dev))
    times = interleaved({"CtcHead.forward_backward (cast, GEMM, 3 launches, mean, gradient GEMMs)":
                         lambda: head.forward_backward(label)}, reps, inner=4)
    for n, ts in times.items():
        print(f"{n}\n{'':56s} {stats(ts)}")


def step_timings(steps, rounds):
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import OneCycle
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    cfg = W2V2Config.from_huggingface_id("facebook/wav2vec2-base")
    N, speakers = 48000, C - 1
    g = torch.Generator().manual_seed(1)
    wav = torch.randn(B, N, generator=g)
    wav = ((wav - wav.mean(dim=1, keepdim=True)) / (wav.std(dim=1, keepdim=True) + 1e-5)).to(dev)
    label = torch.randint(0, speakers, (B,), generator=g).to(dev)
    trainers = {}
    for head in ("ce", "ctc"):
        st = ParamStore(cfg, dev, torch.float16, head=head, num_speakers=speakers, embed_dim=cfg.hidden_size)
        st.init_weights(seed=20211)
        plan = Plan(st, B, N, train=True, reg=Wav2Vec2RegularisationConfig(), pooling="none")
        tr = SpeakerTrainer(st, plan, OneCycle(max_lr=5e-5, total_steps=10 + 2 * (rounds + 1) * steps))
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
    print(f"--- training step, wav2vec2-base, B = {B}, 3 s ({T} frames), fp16, no pooling, {speakers} speakers: {rounds} "
          f"alternating blocks of {steps} steps")
    for head, ts in times.items():
        print(f"{head:5s} step  median {statistics.median(ts):7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}   "
              f"({B / statistics.median(ts) * 1e3:.0f} utterances/s)")
    d = statistics.median(times["ctc"]) - statistics.median(times["ce"])
    spread = max(max(ts) - min(ts) for ts in times.values())
    print(f"ctc - ce (no pooling): {d * 1e3:+.0f} us per step; block-to-block spread of one head: {spread * 1e3:.0f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    print(f"device: {torch.cuda.get_device_name(0)}")
    head_timings(a.reps, a.host_reps)
    step_timings(a.steps, a.rounds)


if __name__ == "__main__":
    main()
