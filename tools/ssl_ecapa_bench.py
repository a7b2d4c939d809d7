"""Time the learned layer mix and the wav2vec2 + ECAPA-TDNN step at the flagship shape -> profiles/ssl_ecapa_bench.txt.

B = 66, 3 s (48,000 samples = 149 frames), wav2vec2-base (H = 768, J = 13 hidden states), bf16 encoder, ECAPA-TDNN in bf16
and in f32.  In ONE process per ECAPA dtype, HIP events around each call, medians of 50 timed calls after 10 warm-up calls,
each HIP piece alternated with the same computation in eager torch on the same device:
  * the mix forward and the mix backward next to their HBM bound (bytes from the shapes over 6.3 TB/s);
  * the 13 injection adds of Plan.backward(dmix=) (one overwrite, twelve adds);
  * a full training step and a frozen step of SslEcapaTrainer.
These are records, not gates.

    python tools/ssl_ecapa_bench.py [--out profiles/ssl_ecapa_bench.txt] [--ecapa bf16 f32]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N = 66, 48000
WARMUP, REPS = 10, 50
HBM = 6.3e12


def timed(fn, reps=REPS, warmup=WARMUP):
    """-> (median, p10, p90) in microseconds of `reps` calls, each between its own pair of HIP events."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[reps // 2], t[reps // 10], t[reps - 1 - reps // 10]


def fmt(t):
    return f"median {t[0]:9.1f} us  p10 {t[1]:9.1f}  p90 {t[2]:9.1f}"


def run(ecapa: str, lines) -> None:
    import torch
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.ecapa import EcapaConfig, EcapaStore
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.ssl_ecapa import SslEcapaPlan, SslEcapaTrainer
    dev, edt = "cuda", {"bf16": torch.bfloat16, "f32": torch.float32}[ecapa]
    cfg = W2V2Config()
    H, J = cfg.hidden_size, cfg.num_hidden_layers + 1
    enc = ParamStore(cfg, dev, torch.bfloat16, head=None, num_speakers=1)
    enc.init_weights(20211)
    ec = EcapaStore(EcapaConfig(input_mel_coefficients=H), dev, edt, num_speakers=5994, feature_weight=J)
    ec.init_weights(20211)
    plan = SslEcapaPlan(enc, ec, B, N, train=True)
    T, M = plan.T, plan.B * plan.T
    gen = torch.Generator().manual_seed(1)
    wav = torch.randn(B, N, generator=gen).to(dev)
    label = torch.randint(0, 5994, (B,), generator=gen).to(dev)
    tag = f"ecapa {ecapa:4s}"
    tr = SslEcapaTrainer(plan, Constant(1e-4, 0.9), ssl_lr_factor=0.1)
    frozen = SslEcapaTrainer(plan, Constant(1e-4, 0.9), num_frozen_steps=None, wav2vec_initially_frozen=True)
    lines.append(f"{tag} full step     {fmt(timed(lambda: tr.train_step(wav, label), 20, 5))}   B = {B}, T = {T}")
    lines.append(f"{tag} frozen step   {fmt(timed(lambda: frozen.train_step(wav, label), 20, 5))}")
    # ---- the mix alone, on the buffers the last step left
    esz, ysz = 2, plan.ecapa.feat.element_size()
    fwd_bytes = M * H * (J * esz + ysz)
    bwd_bytes = M * H * (J * esz + 2 * 2 * ysz + 4)           # hidden states once, g and y twice, dm written
    X = [x.view(B, T, H) for x in plan.enc.X]
    a = ec.p("feature_weight")
    feat, dfeat = plan.ecapa.feat, plan.ecapa.d_feat

    def eager_fwd(a_=a):
        w = torch.softmax(a_, 0)
        m = sum(w[j] * X[j].float() for j in range(J))
        mu = m.mean(1, keepdim=True)
        d = m - mu
        return (d * torch.rsqrt((d * d).mean(1, keepdim=True) + 1e-5)).to(edt)

    def eager_bwd():
        al = a.detach().clone().requires_grad_(True)
        (eager_fwd(al).float() * dfeat.view(B, T, H).float()).sum().backward()
        return al.grad

    t = timed(plan.mix)
    lines.append(f"{tag} mix forward   {fmt(t)}   HBM bound {fwd_bytes / HBM * 1e6:6.1f} us ({fwd_bytes / 1e6:.0f} MB): "
                 f"{fwd_bytes / HBM * 1e6 / t[0] * 100:.0f} % of it")
    lines.append(f"{tag} mix forward, eager torch {fmt(timed(eager_fwd))}")
    bwd = lambda: ops.layer_mix_bwd(plan.table, a, dfeat, dfeat.stride(0), feat, feat.stride(0), plan.rstd, plan.dm,
                                    ec.g("feature_weight"), plan.ws, B, T, instance_norm=True)
    t = timed(bwd)
    lines.append(f"{tag} mix backward  {fmt(t)}   HBM bound {bwd_bytes / HBM * 1e6:6.1f} us ({bwd_bytes / 1e6:.0f} MB): "
                 f"{bwd_bytes / HBM * 1e6 / t[0] * 100:.0f} % of it")
    lines.append(f"{tag} mix backward, eager torch (autograd of the eager forward, d logits only) {fmt(timed(eager_bwd))}")
    # ---- the 13 injection adds
    G, dm, w = plan.enc.G, plan.dm.view(-1), plan.w

    def adds():
        ops.scale_add(G, dm, w, J - 1, J - 1, True)
        for j in range(J - 2, -1, -1):
            ops.scale_add(G, dm, w, j, j, False)

    def eager_adds():
        G.copy_(w[J - 1] * plan.dm)
        for j in range(J - 2, -1, -1):
            G.add_(w[j] * plan.dm)

    add_bytes = M * H * (4 + 2) + (J - 1) * M * H * (4 + 2 + 2)
    t = timed(adds)
    lines.append(f"{tag} 13 injection adds {fmt(t)}   HBM bound {add_bytes / HBM * 1e6:6.1f} us ({add_bytes / 1e6:.0f} MB)")
    lines.append(f"{tag} 13 injection adds, eager torch {fmt(timed(eager_adds))}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssl_ecapa_bench.txt"))
    ap.add_argument("--ecapa", nargs="+", default=["bf16", "f32"])
    args = ap.parse_args()
    lines = [f"tools/ssl_ecapa_bench.py: wav2vec2-base (bf16) + layer mix + ECAPA-TDNN at B = {B}, {N} samples; HIP events around "
             f"each call, {WARMUP} warm-up + {REPS} timed calls (steps: 5 + 20), medians; records, not gates"]
    for e in args.ecapa:
        run(e, lines)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
