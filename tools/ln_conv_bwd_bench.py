"""Timing of the two backward kernels of the layer-norm convolution stack (fp16), medians over single launches:
  (a) w2v2_layernorm_gelu_bwd at H = 512, M = 66 x {4799, 2399, 149}; algorithmic bytes = dy + z read, dz written --
      next to w2v2_layernorm_bwd (fixed-order workspace path) at the same (M, H), which moves the same three streams
  (b) w2v2_conv0_layernorm_gelu_bwd at B = 66, N = 48000; algorithmic bytes = dy read
and one unfrozen fp16 training step of the one-block base-width model, layer-norm family next to the group-norm family.
    python tools/ln_conv_bwd_bench.py [--no-step]"""
import dataclasses, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from w2v2_speaker_amd import ops
dev = "cuda"


def t(fn, reps=30):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


H = 512
g = 1.0 + 0.1 * torch.randn(H, device=dev); b = 0.1 * torch.randn(H, device=dev)
dg, db, dbias = (torch.zeros(H, device=dev) for _ in range(3))
for L in (4799, 2399, 149):
    M = 66 * L
    z = torch.randn(M, H, device=dev).half(); dy = torch.randn(M, H, device=dev).half(); dz = torch.empty_like(dy)
    ws = ops.layernorm_gelu_bwd_workspace(M, H, dev)
    us = t(lambda: ops.layernorm_gelu_bwd(dy, z, g, b, dz, dg, db, dbias, ws))
    gb = 3 * M * H * 2 / 1e9
    mean, rstd = torch.zeros(M, device=dev), torch.ones(M, device=dev)
    us2 = t(lambda: ops.layernorm_bwd(dy, z, mean, rstd, g, dz, None, dg, db))
    print(f"(a) layernorm_gelu_bwd M=66x{L} H={H}: {us:8.1f} us {gb / us * 1e6:7.0f} GB/s   |  layernorm_bwd {us2:8.1f} us "
          f"{gb / us2 * 1e6:7.0f} GB/s   ratio {us2 / us:.2f}")
    del z, dy, dz
B, N, C, k, s = 66, 48000, 512, 10, 5
L0 = (N - k) // s + 1
wav = torch.randn(B, N, device=dev); w = 0.3 * torch.randn(C, 1, k, device=dev); bias = 0.1 * torch.randn(C, device=dev)
dy = torch.randn(B, L0, C, device=dev).half()
dw = torch.zeros(C, 1, k, device=dev)
ws = ops.conv0_layernorm_gelu_bwd_workspace(B, N, C, k, s, dev)
us = t(lambda: ops.conv0_layernorm_gelu_bwd(wav, w, bias, g, b, dy, dw, dbias, dg, db, ws, k, s))
gb = B * L0 * C * 2 / 1e9
print(f"(b) conv0_layernorm_gelu_bwd B={B} N={N} C={C}: {us:8.1f} us {gb / us * 1e6:7.0f} GB/s")
del dy, wav
if "--no-step" not in sys.argv:
    from oracle import w2v2_oracle as O
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    reg = Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, hidden_dropout=0.0,
                                       layerdrop=0.0, mask_time_prob=0.0)
    wavb, label = O.synth_batch(B, N, 100, seed=5)
    wavb, label = wavb.to(dev), label.to(dev)
    for fam, kw in (("group-norm", {}), ("layer-norm", dict(do_stable_layer_norm=True, feat_extract_norm="layer", conv_bias=True))):
        cfg = dataclasses.replace(W2V2Config(), num_hidden_layers=1, **kw)
        st = ParamStore(cfg, dev, torch.float16, head="aam", num_speakers=100, freeze_cnn=False)
        st.init_weights(3)
        tr = SpeakerTrainer(st, Plan(st, B, N, train=True, reg=reg), Constant(1e-5))
        us = t(lambda: tr.train_step(wavb, label, skip_layers=()), reps=10)
        print(f"unfrozen fp16 train step, 1 block, base width, B={B} N={N}, {fam}: {us / 1e3:8.2f} ms")
        del tr, st
