"""Cases and float64 references of the learned layer mix (include/w2v2_hip.h, "layer mix") and of the wav2vec2 + ECAPA-TDNN
model built on it, shared by test_ssl_ecapa_cpu.py and test_ssl_ecapa_gpu.py.

One restatement of the header's definitions, ``mix_forward`` / ``mix_backward``, written in plain torch and evaluated in
float64 (the reference) and in float32 (the yardstick): the bound a kernel result is held to is 4 x the largest error of the
float32 evaluation against the float64 one on the same case -- the 4 because the kernel's wave and tree reductions order the
sums differently from the sequential restatement -- plus one unit in the last place of the stored type (the result is
rounded once to it).  Every reference is evaluated on exactly the kernel's inputs: 16-bit inputs are rounded first and
upcast, and the backward takes the stored y and rstd, as the kernel does.
"""
from __future__ import annotations

import functools
from typing import Dict, List

import torch

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
EPS = 1e-5
PARITY_PREFIX = "ssl-ecapa-parity:"        # lines the GPU tests print; tools collect them into profiles/ssl_ecapa_parity.txt

# name -> dict(B, T, H, J, x=dtype, y=dtype, norm, lens, logits, special)
_BASE = dict(x=F32, y=F32, norm=True, lens=None, logits="random", special=None)
MIX_CASES: Dict[str, dict] = {
    "2x5x64x3": dict(B=2, T=5, H=64, J=3),
    "1x37x1024x25": dict(B=1, T=37, H=1024, J=25),
    "2x149x768x13": dict(B=2, T=149, H=768, J=13, x=BF16, y=BF16),
    "2x149x768x13-f32": dict(B=2, T=149, H=768, J=13),
    "smallest-H-T1": dict(B=2, T=1, H=8, J=3),
    "smallest-H-T2": dict(B=2, T=2, H=8, J=3),
    "J1": dict(B=2, T=5, H=64, J=1),
    "max-J": dict(B=1, T=7, H=16, J=32),
    "constant-channel": dict(B=2, T=5, H=64, J=3, special="constant"),
    "large-mean-channel": dict(B=2, T=37, H=64, J=3, special="large-mean"),
    "logits-zero": dict(B=2, T=5, H=64, J=3, logits="zero"),
    "one-logit-30": dict(B=2, T=5, H=64, J=3, logits="one30"),
    "no-instance-norm": dict(B=2, T=37, H=72, J=4, norm=False),
    "no-instance-norm-bf16": dict(B=2, T=37, H=72, J=4, norm=False, x=BF16, y=BF16),
    "lengths": dict(B=3, T=37, H=64, J=3, lens=(1, 37, 36)),
    "lengths-bf16": dict(B=3, T=37, H=72, J=3, lens=(1, 37, 36), x=BF16, y=BF16),
    "lengths-no-norm": dict(B=3, T=37, H=64, J=3, lens=(1, 37, 36), norm=False),
    "two-row-rounds-partial-tile": dict(B=2, T=70, H=72, J=4),          # 70 > 2 * 32 rows per pass; 72 = one tile + 8 channels
    "beyond-lds-stage": dict(B=1, T=515, H=8, J=2),                     # more than 512 frames: m staged in global memory
    "beyond-lds-stage-lengths": dict(B=2, T=515, H=8, J=2, lens=(513, 40), y=BF16),
}
for _x in (F32, BF16, F16):
    for _y in (F32, BF16):
        MIX_CASES[f"dtypes-{str(_x)[6:]}-{str(_y)[6:]}"] = dict(B=2, T=37, H=72, J=4, x=_x, y=_y)
MIX_CASES = {k: {**_BASE, **v} for k, v in MIX_CASES.items()}
# the backward has no lengths form
BWD_CASES = [k for k, c in MIX_CASES.items() if c["lens"] is None]


@functools.lru_cache(maxsize=None)
def mix_inputs(name: str):
    """-> (xs: J tensors [B, T, H] in the case's input dtype, logits [J] f32, g [B, T, H] in the case's y dtype)."""
    c = MIX_CASES[name]
    B, T, H, J = c["B"], c["T"], c["H"], c["J"]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    xs = [torch.randn(B, T, H, generator=gen) * (0.5 + 0.25 * j) + 0.1 * j for j in range(J)]
    if c["special"] == "constant":        # channel 3 does not move over time: var = 0, y = noise of the f32 mean
        for j, x in enumerate(xs):
            x[:, :, 3] = 0.37 + 0.11 * j
    if c["special"] == "large-mean":      # channel 5: mean 1000 x its deviation
        for x in xs:
            x[:, :, 5] = 1000.0 * x[:, :, 5].std() + x[:, :, 5]
    xs = [x.to(c["x"]) for x in xs]
    if c["logits"] == "zero":
        a = torch.zeros(J)
    else:
        a = torch.randn(J, generator=gen)
        if c["logits"] == "one30":
            a[1] = 30.0
    g = torch.randn(B, T, H, generator=gen).to(c["y"])
    return xs, a, g


def softmax_weights(a: torch.Tensor, dt) -> torch.Tensor:
    a = a.to(dt)
    e = torch.exp(a - a.max())
    return e / e.sum()


def mix_forward(xs: List[torch.Tensor], a: torch.Tensor, lens, norm: bool, dt):
    """The header's forward, steps 1-6, in dtype ``dt``: -> (y [B, T, H], rstd [B, H] or None, w [J]).  Differentiable."""
    w = softmax_weights(a, dt)
    m = None
    for j, x in enumerate(xs):            # ascending j
        t = w[j] * x.to(dt)
        m = t if m is None else m + t
    B, T, H = m.shape
    if lens is None and norm:
        mu = m.sum(1, keepdim=True) / T
        d = m - mu
        r = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / T + EPS)
        return d * r, r[:, 0], w
    ys, rs = [], []
    for b in range(B):
        n = T if lens is None else int(lens[b])
        mb = m[b, :n]
        if norm:
            mu = mb.sum(0, keepdim=True) / n
            d = mb - mu
            r = 1.0 / torch.sqrt((d * d).sum(0, keepdim=True) / n + EPS)
            mb = d * r
            rs.append(r[0])
        ys.append(torch.cat([mb, torch.zeros(T - n, H, dtype=dt)], 0))
    return torch.stack(ys), (torch.stack(rs) if norm else None), w


def mix_backward(xs, a, g, y, r, norm: bool, dt):
    """The header's backward from the STORED y and rstd: -> (dm [B, T, H], da [J], d [J])."""
    w = softmax_weights(a, dt)
    g = g.to(dt)
    if norm:
        y, r = y.to(dt), r.to(dt)
        T = g.shape[1]
        s1 = g.sum(1, keepdim=True) / T
        s2 = (g * y).sum(1, keepdim=True) / T
        dm = r[:, None] * ((g - s1) - y * s2)
    else:
        dm = g
    d = torch.stack([(dm * x.to(dt)).sum() for x in xs])
    return dm, w * (d - (w * d).sum()), d


def ulp(ref: torch.Tensor, dtype) -> torch.Tensor:
    """One unit in the last place of ``dtype`` at the magnitude of each element of ref (float64)."""
    bits = {F32: 23, BF16: 7, F16: 10}[dtype]
    tiny = {F32: -126, BF16: -126, F16: -14}[dtype]
    e = torch.floor(torch.log2(ref.abs().to(F64).clamp_min(2.0 ** tiny)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - bits)


@functools.lru_cache(maxsize=None)
def forward_reference(name: str):
    """-> dict(y, r, w: float64 references; y_err, r_err: max abs error of the float32 restatement; y_max)."""
    c = MIX_CASES[name]
    xs, a, _ = mix_inputs(name)
    y64, r64, w64 = mix_forward(xs, a, c["lens"], c["norm"], F64)
    y32, r32, _ = mix_forward(xs, a, c["lens"], c["norm"], F32)
    out = dict(y=y64, r=r64, w=w64, y_err=float((y32.to(F64) - y64).abs().max()), y_max=float(y64.abs().max()))
    out["r_err"] = float((r32.to(F64) - r64).abs().max()) if c["norm"] else 0.0
    return out


@functools.lru_cache(maxsize=None)
def backward_reference(name: str):
    """The backward's inputs (stored y and rstd = the float64 forward rounded to the stored types) and references:
    -> dict(y_st, r_st, dm, da, d: float64; dm_err, da_err: max abs error of the float32 restatement; fold_bound)."""
    c = MIX_CASES[name]
    xs, a, g = mix_inputs(name)
    fr = forward_reference(name)
    y_st = fr["y"].to(c["y"])
    r_st = fr["r"].to(F32) if c["norm"] else None
    dm64, da64, d64 = mix_backward(xs, a, g, y_st, r_st, c["norm"], F64)
    dm32, da32, _ = mix_backward(xs, a, g, y_st, r_st, c["norm"], F32)
    # |sum_j da_j| = |D (1 - sum_j w_j)| in exact arithmetic on the kernel's f32 weights, D = sum_k w_k d_k: each of the
    # J weights is a correctly rounded quotient of f32 values that sum to within J roundings of the divisor, so
    # |1 - sum w| <= (J + 2) 2^-24.  On top: each da_j is rounded once to f32 when it is added into the arena, and the
    # f64 fold in front of it contributes 2^-53 relative per operation (J products and sums): J (2^-24 + J 2^-52) max|da|
    J = c["J"]
    D = abs(float((softmax_weights(a, F64) * d64).sum()))
    fold = J * (2.0 ** -24 + J * 2.0 ** -52) * float(da64.abs().max()) + (J + 2) * 2.0 ** -24 * D
    return dict(y_st=y_st, r_st=r_st, dm=dm64, da=da64, d=d64, dm_err=float((dm32.to(F64) - dm64).abs().max()),
                da_err=float((da32.to(F64) - da64).abs().max()), fold_bound=fold)


def within(got: torch.Tensor, ref: torch.Tensor, err32: float, stored) -> tuple:
    """-> (ok, worst excess ratio, max abs error): |got - ref| <= 4 * err32 + one ulp of the stored type, per element."""
    diff = (got.to(F64) - ref).abs()
    bound = 4.0 * err32 + ulp(ref, stored)
    ratio = float((diff / bound.clamp_min(1e-300)).max()) if diff.numel() else 0.0
    return bool((diff <= bound).all()), ratio, float(diff.max()) if diff.numel() else 0.0


# ---------------------------------------------------------------------------------------- the composed model (tiny)
# four utterances, like test_ecapa_gpu.py's tiny batch: ECAPA's last BatchNorm normalises over the batch, and over two
# rows it is a sign function of their difference
TINY_SAMPLES, TINY_CLASSES, TINY_BATCH = 4000, 4, 4


def tiny_configs():
    """-> (oracle wav2vec2 config, oracle ECAPA config): H = 64, L = 2, 4000 samples = 12 frames; ECAPA tiny at 64 inputs."""
    from oracle import ecapa_oracle as E
    from oracle import w2v2_oracle as O
    ocfg = O.OracleConfig.tiny()
    ecfg = E.EcapaConfig(input_size=ocfg.hidden_size, lin_neurons=24, channels=(64, 64, 64, 64, 192), attention_channels=16,
                         res2net_scale=4, se_channels=16)
    return ocfg, ecfg


@functools.lru_cache(maxsize=None)
def tiny_state(seed: int = 20211):
    """-> (wav2vec2 state dict (bare names), ECAPA state dict (bare names), AAM weight, logits a [L + 1])."""
    from oracle import ecapa_oracle as E
    from oracle import w2v2_oracle as O
    ocfg, ecfg = tiny_configs()
    sdw = O.make_state_dict(ocfg, seed)
    sde = E.make_state_dict(ecfg, seed)
    fcw = O.synth_tensor("loss_fn.fc_weights", (TINY_CLASSES, ecfg.lin_neurons), seed)
    a = 0.5 * O.synth_tensor("feature_weight", (ocfg.num_hidden_layers + 1,), seed)
    return sdw, sde, fcw, a


@functools.lru_cache(maxsize=None)
def tiny_batch(batch: int = TINY_BATCH, seed: int = 5):
    from oracle import w2v2_oracle as O
    wav, label = O.synth_batch(batch, TINY_SAMPLES, TINY_CLASSES, seed=seed)
    return wav[:, 0, :].contiguous(), label


def hidden_states(wav, sdw, ocfg, skip=(), mask=None):
    """The oracle's hidden states [prologue output, layer 1 .. L]; a LayerDrop-skipped layer repeats its input."""
    from oracle import w2v2_oracle as O
    _, st = O.wav2vec2_forward(wav, sdw, ocfg, mask_time_indices=mask, skip_layers=skip, return_stages=True)
    hs = [st["enc_in"]]
    for l in range(ocfg.num_hidden_layers):
        hs.append(st.get(f"layer{l}", hs[-1]))
    return hs


def composed(dt, skip=(), mask=None, norm: bool = True):
    """The whole chain in dtype ``dt`` with autograd: wav2vec2 oracle -> mix -> ECAPA oracle -> AAM-softmax.
    -> dict(loss, emb, hs, y, grads_w2v, grads_ecapa, grad_fcw, grad_a)."""
    from oracle import ecapa_oracle as E
    from oracle import w2v2_oracle as O
    ocfg, ecfg = tiny_configs()
    sdw, sde, fcw, a = tiny_state()
    wav, label = tiny_batch()
    leaf = lambda t: t.detach().to(dt).clone().requires_grad_(True)
    sdw, sde, fcw, a = {k: leaf(v) for k, v in sdw.items()}, {k: leaf(v) for k, v in sde.items()}, leaf(fcw), leaf(a)
    hs = hidden_states(wav.to(dt), sdw, ocfg, skip, mask)
    y, _, _ = mix_forward(hs, a, None, norm, dt)
    emb = E.ecapa_forward(y, sde, ecfg)
    loss, _ = O.aam_softmax(emb, fcw, label, 0.2, 30.0)
    loss.backward()
    g = lambda t: None if t.grad is None else t.grad.detach()
    return dict(loss=loss.detach(), emb=emb.detach(), hs=[h.detach() for h in hs], y=y.detach(),
                grads_w2v={k: g(v) for k, v in sdw.items()}, grads_ecapa={k: g(v) for k, v in sde.items()},
                grad_fcw=g(fcw), grad_a=g(a))


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.to(F64) - ref.to(F64)).norm() / ref.to(F64).norm().clamp_min(1e-300))


def group_error(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> float:
    """The error of a group of gradients: max over its tensors of |got - ref| / (|ref| + 1e-4 gmax), gmax the largest
    norm in the group -- a tensor whose exact gradient vanishes (a bias in front of a normalisation) is held to the
    scale of the group, not to its own rounding noise."""
    ref = {k: v for k, v in ref.items() if v is not None}
    gmax = max(float(v.to(F64).norm()) for v in ref.values())
    return max(float((got[k].to(F64).reshape(v.shape) - v.to(F64)).norm()) / (float(v.to(F64).norm()) + 1e-4 * gmax)
               for k, v in ref.items())


@functools.lru_cache(maxsize=None)
def composed_reference():
    """Float64 chain and the error of the float32 chain against it: -> (ref64, dict of errors of the f32 run: relative
    for the loss, rel-L2 for embedding / grad_a / grad_fcw, group_error for the two parameter groups)."""
    r64, r32 = composed(F64), composed(F32)
    err = dict(loss=abs(float(r32["loss"]) - float(r64["loss"])) / abs(float(r64["loss"])), emb=rel_l2(r32["emb"], r64["emb"]),
               grad_a=rel_l2(r32["grad_a"], r64["grad_a"]), grad_fcw=rel_l2(r32["grad_fcw"], r64["grad_fcw"]))
    # (the conv feature extractor is frozen in the model, as in every default of the project: not part of the group)
    r64["grads_w2v"] = {k: v for k, v in r64["grads_w2v"].items() if not k.startswith("feature_extractor.")}
    for grp in ("grads_w2v", "grads_ecapa"):
        err[grp] = group_error(r32[grp], r64[grp])
    return r64, err


def layerdrop_patterns(num_layers: int):
    """Every LayerDrop pattern of a ``num_layers``-layer encoder."""
    return [tuple(l for l in range(num_layers) if m >> l & 1) for m in range(1 << num_layers)]
