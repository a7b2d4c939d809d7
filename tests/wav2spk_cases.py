"""Geometries and float64 references for the stages of the wav2spk path (w2v2_speaker_amd/wav2spk.py on csrc/wav2spk.hip and
the GEMMs), shared by tests/test_wav2spk_cpu.py, tests/test_wav2spk_gpu.py and tests/golden/make_wav2spk_goldens.py.  No GPU
and no ``ops`` import here: everything is plain torch on the CPU in float64.

One function per stage, each taking the stage's own operands as the plan stores them ([B*T, C] matrices, channels last)
and written from the model's definition (ref: src/lightning_modules/speaker/wav2spk.py:116-299) with a hand-derived
backward.  ``forward_ref`` / ``backward_ref`` string the stages together; tests/test_wav2spk_cpu.py holds that chain to the
golden (tests/golden/g23_wav2spk.npz: float64 autograd over torch's own modules and the reference's own TemporalGate and
pooling classes), so a sign or index error in a stage reference cannot agree with a kernel that has the same error."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from ecapa_stage_cases import F32_BOUND, pack_conv_weight, rel_l2, sum_scale_error, unpack_conv_grad  # noqa: F401

F64 = torch.float64
IN_EPS = 1e-5
ENCODER = ((1, 40, 10, 5, 4), (40, 200, 5, 4, 2), (200, 300, 5, 2, 2), (300, 512, 3, 2, 1), (512, 512, 3, 2, 1))
AGGREGATOR = ((512, 512, 3, 1, 1),) * 4
FEATURES, HIDDEN, SPEAKERS, SEED = 512, (512, 128), 7, 2310
PARAMETERS = 5590995                       # at 7 speakers, mean+std, hidden (512, 128)

# the whole-step cases (batch, samples): 3200 -> 640, 160, 80, 40, 20 frames; 805 -> 161, 41, 21, 11, 6
STEP_CASES = ((2, 3200), (3, 805))
GATINGS, POOLINGS, EMBEDDING_LAYERS = (True, False), ("mean+std", "mean"), (-1, 0, 2)
EVAL_LENGTHS = (805, 1600, 1601, 3200, 2399)
SAMPLE = 128                               # elements of a large tensor the golden keeps (strided), beside its norm

# stage kernels: C a multiple of 4 but not of 8, a partial last 128-channel strip, more than one strip
CHANNELS = (40, 44, 200)
FRAMES = (2, 127, 128, 129, 257)           # around the 128-frame statistics block
# (k, stride, pad) of the reference's layers 1-4 and the aggregator, and Lin so that the last window does / does not touch
# the right padding
GATHERS = ((5, 4, 2, 41), (5, 4, 2, 43), (5, 2, 2, 21), (5, 2, 2, 20), (3, 2, 1, 11), (3, 2, 1, 12), (3, 1, 1, 9), (3, 1, 1, 2))
FIRST = (10, 5, 4)                         # layer 0
FIRST_SAMPLES = (162, 805, 1282, 1285)     # the minimum; 805 % 5 = 0, 1282 and 1285: the last window in / out of the padding


def frames_of(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def encoder_frames(n: int):
    out = []
    for _, _, k, s, p in ENCODER:
        n = frames_of(n, k, s, p)
        out.append(n)
    return tuple(out)


def pool_dim(pooling: str) -> int:
    return FEATURES * (2 if pooling == "mean+std" else 1)


def param_shapes(pooling="mean+std", hidden=HIDDEN, speakers=SPEAKERS):
    """The state-dict names and shapes of the model, written out independently of wav2spk.wav2spk_param_shapes."""
    s = OrderedDict()
    for i, (cin, cout, k, _, _) in enumerate(ENCODER):
        s[f"encoder.{i}.0.weight"], s[f"encoder.{i}.0.bias"] = (cout, cin, k), (cout,)
    s["temporal_gate.W"], s["temporal_gate.b"] = (FEATURES, FEATURES), (FEATURES, 1)
    for i, (cin, cout, k, _, _) in enumerate(AGGREGATOR):
        s[f"aggregator.{i}.0.weight"], s[f"aggregator.{i}.0.bias"] = (cout, cin, k), (cout,)
    dims = (pool_dim(pooling),) + tuple(hidden) + (speakers,)
    for i in range(len(dims) - 1):
        s[f"fc_list.{i}.0.weight"], s[f"fc_list.{i}.0.bias"] = (dims[i + 1], dims[i]), (dims[i + 1],)
    return s


def make_state_dict(seed: int = SEED, **kw):
    """synth_weight(name, shape, seed) for every parameter (f32 values, so nothing is stored): convolution weights scaled to
    He variance (synth_weight leaves 3-D weights outside the wav2vec2 feature extractor at unit variance), the gate's
    [512, 1] bias at 0.1."""
    from w2v2_speaker_amd.data.synthetic import synth_weight
    sd = OrderedDict()
    for n, shp in param_shapes(**kw).items():
        a = synth_weight(n, shp, seed)
        if len(shp) == 3:
            a = a * np.float32(math.sqrt(2.0 / (shp[1] * shp[2])))
        elif n == "temporal_gate.b":
            a = a * np.float32(0.1)
        sd[n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return sd


def synth_batch(batch: int, samples: int, seed: int = SEED, speakers: int = SPEAKERS):
    """N(0, 1) waveforms normalised per utterance (the reference's input normalisation) [B, N] f32, labels [B] int64."""
    g = np.random.Generator(np.random.PCG64(seed + 1000 * batch + samples))
    wav = torch.from_numpy(g.standard_normal((batch, samples)).astype(np.float32))
    std, mean = torch.std_mean(wav, dim=1, keepdim=True)
    wav = ((wav - mean) / (std + 1e-5)).contiguous()
    return wav, torch.from_numpy(g.integers(0, speakers, size=(batch,)).astype(np.int64))


def strided(t: torch.Tensor, n: int = SAMPLE) -> torch.Tensor:
    """At most n elements of t, evenly strided from the first (what the golden keeps of a large tensor)."""
    f = t.reshape(-1)
    return f[::max(1, -(-f.numel() // n))]


# ------------------------------------------------------------------------------------------------ stages
def im2col_zero_ref(x, k, s, p):
    """x [B, Tin, C] -> col [B * Tout, k * C] (tap-major), zero padding."""
    x = x.to(F64)
    B, Tin, C = x.shape
    Tout = frames_of(Tin, k, s, p)
    xp = F.pad(x, (0, 0, p, p))
    t = torch.arange(Tout) * s
    return torch.stack([xp[:, t + j] for j in range(k)], 2).reshape(B * Tout, k * C)


def col2im_zero_ref(dcol, B, Tin, C, k, s, p):
    """The adjoint of im2col_zero_ref, written as a scatter-add: dcol [B * Tout, k * C] -> dx [B, Tin, C]."""
    Tout = frames_of(Tin, k, s, p)
    d = dcol.to(F64).view(B, Tout, k, C)
    dxp = torch.zeros(B, Tin + 2 * p, C, dtype=F64)
    t = torch.arange(Tout) * s
    for j in range(k):
        dxp.index_add_(1, t + j, d[:, :, j])
    return dxp[:, p:p + Tin]


def conv_fwd_ref(x, W, b, B, Tin, s, p):
    """x [B*Tin, cin], W torch layout [cout, cin, k] -> z [B*Tout, cout]."""
    k = W.shape[2]
    return im2col_zero_ref(x.to(F64).view(B, Tin, -1), k, s, p) @ pack_conv_weight(W.to(F64)).t() + b.to(F64)


def conv_bwd_ref(x, W, dz, B, Tin, s, p):
    """-> (dW [cout, cin, k], db [cout], dx [B*Tin, cin], dW_abs): dW_abs the sums of the |terms| of dW."""
    x, W, dz = x.to(F64), W.to(F64), dz.to(F64)
    cin, k = W.shape[1], W.shape[2]
    col = im2col_zero_ref(x.view(B, Tin, cin), k, s, p)
    dW = unpack_conv_grad(dz.t() @ col, cin, k)
    dW_abs = unpack_conv_grad(dz.abs().t() @ col.abs(), cin, k)
    dx = col2im_zero_ref(dz @ pack_conv_weight(W), B, Tin, cin, k, s, p)
    return dW, dz.sum(0), dx.reshape(B * Tin, cin), dW_abs


def first_fwd_ref(wav, W, b, lengths=None):
    """Layer 0 from the waveform [B, N] -> z [B, T, 40]; lengths: samples past them count as zero, rows past the
    utterance's own frames are zero."""
    k, s, p = FIRST
    wav = wav.to(F64)
    if lengths is not None:
        wav = wav * (torch.arange(wav.shape[1])[None] < torch.tensor(lengths)[:, None])
    z = F.conv1d(wav[:, None], W.to(F64), b.to(F64), stride=s, padding=p).transpose(1, 2).contiguous()
    if lengths is not None:
        own = torch.tensor([frames_of(n, k, s, p) for n in lengths])
        z = z * (torch.arange(z.shape[1])[None] < own[:, None])[..., None]
    return z


def instnorm_relu_ref(z, lengths=None):
    """z [B, T, C] -> dict(y, mean [B, C], var (biased), rstd); lengths: statistics over each utterance's own frames, zero
    rows past them."""
    z = z.to(F64)
    B, T, C = z.shape
    y = torch.zeros_like(z)
    mean, var = torch.zeros(B, C, dtype=F64), torch.zeros(B, C, dtype=F64)
    for b in range(B):
        n = T if lengths is None else lengths[b]
        mean[b] = z[b, :n].mean(0)
        var[b] = ((z[b, :n] - mean[b]) ** 2).mean(0)
        y[b, :n] = ((z[b, :n] - mean[b]) * (var[b] + IN_EPS) ** -0.5).clamp_min(0)
    return {"y": y, "mean": mean, "var": var, "rstd": (var + IN_EPS) ** -0.5}


def instnorm_relu_apply_ref(z, mean_rstd):
    """The normalisation alone, with the statistics a kernel stored (mean_rstd [B, C, 2])."""
    m = mean_rstd.to(F64)
    return ((z.to(F64) - m[:, None, :, 0]) * m[:, None, :, 1]).clamp_min(0)


def instnorm_relu_bwd_ref(z, y, dy, stats=None):
    """-> dict(dz, m1, m2, m1_abs, m2_abs, dz_abs): m1 = mean_t g, m2 = mean_t (g zhat), g = dy where y > 0; the *_abs are
    the sums of the |terms| (dz is a three-term difference).  stats = mean_rstd [B, C, 2] the forward stored."""
    z, g = z.to(F64), torch.where(y > 0, dy.to(F64), torch.zeros((), dtype=F64))
    if stats is None:
        f = instnorm_relu_ref(z)
        mean, rstd = f["mean"], f["rstd"]
    else:
        mean, rstd = stats[..., 0].to(F64), stats[..., 1].to(F64)
    zh = (z - mean[:, None]) * rstd[:, None]
    m1, m2 = g.mean(1), (g * zh).mean(1)
    dz = rstd[:, None] * (g - m1[:, None] - zh * m2[:, None])
    dz_abs = rstd[:, None].abs() * (g.abs() + m1[:, None].abs() + (zh * m2[:, None]).abs())
    return {"dz": dz, "m1": m1, "m2": m2, "m1_abs": g.abs().mean(1), "m2_abs": (g * zh).abs().mean(1), "dz_abs": dz_abs}


def gate_fwd_ref(x, W, b):
    """x [M, F] -> (P, y): P = x W^T + b, y = sigmoid(P) * x."""
    x = x.to(F64)
    P = x @ W.to(F64).t() + b.to(F64).view(-1)
    return P, torch.sigmoid(P) * x


def gate_bwd_ref(x, W, P, dy):
    """-> (dW, db, dx, dP, dx_direct, db_abs)."""
    x, W, P, dy = x.to(F64), W.to(F64), P.to(F64), dy.to(F64)
    s = torch.sigmoid(P)
    dP, direct = dy * x * s * (1 - s), dy * s
    return dP.t() @ x, dP.sum(0), direct + dP @ W, dP, direct, dP.abs().sum(0)


def pool_fwd_ref(x, pooling, lengths=None):
    """x [B, T, C] -> cat(std unbiased, mean) ("mean+std", torch.std_mean's order) or the mean."""
    x = x.to(F64)
    rows = [x[b, :(x.shape[1] if lengths is None else lengths[b])] for b in range(x.shape[0])]
    mean = torch.stack([r.mean(0) for r in rows])
    if pooling == "mean":
        return mean
    std = torch.stack([((r - r.mean(0)) ** 2).sum(0).div(r.shape[0] - 1).sqrt() for r in rows])
    return torch.cat([std, mean], 1)


def pool_bwd_ref(x, dout, pooling):
    x, dout = x.to(F64), dout.to(F64)
    n, C = x.shape[1], x.shape[2]
    if pooling == "mean":
        return (dout[:, None] / n).expand_as(x).clone()
    mean = x.mean(1, keepdim=True)
    std = ((x - mean) ** 2).sum(1, keepdim=True).div(n - 1).sqrt()
    second = dout[:, None, :C] * (x - mean) / ((n - 1) * std)
    return dout[:, None, C:] / n + torch.where((std > 0).expand_as(second), second, torch.zeros_like(second))


def ce_ref(logits, label):
    """-> (loss, log-probabilities, dlogits) of the mean cross-entropy."""
    z = logits.to(F64)
    lp = torch.log_softmax(z, 1)
    onehot = F.one_hot(label, z.shape[1]).to(F64)
    return -(lp * onehot).sum(1).mean(), lp, (lp.exp() - onehot) / z.shape[0]


# ------------------------------------------------------------------------------------------------ the chain
def stage_names(gating: bool):
    return ([f"encoder.{i}" for i in range(5)] + (["temporal_gate"] if gating else []) + [f"aggregator.{i}" for i in range(4)]
            + ["pooled"] + [f"fc.{i}" for i in range(len(HIDDEN))] + ["logprob"])


def forward_ref(sd, wav, label, gating=True, pooling="mean+std", dtype=F64):
    """The training forward -> record of every stage's tensors ([B*T, C] layout before the pooling).  ``dtype`` float32
    runs the same stack in torch f32 (the measure of what f32 arithmetic costs end to end)."""
    sd = {n: v.to(dtype) for n, v in sd.items()}
    B, N = wav.shape
    rec = {"B": B, "N": N, "gating": gating, "pooling": pooling, "z": [], "y": [], "T": [], "stage": OrderedDict()}
    rec["wav"] = x = wav.to(dtype).view(B * N, 1)
    Tin = N
    for i, (cin, cout, k, s, p) in enumerate(ENCODER):
        z = _conv(x, sd[f"encoder.{i}.0.weight"], sd[f"encoder.{i}.0.bias"], B, Tin, s, p, dtype)
        Tin = frames_of(Tin, k, s, p)
        y = _instnorm(z.view(B, Tin, cout), dtype).reshape(B * Tin, cout)
        rec["z"].append(z), rec["y"].append(y), rec["T"].append(Tin)
        rec["stage"][f"encoder.{i}"] = x = y
    T = Tin
    rec["enc_out"] = x
    if gating:
        Wg, bg = sd["temporal_gate.W"], sd["temporal_gate.b"]
        rec["P"] = x @ Wg.t() + bg.view(-1)
        rec["stage"]["temporal_gate"] = x = torch.sigmoid(rec["P"]) * x
    rec["agg_in"], rec["agg"] = [], []
    for i, (cin, cout, k, s, p) in enumerate(AGGREGATOR):
        rec["agg_in"].append(x)
        x = _conv(x, sd[f"aggregator.{i}.0.weight"], sd[f"aggregator.{i}.0.bias"], B, T, s, p, dtype).clamp_min(0)
        rec["agg"].append(x)
        rec["stage"][f"aggregator.{i}"] = x
    x3 = x.view(B, T, FEATURES)
    if dtype == F64:
        rec["pooled"] = pool_fwd_ref(x3, pooling)
    else:
        rec["pooled"] = torch.cat(torch.std_mean(x3, 1), 1) if pooling == "mean+std" else x3.mean(1)
    rec["stage"]["pooled"] = h = rec["pooled"]
    rec["fc"] = [h]
    for i in range(len(HIDDEN)):
        h = (h @ sd[f"fc_list.{i}.0.weight"].t() + sd[f"fc_list.{i}.0.bias"]).clamp_min(0)
        rec["fc"].append(h)
        rec["stage"][f"fc.{i}"] = h
    n = len(HIDDEN)
    rec["logits"] = h @ sd[f"fc_list.{n}.0.weight"].t() + sd[f"fc_list.{n}.0.bias"]
    rec["loss"], rec["logprob"], rec["dlogits"] = ce_ref(rec["logits"], label)
    rec["stage"]["logprob"] = rec["logprob"]
    return rec


def _conv(x, W, b, B, Tin, s, p, dtype):
    if dtype == F64:
        return conv_fwd_ref(x, W, b, B, Tin, s, p)
    z = F.conv1d(x.view(B, Tin, -1).transpose(1, 2), W, b, stride=s, padding=p)
    return z.transpose(1, 2).reshape(-1, W.shape[0])


def _instnorm(z, dtype):
    if dtype == F64:
        return instnorm_relu_ref(z)["y"]
    return F.relu(F.instance_norm(z.transpose(1, 2), eps=IN_EPS)).transpose(1, 2)


def embedding_of(rec, idx: int):
    """ref: wav2spk.py:235-252: -1 the pooled vector, i the post-ReLU output of hidden layer i, len(hidden) the
    log-probabilities."""
    return rec["pooled"] if idx < 0 else rec["fc"][idx + 1] if idx < len(HIDDEN) else rec["logprob"]


def backward_ref(sd, rec):
    """The hand-derived backward chain over a float64 forward_ref record -> {parameter name: gradient}.  The encoder's conv
    biases get exact zeros: InstanceNorm removes a per-channel constant."""
    sd = {n: v.to(F64) for n, v in sd.items()}
    B, T, G = rec["B"], rec["T"][-1], {}
    n = len(HIDDEN)
    d = rec["dlogits"]
    for i in range(n, -1, -1):
        W = sd[f"fc_list.{i}.0.weight"]
        if i < n:
            d = d * (rec["fc"][i + 1] > 0)
        G[f"fc_list.{i}.0.weight"], G[f"fc_list.{i}.0.bias"] = d.t() @ rec["fc"][i], d.sum(0)
        d = d @ W
    d = pool_bwd_ref(rec["agg"][-1].view(B, T, FEATURES), d, rec["pooling"]).reshape(B * T, FEATURES)
    for i in range(len(AGGREGATOR) - 1, -1, -1):
        _, _, k, s, p = AGGREGATOR[i]
        dz = d * (rec["agg"][i] > 0)
        G[f"aggregator.{i}.0.weight"], G[f"aggregator.{i}.0.bias"], d, _ = conv_bwd_ref(
            rec["agg_in"][i], sd[f"aggregator.{i}.0.weight"], dz, B, T, s, p)
    if rec["gating"]:
        dW, db, d, _, _, _ = gate_bwd_ref(rec["enc_out"], sd["temporal_gate.W"], rec["P"], d)
        G["temporal_gate.W"], G["temporal_gate.b"] = dW, db.view(-1, 1)
    else:
        G["temporal_gate.W"], G["temporal_gate.b"] = torch.zeros(FEATURES, FEATURES, dtype=F64), torch.zeros(FEATURES, 1, dtype=F64)
    Tins = [rec["N"]] + rec["T"][:-1]
    for i in range(len(ENCODER) - 1, -1, -1):
        cin, cout, k, s, p = ENCODER[i]
        Ti = rec["T"][i]
        o = instnorm_relu_bwd_ref(rec["z"][i].view(B, Ti, cout), rec["y"][i].view(B, Ti, cout), d.view(B, Ti, cout))
        x = rec["y"][i - 1] if i > 0 else rec["wav"]
        G[f"encoder.{i}.0.weight"], _, d, _ = conv_bwd_ref(x, sd[f"encoder.{i}.0.weight"], o["dz"].reshape(B * Ti, cout), B,
                                                            Tins[i], s, p)
        G[f"encoder.{i}.0.bias"] = torch.zeros(cout, dtype=F64)
    return G


def torch_grads(sd, wav, label, gating, pooling, dtype):
    """Autograd gradients of forward_ref's loss in ``dtype`` -> (record, {name: gradient})."""
    leaves = {n: v.to(dtype).clone().requires_grad_(True) for n, v in sd.items()}
    rec = forward_ref(leaves, wav, label, gating, pooling, dtype)
    rec["loss"].backward()
    return rec, {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in leaves.items()}


def adam_ref(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam (no weight decay) in float64, in place on the moments -> the new parameter."""
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    return p - lr / (1 - beta1 ** step) * m / ((v / (1 - beta2 ** step)).sqrt() + eps)
