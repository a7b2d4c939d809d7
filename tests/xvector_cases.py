"""Geometries and float64 references for the stages of the x-vector path (w2v2_speaker_amd/xvector.py on csrc/tdnn.hip and the
GEMMs), shared by tests/test_xvector_cpu.py and tests/test_xvector_gpu.py.  No GPU and no ``ops`` import here: everything
is plain torch on the CPU in float64.

One function per stage, each taking the stage's own operands as the plan stores them ([B*T, C] matrices, channels
last) and written from the model's definition (speechbrain 0.5.x as recollected, see xvector.py) with a hand-derived
backward.  ``forward_ref`` / ``backward_ref`` string the stages together; tests/test_xvector_cpu.py compares that chain with
float64 autograd over torch's own modules, so a sign or index error in a stage reference cannot agree with a kernel that
has the same error."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from ecapa_stage_cases import F32_BOUND, im2col_reflect, pack_conv_weight, rel_l2, sum_scale_error, unpack_conv_grad  # noqa: F401

F64 = torch.float64
BN_EPS, BN_MOMENTUM, POOL_EPS, SLOPE = 1e-5, 0.1, 1e-5, 0.01
FE, CLS = "feature_extractor.", "classifier."

# the tiny model: 44 % 8 = 4 mirrors the 1500 % 8 = 4 of the reference's last TDNN layer
MELS, CHANNELS, KERNEL_SIZES, DILATIONS, LIN, SPEAKERS = 8, (16, 16, 16, 16, 44), (5, 3, 3, 1, 1), (1, 2, 3, 1, 1), 16, 7
B, T = 3, 100

# LeakyReLU -> BatchNorm kernels: rows M (the classifier's batch rows; both sides of a 256-row partial block; a ragged
# second block) x channels C (one 16-byte vector short of a multiple of 8; more than one 128-channel strip)
BN_ROWS = (2, 255, 257, 300)
BN_CHANNELS = (44, 136)
# statistics pool: T = 2 the minimum of an unbiased std, 7 fewer than the 8 time lanes, 17 more than one lane round, 100 more
# than one round of 8 lanes x 4 frames with a ragged tail; C = 44 inside a row stride of 48
POOL_FRAMES = (2, 7, 17, 100)
POOL_C, POOL_LD = 44, 48


def param_shapes(mels=MELS, channels=CHANNELS, kernel_sizes=KERNEL_SIZES, lin=LIN, speakers=SPEAKERS):
    """The state-dict names and shapes of the model, written out independently of xvector.xvector_param_shapes."""
    s = OrderedDict()
    cin = mels
    for i, (c, k) in enumerate(zip(channels, kernel_sizes)):
        s[f"{FE}blocks.{3 * i}.conv.weight"] = (c, cin, k)
        s[f"{FE}blocks.{3 * i}.conv.bias"] = (c,)
        s[f"{FE}blocks.{3 * i + 2}.norm.weight"] = (c,)
        s[f"{FE}blocks.{3 * i + 2}.norm.bias"] = (c,)
        cin = c
    s[f"{FE}blocks.{3 * len(channels) + 1}.w.weight"] = (lin, 2 * cin)
    s[f"{FE}blocks.{3 * len(channels) + 1}.w.bias"] = (lin,)
    s[CLS + "norm.norm.weight"] = (lin,)
    s[CLS + "norm.norm.bias"] = (lin,)
    s[CLS + "DNN.block_0.linear.w.weight"] = (lin, lin)
    s[CLS + "DNN.block_0.linear.w.bias"] = (lin,)
    s[CLS + "DNN.block_0.norm.norm.weight"] = (lin,)
    s[CLS + "DNN.block_0.norm.norm.bias"] = (lin,)
    s[CLS + "out.w.weight"] = (speakers, lin)
    s[CLS + "out.w.bias"] = (speakers,)
    return s


def make_state_dict(seed: int, **kw):
    """Random parameters with every bias, scale and shift away from its default (f32 values)."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for n, shp in param_shapes(**kw).items():
        if n.endswith("norm.weight"):
            t = 1.0 + 0.2 * torch.randn(shp, generator=g)
        elif n.endswith("bias"):
            t = 0.1 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            t = torch.randn(shp, generator=g) / fan_in ** 0.5
        sd[n] = t.float()
    return sd


def inputs(seed: int, batch=B, frames=T, mels=MELS, speakers=SPEAKERS):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, frames, mels, generator=g), torch.randint(0, speakers, (batch,), generator=g)


# ------------------------------------------------------------------------------------------------ stages
def leaky(a):
    return torch.where(a > 0, a, SLOPE * a)


def leaky_grad(a):
    """torch's convention: slope 0.01 at a == 0."""
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))


def conv_fwd_ref(x, W, b, batch, frames, k, d):
    """x [B*T, cin], W torch layout [cout, cin, k] -> a [B*T, cout]: Conv1d("same", reflect padding, dilation d) + bias."""
    col = im2col_reflect(x.to(F64).view(batch, frames, -1), k, d)
    return col @ pack_conv_weight(W.to(F64)).t() + b.to(F64)


def conv_bwd_ref(x, W, da, batch, frames, k, d):
    """-> (dW [cout, cin, k], db [cout], dx [B*T, cin]), the gather's adjoint written as a scatter-add."""
    x, W, da = x.to(F64), W.to(F64), da.to(F64)
    cin = x.shape[1]
    col = im2col_reflect(x.view(batch, frames, cin), k, d)
    dW = unpack_conv_grad(da.t() @ col, cin, k)
    dcol = (da @ pack_conv_weight(W)).view(batch, frames, k, cin)
    dx = torch.zeros(batch, frames, cin, dtype=F64)
    t = torch.arange(frames)
    for j in range(k):
        p = (t + (j - (k - 1) // 2) * d).abs()
        p = torch.where(p >= frames, 2 * (frames - 1) - p, p)
        dx.index_add_(1, p, dcol[:, :, j])
    return dW, da.sum(0), dx.view(batch * frames, cin)


def act_bn_fwd_ref(a, gamma, beta):
    """BatchNorm1d(LeakyReLU(a)) over the rows of a [M, C] with batch statistics -> dict(y, mu, var, rstd)."""
    r = leaky(a.to(F64))
    mu = r.mean(0)
    var = ((r - mu) ** 2).mean(0)
    rstd = (var + BN_EPS) ** -0.5
    return {"y": (r - mu) * rstd * gamma.to(F64) + beta.to(F64), "mu": mu, "var": var, "rstd": rstd}


def act_bn_apply_ref(a, gamma, beta, mean_rstd):
    """The normalisation alone, with the statistics a kernel stored (mean_rstd [C, 2])."""
    return (leaky(a.to(F64)) - mean_rstd[:, 0].to(F64)) * mean_rstd[:, 1].to(F64) * gamma.to(F64) + beta.to(F64)


def act_bn_eval_ref(a, gamma, beta, running_mean, running_var):
    r = leaky(a.to(F64))
    return (r - running_mean.to(F64)) * (running_var.to(F64) + BN_EPS) ** -0.5 * gamma.to(F64) + beta.to(F64)


def running_ref(running_mean, running_var, mu, var, M):
    """torch's update: momentum 0.1, the unbiased batch variance."""
    unb = var * M / (M - 1) if M > 1 else var
    return ((1 - BN_MOMENTUM) * running_mean.to(F64) + BN_MOMENTUM * mu,
            (1 - BN_MOMENTUM) * running_var.to(F64) + BN_MOMENTUM * unb)


def act_bn_bwd_ref(a, gamma, dy, stats=None):
    """-> dict(da, dgamma, dbeta, dgamma_abs, dbeta_abs, da_abs, db, db_abs): db = the column sums of da (the bias gradient
    of the layer that wrote a); the *_abs are the sums of the |terms| (da_abs per element: da is a three-term difference
    that cancels to nearly nothing over a handful of rows).  stats = (mean, rstd): the statistics the forward stored,
    which the backward kernel reads; None: recomputed here."""
    a, gamma, g = a.to(F64), gamma.to(F64), dy.to(F64)
    if stats is None:
        f = act_bn_fwd_ref(a, gamma, torch.zeros_like(gamma))
        mu, rstd = f["mu"], f["rstd"]
    else:
        mu, rstd = stats[0].to(F64), stats[1].to(F64)
    xh = (leaky(a) - mu) * rstd
    m1, m2 = g.mean(0), (g * xh).mean(0)
    slope = leaky_grad(a)
    da = gamma * rstd * (g - m1 - xh * m2) * slope
    da_abs = (gamma * rstd).abs() * (g.abs() + m1.abs() + (xh * m2).abs()) * slope
    return {"da": da, "dgamma": (g * xh).sum(0), "dbeta": g.sum(0), "dgamma_abs": (g * xh).abs().sum(0),
            "dbeta_abs": g.abs().sum(0), "da_abs": da_abs, "db": da.sum(0), "db_abs": da.abs().sum(0)}


def variance_error(mean_rstd, a):
    """The batch variance a kernel stored as rstd = (var + eps)^-1/2 against float64, as a sum whose terms cancel:
    var + eps = E[r^2] - mean^2 + eps, r = LeakyReLU(a); max over the channels of |error| / (E[r^2] + mean^2 + eps)."""
    r = leaky(a.to(F64))
    mu, ms = r.mean(0), (r * r).mean(0)
    return sum_scale_error(mean_rstd[:, 1].to(F64) ** -2, ((r - mu) ** 2).mean(0) + BN_EPS, ms + mu * mu + BN_EPS)


def stat_pool_fwd_ref(x, lengths=None):
    """x [B, T, C] -> (mean [B, C], std [B, C] unbiased, out [B, 2C] = cat(mean, std + eps)); lengths: frames per utterance."""
    x = x.to(F64)
    rows = [x[b, :(x.shape[1] if lengths is None else lengths[b])] for b in range(x.shape[0])]
    mean = torch.stack([r.mean(0) for r in rows])
    std = torch.stack([((r - r.mean(0)) ** 2).sum(0).div(r.shape[0] - 1).sqrt() for r in rows])
    return mean, std, torch.cat([mean, std + POOL_EPS], 1)


def stat_pool_bwd_ref(x, dout):
    """dx = dmean / T + dstd (x - mean) / ((T - 1) std); the second term is 0 where std = 0 (torch's std backward)."""
    x, dout = x.to(F64), dout.to(F64)
    n, C = x.shape[1], x.shape[2]
    mean, std, _ = stat_pool_fwd_ref(x)
    second = dout[:, None, C:] * (x - mean[:, None]) / ((n - 1) * std[:, None])
    return dout[:, None, :C] / n + torch.where((std > 0)[:, None].expand_as(second), second, torch.zeros_like(second))


def linear_fwd_ref(x, W, b):
    return x.to(F64) @ W.to(F64).t() + b.to(F64)


def linear_bwd_ref(x, W, dy):
    """-> (dW, db, dx, db_abs)."""
    x, W, dy = x.to(F64), W.to(F64), dy.to(F64)
    return dy.t() @ x, dy.sum(0), dy @ W, dy.abs().sum(0)


def ce_ref(logits, label):
    """-> (loss, softmax, dlogits) of the mean cross-entropy."""
    z = logits.to(F64)
    p = torch.softmax(z, 1)
    onehot = F.one_hot(label, z.shape[1]).to(F64)
    loss = -(torch.log_softmax(z, 1) * onehot).sum(1).mean()
    return loss, p, (p - onehot) / z.shape[0]


# ------------------------------------------------------------------------------------------------ the chain
def _names(n_blocks):
    return [(f"{FE}blocks.{3 * i}.conv.", f"{FE}blocks.{3 * i + 2}.norm.") for i in range(n_blocks)], f"{FE}blocks.{3 * n_blocks + 1}.w."


def forward_ref(sd, feat, label, kernel_sizes=KERNEL_SIZES, dilations=DILATIONS):
    """The training forward in float64 -> record of every stage's tensors ([B*T, C] layout before the pooling)."""
    sd = {n: v.to(F64) for n, v in sd.items()}
    batch, frames = feat.shape[:2]
    blocks, lin = _names(len(kernel_sizes))
    rec = {"x": [feat.to(F64).reshape(batch * frames, -1)], "a": [], "bn": [], "B": batch, "T": frames}
    for (cn, nn_), k, d in zip(blocks, kernel_sizes, dilations):
        a = conv_fwd_ref(rec["x"][-1], sd[cn + "weight"], sd[cn + "bias"], batch, frames, k, d)
        f = act_bn_fwd_ref(a, sd[nn_ + "weight"], sd[nn_ + "bias"])
        rec["a"].append(a)
        rec["bn"].append(f)
        rec["x"].append(f["y"])
    x5 = rec["x"][-1].view(batch, frames, -1)
    rec["mean"], rec["std"], rec["pooled"] = stat_pool_fwd_ref(x5)
    rec["emb"] = linear_fwd_ref(rec["pooled"], sd[lin + "weight"], sd[lin + "bias"])
    rec["h1"] = act_bn_fwd_ref(rec["emb"], sd[CLS + "norm.norm.weight"], sd[CLS + "norm.norm.bias"])["y"]
    rec["z"] = linear_fwd_ref(rec["h1"], sd[CLS + "DNN.block_0.linear.w.weight"], sd[CLS + "DNN.block_0.linear.w.bias"])
    rec["h2"] = act_bn_fwd_ref(rec["z"], sd[CLS + "DNN.block_0.norm.norm.weight"], sd[CLS + "DNN.block_0.norm.norm.bias"])["y"]
    rec["logits"] = linear_fwd_ref(rec["h2"], sd[CLS + "out.w.weight"], sd[CLS + "out.w.bias"])
    rec["loss"], rec["softmax"], rec["dlogits"] = ce_ref(rec["logits"], label)
    return rec


def backward_ref(sd, rec, kernel_sizes=KERNEL_SIZES, dilations=DILATIONS):
    """The hand-derived backward chain over a forward_ref record -> {parameter name: gradient}."""
    sd = {n: v.to(F64) for n, v in sd.items()}
    batch, frames = rec["B"], rec["T"]
    blocks, lin = _names(len(kernel_sizes))
    G = {}
    n = CLS + "out.w."
    G[n + "weight"], G[n + "bias"], dh2, _ = linear_bwd_ref(rec["h2"], sd[n + "weight"], rec["dlogits"])
    o = act_bn_bwd_ref(rec["z"], sd[CLS + "DNN.block_0.norm.norm.weight"], dh2)
    G[CLS + "DNN.block_0.norm.norm.weight"], G[CLS + "DNN.block_0.norm.norm.bias"] = o["dgamma"], o["dbeta"]
    n = CLS + "DNN.block_0.linear.w."
    G[n + "weight"], G[n + "bias"], dh1, _ = linear_bwd_ref(rec["h1"], sd[n + "weight"], o["da"])
    o = act_bn_bwd_ref(rec["emb"], sd[CLS + "norm.norm.weight"], dh1)
    G[CLS + "norm.norm.weight"], G[CLS + "norm.norm.bias"] = o["dgamma"], o["dbeta"]
    G[lin + "weight"], G[lin + "bias"], dpooled, _ = linear_bwd_ref(rec["pooled"], sd[lin + "weight"], o["da"])
    dx = stat_pool_bwd_ref(rec["x"][-1].view(batch, frames, -1), dpooled).reshape(batch * frames, -1)
    for i in range(len(kernel_sizes) - 1, -1, -1):
        cn, nn_ = blocks[i]
        o = act_bn_bwd_ref(rec["a"][i], sd[nn_ + "weight"], dx)
        G[nn_ + "weight"], G[nn_ + "bias"] = o["dgamma"], o["dbeta"]
        G[cn + "weight"], G[cn + "bias"], dx = conv_bwd_ref(rec["x"][i], sd[cn + "weight"], o["da"], batch, frames,
                                                            kernel_sizes[i], dilations[i])
    return G
