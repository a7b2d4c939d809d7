"""Geometries and float64 references for the stages of the ECAPA-TDNN backward (w2v2_speaker_amd/ecapa.py on csrc/tdnn.hip,
csrc/skinny.hip and the GEMMs), shared by tests/test_ecapa_stages_cpu.py, tests/test_ecapa_stages_gpu.py and
tools/ecapa_stage_parity.py.  No GPU and no ``ops`` import here: everything is plain torch on the CPU in float64.

One function per stage, each taking the stage's own operands as the plan stores them ([B*T, C] matrices, channels
last).  ``forward_record`` / ``chain_backward`` string the stages together in the plan's order over an f64 forward built
from the pieces of ``oracle.ecapa_oracle``; tests/test_ecapa_stages_cpu.py compares that chain with autograd of the oracle
(which the goldens pin), so a sign or index error in a stage reference cannot agree with a kernel that has the same error."""
import torch
import torch.nn.functional as F

F64 = torch.float64
BN_EPS = 1e-5
F32_BOUND = 2e-5        # the bound of the least exact f32 stage the suite already holds (bn_bwd in test_batchnorm_kernels_vs_torch)

KERNEL_SIZES, DILATIONS = (5, 3, 3, 3, 1), (1, 2, 3, 4, 1)
# name -> (config fields shared by ecapa.EcapaConfig and the oracle's, mel bins, B, T)
#   tiny:   M = 111 is no multiple of 64: the zero-padded tail of every row-padded buffer is in play
#   narrow: w = 128 / 8 = 16, the narrowest slice with C % 8 == 0; seven chunks per block run the two-operand BatchNorm
#           backward six times; M = 265
GEOMETRIES = {
    "tiny": (dict(lin_neurons=24, channels=(64, 64, 64, 64, 192), attention_channels=16, res2net_scale=4, se_channels=16),
             16, 3, 37),
    "narrow": (dict(lin_neurons=48, channels=(128, 128, 128, 128, 384), attention_channels=32, res2net_scale=8,
                    se_channels=32), 24, 5, 53),
}
CLASSES = 9


def oracle_config(name: str):
    from oracle import ecapa_oracle as E
    kw, mels, _, _ = GEOMETRIES[name]
    return E.EcapaConfig(input_size=mels, kernel_sizes=KERNEL_SIZES, dilations=DILATIONS, **kw)


def inputs(name: str, seed: int):
    """-> (feat [B, T, mels] f32, label [B])."""
    _, mels, B, T = GEOMETRIES[name]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, mels, generator=g), torch.randint(0, CLASSES, (B,), generator=g)


# ------------------------------------------------------------------------------------------------ measures and bounds
def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.to(F64), ref.to(F64)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def rounding_floor(ref: torch.Tensor, dtype: torch.dtype) -> float:
    """rel-L2 distance between the reference and itself rounded once to ``dtype``: what a perfect kernel that stores
    ``dtype`` still shows.  Zero for f32 outputs (their rounding is inside F32_BOUND)."""
    if dtype == torch.float32:
        return 0.0
    return rel_l2(ref.to(torch.float32).to(dtype), ref)


def stage_bound(ref: torch.Tensor, dtype: torch.dtype, roundings: int) -> float:
    """2 * r * floor + F32_BOUND: r roundings to the stored dtype between the stored inputs and the stored output, the
    factor 2 the margin over an RMS floor, F32_BOUND the f32 accumulation."""
    return 2.0 * roundings * rounding_floor(ref, dtype) + F32_BOUND


def sum_scale_error(got: torch.Tensor, ref: torch.Tensor, sum_abs: torch.Tensor) -> float:
    """max over the elements of |got - ref| / sum(|terms|): the measure of sums whose terms cancel (0 / 0 counts as 0,
    a non-zero error over a zero scale as inf)."""
    err, scale = (got.to(F64) - ref.to(F64)).abs(), sum_abs.to(F64)
    q = torch.where(err == 0, torch.zeros_like(err), err / scale)
    return float(q.max())


# ------------------------------------------------------------------------------------------------ layouts
def pack_conv_weight(W: torch.Tensor) -> torch.Tensor:
    """torch [cout][cin][tap] -> the GEMM operand [cout][tap * cin + c]."""
    return W.permute(0, 2, 1).reshape(W.shape[0], -1)


def unpack_conv_grad(dwp: torch.Tensor, cin: int, k: int) -> torch.Tensor:
    return dwp.reshape(dwp.shape[0], k, cin).permute(0, 2, 1)


def im2col_reflect(x_btc: torch.Tensor, k: int, d: int) -> torch.Tensor:
    """[B, T, C] -> [B*T, k*C]: tap j of row t is frame t + (j - (k-1)/2) d, reflected at both ends (differentiable)."""
    B, T, C = x_btc.shape
    p = d * (k - 1) // 2
    xp = F.pad(x_btc.transpose(1, 2), (p, p), mode="reflect").transpose(1, 2) if p > 0 else x_btc
    return torch.stack([xp[:, j * d:j * d + T] for j in range(k)], dim=2).reshape(B * T, k * C)


def col2im_reflect(dcol: torch.Tensor, B: int, T: int, C: int, k: int, d: int) -> torch.Tensor:
    """Adjoint of im2col_reflect by autograd: [B*T, k*C] -> [B*T, C]."""
    x = torch.zeros(B, T, C, dtype=F64, requires_grad=True)
    (im2col_reflect(x, k, d) * dcol.to(F64)).sum().backward()
    return x.grad.reshape(B * T, C)


# ------------------------------------------------------------------------------------------------ TDNN block
def bn_bwd_ref(a, gamma, dy, dy2=None):
    """Backward of BatchNorm1d(relu(a)) over the rows of a [M, C], from the saved pre-activation: output gradient
    dy (+ dy2).  -> dict(da, dgamma, dbeta, mu, rstd, dgamma_abs, dbeta_abs); the *_abs are the sums of the |terms|."""
    a, gamma, g = a.to(F64), gamma.to(F64), dy.to(F64)
    if dy2 is not None:
        g = g + dy2.to(F64)
    r = a.clamp_min(0)
    mu = r.mean(0)
    var = ((r - mu) ** 2).mean(0)
    rstd = (var + BN_EPS) ** -0.5
    xh = (r - mu) * rstd
    da = gamma * rstd * (g - g.mean(0) - xh * (g * xh).mean(0)) * (a > 0)
    return {"da": da, "dgamma": (g * xh).sum(0), "dbeta": g.sum(0), "mu": mu, "rstd": rstd,
            "dgamma_abs": (g * xh).abs().sum(0), "dbeta_abs": g.abs().sum(0)}


def tdnn_dx_ref(da, wp, B: int, T: int, cin: int, k: int, d: int):
    """-> (dcol [M, k*cin] or None for k == 1, dx [M, cin]) of conv = im2col_reflect + GEMM with the packed weight wp."""
    dcol = da.to(F64) @ wp.to(F64)
    if k == 1:
        return None, dcol
    return dcol, col2im_reflect(dcol, B, T, cin, k, d)


# ------------------------------------------------------------------------------------------------ SE block
def se_fwd_ref(x_btc, W1, b1, W2, b2):
    """-> (s [B, C] time mean, z [B, S] = relu(W1 s + b1), g [B, C] = sigmoid(W2 z + b2))."""
    s = x_btc.to(F64).mean(1)
    z = (s @ W1.to(F64).t() + b1.to(F64)).clamp_min(0)
    g = torch.sigmoid(z @ W2.to(F64).t() + b2.to(F64))
    return s, z, g


def se_bwd_ref(x_btc, d_se_btc, s, z, g, W1, W2, dg=None, dz=None, ds=None):
    """Backward of y = x * g(x) from the saved s, z, g.  dg / dz / ds: the stored value of that intermediate; when given,
    the stages behind it are evaluated from it instead of from this function's own (so each is checked on its own inputs).
    -> dict(dg, dg_abs, dW2, db2, db2_abs, dz, dW1, db1, db1_abs, ds, d_t2)."""
    x, d, s, z, g, W1, W2 = (t.to(F64) for t in (x_btc, d_se_btc, s, z, g, W1, W2))
    T = x.shape[1]
    o = {"dg": (d * x).sum(1), "dg_abs": (d * x).abs().sum(1)}
    dg_ = o["dg"] if dg is None else dg.to(F64)
    u = dg_ * g * (1 - g)
    o.update(dW2=u.t() @ z, db2=u.sum(0), db2_abs=u.abs().sum(0), dz=u @ W2)
    dz_ = o["dz"] if dz is None else dz.to(F64)
    v = dz_ * (z > 0)
    o.update(dW1=v.t() @ s, db1=v.sum(0), db1_abs=v.abs().sum(0), ds=v @ W1)
    ds_ = o["ds"] if ds is None else ds.to(F64)
    o["d_t2"] = d * g[:, None] + ds_[:, None] / T
    return o


# ------------------------------------------------------------------------------------------------ the chain (CPU test)
def forward_record(feat, sd, cfg):
    """f64 forward from the oracle's own pieces up to the MFA output, keeping per TDNN block what the plan keeps (its
    input x [B, T, cin] and pre-activation a) and per SE block (t2, s, z, g).  -> (record, mfa_out [B, T, C])."""
    from oracle import ecapa_oracle as E
    rec = {}

    def tdnn(p, x, dil):
        a = E.conv1d_same_reflect(x, sd[p + "conv.conv.weight"], sd[p + "conv.conv.bias"], dil)
        rec[p] = {"x": x, "a": a, "dil": dil}
        return E.batchnorm_train(F.relu(a), sd[p + "norm.norm.weight"], sd[p + "norm.norm.bias"])

    sc = cfg.res2net_scale
    x = tdnn("blocks.0.", feat, cfg.dilations[0])
    outs = []
    for i in range(1, len(cfg.channels) - 1):
        p = f"blocks.{i}."
        t1 = tdnn(p + "tdnn1.", x, 1)
        ys = []
        for j, xj in enumerate(torch.chunk(t1, sc, dim=2)):
            if j == 0:
                ys.append(xj)
            else:
                ys.append(tdnn(p + f"res2net_block.blocks.{j - 1}.", xj if j == 1 else xj + ys[-1], cfg.dilations[i]))
        t2 = tdnn(p + "tdnn2.", torch.cat(ys, dim=2), 1)
        q = p + "se_block."
        s, z, g = se_fwd_ref(t2, sd[q + "conv1.conv.weight"][:, :, 0], sd[q + "conv1.conv.bias"],
                             sd[q + "conv2.conv.weight"][:, :, 0], sd[q + "conv2.conv.bias"])
        rec[q] = {"x": t2, "s": s, "z": z, "g": g}
        x = t2 * g[:, None] + x
        outs.append(x)
    return rec, tdnn("mfa.", torch.cat(outs, dim=2), cfg.dilations[-1])


def chain_backward(rec, sd, cfg, d_mfa):
    """The stage references above in the plan's order, from d(loss)/d(MFA output) [B*T, C] down to the features.
    -> (gradient of every TDNN / BatchNorm / SE parameter by name, d_feat [B*T, mels])."""
    grads = {}
    C1, sc = cfg.channels[1], cfg.res2net_scale
    w = C1 // sc
    nb = len(cfg.channels) - 2

    def tdnn_bwd(p, dy, dy2=None):
        x, a, dil = rec[p]["x"], rec[p]["a"], rec[p]["dil"]
        B, T, cin = x.shape
        W = sd[p + "conv.conv.weight"]
        k = W.shape[2]
        o = bn_bwd_ref(a.reshape(B * T, -1), sd[p + "norm.norm.weight"], dy, dy2)
        grads[p + "norm.norm.weight"], grads[p + "norm.norm.bias"] = o["dgamma"], o["dbeta"]
        A = im2col_reflect(x, k, dil) if k > 1 else x.reshape(B * T, cin)
        grads[p + "conv.conv.weight"] = unpack_conv_grad(o["da"].t() @ A, cin, k)
        grads[p + "conv.conv.bias"] = o["da"].sum(0)
        return tdnn_dx_ref(o["da"], pack_conv_weight(W), B, T, cin, k, dil)[1]

    def block_bwd(i, dout):
        p = f"blocks.{i}."
        q = p + "se_block."
        r = rec[q]
        B, T, C = r["x"].shape
        W1, W2 = sd[q + "conv1.conv.weight"][:, :, 0], sd[q + "conv2.conv.weight"][:, :, 0]
        o = se_bwd_ref(r["x"], dout.reshape(B, T, C), r["s"], r["z"], r["g"], W1, W2)
        grads[q + "conv1.conv.weight"], grads[q + "conv1.conv.bias"] = o["dW1"][:, :, None], o["db1"]
        grads[q + "conv2.conv.weight"], grads[q + "conv2.conv.bias"] = o["dW2"][:, :, None], o["db2"]
        d_r2 = tdnn_bwd(p + "tdnn2.", o["d_t2"].reshape(B * T, C))
        d_t1 = torch.zeros_like(d_r2)
        for j in range(sc - 1, 0, -1):        # chunk j < sc - 1 also feeds chunk j + 1
            dy2 = d_t1[:, (j + 1) * w:(j + 2) * w] if j < sc - 1 else None
            d_t1[:, j * w:(j + 1) * w] = tdnn_bwd(p + f"res2net_block.blocks.{j - 1}.", d_r2[:, j * w:(j + 1) * w], dy2)
        d_t1[:, :w] = d_r2[:, :w]
        return tdnn_bwd(p + "tdnn1.", d_t1) + dout

    d_cat = tdnn_bwd("mfa.", d_mfa).clone()
    d_x0 = None
    for i in range(nb, 0, -1):
        dx = block_bwd(i, d_cat[:, (i - 1) * C1:i * C1])
        if i == 1:
            d_x0 = dx
        else:
            d_cat[:, (i - 2) * C1:(i - 1) * C1] += dx
    return grads, tdnn_bwd("blocks.0.", d_x0)
