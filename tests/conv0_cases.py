"""Inputs, float64 references and bounds for the kernels of csrc/conv0.hip, shared by tests/test_conv0_cpu.py,
tests/test_conv0_gpu.py and tools/conv0_parity.py.  No GPU and no ``ops`` import here: plain torch on the CPU in float64.

Layer 0 of the group-norm family: u = conv1d(x, w) (k taps, no bias), per-(utterance, channel) mean / biased variance over
the frames, rstd = 1 / sqrt(var + eps), out = GELU_erf(gamma * (u - mean) * rstd + beta), channels last.

Two yardsticks that are properties of the inputs and of this reference, never of a kernel:
  * ``ideal_f32_stats``: the convolution as an f32 FMA chain in tap order (what any f32 kernel computes per output), its
    moments accumulated in float64, mean and rstd rounded to f32.  Its distance from float64 (``e_mean``, ``e_rstd``) is what
    a statistics pass that makes no avoidable error still shows; the f32 routes are held to 2^-22 + 8 x that.
  * the amplification rms(u) * rstd of the apply pass: u - mean cancels that many times, so the 2e-6 of an f32 kernel
    becomes 2e-6 * max(1, rms_u / sd_u).  Where the variance is exactly zero (one frame, or a constant waveform) the ratio
    is infinite and rel-L2 says nothing: what a correct kernel can promise there is the absolute bound of
    ``degenerate_abs_bound`` (the rounding of u itself, times rstd * |gamma| * max gelu')."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 1e-5
B, K, STRIDE = 2, 10, 5
CLASSES = ("unit", "offset", "quiet", "loud", "const")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)

# ------------------------------------------------------------------------------------------------ the cases of the GPU file
STATS_L, STATS_C = (1, 17, 128, 129, 641), (96, 128, 384, 640)
SPLIT_K, SPLIT_STRIDE, SPLIT_C = 8, 4, (128, 640)          # the split-bf16 convolution statistics: k != 10
APPLY_L, APPLY_C = (1, 17, 129, 641), (96, 128, 384, 512, 640)
APPLY_CLASSES = ("unit", "offset", "quiet", "loud")
BWD_L, BWD_C, BWD_CLASSES = (1, 129, 300), (96, 320), ("unit", "quiet", "loud")
COL2IM_KS, COL2IM_CIN, COL2IM_LOUT = ((3, 2), (2, 2), (10, 5)), (8, 24, 512), (1, 37)
PACK_SHAPES = ((5, 3, 2), (40, 24, 3), (512, 512, 5))
LN0_BL, LN0_C, LN0_CLASSES = (3, 37), (8, 64, 512), ("unit", "offset")
LNG_M, LNG_H = (1, 37), (64, 512)

# ------------------------------------------------------------------------------------------------ bounds
STATS_FLOOR = 2.0 ** -22          # f32 storage of the result plus one division
STATS_ORDER = 8.0                 # a different (but fixed) summation order than the yardstick's
CAP_E_RSTD, CAP_E_MEAN = 4e-6, 1e-4          # what the yardstick itself must stay under on every class
F32_TOL, LP_TOL = 2e-6, 4e-3                 # the project's f32 / 16-bit rel-L2 figures (test_kernels_gpu.py)
SMALL_FRAC, SMALL_CAP = 1e-3, 0.02           # slices below 1e-3 of the tensor's RMS: absolute error on that scale; <= 2 %
BWD_TOL = 2e-5                               # dgamma / dbeta rel-L2, dw max |error| / sum |terms| (ecapa_stage_cases.F32_BOUND)
DU_ROUND = 2.0 ** -22                        # see layer0_backward
GELU_GRAD_MAX = 1.13                         # max |gelu'| = 1.1289
U_ERR_F32 = 2.0 ** -20            # |f32 FMA chain of k <= 10 taps - exact| and the roundings of mean * g and beta - mean * g
U_ERR_SPLIT = 2.0 ** -14          # split-bf16 product (|x_lo| <= 2^-8 |x|): x_lo * w_lo dropped, x_lo and w_lo rounded: 3 * 2^-16 per term


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def tol_of(dtype) -> float:
    return F32_TOL if dtype == torch.float32 else LP_TOL


def n_samples(L: int, k: int = K, stride: int = STRIDE) -> int:
    """Three trailing samples belong to no frame."""
    return (L - 1) * stride + k + 3


def waveform(cls: str, L: int, k: int = K, stride: int = STRIDE, batch: int = B) -> torch.Tensor:
    """[batch, N] f32; the rows hold different content (one draw for the whole batch)."""
    N = n_samples(L, k, stride)
    g = rnd(batch, N, seed=101 + CLASSES.index(cls))
    x = {"unit": g, "offset": 1 + 0.1 * g, "quiet": 1e-3 * g, "loud": 30 * g, "const": torch.full((batch, N), 0.5)}[cls]
    return x.float().contiguous()


def params(C: int, k: int = K):
    """-> w [C, 1, k], gamma [C], beta [C], f32."""
    return rnd(C, 1, k, seed=2, scale=0.4).float(), (1 + 0.1 * rnd(C, seed=3)).float(), (0.1 * rnd(C, seed=4)).float()


def gelu(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_grad(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


# ------------------------------------------------------------------------------------------------ float64 forward
@functools.lru_cache(maxsize=None)
def forward_ref(cls: str, L: int, C: int, k: int = K, stride: int = STRIDE) -> SimpleNamespace:
    """The float64 forward of layer 0 and everything the bounds need.  Cached: treat the result as read-only."""
    wav = waveform(cls, L, k, stride)
    w, gamma, beta = params(C, k)
    u = F.conv1d(wav[:, None].to(F64), w.to(F64), stride=stride)                       # [B, C, L]
    assert u.shape[2] == L
    mean, var = u.mean(dim=2), u.var(dim=2, unbiased=False)
    rstd = (var + EPS).rsqrt()
    yhat = (u - mean[..., None]) * rstd[..., None]
    out = gelu(yhat * gamma.to(F64)[None, :, None] + beta.to(F64)[None, :, None]).transpose(1, 2).contiguous()   # [B, L, C]
    absu = F.conv1d(wav[:, None].to(F64).abs(), w.to(F64).abs(), stride=stride)        # sum_j |w_j| |x_j|
    return SimpleNamespace(cls=cls, L=L, C=C, k=k, stride=stride, wav=wav, w=w, gamma=gamma, beta=beta, u=u, mean=mean,
                           var=var, rstd=rstd, yhat=yhat, out=out, absu=absu)


def ideal_f32_stats(wav: torch.Tensor, w: torch.Tensor, stride: int):
    """-> (mean, rstd) [B, C] as float64 holding f32 values: the convolution as an f32 FMA chain in tap order (product
    exact, one rounding per tap: float64 holds the 48-bit product and the sum to well under half an f32 ulp), the two
    moments of those f32 outputs accumulated in float64, mean and rstd rounded to f32."""
    x, wt = wav.numpy().astype(np.float64), w.numpy().astype(np.float64)[:, 0]         # [B, N], [C, k]
    k = wt.shape[1]
    L = (x.shape[1] - k) // stride + 1
    acc = np.zeros((x.shape[0], wt.shape[0], L), dtype=np.float32)
    for j in range(k):
        xj = x[:, j:j + (L - 1) * stride + 1:stride]                                   # [B, L]
        acc = (wt[None, :, j, None] * xj[:, None, :] + acc.astype(np.float64)).astype(np.float32)
    a = acc.astype(np.float64)
    mean = a.mean(axis=2)
    var = ((a - mean[..., None]) ** 2).mean(axis=2)
    rstd = 1.0 / np.sqrt(var + EPS)
    return (torch.from_numpy(mean.astype(np.float32).astype(np.float64)),
            torch.from_numpy(rstd.astype(np.float32).astype(np.float64)))


def stats_errors(mean: torch.Tensor, rstd: torch.Tensor, ref: SimpleNamespace):
    """-> (max |d mean| * rstd_ref, max rel |d rstd|) over (b, c); NaN or inf anywhere counts as inf."""
    mean, rstd = mean.to(F64), rstd.to(F64)
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(rstd).all())):
        return math.inf, math.inf
    return float(((mean - ref.mean).abs() * ref.rstd).max()), float(((rstd - ref.rstd).abs() / ref.rstd).max())


@functools.lru_cache(maxsize=None)
def yardstick(cls: str, L: int, C: int, k: int = K, stride: int = STRIDE):
    """-> (e_mean, e_rstd) of ideal_f32_stats against float64."""
    ref = forward_ref(cls, L, C, k, stride)
    return stats_errors(*ideal_f32_stats(ref.wav, ref.w, stride), ref)


def stats_bounds(cls: str, L: int, C: int):
    e_mean, e_rstd = yardstick(cls, L, C)
    return STATS_FLOOR + STATS_ORDER * e_mean, STATS_FLOOR + STATS_ORDER * e_rstd


# ------------------------------------------------------------------------------------------------ apply pass
def sliced_rel_l2(got: torch.Tensor, ref: torch.Tensor, dim: int):
    """rel-L2 of every slice along ``dim`` (the other dims index the slices).  A slice whose reference norm is below
    SMALL_FRAC of what a slice of RMS-sized elements has is judged by its absolute error on that scale instead.
    -> (errors, mask of the slices judged absolutely); a non-finite ``got`` gives inf."""
    got, ref = got.to(F64), ref.to(F64)
    err = (got - ref).norm(dim=dim)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    nr = ref.norm(dim=dim)
    scale = ref.pow(2).mean().sqrt() * math.sqrt(ref.shape[dim])
    small = nr < SMALL_FRAC * scale
    return err / torch.where(small, scale, nr).clamp_min(1e-300), small


def degenerate(ref: SimpleNamespace) -> bool:
    """Exactly zero variance: one frame, or a constant waveform."""
    return ref.L == 1 or ref.cls == "const"


def apply_bounds(ref: SimpleNamespace, dtype):
    """-> (per-frame bound [B, L], per-channel bound [B, C]) for rel-L2 against ``ref.out``: tol * max(1, rms_u / sd_u),
    the amplification only for f32 (a 16-bit output is held to the project's 4e-3 as it stands).  The amplification of a
    frame is the RMS over its channels."""
    amp = (ref.u.pow(2).mean(dim=2).sqrt() / ref.var.sqrt()).clamp_min(1.0)            # [B, C]
    if dtype != torch.float32:
        return torch.full((B, ref.L), LP_TOL, dtype=F64), torch.full((B, ref.C), LP_TOL, dtype=F64)
    return F32_TOL * amp.pow(2).mean(dim=1, keepdim=True).sqrt().expand(B, ref.L), F32_TOL * amp


def split_route(C: int, k: int, dtype) -> bool:
    """Which shapes the 16-bit outputs send through the split-bf16 matrix-core convolution (conv0_mfma_ok)."""
    return dtype != torch.float32 and C % 128 == 0 and 3 * k <= 32


def degenerate_abs_bound(ref: SimpleNamespace, dtype) -> torch.Tensor:
    """[B, L, C] bound on |out - ref.out| where var = 0 (float64: u == mean, out = gelu(beta) exactly).  A kernel computes
    u with an absolute error e_u = U_ERR * sum_j |w_j| |x_j| (f32 FMA chain, or the split-bf16 product on the matrix cores)
    and subtracts a mean that carries the same kind of error, so gamma * (u - mean) * rstd is off by up to
    2 * e_u * rstd * |gamma| and the output by max |gelu'| times that, plus the rounding of the output itself."""
    e_u = (U_ERR_SPLIT if split_route(ref.C, ref.k, dtype) else U_ERR_F32) * ref.absu.transpose(1, 2)     # [B, L, C]
    g = (ref.rstd * ref.gamma.to(F64).abs()[None])[:, None, :]
    return tol_of(dtype) * ref.out.abs() + 2 * GELU_GRAD_MAX * g * e_u


def split_bf16_out(ref: SimpleNamespace) -> torch.Tensor:
    """The float64 forward with the convolution replaced by the split-bf16 product x_hi w_hi + x_hi w_lo + x_lo w_hi
    (every term exact) and the float64 statistics kept: the distance of this from ``ref.out`` is the floor of the 16-bit
    matrix-core route before any output rounding."""
    def split(t):
        hi = t.to(torch.bfloat16).float()
        return hi.to(F64), (t - hi).to(torch.bfloat16).to(F64)
    xh, xl = split(ref.wav)
    wh, wl = split(ref.w)
    conv = lambda a, b: F.conv1d(a[:, None], b, stride=ref.stride)      # noqa: E731
    u = conv(xh, wh) + conv(xh, wl) + conv(xl, wh)
    yhat = (u - ref.mean[..., None]) * ref.rstd[..., None]
    return gelu(yhat * ref.gamma.to(F64)[None, :, None] + ref.beta.to(F64)[None, :, None]).transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ float64 backward
def layer0_backward(ref: SimpleNamespace, dz: torch.Tensor):
    """Closed-form backward of layer 0 given dz [B, L, C] (float64) -> dw [C, k], dgamma [C], dbeta [C], the sum of the
    |terms| of dw [C, k], the scale a cancelling sum's error is measured on, and plain sum over (b, l) of |du * x|."""
    ga, be = ref.gamma.to(F64)[None, :, None], ref.beta.to(F64)[None, :, None]
    dy = dz.to(F64).transpose(1, 2) * gelu_grad(ref.yhat * ga + be)                    # [B, C, L]
    dgamma, dbeta = (dy * ref.yhat).sum(dim=(0, 2)), dy.sum(dim=(0, 2))
    du = ref.rstd[..., None] * ga * (dy - dy.mean(dim=2, keepdim=True) - ref.yhat * (dy * ref.yhat).mean(dim=2, keepdim=True))
    x = ref.wav.to(F64).unfold(1, ref.k, ref.stride)[:, :ref.L]                        # [B, L, k]
    dw = torch.einsum("bcl,blj->cj", du, x)
    plain = torch.einsum("bcl,blj->cj", du.abs(), x.abs())
    # du is itself a cancelling sum, dy - mean(dy) - yhat * mean(dy * yhat): at one frame it is exactly zero in exact
    # arithmetic (so is sum |du * x|), and an f32 evaluation leaves 2^-24 |dy| of it whatever the order (a fused
    # dz * gelu' - mean is enough).  The scale is therefore sum |du * x| plus DU_ROUND = 2^-22 (four roundings) of du taken
    # term by term, expressed in units of BWD_TOL: about 2 % on top of sum |du * x| from 129 frames on (checked on the CPU)
    du_abs = ref.rstd[..., None] * ga.abs() * (dy.abs() + dy.mean(dim=2, keepdim=True).abs()
                                               + ref.yhat.abs() * (dy * ref.yhat).mean(dim=2, keepdim=True).abs())
    terms = plain + (DU_ROUND / BWD_TOL) * torch.einsum("bcl,blj->cj", du_abs, x.abs())
    return dw, dgamma, dbeta, terms, plain


def bwd_dz(L: int, C: int, dtype) -> torch.Tensor:
    """dz [B, L, C] rounded to ``dtype``, as float64: only f32 arithmetic separates the kernel from the reference."""
    return rnd(B, L, C, seed=7).to(dtype).to(F64)


def sum_scale_error(got: torch.Tensor, ref: torch.Tensor, sum_abs: torch.Tensor) -> float:
    """max |got - ref| / sum(|terms|) (0 / 0 counts as 0, a non-zero or non-finite error over a zero scale as inf)."""
    err, scale = (got.to(F64) - ref.to(F64)).abs(), sum_abs.to(F64)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    return float(torch.where(err == 0, torch.zeros_like(err), err / scale).max())


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    """0 / 0 counts as 0; NaN counts as inf."""
    d, n = float((got.to(F64) - ref.to(F64)).norm()), float(ref.to(F64).norm())
    if not math.isfinite(d):
        return math.inf
    return 0.0 if d == 0 else d / max(n, 1e-300)


# ------------------------------------------------------------------------------------------------ col2im, pack, unpack
def col2im_case(k: int, stride: int, cin: int, lout: int):
    """-> (col [B * lout, k * cin] integer-valued in [-64, 64] as float64, Lin, fold [B, Lin, cin] float64).
    Lin = (lout - 1) * stride + k + 1: the last row is covered by no frame."""
    lin = (lout - 1) * stride + k + 1
    g = torch.Generator().manual_seed(31 + k + 7 * cin + lout)
    col = torch.randint(-64, 65, (B * lout, k * cin), generator=g).to(F64)
    dx = torch.zeros(B, lin, cin, dtype=F64)
    c4 = col.view(B, lout, k, cin)
    for l in range(lout):
        for tap in range(k):
            dx[:, l * stride + tap] += c4[:, l, tap]
    return col, lin, dx


def pack_ref(w: torch.Tensor) -> torch.Tensor:
    """HF [Cout, Cin, k] -> GEMM operand [Cout, k * Cin] (K index = tap * Cin + ci)."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


# ------------------------------------------------------------------------------------------------ layer-norm family
@functools.lru_cache(maxsize=None)
def ln0_ref(cls: str, C: int, with_bias: bool) -> SimpleNamespace:
    """conv0 -> (+ bias) -> LayerNorm over channels -> GELU in float64, (B, L) = LN0_BL, k = 10, stride 5."""
    nb, L = LN0_BL
    wav = waveform(cls, L, batch=nb)
    w, gamma, beta = params(C)
    bias = (0.1 * rnd(C, seed=5)).float() if with_bias else None
    u = F.conv1d(wav[:, None].to(F64), w.to(F64), None if bias is None else bias.to(F64), stride=STRIDE).transpose(1, 2)
    out = gelu(F.layer_norm(u, (C,), gamma.to(F64), beta.to(F64), EPS)).contiguous()
    return SimpleNamespace(wav=wav, w=w, bias=bias, gamma=gamma, beta=beta, out=out, L=L, B=nb)


def ln_gelu_case(M: int, H: int, dtype):
    """-> (x [M, H] rounded to dtype as f32, gamma, beta, float64 GELU(LN(x)))."""
    x = rnd(M, H, seed=1).to(dtype).float()
    gamma, beta = (1 + 0.1 * rnd(H, seed=3)).float(), (0.1 * rnd(H, seed=4)).float()
    return x, gamma, beta, gelu(F.layer_norm(x.to(F64), (H,), gamma.to(F64), beta.to(F64), EPS))
