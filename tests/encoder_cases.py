"""Inputs, float64 references, yardsticks and bounds for the two kernel families a wav2vec2 train step runs most often,
csrc/norm.hip (w2v2_layernorm_fwd / _bwd / _bwd_fold) and csrc/attention.hip (w2v2_attention_fwd / _bwd), shared by
tests/test_encoder_cases_cpu.py, tests/test_encoder_kernels_gpu.py and tools/encoder_parity.py.  No GPU and no ``ops``
import here: plain torch on the CPU in float64.

Every output is judged per slice (a token row, a column of a column reduction, a 64-element head row), never by one norm
of the whole tensor.  Yardsticks are properties of the inputs and of these references, never of a kernel:
  * ``ln_ideal_f32_stats``: the two-pass mean / rstd of the f32 sum evaluated in f32; the layer-norm forward is held to
    2^-22 + 8 x its error (the statistics convention of conv0_cases.py).
  * ``ideal16_forward`` / ``ideal16_backward``: attention in float64 with exactly the roundings attention.hip documents
    (P after the dropout scale rounded before P V, the recomputed P and dS rounded before the three backward products,
    every output rounded once, delta taken from the rounded ctx).  Its distance from the float64 reference is the floor of
    ANY kernel with those roundings; a kernel is held to 2 x that plus the f32 term."""
import functools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import torch

F64 = torch.float64
EPS = 1e-5
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
LP = (torch.bfloat16, torch.float16)
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
U = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}     # one rounding to the activation type

# ------------------------------------------------------------------------------------------------ bounds
STATS_FLOOR = 2.0 ** -22          # f32 storage of the result plus one division
STATS_ORDER = 8.0                 # a different (but fixed) summation order than the yardstick's
CAP_STATS = 2.0 ** -22            # what the statistics yardstick itself must stay under, times max(1, rms_s * rstd): the f32
                                  # sum and the f32 mean are stored on the scale of |s|, the spread is 1 / rstd
F32_TOL = 2e-6                               # the project's f32 rel-L2 figure (test_kernels_gpu.py)
LN_BWD_F32 = 1e-5                            # ds / d_r in f32, as test_layernorm_fwd_bwd asserts it
BWD_TOL = 2e-5                               # dgamma / dbeta: max |error| / sum |terms| per column
SMALL_FRAC, SMALL_CAP = 1e-3, 0.02           # slices below 1e-3 of the tensor's RMS: absolute error on that scale; <= 2 %
YARD_FACTOR = 2.0                            # two correct implementations draw different roundings of the same size
CAP_YARD_CTX, CAP_YARD_DQKV = 8e-3, 2e-2     # test_fused_attention_fwd_bwd's whole-tensor bounds: no new bound is looser
SENTINEL = -768.0                            # exact in bf16 / fp16 / f32


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rd(t: torch.Tensor, dtype) -> torch.Tensor:
    """One rounding to ``dtype``, held in float64."""
    return t.to(dtype).to(F64)


def sliced_rel_l2(got: torch.Tensor, ref: torch.Tensor, dim: int, abs_scale=None):
    """rel-L2 of every slice along ``dim`` (the other dims index the slices).  A slice whose reference norm is below
    SMALL_FRAC of what a slice of RMS-sized elements has is judged by its absolute error on that scale instead; with
    ``abs_scale`` (an element size) EVERY slice is judged absolutely on it.
    -> (errors, mask of the slices judged absolutely); a non-finite ``got`` gives inf."""
    got, ref = got.to(F64), ref.to(F64)
    err = (got - ref).norm(dim=dim)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    root = math.sqrt(ref.shape[dim])
    if abs_scale is not None:
        return err / max(float(abs_scale) * root, 1e-300), torch.ones_like(err, dtype=torch.bool)
    nr = ref.norm(dim=dim)
    scale = ref.pow(2).mean().sqrt() * root
    small = nr < SMALL_FRAC * scale
    return err / torch.where(small, scale, nr).clamp_min(1e-300), small


def sum_scale_error(got: torch.Tensor, ref: torch.Tensor, sum_abs: torch.Tensor):
    """|got - ref| / sum(|terms|) per element (0 / 0 counts as 0, anything else over a zero scale as inf)."""
    err, scale = (got.to(F64) - ref.to(F64)).abs(), sum_abs.to(F64)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    return torch.where(err == 0, torch.zeros_like(err), err / scale)


# ================================================================================================ layer norm
LN_H = (8, 64, 512, 520, 768, 1024)   # one lane | second chunk empty | quad NC = 2 | second chunk: lane 0 only | quad NC = 3 | both chunks full
LN_M_SMALL = (1, 3, 37)               # 3: fewer rows than a workgroup's waves
LN_BWD_BLOCKS, LN_BWD_BLOCKS_Q = 768, 1024          # csrc/norm.hip; test_encoder_cases_cpu.py reads them back from the source
LN_CLASSES = ("unit", "offset", "outlier", "const")
LN_LARGE_CLASSES = ("unit", "offset")               # `offset` moves the row mean from row to row: a prefetched mean / rstd of
                                                    # the wrong row shows
LN_FWD_VARIANTS = ("plain", "residual", "residual+dropout")
LN_BWD_MODES = ("immediate", "deferred", "none")    # dgamma / dbeta folded at once | through LnFoldGroup | not requested
LN_P, LN_SEED = 0.1, 12345
LN_CHAIN_CLASSES = ("offset", "outlier")


def ln_quad_shape(H: int) -> bool:
    return H in (512, 768)


def ln_block_cap(H: int) -> int:
    """Workgroups of the backward, whatever the dtype (ln_bwd_nblocks of norm.hip)."""
    return LN_BWD_BLOCKS_Q if ln_quad_shape(H) else LN_BWD_BLOCKS


def ln_large_m(H: int) -> int:
    """2 * 4 * cap + 5 rows: the grid stride is 4 * cap rows, so five waves walk three rows and the others two -- the
    next-row prefetch runs in the middle of a wave's walk and at its end, and the column sums add up over several rows."""
    return 2 * 4 * ln_block_cap(H) + 5


def ln_bwd_ms(H: int):
    return LN_M_SMALL + (ln_large_m(H),)


def ln_bwd_kernel(dtype, H: int, mode: str) -> str:
    """The kernel of norm.hip that (dtype, H, dgamma requested or not) reaches."""
    if dtype == torch.float32:
        return "ln_bwd_kernel"
    return "ln_bwd16q_kernel" if ln_quad_shape(H) and mode != "none" else "ln_bwd16_kernel"


def ln_params(H: int):
    return (1 + 0.1 * rnd(H, seed=3)).float(), (0.1 * rnd(H, seed=4)).float()


def ln_s(cls: str, M: int, H: int) -> torch.Tensor:
    """[M, H] f32 by input class.  unit: N(0, 1).  offset: row mean 30 (+- 1, stepping with the row) and spread 0.1, so
    rstd is near 10.  outlier: unit with +50 and -50 sigma at two columns that move with the row.  const: every row one
    dyadic constant, variance exactly 0."""
    g = rnd(M, H, seed=11 + LN_CLASSES.index(cls))
    row = torch.arange(M)
    if cls == "offset":
        g = 30 + 0.5 * ((row % 5) - 2)[:, None] + 0.1 * g
    elif cls == "outlier":
        g[row, (3 * row) % H] = 50.0
        g[row, (3 * row + H // 2) % H] = -50.0
    elif cls == "const":
        g = (0.25 * ((row % 9) - 4))[:, None].expand(M, H).clone()
    return g.float().contiguous()


def ln_residual(cls: str, M: int, H: int) -> torch.Tensor:
    """The residual branch of the forward cases: small against the spread of the class, so x + r * mask keeps the class's
    character; zero for `const` (the sum must stay constant whatever the mask is)."""
    return (rnd(M, H, seed=21) * {"unit": 0.5, "offset": 0.05, "outlier": 0.5, "const": 0.0}[cls]).float()


def ln_forward(x: torch.Tensor, r, mask, gamma: torch.Tensor, beta: torch.Tensor) -> SimpleNamespace:
    """float64 LayerNorm of the UNROUNDED sum s = x + r * mask (``r`` None: s = x; ``mask`` holds 0 or 1 / (1 - p))."""
    s = x.to(F64) if r is None else x.to(F64) + r.to(F64) * (1.0 if mask is None else mask.to(F64))
    mean, var = s.mean(dim=1), s.var(dim=1, unbiased=False)
    rstd = (var + EPS).rsqrt()
    y = (s - mean[:, None]) * rstd[:, None] * gamma.to(F64) + beta.to(F64)
    amp = (s.pow(2).mean(dim=1).sqrt() * rstd).clamp_min(1.0)          # s - mean cancels that many times
    return SimpleNamespace(s=s, mean=mean, rstd=rstd, y=y, amp=amp)


def ln_f32_sums(x: torch.Tensor, r: torch.Tensor, mask):
    """The two f32 evaluations of x + r * mask a kernel may make: product rounded and then added, or one fused
    multiply-add.  They differ only where mask = 1 / (1 - p) is inexact."""
    m = torch.ones_like(x, dtype=torch.float32) if mask is None else mask.float()
    a = x.float() + r.float() * m
    b = (x.to(F64) + r.to(F64) * m.to(F64)).float()
    return a, b


def ln_ideal_f32_stats(s32: torch.Tensor):
    """-> (mean, rstd) [M] as float64 holding f32 values: the two-pass statistics of the f32 rows evaluated in f32
    (numpy's pairwise f32 sums, the division and the square root rounded to f32)."""
    a = s32.numpy().astype(np.float32)
    H = np.float32(a.shape[1])
    mean = (a.sum(axis=1, dtype=np.float32) / H).astype(np.float32)
    d = (a - mean[:, None]).astype(np.float32)
    var = ((d * d).sum(axis=1, dtype=np.float32) / H).astype(np.float32)
    rstd = (np.float32(1.0) / np.sqrt(var + np.float32(EPS), dtype=np.float32)).astype(np.float32)
    return torch.from_numpy(mean.astype(np.float64)), torch.from_numpy(rstd.astype(np.float64))


def ln_stats_errors(mean: torch.Tensor, rstd: torch.Tensor, ref: SimpleNamespace):
    """-> (max |d mean| * rstd_ref, max rel |d rstd|) over the rows; NaN or inf anywhere counts as inf."""
    mean, rstd = mean.to(F64), rstd.to(F64)
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(rstd).all())):
        return math.inf, math.inf
    return float(((mean - ref.mean).abs() * ref.rstd).max()), float(((rstd - ref.rstd).abs() / ref.rstd).max())


def ln_fwd_inputs(cls: str, M: int, H: int, dtype, variant: str):
    """-> (x, r or None) f32 holding ``dtype`` values."""
    x = ln_s(cls, M, H).to(dtype).float()
    return x, (None if variant == "plain" else ln_residual(cls, M, H).to(dtype).float())


def ln_y_bound(ref: SimpleNamespace, dtype) -> torch.Tensor:
    """Per-row rel-L2 bound of y: one output rounding (16-bit) plus the f32 term, F32_TOL * max(1, rms_s * rstd)."""
    return U[dtype] + F32_TOL * ref.amp


def ln_backward(dy, s, mean, rstd, gamma, mask=None) -> SimpleNamespace:
    """The backward as a function of the kernel's own inputs (all float64): xh = (s - mean) rstd, g = dy gamma,
    ds = rstd (g - mean_c(g) - xh mean_c(g xh)), d_r = ds * mask, dgamma = sum_rows dy xh, dbeta = sum_rows dy, and the
    sums of the |terms| of the two column reductions."""
    xh = (s - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    ds = rstd[:, None] * (g - g.mean(dim=1, keepdim=True) - xh * (g * xh).mean(dim=1, keepdim=True))
    return SimpleNamespace(xh=xh, ds=ds, d_r=ds if mask is None else ds * mask.to(F64), dgamma=(dy * xh).sum(dim=0),
                           dbeta=dy.sum(dim=0), terms_g=(dy * xh).abs().sum(dim=0), terms_b=dy.abs().sum(dim=0))


@functools.lru_cache(maxsize=4)
def ln_bwd_case(cls: str, M: int, H: int, dtype) -> SimpleNamespace:
    """Inputs of one backward case and its float64 reference without dropout.  s and dy hold ``dtype`` values; mean and rstd
    are the true statistics of that s rounded to f32, which is what the kernel is handed.  Cached: read-only."""
    s, dy = ln_s(cls, M, H).to(dtype).to(F64), rnd(M, H, seed=5).to(dtype).to(F64)
    gamma, _ = ln_params(H)
    mean = s.mean(dim=1).float()
    rstd = (s.var(dim=1, unbiased=False) + EPS).rsqrt().float()
    ref = ln_backward(dy, s, mean.to(F64), rstd.to(F64), gamma.to(F64))
    return SimpleNamespace(s=s, dy=dy, gamma=gamma, mean=mean, rstd=rstd, ref=ref)


def ln_prefill(H: int):
    """Known non-zero contents of dgamma / dbeta (the fold ADDS): small dyadic values."""
    i = torch.arange(H, dtype=torch.float32)
    return (i % 5 - 2) * 0.5 + 0.25, (i % 3 - 1) * 0.25 + 0.125


def ln_ds_bound(dtype) -> float:
    return U[dtype] + LN_BWD_F32


# ================================================================================================ attention
AT_B, AT_HEADS, AT_D = 2, 2, 64
AT_H = AT_HEADS * AT_D
AT_SCALE = AT_D ** -0.5
AT_T = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 128, 129, 160, 161, 193, 512, 513)
AT_CLASSES = ("gauss", "uniform", "late_max", "early_max", "peaked", "loud", "quiet_grad")
AT_CHAIN_CLASSES, AT_CHAIN_T = ("gauss", "late_max"), (33, 161, 513)
AT_DROP_T, AT_P, AT_SEED = (17, 33, 64, 161, 200), 0.1, 991
ATTN_SMALL_GEOM_MAX_T = 512       # csrc/attention.hip
RAMP_SPAN = 40.0                  # late_max / early_max: s * scale spans at most this much (e^-40 = 4e-18 is a normal f32,
                                  # and below the 6e-8 where a 16-bit fp16 probability underflows)
EXP_F32 = 2.0 ** -23              # the kernels form P = 2^(s * scale * log2 e - lse * log2 e) in f32: two roundings of numbers
                                  # of size |s * scale| log2 e move P by up to 2^-23 max(|s * scale|, |lse|) of itself.
                                  # At |s * scale| = 80 that is 1e-5, enough to turn 2 % of the fp16 roundings of dS the
                                  # other way; the yardstick is therefore taken at P, P (1 + that) and P (1 - that), and a
                                  # row's yardstick is the LARGEST of the three errors
RAMP_STEP_MAX = 0.25              # ... in steps of at most this much per key: at least four keys share a row's weight
LOUD_OFFSET = 80.0                # loud: every score of a row is near +80 (even queries) or -80 (odd queries): exp() of
                                  # the one is beyond fp16 and bf16's 8 bits, of the other below the normal f32
PEAK_GAP = 30.0                   # peaked: the chosen key leads every other by at least this much in s * scale
GEOMS = ("32", "64")


def small_geom(T: int) -> bool:
    """The selection rule of attention.hip (attn_small_geom) when nothing is forced."""
    return T <= ATTN_SMALL_GEOM_MAX_T and ((T + 31) & ~31) < ((T + 63) & ~63)


def heads(x: torch.Tensor) -> torch.Tensor:
    """[B, T, heads * d] -> [B, heads, T, d]"""
    return x.reshape(x.shape[0], x.shape[1], AT_HEADS, AT_D).transpose(1, 2)


def unheads(x: torch.Tensor) -> torch.Tensor:
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], AT_H)


def ramp_step(T: int) -> float:
    """The power of two by which s * scale steps from key to key in late_max / early_max."""
    return min(RAMP_STEP_MAX, 2.0 ** math.floor(math.log2(RAMP_SPAN / max(T - 1, 1))))


def peaked_key(T: int) -> torch.Tensor:
    """The dominant key of query q: (7 q + T - 1) % T, so query 0 looks at the LAST key whatever T is."""
    return (7 * torch.arange(T) + T - 1) % T


def zero_sum(T: int, seed: int, unit: float, levels: int = 3) -> torch.Tensor:
    """[B, heads, T, 16] of +-unit * {1, 2, 4}[:levels] whose sixteen values sum to exactly zero: added to sixteen dimensions
    of q (or k) where the other operand is the same in all sixteen, it leaves every score as it is."""
    pick = torch.randint(0, levels, (AT_B, AT_HEADS, T, 8), generator=torch.Generator().manual_seed(seed))
    sign = torch.where(rnd(AT_B, AT_HEADS, T, 8, seed=seed + 1) >= 0, 1.0, -1.0)
    a = sign * unit * 2.0 ** pick
    return torch.cat([a, -a], dim=-1)


@functools.lru_cache(maxsize=None)
def attn_inputs(cls: str, T: int, dtype):
    """-> (q, k, v, dO) [B, heads, T, d] float64 holding ``dtype`` values.  Cached: read-only."""
    g = rnd(AT_B, T, 3 * AT_H, seed=1000 + T)
    q, k, v = (heads(g[..., i * AT_H:(i + 1) * AT_H]).clone() for i in range(3))
    do = heads(rnd(AT_B, T, AT_H, seed=2000 + T)).clone()
    if cls in ("gauss", "quiet_grad"):
        q, k = 1.5 * q, 1.5 * k
    elif cls == "uniform":
        q, k = torch.zeros_like(q), 1.5 * k
    elif cls in ("late_max", "early_max"):
        # s * scale = -m * step exactly, m = 16 * (m // 16) + m % 16 the distance from the key of the maximum (where k is
        # about 0: dQ = dS K is no difference of large numbers): dimensions 0-15 carry the coarse part (q = 1,
        # k = -8 * (m // 16) * step + w), dimensions 16-31 the fine part (q = 2 + z, k = -(m % 16) * step / 4).  w and z are
        # dyadic (+-2, 4 or 8), differ from dimension to dimension and sum to zero over their sixteen dimensions: the
        # scores do not see them, and they outweigh the constant next to them, so that no row of dQ or dK is one
        # cancelling scalar repeated sixteen times.  Every value is exact in 8 bits.  The other 32 dimensions are small
        # noise that stays below half a step.
        m = T - 1 - torch.arange(T) if cls == "late_max" else torch.arange(T)      # distance from the maximum's key
        step = ramp_step(T)
        q, k = 0.05 * q, 0.05 * k
        q[..., :16] = 1.0
        k[..., :16] = (-(m // 16) * 8 * step).to(k.dtype)[:, None] + zero_sum(T, 4000 + T, 2.0)
        q[..., 16:32] = 2.0 + zero_sum(T, 5000 + T, 2.0)
        k[..., 16:32] = (-(m % 16) * step / 4).to(k.dtype)[:, None]
    elif cls == "peaked":
        code = torch.where(rnd(AT_B, AT_HEADS, T, AT_D, seed=3000 + T) >= 0, 1.0, -1.0)
        k = 4.0 * code
        q = 4.0 * code[:, :, peaked_key(T)]
    elif cls == "loud":
        # the gauss scores of 48 dimensions plus a common +-LOUD_OFFSET per row from the other sixteen (32 * 1.25 / 8 each):
        # softmax does not see it; exp() without the maximum subtracted leaves the 16-bit range (even queries) or the
        # normal f32 range (odd ones).  The offset is a rank-one term, and dQ = dS K meets its key side as
        # |k_off| * sum dS, a pure cancellation: the large factor sits in q, with a zero-sum variation of its own size
        # (+-32: one size, so that no single product outweighs a row), so that no row of dK is one scalar repeated
        # sixteen times either
        q, k = 1.5 * q, 1.5 * k
        q[..., :16] = torch.where(torch.arange(T) % 2 == 0, 32.0, -32.0)[:, None] + zero_sum(T, 6000 + T, 32.0, levels=1)
        k[..., :16] = LOUD_OFFSET / 64
    if cls == "quiet_grad":
        do = do * 2.0 ** -12
    return tuple(rd(t, dtype).contiguous() for t in (q, k, v, do))


def scores(q, k):
    return q @ k.transpose(2, 3) * AT_SCALE


def attention_forward(q, k, v, mask=None, keep: float = 1.0):
    """float64 -> (ctx [B, h, T, d], lse [B, h, T]).  ``mask`` [B, h, T, T] of 0 / 1; the normaliser sums the probabilities
    BEFORE dropout."""
    s = scores(q, k)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    if mask is not None:
        p = p * mask / keep
    return p @ v, lse


def attention_backward(q, k, v, do, ctx, lse, mask=None, keep: float = 1.0):
    """The backward as a function of the kernel's own inputs (float64): P = exp(s - lse), dP = dO V^T,
    delta = sum_d dO ctx, dS = P (dP mask / keep - delta) scale, dV = Pdrop^T dO, dK = dS^T Q, dQ = dS K.
    -> (dq, dk, dv, delta, sum_d |dO ctx|)"""
    p = torch.exp(scores(q, k) - lse[..., None])
    ms = 1.0 if mask is None else mask / keep
    delta = (do * ctx).sum(dim=-1)
    ds = p * ((do @ v.transpose(2, 3)) * ms - delta[..., None]) * AT_SCALE
    return ds @ k, ds.transpose(2, 3) @ q, (p * ms).transpose(2, 3) @ do, delta, (do * ctx).abs().sum(dim=-1)


def ideal16_forward(q, k, v, dtype, mask=None, keep: float = 1.0):
    """The ideal 16-bit forward: the probabilities relative to the row maximum, after the dropout scale, rounded to
    ``dtype`` before P V (the kernel rounds them relative to its RUNNING maximum, which is never smaller: in fp16 it may
    keep a few more subnormal bits than this); the f32 accumulator divided by the unrounded normaliser; ctx rounded once."""
    s = scores(q, k)
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    l = p.sum(dim=-1, keepdim=True)
    if mask is not None:
        p = p * mask / keep
    return rd((rd(p, dtype) @ v) / l, dtype)


def ideal16_backward(q, k, v, do, ctx, lse, dtype, mask=None, keep: float = 1.0, exp_shift: float = 0.0):
    """The ideal 16-bit backward: recomputed P (after the dropout scale) and dS rounded to ``dtype`` before the three
    products, every output rounded once; delta from the ctx it is handed.  dP = dO V^T and delta = sum_d dO ctx are f32 dot
    products of d = 64 terms in the kernels (matrix-core accumulator, fma chain) and are evaluated in f32 here: where P is
    one-hot dS = P (dP - delta) is NOTHING BUT the difference of their roundings, and a float64 difference (1e-17) would
    make the yardstick of `peaked` an exact zero no kernel can be twice.  ``exp_shift`` (-1, 0 or +1) moves every
    recomputed P by the f32 rounding of its exponent, see EXP_F32.  -> (dq, dk, dv)"""
    s = scores(q, k)
    p = torch.exp(s - lse[..., None]) * (1.0 + exp_shift * EXP_F32 * torch.maximum(s.abs(), lse.abs()[..., None]))
    ms = 1.0 if mask is None else mask / keep
    dp = (do.float() @ v.float().transpose(2, 3)).to(F64)
    delta = (do.float() * ctx.float()).sum(dim=-1).to(F64)
    ds = rd(p * (dp * ms - delta[..., None]) * AT_SCALE, dtype)
    return rd(ds @ k, dtype), rd(ds.transpose(2, 3) @ q, dtype), rd(rd(p * ms, dtype).transpose(2, 3) @ do, dtype)


def lse_f32_error(q, k, lse) -> float:
    """max |lse| error of an f32 CPU evaluation (f32 matmul, f32 logsumexp) of the same inputs."""
    s32 = (q.float() @ k.float().transpose(2, 3)) * np.float32(AT_SCALE)
    return float((torch.logsumexp(s32, dim=-1).to(F64) - lse).abs().max())


def lse_bound(lse: torch.Tensor, e_f32: float) -> torch.Tensor:
    return STATS_FLOOR * lse.abs().clamp_min(1.0) + STATS_ORDER * e_f32


def peaked_scale(k, v, do) -> float:
    """dq / dk of the `peaked` class are what is left of a cancellation (dS is about 0): judged absolutely on
    rms(dctx) * rms(v) * rms(k) * scale, the size of one product term of dS K (for dK = dS^T Q pass q: in `peaked` q is a
    permutation of k and the two are one number)."""
    rms = lambda t: float(t.pow(2).mean().sqrt())      # noqa: E731
    return rms(do) * rms(v) * rms(k) * AT_SCALE


def attn_case_of(cls: str, T: int, dtype, mask=None, keep: float = 1.0) -> SimpleNamespace:
    """Everything the tests need of one case.  Forward: float64 ctx / lse and the ideal 16-bit ctx.  Split backward: the
    inputs ctx16 (the float64 ctx rounded to ``dtype``) and lse32 (rounded to f32), the float64 backward OF THOSE INPUTS and
    the ideal 16-bit backward of them (``attn_backward_of`` does the same for any other ctx / lse, the device forward's in
    the chained test)."""
    q, k, v, do = attn_inputs(cls, T, dtype)
    ctx, lse = attention_forward(q, k, v, mask, keep)
    ctx16, lse32 = rd(ctx, dtype), lse.float().to(F64)
    c = SimpleNamespace(cls=cls, T=T, dtype=dtype, q=q, k=k, v=v, do=do, ctx=ctx, lse=lse, ctx16=ctx16, lse32=lse32)
    c.qkv = torch.cat([unheads(t) for t in (q, k, v)], dim=-1).contiguous()            # [B, T, 3 H]
    c.dctx = unheads(do).contiguous()
    c.y_ctx = ideal16_forward(q, k, v, dtype, mask, keep)
    c.e_lse = lse_f32_error(q, k, lse)
    c.term_scale = {"dq": peaked_scale(k, v, do), "dk": peaked_scale(q, v, do)}
    c.mask, c.keep = mask, keep
    return attn_backward_of(c, ctx16, lse32)


def attn_backward_of(c: SimpleNamespace, ctx: torch.Tensor, lse: torch.Tensor) -> SimpleNamespace:
    """Sets the float64 backward (dq, dk, dv, delta, delta_terms) and the ideal 16-bit one (y_dq, y_dk, y_dv) of the case's
    inputs and THIS ctx / lse (float64 holding what the kernel is handed) on a copy of the case."""
    c = SimpleNamespace(**vars(c))
    c.dq, c.dk, c.dv, c.delta, c.delta_terms = attention_backward(c.q, c.k, c.v, c.do, ctx, lse, c.mask, c.keep)
    ys = [ideal16_backward(c.q, c.k, c.v, c.do, ctx, lse, c.dtype, c.mask, c.keep, sh) for sh in (0.0, 1.0, -1.0)]
    c.y_dq, c.y_dk, c.y_dv = (tuple(y[i] for y in ys) for i in range(3))          # three variants each, see EXP_F32
    return c


@functools.lru_cache(maxsize=32)
def attn_case(cls: str, T: int, dtype) -> SimpleNamespace:
    """attn_case_of without dropout.  Cached: read-only."""
    return attn_case_of(cls, T, dtype)


def judged_absolutely(ref, name: str, case: SimpleNamespace) -> bool:
    """dq / dk are judged absolutely on ``case.term_scale`` in the `peaked` class -- and wherever the whole reference is
    below SMALL_FRAC of that scale, the same convention one level up: at T = 1 dS is exactly zero (P = 1, dP = delta), and
    dk is exactly zero in `uniform` (q = 0)."""
    return name in ("dq", "dk") and (case.cls == "peaked" or
                                     float(ref.pow(2).mean().sqrt()) < SMALL_FRAC * case.term_scale[name])


def slice_errors(got, ref, name: str, case: SimpleNamespace):
    """Per-row errors [B, h, T] of one [B, h, T, d] quantity (`ctx`, `dq`, `dk`, `dv`): rel-L2 over the 64 elements of the
    row, small rows on the tensor's scale; see judged_absolutely."""
    return sliced_rel_l2(got, ref, 3, case.term_scale[name] if judged_absolutely(ref, name, case) else None)


def yard_errors(yard, ref, name: str, case: SimpleNamespace) -> torch.Tensor:
    """The ideal 16-bit attention's own per-row error: of one tensor, or the largest over a tuple of variants."""
    ys = yard if isinstance(yard, (tuple, list)) else (yard,)
    return torch.stack([slice_errors(y, ref, name, case)[0] for y in ys]).amax(dim=0)


def f32_term(ref, name: str, case: SimpleNamespace) -> float:
    """F32_TOL relative to a row's own size.  On the absolute scale (one product term) what is left in dS is the difference
    of two f32 dot products of d = 64 such terms, sqrt(d) times the scale: the f32 term is F32_TOL * sqrt(d) there."""
    return F32_TOL * (math.sqrt(AT_D) if judged_absolutely(ref, name, case) else 1.0)


def yard_bound(yard, ref, name: str, case: SimpleNamespace) -> torch.Tensor:
    """Per-row bound: YARD_FACTOR x the ideal 16-bit attention's own error on that row, plus the f32 term."""
    return YARD_FACTOR * yard_errors(yard, ref, name, case) + f32_term(ref, name, case)


def small_share_applies(cls: str, name: str) -> bool:
    """Where at most SMALL_CAP of the rows may be judged absolutely: not in `peaked` (by construction), and not for dK / dV
    of late_max / early_max, where a key RAMP_STEP_MAX * 28 = 7 below the maximum carries less than 1e-3 of a row's weight
    and most keys are further down: their dK / dV rows are small because the class says so."""
    return cls != "peaked" and not (cls in ("late_max", "early_max") and name in ("dk", "dv"))


def yard_capped(cls: str, dtype) -> bool:
    """Where the yardstick must stay under today's whole-tensor bounds: every class but `peaked` (judged absolutely on a
    cancellation) and fp16 `quiet_grad` (dS is subnormal by construction)."""
    return cls != "peaked" and not (cls == "quiet_grad" and dtype == torch.float16)


# ================================================================================================ source constants
def source_constants() -> dict:
    """The block caps and the geometry threshold as csrc/norm.hip and csrc/attention.hip spell them."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "w2v2_speaker_amd", "csrc")
    out = {}
    for fn, names in (("norm.hip", ("LN_BWD_BLOCKS", "LN_BWD_BLOCKS_Q")), ("attention.hip", ("ATTN_SMALL_GEOM_MAX_T",))):
        with open(os.path.join(root, fn)) as f:
            text = f.read()
        for nm in names:
            out[nm] = int(re.search(r"constexpr int %s = (\d+);" % nm, text).group(1))
    return out
