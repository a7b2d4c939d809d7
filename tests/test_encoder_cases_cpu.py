"""CPU checks of tests/encoder_cases.py: the float64 references, yardsticks and input classes that
tests/test_encoder_kernels_gpu.py holds csrc/norm.hip and csrc/attention.hip to are themselves right -- the explicit backward
formulas agree with float64 autograd, every yardstick stays under its cap, every input class has the property it is named
for, and at most SMALL_CAP of the slices of any reference are small enough to be judged absolutely."""
import math

import pytest
import torch
import torch.nn.functional as F

import encoder_cases as K

F64 = torch.float64


def say(line: str) -> None:
    print("encoder-parity: " + line)


def bernoulli_mask(shape, p: float, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) >= p).to(F64)


# ================================================================================================ layer norm
def test_large_m_follows_the_block_caps_of_the_source():
    """The grid-stride case is derived from the caps; a change of the caps in norm.hip must move it, not un-cover it."""
    src = K.source_constants()
    assert (src["LN_BWD_BLOCKS"], src["LN_BWD_BLOCKS_Q"]) == (K.LN_BWD_BLOCKS, K.LN_BWD_BLOCKS_Q)
    assert src["ATTN_SMALL_GEOM_MAX_T"] == K.ATTN_SMALL_GEOM_MAX_T
    for H in K.LN_H:
        cap, M = K.ln_block_cap(H), K.ln_large_m(H)
        assert M == 2 * 4 * cap + 5 and M <= 8197 and H <= 1024
        rows_of_wave = [len(range(w, M, 4 * cap)) for w in (0, 4, 5, 4 * cap - 1)]
        assert rows_of_wave == [3, 3, 2, 2]            # five waves walk three rows, the others two
    assert [K.ln_large_m(H) for H in K.LN_H] == [6149, 6149, 8197, 6149, 8197, 6149]
    assert K.ATTN_SMALL_GEOM_MAX_T in K.AT_T and K.ATTN_SMALL_GEOM_MAX_T + 1 in K.AT_T
    assert K.small_geom(129) and K.small_geom(193) and K.small_geom(1) and not K.small_geom(513)
    assert not K.small_geom(161) and not K.small_geom(512) and not K.small_geom(33)      # pad alike in both geometries
    assert {K.small_geom(T) for T in K.AT_T} == {True, False}


def test_every_backward_kernel_is_reached():
    reached = {K.ln_bwd_kernel(dt, H, mode) for dt in K.DTYPES for H in K.LN_H for mode in K.LN_BWD_MODES}
    assert reached == {"ln_bwd_kernel", "ln_bwd16_kernel", "ln_bwd16q_kernel"}
    assert K.ln_bwd_kernel(torch.bfloat16, 768, "none") == "ln_bwd16_kernel"
    assert K.ln_bwd_kernel(torch.float16, 512, "deferred") == "ln_bwd16q_kernel"


@pytest.mark.parametrize("cls", K.LN_CLASSES)
def test_layernorm_input_classes_are_what_they_say(cls):
    for H in K.LN_H:
        for M in (37, 300):
            s = K.ln_s(cls, M, H).to(F64)
            mean, sd = s.mean(dim=1), s.var(dim=1, unbiased=False).sqrt()
            if cls == "unit":
                assert float(mean.abs().max()) < 2.5 and 0.3 < float(sd.min()) and float(sd.max()) < 2.0
            elif cls == "offset":
                rstd = (sd ** 2 + K.EPS).rsqrt()
                assert float((mean - 30).abs().max()) < 1.2 and 6 < float(rstd.min()) and float(rstd.max()) < 30
                assert len(set((mean[:5] * 2).round().tolist())) == 5          # the mean moves from row to row
            elif cls == "outlier":
                big = s.abs() >= 50
                assert bool((big.sum(dim=1) == 2).all())
                rest_sd = torch.where(big, torch.zeros_like(s), s).pow(2).sum(dim=1).div(H - 2).sqrt()
                assert 0.2 < float(rest_sd.min()) and float(rest_sd.max()) < 2.2
            else:
                assert float(sd.max()) == 0.0 and len(set(mean.tolist())) == 9
                for dtype in K.DTYPES:                                          # exact in all three types
                    assert torch.equal(K.ln_s(cls, M, H).to(dtype).to(F64), s)


@pytest.mark.parametrize("cls", K.LN_CLASSES)
def test_layernorm_backward_formulas_agree_with_float64_autograd(cls):
    """With mean / rstd the true statistics (held in float64 here), the explicit formulas are layer_norm's gradient; with a
    mask, d_r is the gradient of the residual branch of x + r * mask."""
    worst = 0.0
    for M, H in ((3, 8), (37, 520), (300, 768)):
        s = K.ln_s(cls, M, H).to(F64)
        gamma, beta = (t.to(F64) for t in K.ln_params(H))
        dy = K.rnd(M, H, seed=5).to(F64)
        mask = bernoulli_mask((M, H), K.LN_P, 7) / (1 - K.LN_P)
        x = (s - K.ln_residual("unit", M, H).to(F64) * mask).requires_grad_(True)
        r = K.ln_residual("unit", M, H).to(F64).requires_grad_(True)
        ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        F.layer_norm(x + r * mask, (H,), ga, be, K.EPS).backward(dy)
        sx = (x + r * mask).detach()
        mean, rstd = sx.mean(dim=1), (sx.var(dim=1, unbiased=False) + K.EPS).rsqrt()
        got = K.ln_backward(dy, sx, mean, rstd, gamma, mask)
        # zero variance: autograd's own s - mean roundoff is multiplied by rstd = 316 twice
        tol = 1e-12 if cls != "const" else 1e-7
        for a, b in ((got.ds, x.grad), (got.d_r, r.grad), (got.dgamma, ga.grad), (got.dbeta, be.grad)):
            e = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
            worst = max(worst, e)
            assert e < tol, (M, H, e)
        assert bool((got.terms_g >= got.dgamma.abs() * (1 - 1e-12)).all()) and bool((got.terms_b >= got.dbeta.abs() * (1 - 1e-12)).all())
    say(f"cpu layer-norm backward formulas vs autograd (f64) {cls}: max |error| / max |grad| {worst:.2e}")


@pytest.mark.parametrize("cls", K.LN_CLASSES)
def test_layernorm_statistics_yardstick_stays_under_its_caps(cls):
    """2^-22 + 8 x yardstick means something only while the yardstick is small: an f32 two-pass loses nothing to
    E[s^2] - mean^2, whatever the class."""
    wm = wr = 0.0
    for H in K.LN_H:
        for dtype in K.DTYPES:
            for variant in K.LN_FWD_VARIANTS:
                for M in K.LN_M_SMALL:
                    x, r = K.ln_fwd_inputs(cls, M, H, dtype, variant)
                    mask = (bernoulli_mask((M, H), K.LN_P, 9).float() * (1 / torch.tensor(1 - K.LN_P, dtype=torch.float32))
                            if variant.endswith("dropout") else None)
                    gamma, beta = K.ln_params(H)
                    ref = K.ln_forward(x, r, mask, gamma, beta)
                    s32 = x if r is None else K.ln_f32_sums(x, r, mask)[0]
                    e_m, e_r = K.ln_stats_errors(*K.ln_ideal_f32_stats(s32), ref)
                    wm, wr = max(wm, e_m / float(ref.amp.max())), max(wr, e_r / float(ref.amp.max()))
                    if r is not None:          # the two f32 evaluations of the sum differ by at most one f32 rounding
                        a, b = K.ln_f32_sums(x, r, mask)
                        scale = x.abs() + (r * (1 if mask is None else mask)).abs()
                        assert bool(((a - b).abs() <= 2.0 ** -23 * scale).all())
                        if mask is None:
                            assert torch.equal(a, b)
                    if cls == "const":
                        assert float((ref.y - beta.to(F64)).abs().max()) == 0.0
                        assert float((ref.rstd - K.EPS ** -0.5).abs().max()) < 1e-9
    say(f"cpu layer-norm ideal f32 two-pass statistics {cls}, over max(1, rms_s * rstd): |d mean| * rstd {wm:.2e}; "
        f"rel |d rstd| {wr:.2e}; cap {K.CAP_STATS:.2e}")
    assert wm < K.CAP_STATS and wr < K.CAP_STATS


@pytest.mark.parametrize("cls", K.LN_CLASSES)
def test_layernorm_small_slice_share(cls):
    """Rows of y, ds and d_r and columns of dgamma / dbeta judged absolutely: at most SMALL_CAP of them."""
    worst = 0.0
    for H in K.LN_H:
        for M in K.LN_M_SMALL + ((K.ln_large_m(H),) if cls in K.LN_LARGE_CLASSES and H in (8, 512) else ()):
            c = K.ln_bwd_case(cls, M, H, torch.bfloat16)
            gamma, beta = K.ln_params(H)
            y = K.ln_forward(c.s, None, None, gamma, beta).y
            for t in (y, c.ref.ds):
                worst = max(worst, float(K.sliced_rel_l2(t, t, 1)[1].double().mean()))
            if M >= 37:                        # a column sum over one or three rows is one or three products
                for t, terms in ((c.ref.dgamma, c.ref.terms_g), (c.ref.dbeta, c.ref.terms_b)):
                    if float(terms.max()) > 0:
                        worst = max(worst, float((terms < K.SMALL_FRAC * terms.mean()).double().mean()))
    say(f"cpu layer-norm small-slice share {cls}: {worst:.4f} cap {K.SMALL_CAP}")
    assert worst <= K.SMALL_CAP


# ================================================================================================ attention
@pytest.mark.parametrize("cls", K.AT_CLASSES)
def test_attention_input_classes_are_what_they_say(cls):
    for dtype in K.LP:
        for T in K.AT_T:
            q, k, v, do = K.attn_inputs(cls, T, dtype)
            for t in (q, k, v, do):
                assert torch.equal(K.rd(t, dtype), t)                           # representable in the type
            s = K.scores(q, k)
            ctx, lse = K.attention_forward(q, k, v)
            if cls == "uniform":
                assert float(s.abs().max()) == 0.0
                assert float((lse - math.log(T)).abs().max()) < 1e-14
                assert float((ctx - v.mean(dim=2, keepdim=True)).abs().max()) < 1e-14
            elif cls in ("late_max", "early_max"):
                want = T - 1 if cls == "late_max" else 0
                assert bool((s.argmax(dim=-1) == want).all())
                span = float((s.amax(dim=-1) - s.amin(dim=-1)).max())
                assert span <= K.RAMP_SPAN + 0.5 and abs(span - (T - 1) * K.ramp_step(T)) < 0.5, (T, span)
                assert T < 97 or span >= 17             # e^-17 < 2^-24: below the smallest fp16
                # the f32 yardstick's exp2 stays normal: 2^(-span * log2 e) is far above 2^-126
                assert span * 1.4427 < 120
                for tile in (32, 64):                                           # the running maximum of every tile
                    tmax = torch.stack([s[..., t0:t0 + tile].amax(dim=-1) for t0 in range(0, T, tile)], dim=-1)
                    run = tmax.cummax(dim=-1).values
                    if cls == "late_max":                                       # every tile raises it
                        assert bool((tmax[..., 1:] > run[..., :-1]).all())
                    else:                                                       # alpha = 1 after the first tile
                        assert bool((run == tmax[..., :1]).all())
                if cls == "early_max" and T >= 512:                             # later probabilities underflow in fp16
                    assert float(torch.exp(s - s.amax(dim=-1, keepdim=True)).amin()) < 2.0 ** -24
            elif cls == "peaked":
                key = K.peaked_key(T)
                assert int(key[0]) == T - 1 and bool((s.argmax(dim=-1) == key).all())
                if T > 1:
                    top2 = s.topk(2, dim=-1).values
                    assert float((top2[..., 0] - top2[..., 1]).min()) >= K.PEAK_GAP, T
                    assert float((ctx - v[:, :, key]).abs().max()) < 1e-10      # ctx is v[key]
            elif cls == "loud":
                assert 55 < float(s.abs().min()) and float(s.abs().max()) < 105 and float(lse.abs().min()) > 60
                assert bool((s[:, :, 0::2] > 0).all()) and bool((s[:, :, 1::2] < 0).all())
                plain = torch.exp(s.float())            # no maximum subtracted: beyond fp16, and below the normal f32
                assert float(plain[:, :, 0::2].min()) > 65504 and (T < 2 or float(plain[:, :, 1::2].max()) < 2.0 ** -78)
            elif cls == "quiet_grad":
                assert float(do.abs().max()) < 2.0 ** -9
                if T >= 33:                # dS is below the smallest normal fp16 (2^-14) for almost every pair
                    dq, dk, dv, _, _ = K.attention_backward(q, k, v, do, ctx, lse)
                    p = torch.exp(s - lse[..., None])
                    ds = p * (do @ v.transpose(2, 3) - (do * ctx).sum(-1, keepdim=True)) * K.AT_SCALE
                    assert float((ds.abs() < 2.0 ** -14).double().mean()) > 0.95
            else:
                assert 0.5 < float(s.std()) < 4 if T > 1 else True


@pytest.mark.parametrize("cls", K.AT_CLASSES)
def test_attention_backward_formulas_agree_with_float64_autograd(cls):
    """Handed the exact ctx and lse, the explicit backward is autograd's, with and without a dropout mask."""
    worst = 0.0
    for T in (1, 17, 65, 161):
        q, k, v, do = K.attn_inputs(cls, T, torch.bfloat16)
        for mask in (None, bernoulli_mask((K.AT_B, K.AT_HEADS, T, T), K.AT_P, 5)):
            keep = 1 - K.AT_P if mask is not None else 1.0
            qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
            p = torch.softmax(K.scores(qa, ka), dim=-1)
            if mask is not None:
                p = p * mask / keep
            out = p @ va
            out.backward(do)
            ctx, lse = K.attention_forward(q, k, v, mask, keep)
            assert float((ctx - out.detach()).abs().max()) < 1e-12
            dq, dk, dv, delta, terms = K.attention_backward(q, k, v, do, ctx, lse, mask, keep)
            for a, b in ((dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
                scale = max(float(b.abs().max()), K.peaked_scale(k, v, do), K.peaked_scale(q, v, do))       # (T = 1: dq = dk = 0)
                e = float((a - b).abs().max()) / scale
                worst = max(worst, e)
                assert e < 1e-10, (T, e)
            assert bool((terms >= delta.abs() * (1 - 1e-12)).all())
    say(f"cpu attention backward formulas vs autograd (f64) {cls}: max |error| / max |grad| {worst:.2e}")


@pytest.mark.parametrize("dtype", K.LP, ids=K.NAME.get)
@pytest.mark.parametrize("cls", K.AT_CLASSES)
def test_attention_yardstick_caps_and_small_slice_share(cls, dtype):
    """The ideal 16-bit attention's own worst row stays under today's whole-tensor bounds (8e-3 ctx, 2e-2 dqkv) for every
    class but `peaked` and fp16 `quiet_grad`, so 2 x yardstick never asks less than half of what is asserted today per
    TENSOR of any single ROW; and at most SMALL_CAP of the rows of a reference are judged absolutely."""
    wc = wg = wl = share = 0.0
    for T in K.AT_T:
        c = K.attn_case(cls, T, dtype)
        for name, yard, ref in (("ctx", c.y_ctx, c.ctx), ("dq", c.y_dq, c.dq), ("dk", c.y_dk, c.dk), ("dv", c.y_dv, c.dv)):
            err, small = K.yard_errors(yard, ref, name, c), K.slice_errors(ref, ref, name, c)[1]
            assert bool(torch.isfinite(err).all())
            if name == "ctx":
                wc = max(wc, float(err.max()))
            else:
                wg = max(wg, float(err.max()))
            # (a tensor judged absolutely as a whole -- dq / dk where dS is exactly zero -- has no small ROWS: rows cannot all
            # lie below 1e-3 of their own RMS)
            if K.small_share_applies(cls, name) and not bool(small.all()):
                share = max(share, float(small.double().mean()))
        wl = max(wl, c.e_lse / float(c.lse.abs().clamp_min(1.0).max()))
    say(f"cpu ideal 16-bit attention {K.NAME[dtype]} {cls}: worst row ctx {wc:.2e} cap {K.CAP_YARD_CTX:.0e}; dq/dk/dv {wg:.2e} "
        f"cap {K.CAP_YARD_DQKV:.0e}{'' if K.yard_capped(cls, dtype) else ' (not capped)'}; f32 lse error / max(1, |lse|) {wl:.2e}; "
        f"small rows {share:.4f} cap {K.SMALL_CAP}")
    assert wl < 1e-5
    if K.yard_capped(cls, dtype):
        assert wc < K.CAP_YARD_CTX and wg < K.CAP_YARD_DQKV
    assert share <= K.SMALL_CAP


def test_sliced_rel_l2_flags_one_bad_row_that_a_tensor_norm_hides():
    ref = K.rnd(2, 2, 513, 64, seed=1).to(F64)
    got = ref.clone()
    got[1, 0, 300] = ref[1, 0, 301]                     # one row takes its neighbour's values
    whole = float((got - ref).norm() / ref.norm())
    err, _ = K.sliced_rel_l2(got, ref, 3)
    assert whole < 0.05 and float(err.max()) > 1.0 and int((err > 0).sum()) == 1
    nan = ref.clone()
    nan[0, 0, 0, 0] = float("nan")
    assert math.isinf(float(K.sliced_rel_l2(nan, ref, 3)[0].max()))
