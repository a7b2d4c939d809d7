"""CPU checks of tests/conv0_cases.py: the float64 references and yardsticks that tests/test_conv0_gpu.py holds the kernels
of csrc/conv0.hip to are themselves right, and the bounds derived from them are meaningful at every case of the GPU file."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv0_cases as K

F64 = torch.float64


@pytest.mark.parametrize("cls", K.BWD_CLASSES)
@pytest.mark.parametrize("L,C", [(1, 96), (129, 96), (300, 320)])
def test_backward_formulas_agree_with_float64_autograd(cls, L, C):
    ref = K.forward_ref(cls, L, C)
    dz = K.bwd_dz(L, C, torch.float32)
    w = ref.w.to(F64).requires_grad_(True)
    ga, be = ref.gamma.to(F64).requires_grad_(True), ref.beta.to(F64).requires_grad_(True)
    u = F.conv1d(ref.wav[:, None].to(F64), w, stride=ref.stride)
    out = K.gelu(F.group_norm(u, C, ga, be, eps=K.EPS)).transpose(1, 2)
    # the closed-form forward is group_norm's (one frame: group_norm's own roundoff in u - mean, times 1 / sqrt(eps))
    assert K.rel_l2(out.detach(), ref.out) < (1e-12 if L > 1 else 1e-9)
    out.backward(dz)
    dw, dgamma, dbeta, terms, plain = K.layer0_backward(ref, dz)
    if L == 1:      # var = 0: du, dw and dgamma are exactly zero
        assert float(dw.abs().max()) == 0 and float(dgamma.abs().max()) == 0 and float(plain.abs().max()) == 0
    else:           # the scale is sum |du * x| but for the rounding floor of du's own terms: 2 to 3 % from 129 frames on
        assert bool((terms >= plain).all()) and bool((terms <= 1.03 * plain).all()), float((terms / plain).max())
    e_w = K.sum_scale_error(dw, w.grad[:, 0], terms)
    e_g, e_b = K.rel_l2(dgamma, ga.grad), K.rel_l2(dbeta, be.grad)
    if L == 1:
        e_g = float((dgamma - ga.grad).abs().max() / dbeta.abs().max())
    # one frame: autograd forms u - mean(u) in floating point where the formulas have an exact zero, and 1 / sqrt(eps)
    # multiplies what is left of |u|: its own roundoff is 2^-52 |u| rstd, not 2^-52
    cond = max(1.0, float((ref.u.abs().amax(dim=2) * ref.rstd).max())) if L == 1 else 1.0
    print(f"conv0-parity: cpu backward formulas vs autograd (f64) {cls} L={L} C={C}: dw/sum|terms| {e_w:.2e} bound 1e-12; "
          f"dgamma {e_g:.2e} dbeta {e_b:.2e} bound {1e-12 * cond:.1e}")
    assert e_w < 1e-12 and e_g < 1e-12 * cond and e_b < 1e-12 * cond
    assert bool((terms >= dw.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("cls", K.CLASSES)
def test_ideal_f32_stats_stay_under_the_caps(cls):
    """The yardstick of the f32 statistics routes is a small number at every case the GPU file uses: a bound of
    2^-22 + 8 x yardstick cannot be met by a kernel that loses digits to E[u^2] - mean^2."""
    worst_m = worst_r = worst_1 = 0.0
    for L in K.STATS_L:
        for C in K.STATS_C:
            e_mean, e_rstd = K.yardstick(cls, L, C)
            worst_r = max(worst_r, e_rstd)
            if L == 1:
                # one frame: the "mean" is one f32 convolution output and rstd = 1 / sqrt(eps) = 316 multiplies its plain
                # rounding, whatever the kernel; CAP_E_MEAN cannot hold (loud: |u| ~ 40, half an ulp of 40 times 316 is
                # 6e-4), so the yardstick is held to the FMA chain's own bound instead
                ref = K.forward_ref(cls, L, C)
                chain = float(((ref.k + 1) * 2.0 ** -24 * ref.absu[..., 0] * ref.rstd).max())
                assert e_mean <= chain, (cls, C, e_mean, chain)
                worst_1 = max(worst_1, e_mean)
            else:
                worst_m = max(worst_m, e_mean)
    print(f"conv0-parity: cpu ideal-f32 statistics vs float64 {cls}: e_mean {worst_m:.2e} cap {K.CAP_E_MEAN:.0e} "
          f"(one frame: {worst_1:.2e}, held to the FMA chain's bound) e_rstd {worst_r:.2e} cap {K.CAP_E_RSTD:.0e}")
    assert worst_m <= K.CAP_E_MEAN and worst_r <= K.CAP_E_RSTD


def test_const_class_has_rstd_of_eps_alone():
    ref = K.forward_ref("const", 641, 96)
    assert float((ref.rstd * math.sqrt(K.EPS) - 1).abs().max()) < 1e-12
    m, r = K.ideal_f32_stats(ref.wav, ref.w, ref.stride)
    assert float((r * math.sqrt(K.EPS) - 1).abs().max()) < 2.0 ** -23


def test_rows_differ_and_three_samples_trail():
    for cls in K.CLASSES[:4]:
        wav = K.waveform(cls, 17)
        assert wav.shape == (2, 16 * 5 + 10 + 3) and not torch.equal(wav[0], wav[1])
    assert K.forward_ref("unit", 17, 96).u.shape == (2, 96, 17)


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_few_slices_are_judged_absolutely(dtype):
    """No more than 2 % of the frames or channels of any apply case fall under the small-norm rule, so the per-slice
    rel-L2 of the GPU file is a relative measure almost everywhere; and a perfect kernel (the reference rounded to the
    output format) passes the bounds."""
    for cls in K.APPLY_CLASSES:
        for L in K.APPLY_L:
            for C in K.APPLY_C:
                ref = K.forward_ref(cls, L, C)
                if K.degenerate(ref):
                    continue
                got = ref.out.float().to(dtype)
                bf, bc = K.apply_bounds(ref, dtype)
                for dim, bound in ((2, bf), (1, bc)):
                    err, small = K.sliced_rel_l2(got, ref.out, dim)
                    assert float(small.double().mean()) <= K.SMALL_CAP, (cls, L, C, dim)
                    assert bool((err <= bound).all()), (cls, L, C, dim, float((err / bound).max()))


def test_split_bf16_floor_is_far_below_the_16_bit_bound_where_the_variance_is_not_zero():
    """The matrix-core route's own error (split-bf16 product, float64 statistics) before the output rounding: a tenth of
    4e-3 at most on every non-degenerate apply case, so the project's 16-bit figure stands unscaled there; at one frame
    (var = 0) it is amplified 1 / sqrt(eps) times and rel-L2 against gelu(beta) cannot be bounded by 4e-3 -- those cases are
    held to degenerate_abs_bound, which the split product meets."""
    worst = 0.0
    for cls in K.APPLY_CLASSES:
        for L in K.APPLY_L:
            ref = K.forward_ref(cls, L, 128)
            got = K.split_bf16_out(ref)
            if K.degenerate(ref):
                bound = K.degenerate_abs_bound(ref, torch.bfloat16)
                assert bool(((got - ref.out).abs() <= 0.5 * bound).all()), (cls, L)
                continue
            for dim in (2, 1):
                worst = max(worst, float(K.sliced_rel_l2(got, ref.out, dim)[0].max()))
    one = K.forward_ref("unit", 1, 128)
    e1 = float(K.sliced_rel_l2(K.split_bf16_out(one), one.out, 2)[0].max())
    print(f"conv0-parity: cpu split-bf16 floor (f64 statistics) per slice: worst {worst:.2e} (var > 0) bound {K.LP_TOL / 10:.0e}; "
          f"one frame, unit: {e1:.2e} rel-L2, held to the absolute bound instead")
    assert worst <= K.LP_TOL / 10


@pytest.mark.parametrize("k,stride", K.COL2IM_KS)
def test_col2im_inputs_sum_exactly_in_bf16(k, stride):
    for cin in K.COL2IM_CIN:
        for lout in K.COL2IM_LOUT:
            col, lin, dx = K.col2im_case(k, stride, cin, lout)
            assert lin == (lout - 1) * stride + k + 1 and float(col.abs().max()) <= 64
            for dtype in K.DTYPES:
                assert torch.equal(col.to(dtype).to(F64), col) and torch.equal(dx.to(dtype).to(F64), dx)
            assert float(dx[:, -1].abs().max()) == 0 and float(dx.abs().max()) > 0
            # the fold is the adjoint of the unfold
            x = K.rnd(K.B, lin, cin, seed=3).to(F64)
            cols = x.unfold(1, k, stride)[:, :lout].permute(0, 1, 3, 2).reshape(K.B * lout, k * cin)
            assert abs(float((cols * col).sum() - (x * dx).sum())) < 1e-9 * float((x * dx).abs().sum() + 1)


def test_pack_ref_matches_the_implicit_gemm_layout():
    w = K.rnd(5, 3, 2, seed=1).to(F64)
    x = K.rnd(2, 9, 3, seed=2).to(F64)                                                  # channels last
    ref = F.conv1d(x.transpose(1, 2), w, stride=2).transpose(1, 2)
    cols = x.unfold(1, 2, 2).permute(0, 1, 3, 2).reshape(2, 4, 6)                       # K index = tap * Cin + ci
    assert K.rel_l2(cols @ K.pack_ref(w).t(), ref) < 1e-14
