"""The tap gather and its adjoint (csrc/tap_gather.h) through the eight entry points that reach them, at the edges where
the three families used to differ: no padding against zero padding at pad = 0, frames that do not tile the input, mirror
images that coincide or stack, zero against reflect padding, and the workgroup-uniform fast path of the variable-length
gather.  All inputs are small integers (tests/tap_gather_cases.py), so every comparison is bit equality against float64."""
import pytest
import torch

import ecapa_stage_cases as E
import tap_gather_cases as K
from w2v2_speaker_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
NAN = float("nan")


def _same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and a.view(torch.uint8).equal(b.view(torch.uint8))


def _exact(got: torch.Tensor, ref64: torch.Tensor) -> bool:
    """Bit equality with the float64 result: the same values (no NaN), and no negative zero where float64 has +0.0."""
    g = got.cpu().to(F64).reshape(ref64.shape)
    return bool(torch.equal(g, ref64)) and not bool((torch.signbit(g) & (ref64 == 0)).any())


# ------------------------------------------------------------------------------------------------ 1. pad = 0
@pytest.mark.parametrize("Lout", [1, 2, 5])
@pytest.mark.parametrize("k,stride", [(10, 5), (3, 2), (2, 2)])
def test_zero_adjoint_at_pad_0_is_col2im(k, stride, Lout):
    B, C = 2, 8
    Lin = (Lout - 1) * stride + k + 1                       # one row more than the frames reach
    assert K.frames_of(Lin, k, stride, 0) == Lout
    d = K.ints((B * Lout, k * C), 1000 * k + 10 * stride + Lout)
    dz = torch.full((B * Lin, C), NAN, device=DEV)
    dc = torch.full((B * Lin, C), NAN, device=DEV)
    ops.col2im_zero(d.to(DEV, F32), dz, C, B, Lin, C, k, stride, 0)
    ops.col2im(d.to(DEV, F32), dc, B, Lin, Lout, C, k, stride)
    ref = K.adjoint_ref(d, B, Lin, Lout, C, k, stride, 1, 0, "zero")
    assert _same_bytes(dz, dc)
    assert _exact(dz, ref) and _exact(dc, ref)
    assert not bool(dc.view(B, Lin, C)[:, Lin - 1].any()) and not bool(ref[:, Lin - 1].any())


# ------------------------------------------------------------------------------------------------ 2. frames that do not tile
@pytest.mark.parametrize("Tin", [2, 7])
@pytest.mark.parametrize("k,s,p", [(5, 4, 2), (3, 2, 1), (3, 1, 1)])
def test_zero_gather_and_adjoint_where_frames_do_not_tile_the_input(k, s, p, Tin):
    B, C = 2, 4
    ld, Tout = C + 4, K.frames_of(Tin, k, s, p)
    x = K.ints((B * Tin, ld), 100 * k + 10 * s + Tin)
    col = torch.full((B * Tout, k * C), NAN, device=DEV)
    ops.im2col_zero(x.to(DEV, F32), ld, col, B, Tin, C, k, s, p)
    assert _exact(col, K.gather_ref(x[:, :C].reshape(B, Tin, C), Tout, k, s, 1, p, "zero"))     # padding entries: +0.0
    d = K.ints((B * Tout, k * C), 100 * k + 10 * s + Tin + 1)
    dx = torch.full((B * Tin, ld), NAN, device=DEV)
    ops.col2im_zero(d.to(DEV, F32), dx, ld, B, Tin, C, k, s, p)
    assert bool(torch.isnan(dx[:, C:]).all())                                                 # the C channels only
    assert _exact(dx[:, :C], K.adjoint_ref(d, B, Tin, Tout, C, k, s, 1, p, "zero"))          # unreached rows: +0.0


# ------------------------------------------------------------------------------------------------ 3. mirror images
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k,dil,T", [(3, 1, 2), (3, 3, 4), (5, 1, 3), (3, 2, 3)])
def test_reflect_adjoint_where_the_mirror_images_coincide_or_stack(k, dil, T, dtype, accumulate):
    B, C = 2, 8
    ld = C + 8
    d = K.ints((B * T, k * C), 100 * k + 10 * dil + T)
    prior = K.ints((B * T, ld), 100 * k + 10 * dil + T + 1)
    dx = prior.to(DEV, dtype)
    ops.col2im_reflect(d.to(DEV, dtype), dx, ld, B, T, C, k, dil, accumulate)
    ref = E.col2im_reflect(d, B, T, C, k, dil)              # float64 autograd adjoint of the float64 reflect gather
    assert torch.equal(ref, K.adjoint_ref(d, B, T, T, C, k, 1, dil, (k - 1) // 2 * dil, "reflect").reshape(B * T, C))
    if accumulate:
        ref = ref + prior[:, :C]
    assert _exact(dx[:, :C], ref)
    assert _same_bytes(dx[:, C:], prior[:, C:].to(dtype))                                     # columns past Cin untouched


# ------------------------------------------------------------------------------------------------ 4. zero against reflect
def test_zero_and_reflect_gathers_agree_on_interior_rows_and_differ_in_the_out_of_range_tap():
    B, T, C, k = 2, 5, 8, 3
    x = K.ints((B * T, C), 4)
    xd = x.to(DEV, F32)
    cz = torch.full((B * T, k * C), NAN, device=DEV)
    cr = torch.full((B * T, k * C), NAN, device=DEV)
    ops.im2col_zero(xd, C, cz, B, T, C, k, 1, 1)
    ops.im2col_reflect(xd, C, cr, B, T, C, k, 1)
    xb = x.reshape(B, T, C)
    assert _exact(cz, K.gather_ref(xb, T, k, 1, 1, 1, "zero")) and _exact(cr, K.gather_ref(xb, T, k, 1, 1, 1, "reflect"))
    cz, cr = cz.view(B, T, k, C).cpu(), cr.view(B, T, k, C).cpu()
    assert _same_bytes(cz[:, 1:T - 1], cr[:, 1:T - 1])
    xf = xb.float()
    for t, j, mirror in ((0, 0, 1), (T - 1, k - 1, T - 2)):                      # the tap at position -1 and at position T
        others = [q for q in range(k) if q != j]
        assert _same_bytes(cz[:, t, others], cr[:, t, others])
        assert _same_bytes(cz[:, t, j], torch.zeros(B, C)) and _same_bytes(cr[:, t, j], xf[:, mirror])


# ------------------------------------------------------------------------------------------------ 5. variable length
@pytest.mark.parametrize("with_x2", [False, True], ids=["x", "x+x2"])
@pytest.mark.parametrize("C", [8, 64])
def test_variable_length_gather_at_the_fast_path_edge(C, with_x2):
    """A workgroup takes 256 consecutive 16-byte vectors of col.  C = 8 (3 vectors per row: all 80 rows in one workgroup,
    which spans both utterances, so the fast path must not fire); C = 64 (24 vectors per row, 10 2/3 rows per workgroup:
    workgroup 3 holds the end of utterance 0 and the first valid rows of utterance 1, workgroup 4 starts inside valid row 2
    and straddles the last valid row, workgroups 5 to 7 see only padding rows of utterance 1: the fast path)."""
    B, T, k, dil = 2, 40, 3, 1
    lens = [40, 4]
    x = K.ints((B * T, C), 7 + C)
    x2 = K.ints((B * T, C), 8 + C) if with_x2 else None
    xd, x2d = x.to(DEV, BF16), (x2.to(DEV, BF16) if with_x2 else None)
    col = torch.full((B * T, k * C), NAN, device=DEV, dtype=BF16)
    ops.im2col_reflect_len(xd, C, col, torch.tensor(lens, dtype=torch.int32, device=DEV), B, T, C, k, dil, x2=x2d, ldx2=C)
    col = col.view(B, T, k * C)
    xs = (x + x2 if with_x2 else x).reshape(B, T, C)
    for b, n in enumerate(lens):
        alone = torch.full((n, k * C), NAN, device=DEV, dtype=BF16)
        ops.im2col_reflect(xd.view(B, T, C)[b, :n].contiguous(), C, alone, 1, n, C, k, dil,
                           x2=x2d.view(B, T, C)[b, :n].contiguous() if with_x2 else None, ldx2=C)
        assert _same_bytes(col[b, :n], alone)                                     # the fixed-length gather of the slice
        assert _exact(col[b, :n], K.gather_ref(xs[b:b + 1, :n], n, k, 1, dil, (k - 1) // 2 * dil, "reflect"))
        assert _same_bytes(col[b, n:], torch.zeros(T - n, k * C, dtype=BF16))     # rows past the length: +0.0
