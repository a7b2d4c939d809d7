"""GPU unit tests: every C-ABI kernel against a plain torch f32/f64 reference of the same op
(floating-point kernels -> torch reference; tolerances stated per test).  Run with -m gpu."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


LP16 = [torch.bfloat16, torch.float16]      # the two 16-bit activation formats of the matrix-core kernels


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


# ----------------------------------------------------------------------------------------------- GEMM
def _gemm_case(o, M, N, K, ta, tb, dtype, cdtype, epi="none", split=1, seed=0):
    A = rnd(M, K, seed=seed + 1, scale=0.5)
    Bm = rnd(N, K, seed=seed + 2, scale=0.5)
    if dtype != torch.float32:
        A, Bm = A.to(dtype).float(), Bm.to(dtype).float()
    ref = A.double() @ Bm.double().t()
    Ad = (A.t().contiguous() if ta else A).to(dtype).to(DEV)
    Bd = (Bm.t().contiguous() if tb else Bm).to(dtype).to(DEV)
    lda = M if ta else K
    ldb = N if tb else K
    ldc = (N + 3) // 4 * 4
    C = torch.zeros(M, ldc, dtype=cdtype, device=DEV)
    kw = {}
    bias = rnd(N, seed=seed + 3)
    aux_host = rnd(M, ldc, seed=seed + 4)
    if cdtype != torch.float32:
        aux_host = aux_host.to(cdtype).float()
    aux = None
    if epi == "bias":
        kw.update(epilogue=o.EPI_BIAS, bias=bias.to(DEV))
        ref = ref + bias.double()
    elif epi == "bias_gelu":
        aux = torch.zeros(M, ldc, dtype=cdtype, device=DEV)
        kw.update(epilogue=o.EPI_BIAS_GELU, bias=bias.to(DEV), aux=aux, ldaux=ldc)
        pre = ref + bias.double()
        ref = gelu(pre)
    elif epi == "gelu_bwd":
        aux = aux_host.to(cdtype).to(DEV)
        kw.update(epilogue=o.EPI_GELU_BWD, aux=aux, ldaux=ldc)
        a = aux_host[:, :N].double()
        ref = ref * (0.5 * (1 + torch.erf(a / math.sqrt(2))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi))
    elif epi == "bias_gelu_grad":
        aux = torch.zeros(M, ldc, dtype=cdtype, device=DEV)
        kw.update(epilogue=o.EPI_BIAS_GELU_GRAD, bias=bias.to(DEV), aux=aux, ldaux=ldc)
        x = ref + bias.double()
        pre = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)   # aux = gelu'
        ref = gelu(x)
    elif epi == "mul":
        aux = aux_host.to(cdtype).to(DEV)
        kw.update(epilogue=o.EPI_MUL, aux=aux, ldaux=ldc)
        ref = ref * aux_host[:, :N].double()
    elif epi == "add":
        aux = aux_host.to(cdtype).to(DEV)
        kw.update(epilogue=o.EPI_ADD, aux=aux, ldaux=ldc)
        ref = ref + aux_host[:, :N].double()
    elif epi == "scale_rc":
        rs, cs = rnd(M, seed=seed + 5).abs() + 0.5, rnd(N, seed=seed + 6).abs() + 0.5
        kw.update(epilogue=o.EPI_SCALE_RC, row_scale=rs.to(DEV), col_scale=cs.to(DEV))
        ref = ref * rs.double()[:, None] * cs.double()[None, :]
    o.gemm(M, N, K, Ad, Bd, C, lda=lda, ldb=ldb, ldc=ldc, transA=ta, transB=tb, alpha=1.0, split_k=split, **kw)
    torch.cuda.synchronize()
    got = C[:, :N].float().cpu().double()
    tol = 2e-5 if dtype == torch.float32 else (1.2e-2 if cdtype != torch.float32 else 2e-3)
    err = rel_l2(got, ref)
    assert err < tol, (M, N, K, ta, tb, dtype, cdtype, epi, split, err)
    if epi in ("bias_gelu", "bias_gelu_grad"):
        assert rel_l2(aux[:, :N].float().cpu().double(), pre) < tol
    assert float(C[:, N:].abs().max()) == 0.0 if ldc > N else True     # no out-of-bounds columns written


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("lp", LP16)
def test_gemm_bf16_layouts_and_ragged_shapes(ta, tb, lp):
    o = ops()
    for (M, N, K) in [(256, 256, 128), (149, 48, 96), (300, 130, 200), (66, 5994, 72), (1000, 64, 6144 // 8)]:
        _gemm_case(o, M, N, K, ta, tb, lp, torch.float32)
    _gemm_case(o, 298, 768, 256, ta, tb, lp, lp)


@pytest.mark.parametrize("lp", LP16)
def test_gemm_bf16_identity_asymmetric(lp):
    """A = I with an asymmetric B: catches a transposed C write (guide rule 16)."""
    o = ops()
    n = 128
    Bm = torch.arange(n * n, dtype=torch.float32).view(n, n) % 251
    A = torch.eye(n)
    C = torch.zeros(n, n, dtype=torch.float32, device=DEV)
    o.gemm(n, n, n, A.to(lp).to(DEV), Bm.to(lp).to(DEV), C, lda=n, ldb=n, ldc=n)
    torch.cuda.synchronize()
    assert torch.equal(C.cpu(), Bm.to(lp).float().t())


@pytest.mark.parametrize("epi", ["bias", "bias_gelu", "gelu_bwd", "add", "scale_rc", "bias_gelu_grad", "mul"])
@pytest.mark.parametrize("lp", LP16)
def test_gemm_epilogues(epi, lp):
    o = ops()
    _gemm_case(o, 200, 136, 160, False, False, lp, lp, epi)
    _gemm_case(o, 200, 136, 160, False, True, lp, torch.float32, epi)
    _gemm_case(o, 70, 52, 40, True, False, torch.float32, torch.float32, epi)


@pytest.mark.parametrize("M,N,K", [(9834, 3072, 768), (32768, 2048, 64), (16384, 2004, 192), (2100, 768, 256),
                                   (9834, 768, 3072), (19734, 512, 1024), (2005, 1984, 128)])
@pytest.mark.parametrize("epi", ["none", "bias_gelu", "gelu_bwd", "add", "bias_gelu_grad", "mul", "bias", "scale_rc"])
@pytest.mark.parametrize("lp", LP16)
def test_gemm_ring_kernels_at_full_size(M, N, K, epi, lp):
    """The persistent LDS-DMA ring kernels only take products that fill the chip: 256x256 tiles (phased kernel) for
    the first two shapes and conv5's (19734 x 512), 256x128 (3-stage ring) for the others.  N % 64 == 0 shapes store
    through the full-line register epilogue (lanes c, c ^ 8 swap halves), the others (2004, 1984 + ragged M) through the
    per-lane one.  Ragged M, ragged N (2004: scalar tail path), K of
    only two ring steps, every fused epilogue; reference = f32 matmul of the same bf16-rounded operands."""
    o = ops()
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(lp).to(DEV)
    Bm = (torch.randn(N, K, generator=g) / K ** 0.5).to(lp).to(DEV)
    ldc = (N + 7) // 8 * 8
    C = torch.zeros(M, ldc, dtype=lp, device=DEV)
    ref = A.float() @ Bm.float().t()
    kw = {}
    if epi == "bias_gelu":
        bias = torch.randn(N, generator=g).to(DEV)
        aux = torch.zeros(M, ldc, dtype=lp, device=DEV)
        kw.update(epilogue=o.EPI_BIAS_GELU, bias=bias, aux=aux, ldaux=ldc)
        pre = ref + bias
        ref = torch.nn.functional.gelu(pre)
    elif epi == "bias_gelu_grad":
        bias = torch.randn(N, generator=g).to(DEV)
        aux = torch.zeros(M, ldc, dtype=lp, device=DEV)
        kw.update(epilogue=o.EPI_BIAS_GELU_GRAD, bias=bias, aux=aux, ldaux=ldc)
        x = ref + bias
        pre = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        ref = torch.nn.functional.gelu(x)
    elif epi == "bias":
        bias = torch.randn(N, generator=g).to(DEV)
        kw.update(epilogue=o.EPI_BIAS, bias=bias)
        ref = ref + bias
    elif epi == "scale_rc":
        rs, cs = torch.rand(M, generator=g).to(DEV) + 0.5, torch.rand(N, generator=g).to(DEV) + 0.5
        kw.update(epilogue=o.EPI_SCALE_RC, row_scale=rs, col_scale=cs)
        ref = ref * rs[:, None] * cs[None, :]
    elif epi in ("gelu_bwd", "add", "mul"):
        aux = torch.randn(M, ldc, generator=g).to(lp).to(DEV)
        a = aux[:, :N].float()
        if epi == "add":
            kw.update(epilogue=o.EPI_ADD, aux=aux, ldaux=ldc)
            ref = ref + a
        elif epi == "mul":
            kw.update(epilogue=o.EPI_MUL, aux=aux, ldaux=ldc)
            ref = ref * a
        else:
            kw.update(epilogue=o.EPI_GELU_BWD, aux=aux, ldaux=ldc)
            ref = ref * (0.5 * (1 + torch.erf(a / math.sqrt(2))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi))
    o.gemm(M, N, K, A, Bm, C, lda=K, ldb=K, ldc=ldc, **kw)
    torch.cuda.synchronize()
    err = float((C[:, :N].float() - ref).norm() / ref.norm())
    assert err < 4e-3, (M, N, K, epi, err)
    if epi in ("bias_gelu", "bias_gelu_grad"):
        assert float((aux[:, :N].float() - pre).norm() / pre.norm()) < 4e-3
    if ldc > N:
        assert float(C[:, N:].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K", [(9834, 3072, 768), (32768, 2048, 64), (19734, 512, 1024), (16384, 1024, 128)])
@pytest.mark.parametrize("epi", ["none", "bias_gelu_grad", "mul", "add", "bias", "scale_rc"])
@pytest.mark.parametrize("lp", LP16)
def test_gemm_phased_kernel_bit_equal_to_ring_kernel(M, N, K, epi, lp):
    """gemm16_phased_256x256_kernel (family 4 of w2v2_tune_gemm_kernel) against gemm16_ring_256x128_kernel (family 2): the
    two large-tile kernels share the k-slot order of the MFMA chain and the register epilogues, so every output must be
    BIT-EQUAL whichever tile family the dispatch picks -- plus the f32 reference bound.  K = 64 is a single K tile
    (prologue only), ragged M.  (Round 3 ran this comparison against the 4-wave register-staged kernel, deleted in
    round 4 after losing every A/B.)"""
    o = ops()
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(lp).to(DEV)
    Bm = (torch.randn(N, K, generator=g) / K ** 0.5).to(lp).to(DEV)
    ref = A.float() @ Bm.float().t()
    kw, aux_in = {}, None
    if epi in ("bias", "bias_gelu_grad"):
        bias = torch.randn(N, generator=g).to(DEV)
        kw.update(epilogue=o.EPI_BIAS if epi == "bias" else o.EPI_BIAS_GELU_GRAD, bias=bias)
        ref = ref + bias
        if epi == "bias_gelu_grad":
            ref = torch.nn.functional.gelu(ref)
    elif epi == "scale_rc":
        rs, cs = torch.rand(M, generator=g).to(DEV) + 0.5, torch.rand(N, generator=g).to(DEV) + 0.5
        kw.update(epilogue=o.EPI_SCALE_RC, row_scale=rs, col_scale=cs)
        ref = ref * rs[:, None] * cs[None, :]
    elif epi in ("add", "mul"):
        aux_in = torch.randn(M, N, generator=g).to(lp).to(DEV)
        kw.update(epilogue=o.EPI_ADD if epi == "add" else o.EPI_MUL)
        ref = ref + aux_in.float() if epi == "add" else ref * aux_in.float()
    outs = {}
    try:
        for fam in (4, 2):
            for cdt in (lp, torch.float32):
                C = torch.full((M, N), float("nan"), dtype=cdt, device=DEV)
                k2 = dict(kw)
                if epi == "bias_gelu_grad":
                    k2.update(aux=torch.full((M, N), float("nan"), dtype=cdt, device=DEV), ldaux=N)
                elif aux_in is not None:
                    k2.update(aux=aux_in.to(cdt), ldaux=N)
                o.lib().w2v2_tune_gemm_kernel(fam)
                o.gemm(M, N, K, A, Bm, C, lda=K, ldb=K, ldc=N, **k2)
                torch.cuda.synchronize()
                outs[(fam, cdt)] = (C, k2.get("aux") if epi == "bias_gelu_grad" else None)
    finally:
        o.lib().w2v2_tune_gemm_kernel(0)
    for cdt in (lp, torch.float32):
        C4, x4 = outs[(4, cdt)]
        C5, x5 = outs[(2, cdt)]
        assert torch.equal(C4, C5), (M, N, K, epi, cdt, float((C4.float() - C5.float()).abs().max()))
        if x4 is not None:
            assert torch.equal(x4, x5)
        err = float((C5.float() - ref).norm() / ref.norm())
        assert err < (4e-3 if cdt != torch.float32 else 2e-5 * K ** 0.5 + 1e-6), (M, N, K, epi, cdt, err)


@pytest.mark.gpu
def test_gemm_timed_launch_reports_the_kernel_duration():
    """bench.py's roofline hook (w2v2_gemm_timed / w2v2_timer_read): same result as the plain launch, a duration of the
    right magnitude for both hooked kernels (256x128 ring, phased 256x256), and a loud error for a product that runs on
    a kernel family without the hook."""
    import ctypes
    o = ops()
    L = o.lib()
    g = torch.Generator(device="cpu").manual_seed(5)
    for slot, (M, N, K, name) in enumerate([(9834, 768, 768, "gemm16_ring_256x128_kernel"),
                                            (9834, 3072, 768, "gemm16_phased_256x256_kernel")]):
        A = torch.randn(M, K, generator=g).to(torch.float16).to(DEV)
        Bm = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.float16).to(DEV)
        C0 = torch.zeros(M, N, dtype=torch.float16, device=DEV)
        C1 = torch.zeros_like(C0)
        g0 = o.Gemm(M, N, K, A, Bm, C0, lda=K, ldb=K, ldc=N)
        g1 = o.Gemm(M, N, K, A, Bm, C1, lda=K, ldb=K, ldc=N)
        assert g1.kernel_name == name
        g0()
        for _ in range(3):                                   # (warm: the first launch of a kernel loads its code object)
            assert L.w2v2_gemm_timed(g1._ref, o.stream(), slot) == 0
        torch.cuda.synchronize()
        assert torch.equal(C0, C1)
        ms = (ctypes.c_float * 1)()
        assert L.w2v2_timer_read(slot, 1, ctypes.cast(ms, ctypes.c_void_p)) == 0
        tf = 2.0 * M * N * K / (ms[0] * 1e-3) / 1e12
        assert 100.0 < tf < 2500.0, (name, ms[0], tf)        # a kernel duration, not a host-side interval
    # a skinny product runs on the register-staged kernel: no hook -> error, nothing silently bracketed
    A = torch.randn(66, 106, generator=g).to(torch.float16).to(DEV)
    Bm = torch.randn(1536, 106, generator=g).to(torch.float16).to(DEV)
    C = torch.zeros(66, 1536, dtype=torch.float32, device=DEV)
    gs = o.Gemm(66, 1536, 106, A, Bm, C, lda=106, ldb=106, ldc=1536)
    assert L.w2v2_gemm_timed(gs._ref, o.stream(), 7) != 0
    assert b"does not run on" in L.w2v2_last_error()
    assert L.w2v2_timer_read(0, 100000, None) != 0



@pytest.mark.parametrize("M,N,K,nfrom", [(2100, 768, 256, 0), (9834, 2304, 768, 1536), (1500, 640, 64, 256)])
def test_gemm_two_term_weights(M, N, K, nfrom):
    """fp16 products with two-term weights (w2v2_gemm_desc.k_ext): columns >= n_ext_from see W = hi + lo, i.e. the
    f32 weight to ~2^-22, the others fp16(W).  Reference: f64 products of the fp16 activations with the respective
    weights; the residual plane removes the weight-rounding error (asserted 100x below the one-term error)."""
    o = ops()
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(torch.float16)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    planes = torch.zeros(2, N * K, dtype=torch.float16, device=DEV)
    hi = W.to(torch.float16)
    lo = (W - hi.float()).to(torch.float16)
    planes[0].copy_(hi.view(-1))
    planes[1].copy_(lo.view(-1))
    bias = torch.randn(N, generator=g)
    C = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    o.gemm(M, N, K, A.to(DEV), planes[0].view(N, K), C, lda=K, ldb=K, ldc=N, epilogue=o.EPI_BIAS, bias=bias.to(DEV),
           b_lo=planes[1].view(N, K), n_ext_from=nfrom)
    torch.cuda.synchronize()
    got = C.cpu().double()
    exact = A.double() @ W.double().t() + bias.double()
    one = A.double() @ hi.double().t() + bias.double()
    if nfrom:
        assert rel_l2(got[:, :nfrom], one[:, :nfrom]) < 2e-6             # one-term columns: fp16(W) exactly
    e2 = rel_l2(got[:, nfrom:], exact[:, nfrom:])
    e1 = rel_l2(one[:, nfrom:], exact[:, nfrom:])
    print("two-term error", e2, "one-term error", e1)
    assert e2 < 2e-6 and e1 > 100 * e2
    # 16-bit output with the deferred-store epilogue
    C16 = torch.zeros(M, N, dtype=torch.float16, device=DEV)
    o.gemm(M, N, K, A.to(DEV), planes[0].view(N, K), C16, lda=K, ldb=K, ldc=N, epilogue=o.EPI_BIAS, bias=bias.to(DEV),
           b_lo=planes[1].view(N, K), n_ext_from=nfrom)
    torch.cuda.synchronize()
    assert rel_l2(C16.float().cpu()[:, nfrom:], exact[:, nfrom:]) < 4e-4


def test_gemm_split_k_and_accumulate():
    o = ops()
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        _gemm_case(o, 192, 160, 2000, True, True, dtype, torch.float32, "none", split=5)
        _gemm_case(o, 192, 160, 2000, False, False, dtype, torch.float32, "bias", split=3)


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_f32_exact(ta, tb):
    o = ops()
    for (M, N, K) in [(64, 64, 16), (149, 48, 100), (70, 130, 33)]:
        _gemm_case(o, M, N, K, ta, tb, torch.float32, torch.float32)


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("code", [11, 12, 13, 14, 15, 115, 0])
def test_gemm_f32_lds_dma_tiles(ta, tb, code):
    """csrc/gemm_f32_dma.hip: every tile height (32 fi rows, fi = 1..5), XCD-contiguous order, all four
    operand layouts; ragged M / N (zero-source lanes), K tails inside a tile and inside a split, split-K atomics, the
    epilogues of the ECAPA step.  Tolerance 2e-5 relative l2 against f64 (as test_gemm_f32_exact)."""
    from w2v2_speaker_amd import _lib
    if os.environ.get("W2V2_F32_NO_DMA"):
        pytest.skip("W2V2_F32_NO_DMA sends every f32 product to the register-staged kernel")
    o, lib = ops(), _lib.load()
    old = lib.w2v2_tune_gemm_f32_tile(code)
    try:
        for (M, N, K) in [(200, 136, 160), (328, 260, 100), (160, 128, 64), (1000, 384, 36), (68, 5996, 192)]:
            _gemm_case(o, M, N, K, ta, tb, torch.float32, torch.float32)
            want = None if code == 0 else (code % 100 - 10) * 10 + 2
            got = lib.w2v2_gemm_f32_last_kernel()
            assert got == want if want is not None else got > 0, (code, got)
            assert got < 1000, (code, got)      # + 1000 = the DBG (time-attribution) instantiation: tile codes >= 200 only
        for epi in ("bias", "add", "bias_gelu", "mul"):
            _gemm_case(o, 200, 136, 160, ta, tb, torch.float32, torch.float32, epi)
        _gemm_case(o, 192, 160, 2000, ta, tb, torch.float32, torch.float32, "none", split=5)
        _gemm_case(o, 192, 160, 2000, ta, tb, torch.float32, torch.float32, "bias", split=3)
        assert 0 < lib.w2v2_gemm_f32_last_kernel() < 1000
        _gemm_case(o, 149, 70, 33, ta, tb, torch.float32, torch.float32)          # K % 4 != 0: the register-staged kernel
        assert lib.w2v2_gemm_f32_last_kernel() == 0
        if not ta and not tb:                                  # the dry run of the dispatch names the same kernel
            A, Bm = torch.zeros(200, 160, device=DEV), torch.zeros(136, 160, device=DEV)
            C = torch.zeros(200, 136, device=DEV)
            assert o.Gemm(200, 136, 160, A, Bm, C, lda=160, ldb=160, ldc=136).kernel_name == "gemm_f32_dma_kernel"
            lib.w2v2_tune_gemm_f32_tile(1)
            assert o.Gemm(200, 136, 160, A, Bm, C, lda=160, ldb=160, ldc=136).kernel_name == "gemm_f32_mfma_kernel"
    finally:
        lib.w2v2_tune_gemm_f32_tile(old)


def test_lds_dma_gemms_bit_stable_over_repeated_launches():
    """The LDS-DMA pieces of the ring / phased / f32 GEMMs are inline assembly the compiler does not order (round 6: its own
    conservative vmcnt(0) in the K loops was the price of the builtin) -- a missing counted wait would be an intermittent
    difference between launches on the same operands.  40 launches per product against the first, bit for bit; the same
    check with 400 launches per product is tools/gemm_race_check.py (profiles/r06_gemm_race_check.txt)."""
    o = ops()
    M = 66 * 149
    for (m, n, k, dt, name) in [(M, 768, 768, torch.float16, "gemm16_ring_256x128_kernel"),
                                (M, 3072, 768, torch.float16, "gemm16_phased_256x256_kernel"),
                                (M, 768, 3072, torch.float16, "gemm16_ring_256x128_kernel"),
                                (19800, 1024, 1024, torch.float32, "gemm_f32_dma_kernel"),
                                (4004, 260, 100, torch.float32, "gemm_f32_dma_kernel")]:
        A, Bm = rnd(m, k, seed=m + k, scale=0.2).to(dt).to(DEV), rnd(n, k, seed=n + k, scale=0.2).to(dt).to(DEV)
        bias = rnd(n, seed=n).to(DEV)
        C = torch.zeros(m, n, dtype=dt, device=DEV)
        gm = o.Gemm(m, n, k, A, Bm, C, lda=k, ldb=k, ldc=n, epilogue=o.EPI_BIAS, bias=bias)
        if not any(os.environ.get(e) for e in ("W2V2_NO_GEMM_PH", "W2V2_NO_GLDS3", "W2V2_NO_GLDS", "W2V2_F32_NO_DMA", "W2V2_G3N")):
            assert gm.kernel_name == name            # (the A/B switches of the library move products between kernels)
        gm()
        ref = C.clone()
        tol = 5e-3 if dt == torch.float16 else 1e-5
        assert float((ref.float() - (A.float() @ Bm.float().t() + bias)).abs().max()) < tol * max(1.0, k ** 0.5 / 8)
        for r in range(40):
            C.zero_()
            gm()
            if r % 8 == 7:
                assert torch.equal(C, ref), (name, m, n, k, r)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_gemm_batched_heads_and_implicit_conv(dtype):
    o = ops()
    # attention-style batch: q,k from a fused [B,T,3,heads,d] buffer
    B, T, heads, d = 2, 21, 3, 16
    H = heads * d
    qkv = rnd(B, T, 3 * H, seed=3, scale=0.5)
    if dtype != torch.float32:
        qkv = qkv.to(dtype).float()
    q = qkv[:, :, :H].view(B, T, heads, d).transpose(1, 2)
    k = qkv[:, :, H:2 * H].view(B, T, heads, d).transpose(1, 2)
    ref = (q.double() @ k.double().transpose(2, 3)) * 0.25
    Tl = 24
    S = torch.zeros(B * heads * T, Tl, dtype=torch.float32, device=DEV)
    qd = qkv.to(dtype).to(DEV).view(-1)
    o.gemm(T, T, d, qd, qd[H:], S, lda=3 * H, ldb=3 * H, ldc=Tl, batch=B * heads, batch_inner=heads,
           a_strides=(T * 3 * H, d), b_strides=(T * 3 * H, d), c_strides=(heads * T * Tl, T * Tl), alpha=0.25)
    torch.cuda.synchronize()
    got = S.view(B, heads, T, Tl)[..., :T].cpu().double()
    assert rel_l2(got, ref) < (1e-5 if dtype == torch.float32 else 3e-3)
    # implicit im2col: Conv1d(Cin->Cout, k=3, stride=2) over channels-last [B, L, Cin]
    Bn, L, Cin, Cout, kk, st = 3, 41, 32, 40, 3, 2
    x = rnd(Bn, L, Cin, seed=5)
    w = rnd(Cout, Cin, kk, seed=6, scale=0.2)
    if dtype != torch.float32:
        x, w = x.to(dtype).float(), w.to(dtype).float()
    ref = torch.nn.functional.conv1d(x.transpose(1, 2).double(), w.double(), stride=st).transpose(1, 2)
    Lo = (L - kk) // st + 1
    wp = torch.zeros(Cout, kk * Cin, dtype=dtype, device=DEV)
    o.pack_conv_weight(w.to(DEV), wp)
    y = torch.zeros(Bn * Lo, Cout, dtype=dtype, device=DEV)
    o.gemm(Bn * Lo, Cout, kk * Cin, x.to(dtype).to(DEV), wp, y, lda=st * Cin, ldb=kk * Cin, ldc=Cout,
           a_seg=(Lo, L * Cin))
    torch.cuda.synchronize()
    assert rel_l2(y.float().cpu().view(Bn, Lo, Cout), ref) < (1e-5 if dtype == torch.float32 else 1e-2)


# ----------------------------------------------------------------------------------------------- conv0
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_conv0_groupnorm_gelu(dtype):
    o = ops()
    B, N, C, k, s = 3, 4000, 96, 10, 5
    wav = rnd(B, N, seed=1)
    w = rnd(C, 1, k, seed=2, scale=0.4)
    gamma, beta = 1 + 0.1 * rnd(C, seed=3), 0.1 * rnd(C, seed=4)
    y = torch.nn.functional.conv1d(wav[:, None].double(), w.double(), stride=s)
    y = torch.nn.functional.group_norm(y, C, gamma.double(), beta.double(), eps=1e-5)
    ref = gelu(y).transpose(1, 2)
    L = ref.shape[1]
    out = torch.zeros(B, L, C, dtype=dtype, device=DEV)
    stats = o.conv0_workspace(B, N, C, k, s, DEV)
    o.conv0_groupnorm_gelu(wav.to(DEV), w.to(DEV), gamma.to(DEV), beta.to(DEV), out, stats, k, s)
    torch.cuda.synchronize()
    assert rel_l2(out.float().cpu(), ref) < (2e-6 if dtype == torch.float32 else 4e-3)


@pytest.mark.parametrize("C,N", [(128, 4000), (512, 3333), (640, 1291), (128, 161234)])   # (last: 51 window-moment blocks)
@pytest.mark.parametrize("lp", LP16)
def test_conv0_matrix_core_path(C, N, lp):
    """bf16 outputs with C % 128 == 0 take the split-bf16 MFMA convolution (conv0.hip): f32-class statistics
    (mean / rstd within 1e-5 of the f64 reference), ragged tail chunk, several channel groups per wave."""
    o = ops()
    B, k, s = 2, 10, 5
    wav = rnd(B, N, seed=11)
    w = rnd(C, 1, k, seed=12, scale=0.4)
    gamma, beta = 1 + 0.1 * rnd(C, seed=13), 0.1 * rnd(C, seed=14)
    u = torch.nn.functional.conv1d(wav[:, None].double(), w.double(), stride=s)          # [B, C, L]
    ref = gelu(torch.nn.functional.group_norm(u, C, gamma.double(), beta.double(), eps=1e-5)).transpose(1, 2)
    L = ref.shape[1]
    out = torch.zeros(B, L, C, dtype=lp, device=DEV)
    work = o.conv0_workspace(B, N, C, k, s, DEV)
    o.conv0_groupnorm_gelu(wav.to(DEV), w.to(DEV), gamma.to(DEV), beta.to(DEV), out, work, k, s)
    torch.cuda.synchronize()
    mr = work[work.numel() - B * C * 2:].view(B, C, 2).cpu().double()
    mean_ref, var_ref = u.mean(dim=2), u.var(dim=2, unbiased=False)
    # split-bf16 products carry ~2^-16 relative error per output: the mean over L frames sees its random walk
    assert (mr[..., 0] - mean_ref).abs().max() < 4 * 2.0 ** -16 * u.abs().max() / L ** 0.5
    assert ((mr[..., 1] - (var_ref + 1e-5).rsqrt()) / (var_ref + 1e-5).rsqrt()).abs().max() < 2e-5
    assert rel_l2(out.float().cpu(), ref) < 4e-3
    # against the exact-f32 VALU kernel rounded to the output format: at most an occasional one-ulp flip (the split
    # product's 2^-16 error is 1/128 of a bf16 ulp but 1/16 of an fp16 ulp)
    out32 = torch.zeros(B, L, C, dtype=torch.float32, device=DEV)
    o.conv0_groupnorm_gelu(wav.to(DEV), w.to(DEV), gamma.to(DEV), beta.to(DEV), out32, work, k, s)
    torch.cuda.synchronize()
    d = (out.float() - out32.to(lp).float()).abs().cpu()
    assert (d > 0).float().mean() < (0.02 if lp == torch.bfloat16 else 0.08) and rel_l2(out.float().cpu(), out32.cpu().double()) < 3e-3


# ----------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("dtype,H", [(torch.float32, 768), (torch.bfloat16, 768), (torch.float32, 64),
                                     (torch.bfloat16, 1024), (torch.float32, 512), (torch.float16, 768),
                                     (torch.float16, 1024)])
def test_layernorm_fwd_bwd(dtype, H):
    o = ops()
    M = 37
    x, r = rnd(M, H, seed=1), rnd(M, H, seed=2)
    if dtype != torch.float32:
        x, r = x.to(dtype).float(), r.to(dtype).float()
    gamma, beta = 1 + 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    dy = rnd(M, H, seed=5)
    if dtype != torch.float32:
        dy = dy.to(dtype).float()
    xs = (x + r).double().requires_grad_(True)
    if dtype != torch.float32:
        xs = (x + r).to(dtype).double().requires_grad_(True)       # the kernel saves s in bf16 and normalises that
    gd = gamma.double().requires_grad_(True)
    bd = beta.double().requires_grad_(True)
    yref = torch.nn.functional.layer_norm(xs, (H,), gd, bd, 1e-5)
    yref.backward(dy.double())
    xd, rd = x.to(dtype).to(DEV), r.to(dtype).to(DEV)
    y = torch.zeros(M, H, dtype=dtype, device=DEV)
    mean, rstd = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
    o.layernorm_fwd(xd, rd, gamma.to(DEV), beta.to(DEV), y, mean, rstd, 1e-5)
    torch.cuda.synchronize()
    tol = 2e-6 if dtype == torch.float32 else 4e-3
    assert rel_l2(y.float().cpu(), yref.detach()) < tol
    assert rel_l2(rd.float().cpu(), xs.detach()) < tol           # r now holds s = x + r
    ds = torch.zeros(M, H, dtype=dtype, device=DEV)
    dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    o.layernorm_bwd(dy.to(dtype).to(DEV), rd, mean, rstd, gamma.to(DEV), ds, None, dg, db)
    torch.cuda.synchronize()
    assert rel_l2(ds.float().cpu(), xs.grad) < (1e-5 if dtype == torch.float32 else 6e-3)
    assert rel_l2(dg.cpu(), gd.grad) < (1e-5 if dtype == torch.float32 else 3e-3)
    assert rel_l2(db.cpu(), bd.grad) < 1e-5
    # no-residual form
    y2 = torch.zeros_like(y)
    o.layernorm_fwd(xd, None, gamma.to(DEV), beta.to(DEV), y2, mean, rstd, 1e-5)
    torch.cuda.synchronize()
    ref2 = torch.nn.functional.layer_norm(x.double(), (H,), gamma.double(), beta.double(), 1e-5)
    assert rel_l2(y2.float().cpu(), ref2) < tol


def test_layernorm_dropout_mask_consistent_fwd_bwd():
    o = ops()
    M, H, p, seed = 64, 768, 0.1, 12345
    x, r = rnd(M, H, seed=1), rnd(M, H, seed=2)
    ones = torch.ones(M, H, device=DEV)
    o.dropout_(ones, p, seed)                 # the same (seed, index) stream as the LN kernels
    torch.cuda.synchronize()
    mask = ones.cpu()
    keep = float((mask > 0).float().mean())
    assert abs(keep - (1 - p)) < 0.01 and abs(float(mask.max()) - 1 / (1 - p)) < 1e-6
    gamma, beta = torch.ones(H), torch.zeros(H)
    rd = r.to(DEV)
    y = torch.zeros(M, H, device=DEV)
    mean, rstd = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
    o.layernorm_fwd(x.to(DEV), rd, gamma.to(DEV), beta.to(DEV), y, mean, rstd, 1e-5, p, seed)
    torch.cuda.synchronize()
    s_ref = x + r * mask
    assert rel_l2(rd.cpu(), s_ref) < 1e-6
    assert rel_l2(y.cpu(), torch.nn.functional.layer_norm(s_ref, (H,))) < 1e-5
    dy = rnd(M, H, seed=3)
    ds, dr = torch.zeros(M, H, device=DEV), torch.zeros(M, H, device=DEV)
    dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    o.layernorm_bwd(dy.to(DEV), rd, mean, rstd, gamma.to(DEV), ds, dr, dg, db, p, seed)
    torch.cuda.synchronize()
    assert rel_l2(dr.cpu(), ds.cpu() * mask) < 1e-6


# ----------------------------------------------------------------------------------------------- elementwise
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_elementwise_family(dtype):
    o = ops()
    n = 8 * 1000 + 5
    a, b = rnd(n, seed=1), rnd(n, seed=2)
    if dtype != torch.float32:
        a, b = a.to(dtype).float(), b.to(dtype).float()
    ad, bd = a.to(dtype).to(DEV), b.to(dtype).to(DEV)
    out = torch.zeros(n, dtype=dtype, device=DEV)
    o.add(ad, bd, out)
    torch.cuda.synchronize()
    tol = 1e-6 if dtype == torch.float32 else 4e-3
    assert rel_l2(out.float().cpu(), a + b) < tol
    o.gelu_bwd(ad, bd, out)
    torch.cuda.synchronize()
    bb = b.double().requires_grad_(True)
    gelu(bb).backward(a.double())
    assert rel_l2(out.float().cpu(), bb.grad) < (2e-6 if dtype == torch.float32 else 4e-3)
    # colsum (vector path and ragged scalar path)
    for (M, N, ld) in [(333, 768, 768), (50, 30, 34)]:
        x = rnd(M, ld, seed=3)
        if dtype != torch.float32:
            x = x.to(dtype).float()
        acc = torch.ones(N, device=DEV)
        o.colsum(x.to(dtype).to(DEV), acc, M, N, ld)
        torch.cuda.synchronize()
        assert rel_l2(acc.cpu(), 1 + x[:, :N].double().sum(0)) < 1e-5
    # cast
    src = rnd(n, seed=4)
    dst = torch.zeros(n, dtype=dtype, device=DEV)
    o.cast(src.to(DEV), dst)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), src.to(dtype))
    # mask fill fwd / bwd
    M, H = 40, 64
    h = rnd(M, H, seed=5)
    if dtype != torch.float32:
        h = h.to(dtype).float()
    mask = (torch.arange(M) % 7 == 0)
    emb = rnd(H, seed=6)
    hd = h.to(dtype).to(DEV)
    o.mask_fill(hd, mask.to(torch.uint8).to(DEV), emb.to(DEV))
    torch.cuda.synchronize()
    ref = torch.where(mask[:, None], emb.to(dtype).float()[None], h)
    assert torch.equal(hd.float().cpu(), ref)
    dh = h.to(dtype).to(DEV)
    de = torch.zeros(H, device=DEV)
    o.mask_fill_bwd(dh, mask.to(torch.uint8).to(DEV), de)
    torch.cuda.synchronize()
    assert rel_l2(de.cpu(), h[mask].double().sum(0)) < 1e-5
    assert float(dh.float().cpu()[mask].abs().max()) == 0.0 and torch.equal(dh.float().cpu()[~mask], h[~mask])
    # CLS prepend
    x = rnd(2, 5, 16, seed=7)
    y = torch.zeros(2, 6, 16, dtype=dtype, device=DEV)
    o.prepend_token(x.to(dtype).to(DEV), y, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(y[:, 1:].cpu(), x.to(dtype)) and float((y[:, 0].float() - 1).abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------- pos-conv
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_posconv_forward_backward(dtype):
    """Grouped weight-normed conv (HF:326-379) through regroup + weightnorm_pack + implicit GEMM."""
    o = ops()
    B, T, H, G, K = 2, 19, 64, 4, 16
    Cg, Tp = H // G, T + K - 1
    x = rnd(B, T, H, seed=1)
    g = 1 + 0.2 * rnd(1, 1, K, seed=2)
    v = rnd(H, Cg, K, seed=3, scale=0.1)
    bias = 0.1 * rnd(H, seed=4)
    up = rnd(B, T, H, seed=5)
    if dtype != torch.float32:
        x, up = x.to(dtype).float(), up.to(dtype).float()
    xr = x.double().requires_grad_(True)
    gr, vr = g.double().requires_grad_(True), v.double().requires_grad_(True)
    w = gr * vr / torch.sqrt((vr * vr).sum(dim=(0, 1), keepdim=True))
    pre = torch.nn.functional.conv1d(xr.transpose(1, 2), w, bias.double(), padding=K // 2, groups=G)[:, :, :-1]
    yref = gelu(pre).transpose(1, 2)
    yref.backward(up.double())
    xd = x.to(dtype).to(DEV)
    xg = torch.zeros(B, G, Tp, Cg, dtype=dtype, device=DEV)
    o.posconv_regroup(xd, xg, B, T, H, G, K, K // 2)
    wf, wb = torch.zeros(G, Cg, K * Cg, dtype=dtype, device=DEV), torch.zeros(G, Cg, K * Cg, dtype=dtype, device=DEV)
    sumsq = o.weightnorm_scratch(H, G, K, DEV)
    o.weightnorm_pack(g.to(DEV), v.to(DEV), sumsq, wf, wb, H, G, K)
    y = torch.zeros(B * T, H, dtype=dtype, device=DEV)
    ypre = torch.zeros(B * T, H, dtype=dtype, device=DEV)
    M = B * T
    o.gemm(M, Cg, K * Cg, xg, wf, y, lda=Cg, ldb=K * Cg, ldc=H, a_seg=(T, G * Tp * Cg), batch=G, batch_inner=G,
           a_strides=(0, Tp * Cg), b_strides=(0, Cg * K * Cg), c_strides=(0, Cg), epilogue=o.EPI_BIAS_GELU,
           bias=bias.to(DEV), bias_stride1=Cg, aux=ypre, ldaux=H, aux_strides=(0, Cg))
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == torch.float32 else 1.5e-2
    assert rel_l2(y.float().cpu().view(B, T, H), yref.detach()) < tol
    # backward
    P1 = torch.zeros(M, H, dtype=dtype, device=DEV)
    o.gelu_bwd(up.to(dtype).to(DEV).view(M, H), ypre, P1)
    dwf = torch.zeros(G, K * Cg, Cg, device=DEV)
    o.gemm(K * Cg, Cg, M, xg, P1, dwf, lda=Cg, ldb=H, ldc=Cg, transA=True, transB=True,
           a_seg=(T, G * Tp * Cg), batch=G, batch_inner=G, a_strides=(0, Tp * Cg), b_strides=(0, Cg),
           c_strides=(0, K * Cg * Cg))
    dot, dg, dv = o.weightnorm_scratch(H, G, K, DEV), torch.zeros(K, device=DEV), torch.zeros(H, Cg, K, device=DEV)
    o.weightnorm_bwd(g.to(DEV), v.to(DEV), sumsq, dwf, dot, dg, dv, H, G, K)
    dyg = torch.zeros(B, G, Tp, Cg, dtype=dtype, device=DEV)
    o.posconv_regroup(P1, dyg, B, T, H, G, K, K - 1 - K // 2)
    dx = torch.zeros(M, H, dtype=dtype, device=DEV)
    o.gemm(M, Cg, K * Cg, dyg, wb, dx, lda=Cg, ldb=K * Cg, ldc=H, a_seg=(T, G * Tp * Cg), batch=G, batch_inner=G,
           a_strides=(0, Tp * Cg), b_strides=(0, Cg * K * Cg), c_strides=(0, Cg))
    torch.cuda.synchronize()
    tolb = 2e-5 if dtype == torch.float32 else 2.5e-2
    assert rel_l2(dx.float().cpu().view(B, T, H), xr.grad) < tolb
    assert rel_l2(dv.cpu(), vr.grad) < tolb
    assert rel_l2(dg.cpu(), gr.grad.view(-1)) < tolb


# ----------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_softmax_fwd_bwd_unfused(dtype):
    o = ops()
    rows, T, ld = 50, 149, 152
    s = torch.zeros(rows, ld)
    s[:, :T] = rnd(rows, T, seed=1, scale=2.0)
    p = torch.zeros(rows, ld, dtype=dtype, device=DEV)
    o.softmax_fwd(s.to(DEV), p, None, rows, T, ld, 0.0, 0)
    torch.cuda.synchronize()
    sr = s[:, :T].double().requires_grad_(True)
    pref = torch.softmax(sr, dim=-1)
    tol = 1e-6 if dtype == torch.float32 else 4e-3
    assert rel_l2(p[:, :T].float().cpu(), pref.detach()) < tol
    dp = torch.zeros(rows, ld)
    dp[:, :T] = rnd(rows, T, seed=2)
    ds = torch.zeros(rows, ld, dtype=dtype, device=DEV)
    o.softmax_bwd(dp.to(DEV), p, ds, rows, T, ld, 0.0, 0)
    torch.cuda.synchronize()
    pref.backward(dp[:, :T].double())
    assert rel_l2(ds[:, :T].float().cpu(), sr.grad) < (1e-5 if dtype == torch.float32 else 1e-2)


def _attn_ref(qkv, B, T, heads, d, mask=None, keep=1.0):
    H = heads * d
    q, k, v = [qkv[:, :, i * H:(i + 1) * H].reshape(B, T, heads, d).transpose(1, 2) for i in range(3)]
    p = torch.softmax(q @ k.transpose(2, 3) * d ** -0.5, dim=-1)
    if mask is not None:
        p = p * mask / keep
    return (p @ v).transpose(1, 2).reshape(B, T, H)


@pytest.mark.parametrize("T", [149, 150, 249, 64, 12, 256, 161, 301, 1024, 7249])
@pytest.mark.parametrize("lp", LP16)
def test_fused_attention_fwd_bwd(T, lp):
    """T <= 160: one workgroup per (batch, head); longer: the tiled (online-softmax) kernels -- the paired-input
    model's T = 301, 1024, and a ~145 s evaluation utterance (T = 7249) -- against an f64 reference of the same
    16-bit-rounded inputs."""
    o = ops()
    B, heads, d = (2, 3, 64) if T <= 1024 else (1, 2, 64)
    H = heads * d
    qkv = rnd(B, T, 3 * H, seed=T, scale=1.0)
    qkv[..., :2 * H] *= 1.5                         # non-trivial softmax
    qkv = qkv.to(lp).float()
    dctx = (rnd(B, T, H, seed=T + 1)).to(lp).float()
    qr = qkv.double().requires_grad_(True)
    ref = _attn_ref(qr, B, T, heads, d)
    ref.backward(dctx.double())
    qd = qkv.to(lp).to(DEV)
    ctx = torch.zeros(B, T, H, dtype=lp, device=DEV)
    lse = torch.zeros(B * heads * T, device=DEV)
    o.attention_fwd(qd, ctx, lse, B, T, heads, d, d ** -0.5, 0.0, 0)
    torch.cuda.synchronize()
    assert rel_l2(ctx.float().cpu(), ref.detach()) < 8e-3, T
    q_, k_ = [qkv[:, :, i * H:(i + 1) * H].reshape(B, T, heads, d).transpose(1, 2).double() for i in range(2)]
    lref = torch.logsumexp(q_ @ k_.transpose(2, 3) * d ** -0.5, dim=-1)
    assert float((lse.cpu().view(B, heads, T) - lref).abs().max()) < 2e-2
    dqkv = torch.zeros(B, T, 3 * H, dtype=lp, device=DEV)
    delta = torch.zeros(B * heads * T, device=DEV)
    o.attention_bwd(qd, ctx, dctx.to(lp).to(DEV), lse, dqkv, delta, B, T, heads, d, d ** -0.5, 0.0, 0)
    torch.cuda.synchronize()
    g = dqkv.float().cpu()
    for i, nm in enumerate("qkv"):
        assert rel_l2(g[..., i * H:(i + 1) * H], qr.grad[..., i * H:(i + 1) * H]) < 2e-2, (T, nm)


@pytest.mark.parametrize("lp", LP16)
@pytest.mark.parametrize("T", [64, 200])
def test_fused_attention_dropout_mask_recovered_and_consistent(lp, T):
    """With q = k = 0 (uniform P) and V = one-hot rows the output IS the dropout mask (T = 64: V = identity; T = 200,
    the tiled kernels: four passes of 64 keys each, V rows of the pass's keys one-hot); then the forward/backward
    with that exact mask must match the torch reference."""
    o = ops()
    B, heads, d, p, seed = 2, 2, 64, 0.1, 991
    H = heads * d
    if T > 64:
        return _attention_dropout_tiled(o, lp, B, heads, d, T, p, seed)
    probe = torch.zeros(B, T, 3 * H)
    probe[..., 2 * H:] = torch.eye(T).repeat(1, heads)[None]
    ctx = torch.zeros(B, T, H, dtype=lp, device=DEV)
    lse = torch.zeros(B * heads * T, device=DEV)
    o.attention_fwd(probe.to(lp).to(DEV), ctx, lse, B, T, heads, d, d ** -0.5, p, seed)
    torch.cuda.synchronize()
    m = (ctx.float().cpu().view(B, T, heads, d).transpose(1, 2) > 0).double()       # [B,h,q,key]
    keep = float(m.mean())
    assert abs(keep - (1 - p)) < 0.02
    qkv = (rnd(B, T, 3 * H, seed=5)).to(lp).float()
    dctx = (rnd(B, T, H, seed=6)).to(lp).float()
    qr = qkv.double().requires_grad_(True)
    ref = _attn_ref(qr, B, T, heads, d, mask=m, keep=1 - p)
    ref.backward(dctx.double())
    qd = qkv.to(lp).to(DEV)
    o.attention_fwd(qd, ctx, lse, B, T, heads, d, d ** -0.5, p, seed)
    dqkv = torch.zeros(B, T, 3 * H, dtype=lp, device=DEV)
    delta = torch.zeros(B * heads * T, device=DEV)
    o.attention_bwd(qd, ctx, dctx.to(lp).to(DEV), lse, dqkv, delta, B, T, heads, d, d ** -0.5, p, seed)
    torch.cuda.synchronize()
    assert rel_l2(ctx.float().cpu(), ref.detach()) < 1e-2
    assert rel_l2(dqkv.float().cpu(), qr.grad) < 2.5e-2


def _attention_dropout_tiled(o, lp, B, heads, d, T, p, seed):
    H = heads * d
    m = torch.zeros(B, heads, T, T, dtype=torch.float64)
    ctx = torch.zeros(B, T, H, dtype=lp, device=DEV)
    lse = torch.zeros(B * heads * T, device=DEV)
    for k0 in range(0, T, d):                       # keys k0 .. k0+63 made visible through one-hot value rows
        probe = torch.zeros(B, T, 3 * H)
        n = min(d, T - k0)
        for h in range(heads):
            probe[:, k0:k0 + n, 2 * H + h * d:2 * H + h * d + n] = torch.eye(n)
        o.attention_fwd(probe.to(lp).to(DEV), ctx, lse, B, T, heads, d, d ** -0.5, p, seed)
        torch.cuda.synchronize()
        c = ctx.float().cpu().view(B, T, heads, d).transpose(1, 2)            # [B, h, q, d] = P_drop[q, k0 + d]
        m[..., k0:k0 + n] = (c[..., :n] > 0).double()
    assert abs(float(m.mean()) - (1 - p)) < 0.02
    qkv = (rnd(B, T, 3 * H, seed=5)).to(lp).float()
    dctx = (rnd(B, T, H, seed=6)).to(lp).float()
    qr = qkv.double().requires_grad_(True)
    ref = _attn_ref(qr, B, T, heads, d, mask=m, keep=1 - p)
    ref.backward(dctx.double())
    qd = qkv.to(lp).to(DEV)
    o.attention_fwd(qd, ctx, lse, B, T, heads, d, d ** -0.5, p, seed)
    dqkv = torch.zeros(B, T, 3 * H, dtype=lp, device=DEV)
    delta = torch.zeros(B * heads * T, device=DEV)
    o.attention_bwd(qd, ctx, dctx.to(lp).to(DEV), lse, dqkv, delta, B, T, heads, d, d ** -0.5, p, seed)
    torch.cuda.synchronize()
    assert rel_l2(ctx.float().cpu(), ref.detach()) < 1e-2
    assert rel_l2(dqkv.float().cpu(), qr.grad) < 2.5e-2


@pytest.mark.parametrize("lp", LP16)
@pytest.mark.parametrize("T", [149, 37, 301, 700])
def test_fused_attention_two_geometries_agree_and_draw_the_same_mask(lp, T):
    """Round 6: the attention kernels exist in two geometries (attention.hip: <4 waves, 64-row tiles> and <2 waves, 32-row
    tiles>, chosen by T; W2V2_ATTN_GEOM forces one, read per call).  Same inputs, dropout on: the two must draw the SAME
    mask (the stream is indexed by absolute (query, key)) and agree to 16-bit rounding on ctx / LSE / dQKV."""
    import os
    o = ops()
    B, heads, d, p, seed = 2, 3, 64, 0.1, 4242
    H = heads * d
    qkv = rnd(B, T, 3 * H, seed=T + 7, scale=1.0)
    qkv[..., :2 * H] *= 1.5
    qd = qkv.to(lp).to(DEV)
    dctx = rnd(B, T, H, seed=T + 8).to(lp).to(DEV)
    probe = torch.zeros(B, T, 3 * H)
    n = min(d, T)
    for h in range(heads):
        probe[:, :n, 2 * H + h * d:2 * H + h * d + n] = torch.eye(n)
    probe = probe.to(lp).to(DEV)
    got = {}
    old = {k: os.environ.get(k) for k in ("W2V2_ATTN_GEOM", "W2V2_ATTN_IDX64")}
    try:
        for geom, idx64 in (("64", True), ("32", False), ("32", True), ("64", False)):
            os.environ["W2V2_ATTN_GEOM"] = geom
            os.environ.pop("W2V2_ATTN_IDX64", None)
            if idx64:
                os.environ["W2V2_ATTN_IDX64"] = "1"
            ctx = torch.zeros(B, T, H, dtype=lp, device=DEV)
            lse = torch.zeros(B * heads * T, device=DEV)
            o.attention_fwd(probe, ctx, lse, B, T, heads, d, d ** -0.5, p, seed)
            torch.cuda.synchronize()
            mask = ctx.float().cpu() > 0
            o.attention_fwd(qd, ctx, lse, B, T, heads, d, d ** -0.5, p, seed)
            dqkv = torch.zeros(B, T, 3 * H, dtype=lp, device=DEV)
            delta = torch.zeros(B * heads * T, device=DEV)
            o.attention_bwd(qd, ctx, dctx, lse, dqkv, delta, B, T, heads, d, d ** -0.5, p, seed)
            torch.cuda.synchronize()
            got[geom, idx64] = (mask, ctx.float().cpu(), lse.cpu(), dqkv.float().cpu(), delta.cpu())
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    # the 32-bit dropout counters are the same bits as the 64-bit ones: everything equal, bit for bit, per geometry
    for geom in ("64", "32"):
        for x, y in zip(got[geom, True], got[geom, False]):
            assert torch.equal(x, y), geom
    a, b = got["64", True], got["32", False]
    assert torch.equal(a[0], b[0]) and 0.85 < float(a[0][:, :, :n].float().mean()) < 0.95
    tol = 3e-3 if lp == torch.float16 else 1.2e-2
    assert rel_l2(b[1], a[1]) < tol
    assert float((a[2] - b[2]).abs().max()) < 1e-4
    assert rel_l2(b[3], a[3]) < 2 * tol
    assert rel_l2(b[4], a[4]) < tol


@pytest.mark.parametrize("lp", LP16)
@pytest.mark.parametrize("T", [149, 33, 160, 97])
def test_attention_dkdv_lds_dma_tile_loads_bit_equal_to_register_staging(lp, T):
    """Round 6: in the 32-row geometry the dK / dV kernel takes its Q / dO tiles by LDS-DMA (no staging registers: 126
    VGPRs, four waves per SIMD instead of three).  The DMA cannot zero-fill the rows past T -- they arrive as copies of
    the last row and are silenced through lse = +inf -- so the result must be BIT-equal to the register-staged kernel
    (W2V2_ATTN_KV_NO_DMA=1, read per call), ragged tiles included."""
    import os
    o = ops()
    B, heads, d, p, seed = 3, 2, 64, 0.1, 77
    H = heads * d
    qd = (rnd(B, T, 3 * H, seed=T + 1, scale=1.2)).to(lp).to(DEV)
    dctx = rnd(B, T, H, seed=T + 2).to(lp).to(DEV)
    ctx = torch.zeros(B, T, H, dtype=lp, device=DEV)
    lse = torch.zeros(B * heads * T, device=DEV)
    outs = []
    old = {k: os.environ.get(k) for k in ("W2V2_ATTN_GEOM", "W2V2_ATTN_KV_NO_DMA")}
    try:
        os.environ["W2V2_ATTN_GEOM"] = "32"
        o.attention_fwd(qd, ctx, lse, B, T, heads, d, d ** -0.5, p, seed)
        for no_dma in (True, False):
            os.environ.pop("W2V2_ATTN_KV_NO_DMA", None)
            if no_dma:
                os.environ["W2V2_ATTN_KV_NO_DMA"] = "1"
            dqkv = torch.full((B, T, 3 * H), float("nan"), dtype=lp, device=DEV)
            delta = torch.zeros(B * heads * T, device=DEV)
            o.attention_bwd(qd, ctx, dctx, lse, dqkv, delta, B, T, heads, d, d ** -0.5, p, seed)
            torch.cuda.synchronize()
            outs.append(dqkv.clone())
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


def test_dropout_stream_statistics():
    """Counter-based dropout (common.h rng_pair): keep rate, independence of the two elements that share one
    32-bit hash, independence of neighbouring hashes, and decorrelation of consecutive seeds."""
    o = ops()
    n, p = 1 << 22, 0.1
    masks = []
    for seed in (1234, 1235):
        x = torch.ones(n, dtype=torch.float32, device=DEV)
        o.dropout_(x, p, seed)
        torch.cuda.synchronize()
        xc = x.cpu()
        vals = xc.unique().tolist()
        assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1 / (1 - p)) < 1e-6
        masks.append((xc > 0).double())
    m = masks[0]
    se = (p * (1 - p) / n) ** 0.5
    assert abs(m.mean().item() - (1 - p)) < 5 * se

    def corr(a, b):
        a, b = a - a.mean(), b - b.mean()
        return float((a * b).mean() / (a.std() * b.std()))
    assert abs(corr(m[0::2], m[1::2])) < 5 / (n / 2) ** 0.5          # halves of one hash
    assert abs(corr(m[1:-1:2], m[2::2])) < 5 / (n / 2) ** 0.5        # neighbouring hashes
    assert abs(corr(m[:-64], m[64:])) < 5 / n ** 0.5                 # one wave apart
    assert abs(corr(masks[0], masks[1])) < 5 / n ** 0.5              # consecutive seeds


# ----------------------------------------------------------------------------------------------- attentive pooling
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_attentive_pooling_stages_at_base_size_vs_unpinned_restatement(dtype):
    """Every stage of csrc/asp.hip (+ its GEMMs) at the BASELINE configs[2] size (T=149, C=768, A=128) against an
    f64 torch evaluation of the SAME stage on the stage's own inputs as stored by the HIP path -- so bf16 is tested
    per stage, free of the noise amplification of the chained BatchNorm backward."""
    from w2v2_speaker_amd.asp import ASP_PREFIX, AttentivePool
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    B, T, C, A = 4, 149, 768, 128
    st = ParamStore(W2V2Config(num_hidden_layers=1), DEV, dtype, head=None, attentive_pool=True)
    g = torch.Generator().manual_seed(3)
    for n, shp in st.shapes.items():
        if n.startswith(ASP_PREFIX):
            t = torch.randn(shp, generator=g)
            t = 1 + 0.1 * t if n.endswith("norm.norm.weight") else (t / shp[1] ** 0.5 if t.dim() == 3 else 0.1 * t)
            st.p(n).copy_(t.to(DEV))
    st.sync_lowp()
    rows = (B * T + 63) // 64 * 64
    full = torch.zeros(rows, C, dtype=dtype, device=DEV)
    x = full[:B * T]
    x.copy_((rnd(B * T, C, seed=8) * 2 + 0.3).to(dtype))
    x._w2v2_padded = full
    emb = torch.zeros(B, 2 * C, device=DEV)
    dx = torch.zeros(rows, C, dtype=dtype, device=DEV)[:B * T]
    ap = AttentivePool(st, x, emb, dx, B, T, train=True)
    st.zero_grad()
    ap.forward()
    demb = rnd(B, 2 * C, seed=9).to(DEV)
    ap.backward(demb)
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == torch.float32 else 1.5e-2
    D = lambda t: t.detach().double().cpu()
    P = lambda n: D(st.p(ASP_PREFIX + n))
    G = lambda n: D(st.g(ASP_PREFIX + n))
    xd = D(x).view(B, T, C)
    W1, b1 = P("tdnn.conv.conv.weight").view(A, 3 * C), P("tdnn.conv.conv.bias")
    W1q = D(st.w(ASP_PREFIX + "tdnn.conv.conv.weight")).view(A, 3 * C)          # operand copy the GEMMs read
    W2q, b2 = D(st.w(ASP_PREFIX + "conv.conv.weight")).view(C, A), P("conv.conv.bias")
    gam, bet = P("tdnn.norm.norm.weight"), P("tdnn.norm.norm.bias")
    # forward stages
    mean = xd.mean(1)
    std = ((xd - mean[:, None]) ** 2).mean(1).clamp_min(1e-12).sqrt()
    ctx = torch.cat([mean, std], 1)
    assert rel_l2(D(ap.ctx), ctx) < 1e-5
    cb = D(ap.ctx) @ W1[:, C:].t() + b1
    assert rel_l2(D(ap.cb), cb) < 1e-5
    a_pre = (xd @ W1q[:, :C].t() + D(ap.cb)[:, None]).view(B * T, A)
    assert rel_l2(D(ap.a_pre), a_pre) < tol
    r = D(ap.a_pre).clamp_min(0)
    mu, var = r.mean(0), r.var(0, unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    assert rel_l2(D(ap.mean_rstd)[:, 0], mu) < 1e-5 and rel_l2(D(ap.mean_rstd)[:, 1], rstd) < 1e-5
    rh = (r - mu) * rstd
    h = torch.tanh(rh * gam + bet)
    assert rel_l2(D(ap.h), h) < tol
    s_ref = D(ap.h) @ W2q.t() + b2
    assert rel_l2(D(ap.s), s_ref) < tol
    sd_ = D(ap.s).view(B, T, C)
    w = torch.softmax(sd_, 1)
    wm = (w * xd).sum(1)
    wvar = (w * (xd - wm[:, None]) ** 2).sum(1)
    out = torch.cat([wm, wvar.clamp_min(1e-12).sqrt()], 1)
    assert rel_l2(D(emb), out) < 1e-5
    # backward stages (each from the HIP path's own stored inputs)
    dm, dsd = D(demb)[:, :C], D(demb)[:, C:]
    dvar = dsd / (2 * out[:, C:])
    dwt = xd * dm[:, None] + dvar[:, None] * (xd - wm[:, None]) ** 2
    ds_ref = w * (dwt - (w * dwt).sum(1, keepdim=True))
    dx_direct = w * (dm[:, None] + 2 * dvar[:, None] * (xd - wm[:, None]))
    assert rel_l2(D(ap.ds).view(B, T, C), ds_ref) < tol
    dh_ref = D(ap.ds) @ W2q
    assert rel_l2(D(ap.dh), dh_ref) < tol
    dz = D(ap.dh) * (1 - h * h)
    da_ref = (gam * rstd * (dz - dz.mean(0) - rh * (dz * rh).mean(0))) * (D(ap.a_pre) > 0)
    assert rel_l2(D(ap.da), da_ref) < tol
    assert rel_l2(G("tdnn.norm.norm.weight"), (dz * rh).sum(0)) < tol and rel_l2(G("tdnn.norm.norm.bias"), dz.sum(0)) < tol
    assert rel_l2(G("conv.conv.weight").view(C, A), D(ap.ds).t() @ D(ap.h)) < tol
    # sum_t ds == 0 exactly (softmax backward): only rounding noise is left, compare on the scale of the summands
    assert (G("conv.conv.bias") - D(ap.ds).sum(0)).abs().max() < tol * D(ap.ds).abs().sum(0).max()
    dW1 = G("tdnn.conv.conv.weight").view(A, 3 * C)
    dad = D(ap.da)
    assert rel_l2(dW1[:, :C], dad.t() @ xd.view(B * T, C)) < tol
    dsum = dad.view(B, T, A).sum(1)
    assert rel_l2(dW1[:, C:], dsum.t() @ D(ap.ctx)) < tol
    assert rel_l2(G("tdnn.conv.conv.bias"), dad.sum(0)) < tol
    dctx = dsum @ W1[:, C:]
    dx_ref = dx_direct + (dad @ W1q[:, :C]).view(B, T, C) + dctx[:, None, :C] / T \
        + dctx[:, None, C:] * (xd - mean[:, None]) / (T * std[:, None])
    assert rel_l2(D(dx).view(B, T, C), dx_ref) < tol


# ----------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_pooling_all_modes(dtype):
    o = ops()
    B, T, H = 3, 149, 768
    x = rnd(B, T, H, seed=1, scale=2.0) + 0.5
    if dtype != torch.float32:
        x = x.to(dtype).float()
    xd = x.to(dtype).to(DEV)
    refs = {"mean+std": lambda t: torch.cat(torch.std_mean(t, dim=1), 1), "mean": lambda t: t.mean(1),
            "max": lambda t: t.max(1).values, "first": lambda t: t[:, 0], "last": lambda t: t[:, -1],
            "middle": lambda t: t[:, -1],
            "quantile": lambda t: torch.flatten(torch.quantile(
                t, torch.tensor([0, 0.25, 0.5, 0.75, 1.0], dtype=t.dtype), dim=1).transpose(0, 1), 1, 2)}
    for name, fn in refs.items():
        xr = x.double().requires_grad_(True)
        ref = fn(xr)
        up = rnd(*ref.shape, seed=9)
        ref.backward(up.double())
        out = torch.zeros(*ref.shape, device=DEV)
        o.pool_fwd(xd, out, o.POOL_MODES[name])
        torch.cuda.synchronize()
        assert rel_l2(out.cpu(), ref.detach()) < 1e-5, name
        dx = torch.zeros(B, T, H, dtype=dtype, device=DEV)
        o.pool_bwd(xd, out, up.to(DEV), dx, o.POOL_MODES[name])
        torch.cuda.synchronize()
        if name == "quantile" and dtype != torch.float32:
            # 16-bit values repeat within a column: which of two EQUAL values receives the gradient is a tie-break
            # (ours: stable, by time index); compare what is invariant, the gradient summed over each column
            assert rel_l2(dx.float().sum(1).cpu(), xr.grad.sum(1)) < 4e-3
            continue
        assert rel_l2(dx.float().cpu(), xr.grad) < (1e-5 if dtype == torch.float32 else 4e-3), name


@pytest.mark.parametrize("T", [1, 2, 5, 150, 1000])
def test_quantile_pooling_lengths_and_ties(T):
    """ref: src/layers/pooling.py:51-67 at odd lengths: T = 1 (every quantile is the value), interpolated ranks,
    long sequences, and heavy ties (values from a 7-element set): forward equals torch.quantile; the gradient lands on
    elements that hold the selected value and sums to the upstream gradient."""
    o = ops()
    B, H = 2, 72
    g = torch.Generator().manual_seed(T)
    qs = torch.tensor([0, 0.25, 0.5, 0.75, 1.0])
    for ties in (False, True):
        x = torch.randint(-3, 4, (B, T, H), generator=g).float() if ties else torch.randn(B, T, H, generator=g) * 3 - 0.5
        ref = torch.flatten(torch.quantile(x, qs, dim=1).transpose(0, 1), 1, 2)
        out = torch.zeros(B, 5 * H, device=DEV)
        o.pool_fwd(x.to(DEV), out, o.POOL_MODES["quantile"])
        torch.cuda.synchronize()
        assert torch.allclose(out.cpu(), ref, rtol=1e-6, atol=1e-6), (T, ties)
        up = torch.randn(B, 5 * H, generator=g)
        dx = torch.zeros(B, T, H, device=DEV)
        o.pool_bwd(x.to(DEV), out, up.to(DEV), dx, o.POOL_MODES["quantile"])
        torch.cuda.synchronize()
        assert torch.allclose(dx.cpu().sum(1), up.view(B, 5, H).sum(1), rtol=1e-5, atol=1e-5)
        if not ties:
            xr = x.clone().requires_grad_(True)
            torch.flatten(torch.quantile(xr, qs, dim=1).transpose(0, 1), 1, 2).backward(up)
            assert torch.allclose(dx.cpu(), xr.grad, rtol=1e-5, atol=1e-6)


def test_pooling_golden_edges():
    """Reference-generated vectors incl. T = 1 (unbiased std -> NaN, like torch) and T = 7249."""
    o = ops()
    g = np.load(os.path.join(GOLDEN, "g5_pool.npz"))
    for name in ("t1", "long"):
        x = torch.from_numpy(g[name + ".x"])
        B, T, H = x.shape
        out = torch.zeros(B, 2 * H, device=DEV)
        o.pool_fwd(x.to(DEV), out, 0)
        torch.cuda.synchronize()
        assert np.allclose(out.cpu().numpy(), g[name + ".mean+std"], atol=2e-5, equal_nan=True), name
        if name == "long":
            dx = torch.zeros(B, T, H, device=DEV)
            o.pool_bwd(x.to(DEV), out, torch.from_numpy(g["long.upstream"]).to(DEV), dx, 0)
            torch.cuda.synchronize()
            assert np.allclose(dx.cpu().numpy(), g["long.dx"], atol=1e-7)


# ----------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("lp", LP16)
def test_fused_adam_matches_torch_and_golden(lp):
    o = ops()
    g = np.load(os.path.join(GOLDEN, "g8_optim.npz"))
    p = torch.from_numpy(g["p0"]).clone().to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    pb = torch.zeros(16, dtype=lp, device=DEV)
    for i in range(100):
        gr = torch.from_numpy(g["grads"][i]).to(DEV)
        o.adam_step(p, gr, m, v, pb, 16, float(g["lr"][i]), float(g["beta1"][i]), 0.999, 1e-8, i + 1)
    torch.cuda.synchronize()
    assert np.allclose(p.cpu().numpy(), g["params"][99], atol=2e-7)
    assert torch.equal(pb.cpu(), p.cpu().to(lp))
    n = 4 * 1000 + 3
    pp = rnd(n, seed=1)
    ref = torch.nn.Parameter(pp.clone())
    opt = torch.optim.Adam([ref], lr=1e-3)
    pd = pp.clone().to(DEV)
    md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
    for i in range(3):
        gr = rnd(n, seed=10 + i)
        ref.grad = gr.clone() * 0.5
        opt.step()
        o.adam_step(pd, gr.to(DEV), md, vd, None, n, 1e-3, 0.9, 0.999, 1e-8, i + 1, grad_scale=0.5)
    torch.cuda.synchronize()
    assert np.allclose(pd.cpu().numpy(), ref.detach().numpy(), atol=1e-6)


def test_bce_head_vs_reference_golden():
    """w2v2_bce_head_fwd_bwd (Linear(H, 1) + BCE-with-logits) against the reference's BinaryCrossEntropyLoss golden
    (ref: src/optim/loss/binary_cross_entropy.py:24-40; logits produced by a known embedding / weight pair), incl. the
    saturated logits of the stable branch, the loss scale and an out-of-range label (NaN loss row, zero gradient)."""
    o = ops()
    g = np.load(os.path.join(GOLDEN, "g9_bce.npz"))
    logits, label = torch.from_numpy(g["logits"])[:, 0], torch.from_numpy(g["label"])
    B, H = logits.shape[0], 16
    w = rnd(H, seed=1)
    emb = torch.zeros(B, H)
    emb[:, 0] = (logits - 0.25) / w[0]                     # emb . w + b == logits with b = 0.25
    b = torch.tensor([0.25])
    prob, rows = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
    dl, de = torch.zeros(B, device=DEV), torch.zeros(B, H, device=DEV)
    dw, db = torch.zeros(H, device=DEV), torch.zeros(1, device=DEV)
    o.bce_head_fwd_bwd(emb.to(DEV), w.to(DEV), b.to(DEV), label.to(DEV), prob, rows, dl, de, dw, db, B, H)
    torch.cuda.synchronize()
    assert abs(float(rows.mean()) - float(g["loss"])) < 2e-5
    assert np.allclose(prob.cpu().numpy(), g["prediction"], atol=2e-6)
    assert np.allclose(dl.cpu().numpy(), g["dlogits"][:, 0], atol=1e-7)
    assert rel_l2(de.cpu(), torch.from_numpy(g["dlogits"]) * w[None, :]) < 1e-5
    assert rel_l2(dw.cpu(), (torch.from_numpy(g["dlogits"]) * emb).sum(0)) < 1e-5
    scale = torch.tensor([8.0, 0, 0, 0], device=DEV)
    lab2 = label.clone()
    lab2[5] = 2
    o.bce_head_fwd_bwd(emb.to(DEV), w.to(DEV), b.to(DEV), lab2.to(DEV), prob, rows, dl, de, dw, db, B, H, scale)
    torch.cuda.synchronize()
    ref = torch.from_numpy(g["dlogits"][:, 0]).clone() * 8.0
    ref[5] = 0.0
    assert np.allclose(dl.cpu().numpy(), ref.numpy(), atol=1e-6) and bool(torch.isnan(rows[5])) and float(de[5].abs().max()) == 0


def test_grad_scaler_check_update_and_adam_skip():
    """Dynamic loss scaling (csrc/optim.hip) = torch.cuda.amp.GradScaler: gradients are divided by the scale inside
    Adam, a step with a non-finite gradient changes nothing and halves the scale, `growth_interval` clean steps
    double it; all on a 4-float device record."""
    o = ops()
    n = 4 * 1000 + 3
    pp = rnd(n, seed=1)
    ref = torch.nn.Parameter(pp.clone())
    opt = torch.optim.Adam([ref], lr=1e-3)
    pd = pp.clone().to(DEV)
    md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
    state = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=DEV)
    for i in range(2):
        gr = rnd(n, seed=10 + i)
        ref.grad = gr.clone()
        opt.step()
        gs = (gr * 1024.0).to(DEV)
        o.grad_scaler_check(gs, n, state)
        o.adam_step(pd, gs, md, vd, None, n, 1e-3, 0.9, 0.999, 1e-8, i + 1, scaler=state)
        o.grad_scaler_update(state, 2.0, 0.5, 2)
    torch.cuda.synchronize()
    assert np.allclose(pd.cpu().numpy(), ref.detach().numpy(), atol=1e-6)
    assert state.tolist() == [2048.0, 0.0, 0.0, 0.0]          # two clean steps at interval 2: doubled, tracker reset
    before = (pd.clone(), md.clone(), vd.clone())
    for bad, pos in ((float("inf"), n - 1), (float("nan"), 17), (-float("inf"), 4 * 512)):
        gs = rnd(n, seed=3).to(DEV)
        gs[pos] = bad
        sc = float(state[0])
        o.grad_scaler_check(gs, n, state)
        torch.cuda.synchronize()
        assert float(state[1]) == 1.0
        o.adam_step(pd, gs, md, vd, None, n, 1e-3, 0.9, 0.999, 1e-8, 3, scaler=state)
        o.grad_scaler_update(state, 2.0, 0.5, 2)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, (pd, md, vd)))      # the whole step was skipped
        assert float(state[0]) == sc * 0.5 and float(state[1]) == 0.0 and float(state[2]) == 0.0
    assert float(state[3]) == 3.0
    ok = rnd(n, seed=4).to(DEV)
    o.grad_scaler_check(ok, n, state)
    torch.cuda.synchronize()
    assert float(state[1]) == 0.0


# ----------------------------------------------------------------------------------------------- grouped wgrad
@pytest.mark.parametrize("shapes", [
    [(768, 3072), (3072, 768), (768, 768), (2304, 768), (64, 128), (136, 72)],            # 256x128 ring kernel
    [(768, 3072), (3072, 768), (768, 776), (2304, 768), (768, 3072), (3072, 768), (520, 768), (2304, 768)],  # 256x256
    [(64, 128), (136, 72)]])                                                               # 128x128 kernel
@pytest.mark.parametrize("lp", LP16)
def test_grouped_weight_gradient_gemm(shapes, lp):
    """dW = dY^T X and dbias = colsum(dY) for several Linear layers in one launch (LDS-DMA staging +
    ds_read_b64_tr_b16 transposing fragment reads); ragged feature sizes, token tail zero-padded.  The second
    set is two transformer blocks' worth of problems: 219 tiles of 256x256 -> the four-stage ring kernel."""
    o = ops()
    tokens = 2 * 149
    tp = (tokens + 63) // 64 * 64
    probs, refs = [], []
    for i, (no, ni) in enumerate(shapes):
        dY = torch.zeros(tp, no)
        X = torch.zeros(tp, ni)
        dY[:tokens] = (rnd(tokens, no, seed=2 * i + 1, scale=0.5)).to(lp).float()
        X[:tokens] = (rnd(tokens, ni, seed=2 * i + 2, scale=0.5)).to(lp).float()
        dW = torch.full((no, ni), 7.0, device=DEV)           # must be overwritten, not accumulated
        db = torch.full((no,), 7.0, device=DEV)
        probs.append((dY.to(lp).to(DEV), X.to(lp).to(DEV), dW, db))
        refs.append((dY.double().t() @ X.double(), dY.double().sum(0)))
    o.WgradGroup(probs, tokens, tp)()
    torch.cuda.synchronize()
    for (dY, X, dW, db), (rw, rb), shp in zip(probs, refs, shapes):
        assert rel_l2(dW.cpu(), rw) < 1e-5, shp
        assert rel_l2(db.cpu(), rb) < 1e-5, shp
    # bitwise reproducible (no atomics)
    first = [p[2].clone() for p in probs]
    o.WgradGroup(probs, tokens, tp)()
    torch.cuda.synchronize()
    assert all(torch.equal(a, p[2]) for a, p in zip(first, probs))


@pytest.mark.gpu
@pytest.mark.parametrize("lp", LP16)
def test_transpose_many_vector_and_scalar_paths(lp):
    """Batched weight transposes (the bf16 W^T copies of the dX products): 16-byte path for aligned matrices,
    scalar path for ragged ones, both inside one table."""
    import torch
    from w2v2_speaker_amd import ops
    dev = "cuda"
    shapes = [(768, 3072, 0), (2304, 768, 0), (200, 136, 0), (50, 70, 3), (64, 64, 0)]      # (R, C, extra offset)
    offs, total = [], 0
    for R, C, extra in shapes:
        total += extra
        offs.append(total)
        total += R * C
        total = (total + 7) // 8 * 8
    src = torch.randn(total, device=dev).to(lp)
    dst = torch.zeros_like(src)
    table = torch.tensor([[o, o, R, C] for (R, C, _), o in zip(shapes, offs)], dtype=torch.int64, device=dev)
    ops.transpose_many(src, dst, table, len(shapes))
    torch.cuda.synchronize()
    for (R, C, _), o in zip(shapes, offs):
        want = src[o:o + R * C].view(R, C).t().contiguous().view(-1)
        assert torch.equal(dst[o:o + R * C], want), (R, C)


@pytest.mark.gpu
@pytest.mark.parametrize("Cg", [48, 64])
@pytest.mark.parametrize("B,T", [(3, 149), (2, 301), (5, 37), (1, 160), (2, 161), (2, 249)])
@pytest.mark.parametrize("lp", LP16)
def test_posconv_direct_convolution_bit_equal_to_implicit_gemm(B, T, lp, Cg):
    """csrc/posconv_direct.hip (image of one (utterance, group) resident in LDS, weights streamed): forward (bias + GELU,
    pre-activation saved) and data-gradient (+ aux, in place) modes at the w2v2-base geometry (16 groups x 48 channels,
    128 taps) against (a) an f64 grouped convolution and (b) the implicit GEMM of w2v2_gemm over the SAME operands --
    bit for bit (same k order per accumulator).  T = 301 / 161: two frame blocks per utterance; T = 37: shorter than
    the kernel's halo."""
    o = ops()
    G, K = 16, 128               # Cg = 48: w2v2-base (H = 768); Cg = 64: wav2vec2-large (H = 1024; swizzled image rows, round 6)
    H, Tp, M = G * Cg, T + K - 1, B * T
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + T)
    x = (torch.randn(B, T, H, generator=g)).to(lp)
    wf = (torch.randn(G, Cg, K * Cg, generator=g) / (K * Cg) ** 0.5).to(lp)       # [g][co][tap*Cg + ci]
    bias = torch.randn(H, generator=g)
    res = (torch.randn(M, H, generator=g)).to(lp)
    xd, wd, bd = x.to(DEV), wf.to(DEV), bias.to(DEV)
    xg = torch.zeros(B, G, Tp, Cg, dtype=lp, device=DEV)
    o.posconv_regroup(xd.view(M, H), xg, B, T, H, G, K, K // 2)
    # f64 reference: out[b, t, g*Cg + co] = sum_{tap, ci} xpad[b, t + tap, g*Cg + ci] * w[g][co][tap][ci]
    xp = torch.nn.functional.pad(x.double().transpose(1, 2), (K // 2, K - 1 - K // 2))          # [B, H, Tp]
    w4 = wf.double().view(G, Cg, K, Cg).permute(0, 1, 3, 2).reshape(H, Cg, K)                      # torch layout [H][ci][tap]
    ref = torch.nn.functional.conv1d(xp, w4, groups=G).transpose(1, 2).reshape(M, H)              # [M, H]
    # (a) + (b), forward
    out_d, pre_d = torch.full((M, H), float("nan"), dtype=lp, device=DEV), torch.full((M, H), float("nan"), dtype=lp, device=DEV)
    o.posconv_direct(xg, wd, out_d, pre_d, bd, B, T, G, Cg, K, H, 0)
    out_g, pre_g = torch.zeros(M, H, dtype=lp, device=DEV), torch.zeros(M, H, dtype=lp, device=DEV)
    o.gemm(M, Cg, K * Cg, xg, wd, out_g, lda=Cg, ldb=K * Cg, ldc=H, a_seg=(T, G * Tp * Cg), batch=G, batch_inner=G,
           a_strides=(0, Tp * Cg), b_strides=(0, Cg * K * Cg), c_strides=(0, Cg), epilogue=o.EPI_BIAS_GELU, bias=bd,
           bias_stride1=Cg, aux=pre_g, ldaux=H, aux_strides=(0, Cg))
    torch.cuda.synchronize()
    tol = 4e-3 if lp == torch.float16 else 2e-2
    assert rel_l2(pre_d.float().cpu(), ref + bias.double()) < tol
    assert rel_l2(out_d.float().cpu(), torch.nn.functional.gelu(ref + bias.double())) < tol
    assert torch.equal(out_d, out_g) and torch.equal(pre_d, pre_g)
    # eval mode: no pre-activation buffer
    out_e = torch.zeros(M, H, dtype=lp, device=DEV)
    o.posconv_direct(xg, wd, out_e, None, bd, B, T, G, Cg, K, H, 0)
    torch.cuda.synchronize()
    assert torch.equal(out_e, out_d)
    # data-gradient mode: in place + aux
    acc_d, acc_g = res.to(DEV).clone(), res.to(DEV).clone()
    o.posconv_direct(xg, wd, acc_d, acc_d, None, B, T, G, Cg, K, H, 1)
    o.gemm(M, Cg, K * Cg, xg, wd, acc_g, lda=Cg, ldb=K * Cg, ldc=H, a_seg=(T, G * Tp * Cg), batch=G, batch_inner=G,
           a_strides=(0, Tp * Cg), b_strides=(0, Cg * K * Cg), c_strides=(0, Cg), epilogue=o.EPI_ADD, aux=acc_g, ldaux=H,
           aux_strides=(0, Cg))
    torch.cuda.synchronize()
    assert rel_l2(acc_d.float().cpu(), ref + res.double()) < tol
    assert torch.equal(acc_d, acc_g)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,G,Cg,K", [(3, 149, 16, 48, 128), (2, 249, 16, 64, 128), (2, 37, 4, 16, 16),
                                         (2, 170, 2, 32, 32)])
@pytest.mark.parametrize("lp", LP16)
def test_posconv_wgrad_correlation_kernel(B, T, G, Cg, K, lp):
    """dW[g][(j,c)][o] = sum_{b,t} xg[b,g,t+j,c] dY[b,t,g*Cg+o] against an f64 einsum on the same bf16 inputs
    (T > 160 exercises the second time chunk, T = 37 the zero-filled tail rows)."""
    import torch
    from w2v2_speaker_amd import ops
    dev = "cuda"
    H = G * Cg
    torch.manual_seed(B * 1000 + T)
    x = torch.randn(B, T, H, device=dev).to(lp)
    dY = torch.randn(B * T, H, device=dev).to(lp)
    Tp = T + K - 1
    xg = torch.zeros(B, G, Tp, Cg, dtype=lp, device=dev)
    ops.posconv_regroup(x, xg, B, T, H, G, K, K // 2)
    dwf = torch.full((G, K * Cg, Cg), float("nan"), dtype=torch.float32, device=dev)
    ops.posconv_wgrad(dY, xg, dwf, B, T, H, G, K)
    torch.cuda.synchronize()
    xw = xg.double().unfold(2, T, 1)                     # [B, G, K, Cg, T]: xw[b,g,j,c,t] = xg[b,g,t+j,c]
    dy = dY.double().view(B, T, G, Cg)
    want = torch.einsum("bgjct,btgo->gjco", xw, dy).reshape(G, K * Cg, Cg)
    err = float((dwf.double() - want).abs().max() / want.abs().max())
    assert torch.isfinite(dwf).all() and err < 2e-5, err
    dwf2 = torch.zeros_like(dwf)
    ops.posconv_wgrad(dY, xg, dwf2, B, T, H, G, K)
    assert torch.equal(dwf, dwf2)                        # deterministic


@pytest.mark.gpu
@pytest.mark.parametrize("lp", LP16)
def test_layernorm_bwd_deferred_fold_equals_immediate(lp):
    """w2v2_layernorm_bwd with dgamma = NULL + w2v2_layernorm_bwd_fold (one launch for several LayerNorms) must give
    bitwise the same dgamma / dbeta and ds as the immediate path."""
    import torch
    from w2v2_speaker_amd import ops
    dev = "cuda"
    M, H = 66 * 149, 768
    torch.manual_seed(5)
    group = ops.LnFoldGroup(H, dev)
    want, got = [], []
    for k in range(3):
        dy = torch.randn(M, H, device=dev).to(lp)
        s = torch.randn(M, H, device=dev).to(lp)
        mean, rstd = torch.randn(M, device=dev), torch.rand(M, device=dev) + 0.5
        gamma = torch.randn(H, device=dev)
        out = []
        for defer in (None, group):
            ds, dr = torch.empty_like(dy), torch.empty_like(dy)
            dg, db = torch.full((H,), 0.25, device=dev), torch.full((H,), -1.0, device=dev)   # fold ADDS
            ops.layernorm_bwd(dy, s, mean, rstd, gamma, ds, dr, dg, db, 0.1, 11 + k, defer_to=defer)
            out.append((ds, dr, dg, db))
        want.append(out[0])
        got.append(out[1])
    group.fold()
    torch.cuda.synchronize()
    for w, g in zip(want, got):
        for a, b in zip(w, g):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_zero_ranges_and_mean_kernels():
    o = ops()
    x = torch.ones(100_003, device=DEV)
    ranges = [(0, 5), (7, 1), (64, 4096), (4161, 3), (50_001, 49_999)]        # unaligned heads / tails, 1 element
    tab = torch.tensor(ranges, dtype=torch.int64, device=DEV)
    o.zero_ranges(x, tab, blocks_per_range=3)
    ref = torch.ones(100_003)
    for a, n in ranges:
        ref[a:a + n] = 0
    assert torch.equal(x.cpu(), ref)
    v = torch.randn(66, device=DEV)
    out = torch.empty((), device=DEV)
    o.mean(v, out)
    assert abs(float(out) - float(v.double().mean())) < 1e-6


@pytest.mark.gpu
def test_selective_zero_grad_equals_full_zero_under_layerdrop():
    """ParamStore.zero_grad(skip_layers) clears only what the backward accumulates into (+ the LayerDrop-skipped
    layers); the gradients of a step must be bit-identical to those after a full memset, whatever garbage the arena
    held before (the step before used a different skip pattern)."""
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    from oracle import w2v2_oracle as O
    cfg = W2V2Config.tiny()
    reg = Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                       hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)
    wav, label = O.synth_batch(3, 4000, 10, seed=11)
    wav, label = wav.to(DEV), label.to(DEV)
    grads = []
    for selective in (False, True):
        st = ParamStore(cfg, DEV, torch.float16, head="aam", num_speakers=10)
        st.init_weights(5)
        st.scaler[0] = 256.0
        plan = Plan(st, 3, 4000, train=True, reg=reg)
        tr = SpeakerTrainer(st, plan, Constant(0.0))
        if not selective:
            st.zero_grad = (lambda orig: (lambda skip_layers=None: orig(None)))(st.zero_grad)
        for name, off in st.offsets.items():                         # garbage in every gradient tensor (the 64-element
            if off < st.n_train:                                      # alignment gaps of the arena are never written)
                st.grad[off:off + int(np.prod(st.shapes[name]))] = float("nan")
        tr.train_step(wav, label, skip_layers=(0,))
        tr.train_step(wav, label, skip_layers=(1,))                   # layer 0 now written, layer 1 must be zeroed
        torch.cuda.synchronize()
        grads.append(st.grad.clone())
    assert torch.isfinite(grads[1]).all()
    assert torch.equal(grads[0], grads[1])
    lay1 = [s for n, s, e in st.grad_buckets() if n == "layer1"][0]
    lay1e = [e for n, s, e in st.grad_buckets() if n == "layer1"][0]
    assert float(grads[1][lay1:lay1e].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("lp", [torch.float16, torch.float32])
def test_aam_head_gradients_are_bitwise_reproducible(lp):
    """The AAM head's class-weight gradient needs coldot[c] = sum_b g * cos for the F.normalize backward.  It used to be
    accumulated with f32 atomics from one workgroup per batch row (run-to-run differences in the last bit of
    loss_fn.fc_weights' gradient, which made test_selective_zero_grad_... flaky); now the kernel stores the products and
    a one-writer column sum folds them in a fixed order.  66 rows x 5994 classes (the benchmark's head), ten repeats of
    the same head step on the same embedding: every gradient and d(emb) bit-equal."""
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    st = ParamStore(cfg, DEV, lp, head="aam", num_speakers=5994)
    st.init_weights(3)
    plan = Plan(st, 66, 4000, train=True)
    g = torch.Generator(device="cpu").manual_seed(5)
    plan.emb.copy_(torch.randn(plan.emb.shape, generator=g).to(DEV))
    label = torch.randint(0, 5994, (66,), generator=g).to(DEV)
    ref = None
    for _ in range(10):
        st.grad.zero_()
        loss, _ = plan.head_forward_backward(label)
        torch.cuda.synchronize()
        got = (st.g("loss_fn.fc_weights").clone(), plan.demb.clone(), loss.clone())
        assert all(bool(torch.isfinite(t).all()) for t in got)
        if ref is None:
            ref = got
        else:
            assert all(torch.equal(a, b) for a, b in zip(ref, got))
    assert float(ref[0].abs().max()) > 0


@pytest.mark.gpu
def test_adam_step_count_does_not_advance_on_skipped_steps():
    """torch's GradScaler does not call optimizer.step() when the gradients overflowed, so Adam's step count -- and its
    bias corrections -- only count applied updates.  The host-side counter of the engine advances every call (it never
    reads the device); with skip_slot the kernel subtracts the skipped count kept in the 8-float scaler record.
    Sequence: overflow, overflow, clean, overflow, clean, clean  ==  three torch Adam steps."""
    o = ops()
    n = 4 * 300 + 2
    pp = rnd(n, seed=1)
    ref = torch.nn.Parameter(pp.clone())
    opt = torch.optim.Adam([ref], lr=1e-2)
    pd = pp.clone().to(DEV)
    md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
    state = torch.tensor([64.0, 0, 0, 0, 0, 0, 0, 0], device=DEV)
    for call, overflow in enumerate([True, True, False, True, False, False]):
        gr = rnd(n, seed=20 + call)
        scale = float(state[0])
        gs = (gr * scale).to(DEV)
        if overflow:
            gs[call] = float("inf")
        else:
            ref.grad = gr.clone()
            opt.step()
        o.grad_scaler_check(gs, n, state)
        o.adam_step(pd, gs, md, vd, None, n, 1e-2, 0.9, 0.999, 1e-8, call + 1, scaler=state, skip_slot=5)
        o.grad_scaler_update(state, 2.0, 0.5, 1000, skipped_ranges=3)
    torch.cuda.synchronize()
    assert state.tolist()[:6] == [8.0, 0.0, 2.0, 3.0, 3.0, 3.0]      # scale 64 / 2^3, two clean steps since the last overflow
    assert np.allclose(pd.cpu().numpy(), ref.detach().numpy(), atol=2e-6)
    # without the correction the first applied update would use t = 3: (1 - 0.9^1) / (1 - 0.9^3) = 0.37x ... visible
    assert float((pd.cpu() - pp).abs().max()) > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("lp", LP16)
@pytest.mark.parametrize("tokens", [9834, 2 * 64 * 7 + 5, 64])
def test_grouped_weight_gradient_phased_kernel_two_block_group(lp, tokens):
    """wgrad_grouped_phased_kernel (csrc/wgrad_phased.hip; family 4 of w2v2_tune_wgrad_kernel, the library's choice for the
    two-block groups of the training step): the 8 problems of two w2v2-base transformer blocks = 216 tiles of 256x256.
    Checked: every dW / dbias element against an f64 reference; BIT-EQUAL to the 256x256x32 ring kernel (family 3: same
    k order per accumulator) and to itself over repeated launches while another stream saturates HBM; tokens = 901 is a
    ragged token count (rows up to the padded count are zero by contract), tokens = 64 a single K tile (prologue only)."""
    from w2v2_speaker_amd import _lib
    o = ops()
    H, I = 768, 3072
    Mp = (tokens + 63) // 64 * 64
    g = torch.Generator(device="cpu").manual_seed(tokens)

    def mk(c):
        t = torch.zeros(Mp, c, dtype=lp, device=DEV)
        t[:tokens] = (torch.randn(tokens, c, generator=g) * 0.5).to(lp).to(DEV)
        return t
    probs = []
    for _ in range(2):
        probs += [(mk(H), mk(I)), (mk(I), mk(H)), (mk(H), mk(H)), (mk(3 * H), mk(H))]
    res = {}
    try:
        for fam in (4, 3):
            outs = [(torch.full((dy.shape[1], x.shape[1]), float("nan"), device=DEV),
                     torch.full((dy.shape[1],), float("nan"), device=DEV)) for dy, x in probs]
            wg = o.WgradGroup([(dy, x, dw, db) for (dy, x), (dw, db) in zip(probs, outs)], tokens, Mp)
            o.lib().w2v2_tune_wgrad_kernel(fam)
            wg()
            torch.cuda.synchronize()
            res[fam] = (wg, outs, [(dw.clone(), db.clone()) for dw, db in outs])
    finally:
        o.lib().w2v2_tune_wgrad_kernel(0)
    for (dy, x), (dw, db), (rw, rb) in zip(probs, res[4][2], res[3][2]):
        ref = dy[:tokens].double().t() @ x[:tokens].double()
        assert float((dw.double() - ref).norm() / ref.norm()) < 2e-6
        refb = dy[:tokens].double().sum(0)
        assert float((db.double() - refb).norm() / refb.norm()) < 2e-6
        assert torch.equal(dw, rw) and torch.equal(db, rb)
    # repeatable under HBM load (the library's own dispatch must pick the phased kernel for this group: same bits)
    wg, outs, first = res[4]
    hog_a = torch.empty(128 << 20, dtype=torch.float32, device=DEV)
    hog_b = torch.empty_like(hog_a)
    side = torch.cuda.Stream()
    for it in range(4):
        for dw, db in outs:
            dw.fill_(float("nan")); db.fill_(float("nan"))
        with torch.cuda.stream(side):
            for _ in range(2 + it % 3):
                hog_b.copy_(hog_a); hog_a.copy_(hog_b)
        wg()
        torch.cuda.synchronize()
        for (dw, db), (fw, fb) in zip(outs, first):
            assert torch.equal(dw, fw) and torch.equal(db, fb), it


@pytest.mark.gpu
@pytest.mark.parametrize("lp", LP16)
def test_grouped_weight_gradient_phased_kernel_ragged_problems(lp):
    """The phased kernel on tile grids with ragged edges: n_out / n_in that are multiples of 8 but not of 256 (columns
    past the edge are clamped on the DMA side and never stored), a problem narrower than one tile, no bias pointer."""
    o = ops()
    tokens, Mp = 1000, 1024
    g = torch.Generator(device="cpu").manual_seed(11)

    def mk(c):
        t = torch.zeros(Mp, c, dtype=lp, device=DEV)
        t[:tokens] = (torch.randn(tokens, c, generator=g) * 0.5).to(lp).to(DEV)
        return t
    shapes = [(1536, 520, True), (264, 768, False), (1024, 1024, True), (72, 40, True), (512, 3072, True)]
    probs = [(mk(no), mk(ni)) for no, ni, _ in shapes]
    outs = [(torch.full((no, ni), float("nan"), device=DEV), torch.full((no,), float("nan"), device=DEV) if hb else None)
            for no, ni, hb in shapes]
    wg = o.WgradGroup([(dy, x, dw, db) for (dy, x), (dw, db) in zip(probs, outs)], tokens, Mp)
    try:
        o.lib().w2v2_tune_wgrad_kernel(4)
        wg()
        torch.cuda.synchronize()
    finally:
        o.lib().w2v2_tune_wgrad_kernel(0)
    for (dy, x), (dw, db) in zip(probs, outs):
        ref = dy[:tokens].double().t() @ x[:tokens].double()
        assert float((dw.double() - ref).norm() / ref.norm()) < 2e-6
        if db is not None:
            refb = dy[:tokens].double().sum(0)
            assert float((db.double() - refb).norm() / refb.norm()) < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("lp", LP16)
def test_grouped_weight_gradient_forced_families_small_ragged_group(lp):
    """Every forced family of w2v2_tune_wgrad_kernel (1 = 128x128, 2 = 256x128 ring, 3 = 256x256x32 ring, 4 = phased) on
    one small ragged group, which the library's own choice would send to one of them only.  tokens = 261 pads to 320 =
    five 64-token K tiles: the 3-stage ring wraps, the 4-stage ring runs ten stages, the phased kernel uses both buffers
    and both tail branches.  Problems with edges in both dimensions, one narrower than any tile and without bias.
    Checked: every dW / dbias against the float64 product over the first 261 rows (rel-L2 < 1e-5, the bound of
    test_grouped_weight_gradient_gemm), no NaN of the pre-fill left, family 4 bit-equal to family 3 (wgrad_phased.hip)."""
    o = ops()
    tokens, Mp = 261, 320
    g = torch.Generator(device="cpu").manual_seed(261)

    def mk(c):
        t = torch.zeros(Mp, c, dtype=lp, device=DEV)
        t[:tokens] = (torch.randn(tokens, c, generator=g) * 0.5).to(lp).to(DEV)
        return t
    shapes = [(264, 136, True), (72, 40, False), (520, 264, True)]
    probs = [(mk(no), mk(ni)) for no, ni, _ in shapes]
    refs = [(dy[:tokens].double().t() @ x[:tokens].double(), dy[:tokens].double().sum(0)) for dy, x in probs]
    res = {}
    try:
        for fam in (1, 2, 3, 4):
            outs = [(torch.full((no, ni), float("nan"), device=DEV),
                     torch.full((no,), float("nan"), device=DEV) if hb else None) for no, ni, hb in shapes]
            wg = o.WgradGroup([(dy, x, dw, db) for (dy, x), (dw, db) in zip(probs, outs)], tokens, Mp)
            o.lib().w2v2_tune_wgrad_kernel(fam)
            wg()
            torch.cuda.synchronize()
            res[fam] = outs
    finally:
        o.lib().w2v2_tune_wgrad_kernel(0)
    for fam, outs in res.items():
        for (dw, db), (rw, rb), shp in zip(outs, refs, shapes):
            assert not bool(torch.isnan(dw).any()), (fam, shp)
            assert rel_l2(dw.cpu(), rw.cpu()) < 1e-5, (fam, shp)
            if db is not None:
                assert not bool(torch.isnan(db).any()), (fam, shp)
                assert rel_l2(db.cpu(), rb.cpu()) < 1e-5, (fam, shp)
    for (dw4, db4), (dw3, db3) in zip(res[4], res[3]):
        assert torch.equal(dw4, dw3)
        assert db4 is None or torch.equal(db4, db3)


# ----------------------------------------------------------------------------------------------- round-5 small kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,C,E", [(66, 5994, 1536), (7, 37, 192), (150, 1211, 768), (3, 16, 520)])
def test_fused_aam_class_weight_gradient_vs_torch(B, C, E, dtype):
    """w2v2_aam_dw (csrc/heads.hip): dW[c][e] = inv_w[c] * (sum_b dcos[b][c] emb[b][e] - W[c][e] inv_w[c] sum_b colprod[b][c])
    = the autograd of F.linear(F.normalize(x), F.normalize(W)) wrt W (ref: src/optim/loss/aam_softmax.py:55) for a given
    d(loss)/d(cos); ragged class / column / batch-chunk counts (B > 36 = several staged passes), every operand dtype."""
    o = ops()
    ldc = (C + 7) // 8 * 8
    dcos = rnd(B, ldc, seed=1, scale=1e-2).to(dtype)
    emb = rnd(B, E, seed=2).to(dtype)
    W = rnd(C, E, seed=3)
    colprod = rnd(B, C, seed=4, scale=1e-2)
    inv_w = 1.0 / W.norm(dim=1)
    dW = torch.full((C, E), float("nan"), device=DEV)
    o.aam_dw(dcos.to(DEV), emb.to(DEV), colprod.to(DEV), W.to(DEV), inv_w.to(DEV), dW, B, C, E, ldc)
    torch.cuda.synchronize()
    H1 = dcos[:, :C].double().t() @ emb.double()
    dot = colprod.double().sum(0)
    ref = inv_w.double()[:, None] * (H1 - W.double() * (inv_w.double() * dot)[:, None])
    assert torch.isfinite(dW).all()
    assert rel_l2(dW.cpu(), ref) < 2e-6
    # and it is the autograd of the normalised linear map when dcos / colprod come from an upstream gradient G
    if dtype == torch.float32 and B <= 66:
        Wr = W.double().clone().requires_grad_(True)
        x = rnd(B, E, seed=2).double()
        G = rnd(B, C, seed=9, scale=1e-2).double()
        cos = torch.nn.functional.normalize(x) @ torch.nn.functional.normalize(Wr).t()
        (cos * G).sum().backward()
        inv_x = 1.0 / x.norm(dim=1)
        dcx = torch.zeros(B, ldc)
        dcx[:, :C] = (G * inv_x[:, None]).float()              # d(loss)/d(cos) * inv_x: what the row kernel hands over
        dW2 = torch.empty(C, E, device=DEV)
        o.aam_dw(dcx.to(DEV), x.float().to(DEV), (G * cos.detach()).float().to(DEV), W.to(DEV), inv_w.to(DEV), dW2, B, C, E, ldc)
        torch.cuda.synchronize()
        assert rel_l2(dW2.cpu(), Wr.grad) < 1e-5


@pytest.mark.parametrize("M", [9834, 40000])
def test_pos_conv_bias_and_mask_embed_gradients_are_bitwise_reproducible(M):
    """The column sums of gelu_bwd_colsum (pos-conv bias gradient) and mask_fill_bwd (masked_spec_embed gradient) go
    through a fixed-order fold of per-block partial rows: repeated calls on the same inputs give the same bits (the former
    cross-block atomics did not), and the sums stay within rounding of an f64 reference.  M = 40000 exceeds the 256
    partial rows mask_fill_bwd can use at 64 rows per block."""
    o = ops()
    H = 768
    dy, pre = rnd(M, H, seed=1).half().to(DEV), rnd(M, H, seed=2, scale=1.5).half().to(DEV)
    h = rnd(M, H, seed=3).half()
    mask = (torch.arange(M) % 3 == 0).to(torch.uint8).to(DEV)
    cs, de = [], []
    for _ in range(4):
        dx, c = torch.empty_like(dy), torch.full((H,), 0.25, device=DEV)
        o.gelu_bwd_colsum(dy, pre, dx, c, M, H)
        dh, d = h.to(DEV), torch.zeros(H, device=DEV)
        o.mask_fill_bwd(dh, mask, d)
        torch.cuda.synchronize()
        cs.append(c.cpu())
        de.append(d.cpu())
    assert all(torch.equal(cs[0], c) for c in cs[1:]) and all(torch.equal(de[0], d) for d in de[1:])
    # a call on a side stream gets a workspace of its own (no race with the compute stream) and the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dx2, c2 = torch.empty_like(dy), torch.full((H,), 0.25, device=DEV)
        o.gelu_bwd_colsum(dy, pre, dx2, c2, M, H)
        ws_side = o._partial_workspace(H, dy.device, o.stream())
    torch.cuda.synchronize()
    assert ws_side.data_ptr() != o._partial_workspace(H, dy.device, o.stream()).data_ptr()
    assert torch.equal(c2.cpu(), cs[0])
    ref = 0.25 + dx.double().sum(0).cpu()
    assert float((cs[0].double() - ref).abs().max()) < 1e-4 * float(dx.double().abs().sum(0).max()) + 1e-6
    assert rel_l2(de[0], h.double()[mask.cpu().bool()].sum(0)) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N", [(9834, 768), (301, 64), (17, 1024)])
def test_gelu_backward_with_column_sums_in_one_pass(M, N, dtype):
    """w2v2_gelu_bwd_colsum == w2v2_gelu_bwd followed by w2v2_colsum of the stored product (the pos-conv bias gradient)."""
    o = ops()
    dy, pre = rnd(M, N, seed=1).to(dtype).to(DEV), rnd(M, N, seed=2, scale=1.5).to(dtype).to(DEV)
    dx_a, dx_b = torch.empty_like(dy), torch.empty_like(dy)
    cs_a, cs_b = torch.full((N,), 0.25, device=DEV), torch.full((N,), 0.25, device=DEV)      # accumulates into its target
    o.gelu_bwd_colsum(dy, pre, dx_a, cs_a, M, N)
    o.gelu_bwd(dy, pre, dx_b)
    o.colsum(dx_b, cs_b, M, N)
    torch.cuda.synchronize()
    assert torch.equal(dx_a, dx_b)
    ref = 0.25 + dx_b.double().sum(0)
    assert float((cs_a.double() - ref).abs().max()) < 1e-4 * float(dx_b.double().abs().sum(0).max()) + 1e-6
    assert float((cs_b.double() - ref).abs().max()) < 1e-4 * float(dx_b.double().abs().sum(0).max()) + 1e-6
