"""Cases, operand builders, float64 references and per-element bounds for w2v2_gemm (csrc/gemm*.hip), shared by
tests/test_gemm_cases_cpu.py, tests/test_gemm_edges_gpu.py and tools/gemm_parity.py.  No GPU and no ``ops`` import here:
everything is plain torch on the CPU.

A case names the kernel family it must run on, how it gets there (default route, a tuner call, or an operand property
such as a transposed layout or K % 64 != 0), its shape and its descriptor options.  Every case is judged PER ELEMENT over
EVERY element of C (and of a written aux), never by one whole-matrix norm:

exact class   A and B hold small integers times a power of two, bias / aux integers |v| <= 8, scales powers of two,
              alpha a power of two.  ``problem`` asserts that (|A| @ |B|^T).max() * |alpha| and the epilogue's result stay
              below 2^24 units of the finest grid, so every partial sum in ANY order is exact in f32: an f32 C must be
              torch.equal to the float64 reference, a 16-bit C to the reference rounded once (.to(lp), nearest even).
              Split-K and accumulate atomics included.
real class    normal operands rounded to the operand type, float64 reference, and per element
                  |got - ref| <= nterms * 2^-24 * S + u_out * |ref| (+ 2^-25 for an fp16 C: its subnormal grid),
              S = |alpha| (|A| @ |B|^T) + the magnitudes of the epilogue's terms, u_out = 0 / 2^-8 / 2^-11 for f32 / bf16 /
              fp16 C (the unit roundoff of the type).  nterms = K: the worst-case bound of an f32 sum of K terms in any order (K - 1 additions) with one
              more rounding for the epilogue's addition; the multiplying epilogues (MUL, SCALE_RC) round twice more and
              take K + 2, and a launch that adds into what C holds (accumulate, split-K) one more for that term.
              Derived, not tuned: at K = 768 it is 4.6e-5 of S.
gelu class    exact-class operands with alpha = +-2^-5 / 2^-6 and bias in multiples of 1/4, so the pre-activation x is
              known exactly.  gelu(x) and gelu'(x) are held to (0.75e-7 + 2 E) max(1, |x|) + u_out |ref|: 0.75e-7 is half
              of the published error 1.5e-7 of Abramowitz & Stegun 7.1.26 (the formula erf_fast implements; gelu halves
              it and multiplies by x), E the error of torch's CPU f32 F.gelu (its autograd for the derivative) against
              float64 on the same x over max(1, |x|), maximised over the case and recomputed every time.  GELU_BWD
              multiplies the exact product g = alpha acc by gelu'(aux): its bound is |g| times the same factor plus
              2^-24 |ref| for that multiplication.

Buffers.  C and a written aux carry 8 guard rows in front, 16 behind and >= 8 guard columns (ldc >= N + 8), prefilled
with NaN (integers for the accumulate and split-K cases, which add into what C holds): ``judge`` asserts that no valid
element is NaN afterwards and that every guard cell still holds its prefill bit for bit.  Operand padding (lda > K, ...)
is NaN as well.

Run as a script it prints the families ``w2v2_gemm_kernel_of`` answers for the cases of one tuner setting (ROUTE_TUNE
= "", "kernel=2", "f32_tile=13", ...) as one JSON list; tests/test_gemm_cases_cpu.py starts it in a fresh process per
setting, like tests/gemm_route_cases.py."""
import functools
import json
import math
import os
import sys

import torch

F64 = torch.float64
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
DT_CODE = {"f32": 0, "bf16": 1, "f16": 2}
# unit roundoff of one round-to-nearest into the output type: half an ulp of a p-bit significand is 2^-p of the value
# (bf16 p = 8, fp16 p = 11).  Nothing smaller can hold: torch's own .to(bfloat16) of an exact value reaches 2^-8.
U_OUT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
EPI = {"none": 0, "bias": 1, "bias_gelu": 2, "gelu_bwd": 3, "add": 4, "scale_rc": 5, "bias_gelu_grad": 6, "mul": 7}
# below its smallest normal (2^-14) fp16 is a fixed grid of 2^-24: rounding onto it moves a value by up to 2^-25 whatever
# its size.  (bf16 has the exponent range of f32: its subnormal grid is below anything these cases produce.)
U_ABS = {"f32": 0.0, "bf16": 0.0, "f16": 2.0 ** -25}
EXACT_EPIS = ("none", "bias", "add", "mul", "scale_rc")
GELU_EPIS = ("bias_gelu", "bias_gelu_grad", "gelu_bwd")
READS_AUX, WRITES_AUX = ("add", "mul", "gelu_bwd"), ("bias_gelu", "bias_gelu_grad")
KERNEL_OF = {4: "gemm16_phased_256x256_kernel", 2: "gemm16_ring_256x128_kernel", 1: "gemm16_dma_128_kernel",
             3: "gemm16_regstage_kernel", 9: "gemm_f32_mfma_kernel", 10: "gemm_f32_dma_kernel"}
# the library's A/B switches that move products between kernels: the GPU tests skip under any of them
SWITCHES = ("W2V2_NO_GEMM_PH", "W2V2_NO_GLDS3", "W2V2_NO_GLDS", "W2V2_F32_NO_DMA", "W2V2_G3N", "W2V2_NO_DEFER",
            "W2V2_G3_NONPERSISTENT", "W2V2_RESERVE_CUS")
LP = ("bf16", "f16")
EPS32 = 2.0 ** -24
GELU_POLY_HALF = 0.75e-7
GUARD_FRONT, GUARD_BACK, GUARD_COLS = 8, 16, 8

DEFAULTS = dict(tune=None, ta=False, tb=False, alpha=1.0, lda_x=0, ldb_x=0, ldc_x=0, ldaux_x=0, aux_is_c=False, aux_off=0,
                bias_off=0, accumulate=False, split=1, conv=None, batch=None, n_ext_from=None)


# ------------------------------------------------------------------------------------------------ case table
def case(group, fam, M, N, K, ab, c=None, cls="exact", epi="none", **kw):
    assert not set(kw) - set(DEFAULTS), kw
    cs = dict(DEFAULTS, group=group, fam=fam, M=M, N=N, K=K, ab=ab, c=c or ab, cls=cls, epi=epi, **kw)
    if cs["conv"]:
        Bn, Lo, Cin, k, st = cs["conv"]
        assert M == Bn * Lo and K == k * Cin
    opts = ",".join(f"{k}={cs[k]}" for k in DEFAULTS if cs[k] != DEFAULTS[k])
    cs["name"] = f"{group}/fam{fam}/{M}x{N}x{K}/{ab}>{cs['c']}/{cls}/{epi}" + (f"/{opts}" if opts else "")
    return cs


def tune_name(cs):
    return "" if cs["tune"] is None else f"{cs['tune'][0]}={cs['tune'][1]}"


def lines_rule(cs, lay):
    """gemm_common.h lines_ok as the case table claims it: 16-bit C, 16-byte aligned rows of C and aux, N % 64 == 0.
    The case table restates this piece of the route ON PURPOSE (as ``forced``, ``f32_case`` and ``wide_cases`` restate
    theirs): a case has to name its family before the library is asked.  The restatement is held to the library twice,
    by tests/test_gemm_cases_cpu.py through w2v2_gemm_kernel_of and by the kernel_name assertion in front of every
    launch, so a change to lines_ok or to the route fails here by design and the table is then brought in line."""
    aux = cs["epi"] in READS_AUX + WRITES_AUX
    return (cs["c"] != "f32" and cs["N"] % 64 == 0 and lay["ldc"] % 8 == 0 and lay["c_base"] % 8 == 0 and cs["split"] == 1
            and not cs["accumulate"] and (not aux or (lay["ldaux"] % 8 == 0 and lay["aux_base"] % 8 == 0)))


def forced(group, force, M, N, K, ab, c=None, cls="exact", epi="none", **kw):
    """A K-contiguous 16-bit product under w2v2_tune_gemm_kernel(force): the family the route must answer -- 1 for split-K
    and accumulate whatever is forced, the ring instead of the phased kernel for a 16-bit C without whole lines.
    (An intended mirror of gemm_route, checked against the library: see lines_rule.)"""
    cs = case(group, force, M, N, K, ab, c, cls, epi, tune=("kernel", force), **kw)
    fam = force
    if cs["split"] > 1 or cs["accumulate"]:
        fam = 1
    elif force == 4 and cs["c"] != "f32" and not lines_rule(cs, layout(cs)):
        fam = 2
    return case(group, fam, M, N, K, ab, c, cls, epi, tune=("kernel", force), **kw)


def f32_case(group, code, M, N, K, cls="exact", epi="none", **kw):
    """An f32 product under w2v2_tune_gemm_f32_tile(code): family 10 where the LDS-DMA kernel can take it, else 9.
    (An intended mirror of the f32 route's eligibility test, checked against the library: see lines_rule.)"""
    cs = case(group, 9, M, N, K, "f32", "f32", cls, epi, tune=("f32_tile", code), **kw)
    lay = layout(cs)
    ok = (lay["lda"] % 4 == 0 and lay["ldb"] % 4 == 0 and K % 4 == 0 and M > 64 and N > 64 and
          (not cs["ta"] or M % 4 == 0) and (not cs["tb"] or N % 4 == 0))
    fam = 10 if (ok and (code % 100 >= 11 or code == 0)) else 9
    return case(group, fam, M, N, K, "f32", "f32", cls, epi, tune=("f32_tile", code), **kw)


SWEEP_M, SWEEP_N, SWEEP_K = (9, 255, 257, 391, 520), (64, 72, 100, 129, 192, 256, 320), (64, 128, 192, 256, 320)
EPI_SHAPES = ((391, 192, 192), (257, 100, 128))
FEATURE_SHAPE = (391, 192, 192)
F32_CODES = (1, 2, 3, 4, 11, 12, 13, 14, 15, 115)
F32_SHAPES = ((97, 70, 36), (65, 132, 8), (200, 136, 160), (328, 260, 100))
LAYOUTS = ((False, False), (False, True), (True, False), (True, True))
CONV_GEOM = ((32, 2, 2), (64, 3, 2))
CONV_LO = (100, 256, 300)
ROUND_K = (64, 192, 256, 320)


def sweep_cases(ab, c, cls):
    """Families 1, 2 and 4 forced on the same operands over the tile edges of M, N and nk = 1..5."""
    return [forced("sweep", f, M, N, K, ab, c, cls) for M in SWEEP_M for N in SWEEP_N for K in SWEEP_K for f in (1, 2, 4)]


def epilogue_cases(ab, c):
    """Every epilogue kind on the three LDS-DMA families, with 16-byte rows of C and with an odd ldc (scalar stores)."""
    out = []
    for (M, N, K) in EPI_SHAPES:
        for ldc_x in (0, 1):
            for epi in EXACT_EPIS + GELU_EPIS:
                kw = dict(alpha=2.0 ** -5, cls="gelu") if epi in GELU_EPIS else dict(cls="exact")
                out += [forced("epilogue", f, M, N, K, ab, c, epi=epi, ldc_x=ldc_x, **kw) for f in (1, 2, 4)]
            out += [forced("epilogue", f, M, N, K, ab, c, "real", epi, ldc_x=ldc_x) for epi in ("bias", "add", "mul")
                    for f in (1, 2, 4)]
    return out


def round_shape(family, cus):
    """N = 512 and just over one round of tiles on `cus` CUs: a partial second round and a ragged last M tile."""
    tiles_m = -(-(cus + 5) // (4 if family == 2 else 2))
    return 256 * tiles_m - 37, 512


def round_cases(family, ab, K, cus):
    """Persistent rounds: more tiles than CUs, so a workgroup runs a second tile (deferred stores on the ring for the
    16-bit C of NONE / ADD / BIAS) or leaves the tile loop early."""
    M, N = round_shape(family, cus)
    return [forced("rounds", family, M, N, K, ab, ab), forced("rounds", family, M, N, K, ab, ab, epi="add", aux_is_c=True),
            forced("rounds", family, M, N, K, ab, ab, epi="bias"), forced("rounds", family, M, N, K, ab, "f32")]


def conv_cases(ab):
    """Segmented A (implicit convolution over channels-last [B, L, Cin]) on families 1, 2 and 4: tiles inside one
    segment, equal to one, across a boundary, and the ragged last tile."""
    out = []
    for (Cin, k, st) in CONV_GEOM:
        for Lo in CONV_LO:
            for c in (ab, "f32"):
                out += [forced("conv", f, 3 * Lo, 128, k * Cin, ab, c, conv=(3, Lo, Cin, k, st)) for f in (1, 2, 4)]
    return out


def feature_options():
    """(epilogue, class, options) of the descriptor features: alpha, ldaux != ldc, aux == C, misaligned aux, a bias
    slice from element 1."""
    out = [(e, "exact", dict(alpha=a)) for e in EXACT_EPIS for a in (0.5, -2.0)]
    out += [(e, "gelu", dict(alpha=a)) for e in GELU_EPIS for a in (2.0 ** -6, -2.0 ** -5)]
    out += [("add", "exact", dict(ldaux_x=8)), ("bias_gelu", "gelu", dict(ldaux_x=8, alpha=2.0 ** -5)),
            ("add", "exact", dict(aux_is_c=True)), ("mul", "exact", dict(aux_is_c=True)),
            ("gelu_bwd", "gelu", dict(aux_is_c=True, alpha=2.0 ** -5)),
            ("add", "exact", dict(aux_off=1)), ("bias_gelu", "gelu", dict(aux_off=1, alpha=2.0 ** -5)),
            ("bias", "exact", dict(bias_off=1)), ("add", "real", dict(alpha=0.5, ldaux_x=8)), ("bias", "real", dict(bias_off=1))]
    return out


def feature_cases(ab, c):
    M, N, K = FEATURE_SHAPE
    out = [forced("feature", f, M, N, K, ab, c, cls, epi, **kw) for (epi, cls, kw) in feature_options() for f in (1, 2, 4)]
    if c == "f32":
        out += [forced("feature", f, M, N, K, ab, c, cls, accumulate=True) for cls in ("exact", "real") for f in (1, 2, 4)]
        for split in (2, 3, 5):
            out += [forced("feature", 1, M, N, 320, ab, c, cls, "bias", split=split) for cls in ("exact", "real")]
            out += [case("feature", 3, M, N, 200, ab, c, cls, "bias", split=split) for cls in ("exact", "real")]
    return out


REGSTAGE_FEATURE_K = 200                           # K % 64 != 0: the default route's way to the register-staged kernel
REGSTAGE_FEATURE_LAYOUTS = ((False, False), (True, False), (False, True))


def feature_cases_regstage(ab, c):
    """The descriptor features on family 3 (its split-K cases are in feature_cases): every feature_options() entry and
    accumulate onto an integer C at K = 200 on the default route, K-contiguous and with A or B transposed (the
    transposed A has lda = 391: its loads take the scalar path)."""
    M, N, _ = FEATURE_SHAPE
    K, out = REGSTAGE_FEATURE_K, []
    for (ta, tb) in REGSTAGE_FEATURE_LAYOUTS:
        out += [case("feature", 3, M, N, K, ab, c, cls, epi, ta=ta, tb=tb, **kw) for (epi, cls, kw) in feature_options()]
        if c == "f32":
            out += [case("feature", 3, M, N, K, ab, c, cls, ta=ta, tb=tb, accumulate=True) for cls in ("exact", "real")]
    return out


def wide_shape(cus):
    """N = 256 and just enough 128-row tiles that 128 x 128 tiles fill more than half of `cus` CUs: gemm_route then
    leaves the 64-column tile (narrow) and family 1 runs its 128 x 128 instantiation, the one the conv stack uses.
    The last M tile is ragged."""
    tiles_m = cus // 4 + 1
    return 128 * tiles_m - 37, 256


def wide_cases(ab, cus):
    """Family 1 forced where it takes 128 x 128 tiles (every other family-1 case here is small enough for the
    128 x 64 tile on a 256-CU device): whole lines and ragged columns, each epilogue path, both output types."""
    M, N = wide_shape(cus)
    out = []
    for c in (ab, "f32"):
        out += [forced("wide", 1, M, N, 128, ab, c), forced("wide", 1, M, N, 192, ab, c, "real", "bias"),
                forced("wide", 1, M, N, 128, ab, c, epi="add", aux_is_c=True),
                forced("wide", 1, M, N, 128, ab, c, "gelu", "bias_gelu", alpha=2.0 ** -5),
                forced("wide", 1, M, N - 56, 192, ab, c, "real"), forced("wide", 1, M, N - 56, 128, ab, c, epi="scale_rc", alpha=0.5)]
    return out


def feature_cases_f32():
    M, N, K = FEATURE_SHAPE
    out = [f32_case("feature", 0, M, N, K, cls, epi, **kw) for (epi, cls, kw) in feature_options()]
    out += [f32_case("feature", 0, M, N, K, cls, accumulate=True) for cls in ("exact", "real")]
    out += [f32_case("feature", 0, M, N, 320, cls, "bias", split=s) for s in (2, 3, 5) for cls in ("exact", "real")]
    return out


def regstage_cases(ab, c):
    """Family 3: the four layouts, K tails, leading dimensions that are no multiple of 8, the 64-column tile."""
    out = []
    for (ta, tb) in LAYOUTS:
        for K in (1, 8, 63, 65, 100, 136):
            for (M, N) in ((149, 48), (300, 130)):
                for x in (0, 3):
                    for cls in ("exact", "real"):
                        out.append(case("regstage", 3, M, N, K, ab, c, cls, ta=ta, tb=tb, lda_x=x, ldb_x=x, ldc_x=x))
    return out


def batched_cases(ab):
    """Family 1, batched as the positional convolution calls it: 2 x 3 products, per-group bias and aux."""
    out = []
    for c in (ab, "f32"):
        out += [case("batched", 1, 150, 128, 128, ab, c, batch=(2, 3)),
                case("batched", 1, 150, 128, 128, ab, c, "real", "bias", batch=(2, 3)),
                case("batched", 1, 150, 128, 128, ab, c, "gelu", "bias_gelu", batch=(2, 3), alpha=2.0 ** -5)]
    return out


def two_term_cases(ab, cus):
    out = []
    Mr, Nr = round_shape(2, cus)
    for c in (ab, "f32"):
        out += [case("two_term", 2, 300, 384, 128, ab, c, n_ext_from=nf) for nf in (0, 128, 256)]
        out += [case("two_term", 2, Mr, Nr, 128, ab, c, n_ext_from=256), case("two_term", 2, Mr, Nr, 128, ab, c, epi="bias", n_ext_from=256)]
    return out


def f32_cases(code):
    out = []
    for (ta, tb) in LAYOUTS:
        for (M, N, K) in F32_SHAPES:
            out += [f32_case("f32", code, M, N, K, cls, ta=ta, tb=tb) for cls in ("exact", "real")]
        out.append(f32_case("f32", code, 192, 160, 2000, "exact", ta=ta, tb=tb, split=5))
    return out


def all_cases(cus=256):
    """Every case, as tests/test_gemm_edges_gpu.py groups them (the persistent-round shapes follow the CU count)."""
    out = []
    for ab in LP:
        for c in (ab, "f32"):
            out += sweep_cases(ab, c, "exact") + sweep_cases(ab, c, "real") + epilogue_cases(ab, c) + feature_cases(ab, c)
            out += feature_cases_regstage(ab, c) + regstage_cases(ab, c)
        for fam in (2, 4):
            for K in ROUND_K:
                out += round_cases(fam, ab, K, cus)
        out += conv_cases(ab) + batched_cases(ab) + two_term_cases(ab, cus) + wide_cases(ab, cus)
    out += feature_cases_f32()
    for code in F32_CODES:
        out += f32_cases(code)
    return out


# ------------------------------------------------------------------------------------------------ layout
def layout(cs):
    """Leading dimensions, strides, buffer sizes and element offsets of a case (all in elements)."""
    M, N, K = cs["M"], cs["N"], cs["K"]
    Z0, Z1 = cs["batch"] or (1, 1)
    lay = dict(Z0=Z0, Z1=Z1, a_seg=(0, 0), a_strides=(0, 0), b_strides=(0, 0), c_strides=(0, 0), aux_strides=(0, 0),
               bias_stride1=0)
    if cs["conv"]:
        Bn, Lo, Cin, k, st = cs["conv"]
        L = (Lo - 1) * st + k + 1
        lay.update(lda=st * Cin, a_seg=(Lo, L * Cin), a_size=Bn * L * Cin, conv_L=L)
    elif cs["batch"]:
        lay.update(lda=Z1 * K, a_strides=(M * Z1 * K, K), a_size=Z0 * M * Z1 * K)
    else:
        lay["lda"] = (M if cs["ta"] else K) + cs["lda_x"]
        lay["a_size"] = (K if cs["ta"] else M) * lay["lda"]
    lay["ldb"] = (N if cs["tb"] else K) + cs["ldb_x"]
    lay["b_size"] = (K if cs["tb"] else N) * lay["ldb"]
    if cs["batch"]:
        lay.update(b_strides=(0, N * K), b_size=Z1 * N * K, bias_stride1=N)
    if cs["n_ext_from"] is not None:
        lay.update(b_size=2 * N * K, b_lo_off=N * K)
    ldc = Z1 * N + GUARD_COLS + cs["ldc_x"]
    ldaux = ldc + cs["ldaux_x"]
    rows = GUARD_FRONT + Z0 * M + GUARD_BACK
    lay.update(ldc=ldc, c_base=GUARD_FRONT * ldc, c_size=rows * ldc, ldaux=ldaux, aux_base=GUARD_FRONT * ldaux + cs["aux_off"],
               aux_size=rows * ldaux + 8)
    if cs["batch"]:
        lay.update(c_strides=(M * ldc, N), aux_strides=(M * ldaux, N))
    if cs["aux_is_c"]:
        assert cs["ldaux_x"] == 0 and cs["aux_off"] == 0 and cs["epi"] in READS_AUX
    return lay


def _index(base, s0, s1, ld, Z0, Z1, M, N):
    ar = torch.arange
    return (base + ar(Z0)[:, None, None, None] * s0 + ar(Z1)[None, :, None, None] * s1 + ar(M)[None, None, :, None] * ld +
            ar(N)[None, None, None, :])


def gemm_kwargs(cs, lay):
    """The keyword arguments of ops.Gemm that are plain numbers."""
    kw = dict(lda=lay["lda"], ldb=lay["ldb"], ldc=lay["ldc"], transA=cs["ta"], transB=cs["tb"], batch=lay["Z0"] * lay["Z1"],
              batch_inner=lay["Z1"], a_strides=lay["a_strides"], b_strides=lay["b_strides"], c_strides=lay["c_strides"],
              a_seg=lay["a_seg"], epilogue=EPI[cs["epi"]], bias_stride1=lay["bias_stride1"], alpha=cs["alpha"],
              split_k=cs["split"], accumulate=cs["accumulate"])
    if cs["epi"] in READS_AUX + WRITES_AUX:
        kw.update(ldaux=lay["ldaux"], aux_strides=lay["aux_strides"])
    if cs["n_ext_from"] is not None:
        kw.update(n_ext_from=cs["n_ext_from"])
    return kw


# ------------------------------------------------------------------------------------------------ operands, references
def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def dgelu64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def gelu_E(x, deriv):
    """Error of torch's CPU f32 gelu (deriv: of its autograd) against float64 on x, over max(1, |x|), maximised."""
    x32 = x.to(torch.float32)
    assert torch.equal(x32.to(F64), x), "the pre-activation must be exact in f32"
    if deriv:
        x32 = x32.clone().requires_grad_(True)
        torch.nn.functional.gelu(x32).sum().backward()
        got, ref = x32.grad.to(F64), dgelu64(x)
    else:
        got, ref = torch.nn.functional.gelu(x32).to(F64), gelu64(x)
    return float(((got - ref).abs() / x.abs().clamp_min(1.0)).max())


def erf_poly_f32(x):
    """f32 restatement of erf_fast (csrc/common.h): Abramowitz & Stegun 7.1.26 in Horner form on 1 / (1 + p |x|)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    ax = x.abs()
    t = 1.0 / (f(0.3275911) * ax + 1.0)
    poly = f(1.061405429) * t + f(-1.453152027)
    for cst in (1.421413741, -0.284496736, 0.254829592):
        poly = poly * t + f(cst)
    return torch.copysign(1.0 - poly * t * torch.exp(-ax * ax), x)


def gelu_poly_f32(x):
    return 0.5 * x * (1.0 + erf_poly_f32(x * torch.tensor(0.70710678118654752, dtype=torch.float32)))


def dgelu_poly_f32(x):
    cdf = 0.5 * (1.0 + erf_poly_f32(x * torch.tensor(0.70710678118654752, dtype=torch.float32)))
    return cdf + x * (torch.tensor(0.39894228040143268, dtype=torch.float32) * torch.exp(-0.5 * x * x))


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64)


def _operand_key(cs):
    return tuple((k, cs[k]) for k in sorted(cs) if k not in ("name", "fam", "tune", "group"))


def problem(cs):
    """Host tensors of a case (cached per operand set, so the families forced on the same operands share them; treat as
    read-only): flat buffers a / b / bias / rs / cs in their device dtypes, prefilled c0 (and aux0), the float64
    references ref_c / ref_aux [Z0, Z1, M, N] with their bounds (None: exact class) and the index tensors."""
    return _problem(_operand_key(cs))


@functools.lru_cache(maxsize=2)
def _problem(key):
    cs = dict(key)
    lay = layout(cs)
    cs["name"] = "%dx%dx%d/%s>%s/%s/%s" % (cs["M"], cs["N"], cs["K"], cs["ab"], cs["c"], cs["cls"], cs["epi"])
    M, N, K, cls, epi, alpha = cs["M"], cs["N"], cs["K"], cs["cls"], cs["epi"], cs["alpha"]
    Z0, Z1 = lay["Z0"], lay["Z1"]
    ab, cdt = DT[cs["ab"]], DT[cs["c"]]
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K * 17 + EPI[epi] + 131 * sum(map(ord, cls + cs["ab"])))
    shape_a, shape_b, shape_c = (Z0, Z1, M, K), (Z1, N, K), (Z0, Z1, M, N)
    unit = 1.0                                       # finest grid of the exact-class values
    p = {"lay": lay}
    # ---- A and B
    if cls == "real":
        draw = lambda shape: (torch.randn(shape, generator=g, dtype=F64) * 0.5).to(ab).to(F64)
        sa = sb = 1.0
    elif cls == "gelu":
        draw, sa, sb = None, 1.0, 1.0
        lim_a, lim_b = 7, 3
    elif cs["ab"] == "f32":
        draw, sa, sb = None, 1.0, 1.0
        lim_a, lim_b = 31, 15
    else:
        draw, sa, sb = None, 2.0 ** -5, 2.0 ** -2
        lim_a, lim_b = 127, 15
        unit = sa * sb
    if cs["conv"]:
        Bn, Lo, Cin, k, st = cs["conv"]
        x = draw((lay["a_size"],)) if draw else _ints(g, (lay["a_size"],), lim_a) * sa
        a_idx = _index(0, 0, 0, 1, 1, 1, 1, K) + ((torch.arange(M) // Lo) * lay["a_seg"][1] +
                                                   (torch.arange(M) % Lo) * lay["lda"])[None, None, :, None]
        a_buf, A = x.clone(), x[a_idx]
        p["conv_x"] = x.view(Bn, lay["conv_L"], Cin)
    else:
        A = draw(shape_a) if draw else _ints(g, shape_a, lim_a) * sa
        if cs["ta"]:
            a_idx = torch.arange(K)[None, None, None, :] * lay["lda"] + torch.arange(M)[None, None, :, None]
        else:
            a_idx = _index(0, lay["a_strides"][0], lay["a_strides"][1], lay["lda"], Z0, Z1, M, K)
        a_buf = torch.full((lay["a_size"],), float("nan"), dtype=F64)
        a_buf[a_idx] = A
    Bm = draw(shape_b) if draw else _ints(g, shape_b, lim_b) * sb
    if cs["tb"]:
        b_idx = torch.arange(K)[None, None, :] * lay["ldb"] + torch.arange(N)[None, :, None]
    else:
        b_idx = (torch.arange(Z1)[:, None, None] * lay["b_strides"][1] + torch.arange(N)[None, :, None] * lay["ldb"] +
                 torch.arange(K)[None, None, :])
    b_buf = torch.full((lay["b_size"],), float("nan"), dtype=F64)
    b_buf[b_idx] = Bm
    Beff = Bm
    if cs["n_ext_from"] is not None:                 # residual plane: integers on the same grid, behind the hi plane
        lo = (draw(shape_b) * 2.0 ** -8).to(ab).to(F64) if draw else _ints(g, shape_b, 3) * sb
        b_buf[b_idx + lay["b_lo_off"]] = lo
        Beff = Bm.clone()
        Beff[:, cs["n_ext_from"]:] += lo[:, cs["n_ext_from"]:]
        p["b_hi"], p["b_lo"] = Bm, lo
        Sabs = A.abs() @ Bm.abs().transpose(1, 2)
        Sabs[..., cs["n_ext_from"]:] += (A.abs() @ lo.abs().transpose(1, 2))[..., cs["n_ext_from"]:]
        P = A @ Bm.transpose(1, 2)
        P[..., cs["n_ext_from"]:] += (A @ lo.transpose(1, 2))[..., cs["n_ext_from"]:]
    else:
        Sabs = A.abs() @ Bm.abs().transpose(1, 2)    # [Z0, Z1, M, N]
        P = A @ Bm.transpose(1, 2)
    if cs["conv"]:                                   # the reference of the implicit convolution is conv1d itself
        Bn, Lo, Cin, k, st = cs["conv"]
        W = Bm[0].view(N, k, Cin).permute(0, 2, 1)
        P = torch.nn.functional.conv1d(p["conv_x"].transpose(1, 2), W, stride=st).transpose(1, 2).reshape(1, 1, M, N)
    P, S = P * alpha, Sabs * abs(alpha)
    p.update(A=A, B=Beff, a=a_buf.to(ab), b=b_buf.to(ab))
    assert torch.equal(p["a"].to(F64)[a_idx], A) and torch.equal(p["b"].to(F64)[b_idx], Bm), "operands exact in their type"
    # ---- epilogue operands
    bias = aux = rs = csc = None
    if epi in ("bias", "bias_gelu", "bias_gelu_grad"):
        bias = (torch.randn((Z1, N), generator=g, dtype=F64).float().to(F64) if cls == "real" else
                _ints(g, (Z1, N), 8) * (0.25 if cls == "gelu" else 1.0))
    if epi in READS_AUX:
        if cls == "real":
            aux = torch.randn(shape_c, generator=g, dtype=F64).to(cdt).to(F64)
        elif epi == "gelu_bwd":
            aux = _ints(g, shape_c, 32) * 0.25
        else:
            aux = _ints(g, shape_c, 8)
    if epi == "scale_rc":
        if cls == "real":
            rs = (torch.rand((M,), generator=g, dtype=F64) + 0.5).float().to(F64)
            csc = (torch.rand((N,), generator=g, dtype=F64) + 0.5).float().to(F64)
        else:
            rs = 2.0 ** torch.randint(-1, 3, (M,), generator=g).to(F64)
            csc = 2.0 ** torch.randint(-1, 3, (N,), generator=g).to(F64)
    c_init = None
    accum = cs["accumulate"] or cs["split"] > 1          # split-K adds its partial sums into what C holds
    if accum:
        c_init = torch.randn(shape_c, generator=g, dtype=F64).float().to(F64) if cls == "real" else _ints(g, shape_c, 8)
    # ---- reference, magnitude, bound
    ref_aux = bound_aux = None
    nterms = K
    bb = None if bias is None else bias[None, :, None, :]
    if epi == "none":
        ref = P
    elif epi == "bias":
        ref, S = P + bb, S + bb.abs()
    elif epi == "add":
        ref, S = P + aux, S + aux.abs()
    elif epi == "mul":
        ref, S, nterms = P * aux, S * aux.abs(), K + 2
    elif epi == "scale_rc":
        sc = rs[:, None] * csc[None, :]
        ref, S, nterms = P * sc, S * sc, K + 2
    u, ua = U_OUT[cs["c"]], U_ABS[cs["c"]]
    if epi in GELU_EPIS:
        assert cls == "gelu"
        xpre = aux if epi == "gelu_bwd" else P + bb
        Eg, Ed = gelu_E(xpre, False), gelu_E(xpre, True)
        p["gelu_E"] = (Eg, Ed)
        mx = xpre.abs().clamp_min(1.0)
        if epi == "gelu_bwd":
            ref = P * dgelu64(xpre)
            bound = P.abs() * (GELU_POLY_HALF + 2 * Ed) * mx + (EPS32 + u) * ref.abs() + ua
        else:
            ref = gelu64(xpre)
            bound = (GELU_POLY_HALF + 2 * Eg) * mx + u * ref.abs() + ua
            if epi == "bias_gelu":
                ref_aux, bound_aux = xpre, u * xpre.abs() + ua
            else:
                ref_aux = dgelu64(xpre)
                bound_aux = (GELU_POLY_HALF + 2 * Ed) * mx + u * ref_aux.abs() + ua
        assert float((S + (0 if bb is None else bb.abs())).max()) / (unit * abs(alpha) * 0.25) < 2 ** 24
    else:
        if c_init is not None:
            ref, S, nterms = ref + c_init, S + c_init.abs(), nterms + 1
        if cls == "exact":
            # every partial sum, in any order, is an integer multiple of the grid below 2^24 of it: exact in f32
            grid = unit * min(1.0, abs(alpha)) * (0.5 if epi == "scale_rc" else 1.0) ** 2
            assert float(Sabs.max()) * max(1.0, abs(alpha)) / unit < 2 ** 24, cs["name"]
            assert float(S.max()) / grid < 2 ** 24 and float(ref.abs().max()) / grid < 2 ** 24, cs["name"]
            assert cs["c"] != "f16" or float(ref.abs().max()) < 60000.0, "inside the fp16 range"
            bound = None
        else:
            bound = nterms * EPS32 * S + u * ref.abs() + ua
    p.update(ref_c=ref, bound_c=bound, ref_aux=ref_aux, bound_aux=bound_aux, S=S)
    # ---- buffers of C and aux, prefilled
    c_idx = _index(lay["c_base"], lay["c_strides"][0], lay["c_strides"][1], lay["ldc"], Z0, Z1, M, N)
    if accum:
        c0 = _ints(g, (lay["c_size"],), 8)
        c0[c_idx] = c_init
    else:
        c0 = torch.full((lay["c_size"],), float("nan"), dtype=F64)
    if cs["aux_is_c"]:
        c0[c_idx] = aux
    p.update(c_idx=c_idx, c0=c0.to(cdt))
    if epi in READS_AUX + WRITES_AUX and not cs["aux_is_c"]:
        aux_idx = _index(lay["aux_base"], lay["aux_strides"][0], lay["aux_strides"][1], lay["ldaux"], Z0, Z1, M, N)
        aux0 = torch.full((lay["aux_size"],), float("nan"), dtype=F64)
        if epi in READS_AUX:
            aux0[aux_idx] = aux
        p.update(aux_idx=aux_idx, aux0=aux0.to(cdt))
    if bias is not None:
        bbuf = torch.full((Z1 * N + cs["bias_off"],), float("nan"), dtype=torch.float32)
        bbuf[cs["bias_off"]:] = bias.reshape(-1).float()
        p["bias"] = bbuf
    if rs is not None:
        p["rs"], p["cs"] = rs.float(), csc.float()
    p.update(aux_in=aux, bias_v=bias, c_init=c_init, rs_v=rs, cs_v=csc)
    return p


# ------------------------------------------------------------------------------------------------ judging
def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _judge_one(what, cs, after, before, idx, ref, bound, written):
    """-> (max error / bound, valid values in their dtype).  Asserts NaN-free valid elements, untouched guard cells and
    the class's element check over every element."""
    name = cs["name"]
    assert after.dtype == before.dtype and after.shape == before.shape
    guard = torch.ones(before.numel(), dtype=torch.bool)
    guard[idx.reshape(-1)] = False
    same = _bits(after)[guard] == _bits(before)[guard]
    assert bool(same.all()), f"{name}: {what}: {int((~same).sum())} guard cells changed"
    vals = after[idx]
    if not written:                                   # an aux that is only read: all of it stays as it was
        assert torch.equal(_bits(vals), _bits(before[idx])), f"{name}: {what}: a read-only operand changed"
        return 0.0, vals
    bad = torch.isnan(vals)
    assert not bool(bad.any()), f"{name}: {what}: {int(bad.sum())} NaN among the valid elements, first at {bad.nonzero()[0].tolist()}"
    if bound is None:
        want = ref.to(after.dtype)
        diff = vals != want
        assert not bool(diff.any()), (f"{name}: {what}: {int(diff.sum())} elements differ from the reference rounded once, first at "
                                      f"{diff.nonzero()[0].tolist()}: {vals[diff][0].item()} != {want[diff][0].item()}")
        return 0.0, vals
    err = (vals.to(F64) - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max())
    at = (ratio == ratio.max()).nonzero()[0].tolist()
    assert worst <= 1.0, (f"{name}: {what}: error / bound {worst:.3f} at {at}, {int((ratio > 1).sum())} elements outside "
                          f"(error {float(err[tuple(at)]):.3e}, bound {float(bound[tuple(at)]):.3e})")
    return worst, vals


def judge(cs, p, c_after, aux_after=None):
    """Check the buffers a launch left (CPU tensors, flat, the dtypes of p["c0"] / p["aux0"]) -> dict(ratio=largest error
    over bound (0 for the exact class), c=valid C [Z0, Z1, M, N], aux=valid written aux or None)."""
    r, c = _judge_one("C", cs, c_after, p["c0"], p["c_idx"], p["ref_c"], p["bound_c"], True)
    out = dict(ratio=r, c=c, aux=None)
    if "aux0" in p:
        w = cs["epi"] in WRITES_AUX
        ra, a = _judge_one("aux", cs, aux_after, p["aux0"], p["aux_idx"], p["ref_aux"], p["bound_aux"], w)
        out.update(ratio=max(r, ra), aux=a if w else None)
    if cs["n_ext_from"] is not None and cs["cls"] == "exact" and cs["epi"] == "none":
        # a column below n_ext_from never sees the residual plane; the others see hi + lo
        nf, A = cs["n_ext_from"], p["A"]
        assert torch.equal(c[..., :nf], (A @ p["b_hi"].transpose(1, 2))[..., :nf].to(c.dtype))
        assert torch.equal(c[..., nf:], (A @ (p["b_hi"] + p["b_lo"]).transpose(1, 2))[..., nf:].to(c.dtype))
    return out


def emulate_f32(cs, p):
    """What a plain f32 implementation leaves in the buffers: torch's CPU f32 matmul and f32 epilogue arithmetic, stored
    in the output type.  -> (c_after, aux_after or None).  Ties the cases to their references without a GPU."""
    f = lambda t: None if t is None else t.to(torch.float32)
    acc = f(p["A"]) @ f(p["B"]).transpose(1, 2)
    if cs["n_ext_from"] is not None:
        nf = cs["n_ext_from"]
        acc = f(p["A"]) @ f(p["b_hi"]).transpose(1, 2)
        acc[..., nf:] += (f(p["A"]) @ f(p["b_lo"]).transpose(1, 2))[..., nf:]
    v = acc * torch.tensor(cs["alpha"], dtype=torch.float32)
    epi, aux_v = cs["epi"], None
    bb = None if p["bias_v"] is None else f(p["bias_v"])[None, :, None, :]
    if epi == "bias":
        v = v + bb
    elif epi == "add":
        v = v + f(p["aux_in"])
    elif epi == "mul":
        v = v * f(p["aux_in"])
    elif epi == "scale_rc":
        v = v * (f(p["rs_v"])[:, None] * f(p["cs_v"])[None, :])
    elif epi == "gelu_bwd":
        v = v * dgelu_poly_f32(f(p["aux_in"]))
    elif epi in WRITES_AUX:
        x = v + bb
        v, aux_v = gelu_poly_f32(x), (x if epi == "bias_gelu" else dgelu_poly_f32(x))
    if p["c_init"] is not None:
        v = v + f(p["c_init"])
    c_after = p["c0"].clone()
    c_after[p["c_idx"]] = v.to(c_after.dtype)
    aux_after = None
    if "aux0" in p:
        aux_after = p["aux0"].clone()
        if aux_v is not None:
            aux_after[p["aux_idx"]] = aux_v.to(aux_after.dtype)
    return c_after, aux_after


# ------------------------------------------------------------------------------------------------ routing (script mode)
def descriptor(_lib, cs):
    """The GemmDesc of a case over made-up addresses (the route looks at pointer alignment only)."""
    lay = layout(cs)
    kw = gemm_kwargs(cs, lay)
    esz, csz = (4 if cs["ab"] == "f32" else 2), (4 if cs["c"] == "f32" else 2)
    base = 0x7F0000000000
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch, d.batch_inner = cs["M"], cs["N"], cs["K"], kw["batch"], kw["batch_inner"]
    d.dtype_ab, d.dtype_c, d.epilogue = DT_CODE[cs["ab"]], DT_CODE[cs["c"]], kw["epilogue"]
    d.A.ptr, d.A.ld, d.A.trans = base, kw["lda"], int(cs["ta"])
    d.A.seg_len, d.A.seg_stride = kw["a_seg"]
    d.A.stride0, d.A.stride1 = kw["a_strides"]
    d.B.ptr, d.B.ld, d.B.trans = base + (1 << 36), kw["ldb"], int(cs["tb"])
    d.B.stride0, d.B.stride1 = kw["b_strides"]
    d.C, d.ldc = base + (2 << 36) + lay["c_base"] * csz, kw["ldc"]
    d.c_stride0, d.c_stride1 = kw["c_strides"]
    if cs["epi"] in READS_AUX + WRITES_AUX:
        d.aux = d.C if cs["aux_is_c"] else base + (3 << 36) + lay["aux_base"] * csz
        d.ldaux = kw["ldaux"]
        d.aux_stride0, d.aux_stride1 = kw["aux_strides"]
    if cs["epi"] in ("bias", "bias_gelu", "bias_gelu_grad"):
        d.bias, d.bias_stride1 = base + (4 << 36) + cs["bias_off"] * 4, kw["bias_stride1"]
    if cs["epi"] == "scale_rc":
        d.row_scale, d.col_scale = base + (5 << 36), base + (6 << 36)
    d.alpha, d.split_k, d.accumulate = cs["alpha"], cs["split"], int(cs["accumulate"])
    if cs["n_ext_from"] is not None:
        d.k_ext, d.n_ext_from, d.b_lo_offset = cs["K"], cs["n_ext_from"], lay["b_lo_off"]
    return d


def tune_settings(cases):
    return sorted({tune_name(cs) for cs in cases})


def routed_families(tune=""):
    """[(case name, family claimed, family answered)] of the cases of one tuner setting, at the 256-CU fallback."""
    import ctypes as C
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from w2v2_speaker_amd import _lib
    lib = _lib.load()
    if tune:
        name, val = tune.split("=")
        {"kernel": lib.w2v2_tune_gemm_kernel, "f32_tile": lib.w2v2_tune_gemm_f32_tile}[name](int(val))
    return [(cs["name"], cs["fam"], lib.w2v2_gemm_kernel_of(C.byref(descriptor(_lib, cs))))
            for cs in all_cases(256) if tune_name(cs) == tune]


if __name__ == "__main__":
    print("ROUTE " + json.dumps(routed_families(os.environ.get("ROUTE_TUNE", ""))))
