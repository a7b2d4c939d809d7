"""GPU tests of every w2v2_gemm kernel family (csrc/gemm*.hip) at its tile and route edges, element by element: the cases,
float64 references and bounds of tests/gemm_cases.py (exact class: bit for bit; real class: the derived f32-sum bound
per element; gelu class: the polynomial's published error plus torch's own).  Every launch goes into NaN-prefilled
buffers with guard rows and columns, asserts the kernel family it claims BEFORE it launches (a case that silently ran
elsewhere fails), then that no valid element is NaN, that every guard cell kept its bits, and the class's check over
every element of C and of a written aux.

Lines that start with ``gemm-parity:`` are the measured figures recorded in profiles/gemm_parity.txt (largest error over
bound per group, family and class; an exact-class line counts launches that were bit-equal to the reference)."""
import collections
import os

import pytest
import torch

import gemm_cases as GC

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(any(os.environ.get(e) for e in GC.SWITCHES),
                                 reason="an A/B switch of the library moves products between kernels")]
DEV = "cuda"


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_dev = {}      # the device copies of the last operand set (families forced on the same operands share them)


def _operands(cs, p):
    key = GC._operand_key(cs)
    if _dev.get("key") != key:
        _dev.clear()
        _dev.update(key=key, a=p["a"].to(DEV), b=p["b"].to(DEV), bias=None if "bias" not in p else p["bias"].to(DEV),
                    rs=None if "rs" not in p else p["rs"].to(DEV), cs=None if "cs" not in p else p["cs"].to(DEV))
    return _dev


def run(cs):
    """Launch one case and judge it -> gemm_cases.judge's dict."""
    from w2v2_speaker_amd import _lib
    o, lib = ops(), _lib.load()
    p = GC.problem(cs)
    lay, d = p["lay"], _operands(cs, p)
    kw = GC.gemm_kwargs(cs, lay)
    c = p["c0"].to(DEV)
    aux = None
    if cs["aux_is_c"]:
        kw["aux"] = c[lay["c_base"]:]
    elif "aux0" in p:
        aux = p["aux0"].to(DEV)
        kw["aux"] = aux[lay["aux_base"]:]
    if d["bias"] is not None:
        kw["bias"] = d["bias"][cs["bias_off"]:]
    if d["rs"] is not None:
        kw.update(row_scale=d["rs"], col_scale=d["cs"])
    if cs["n_ext_from"] is not None:
        kw["b_lo"] = d["b"][lay["b_lo_off"]:]
    tuner = {None: None, "kernel": lib.w2v2_tune_gemm_kernel, "f32_tile": lib.w2v2_tune_gemm_f32_tile}[cs["tune"] and cs["tune"][0]]
    old = tuner(cs["tune"][1]) if tuner else None
    try:
        gm = o.Gemm(cs["M"], cs["N"], cs["K"], d["a"], d["b"], c[lay["c_base"]:], **kw)
        assert gm.kernel_name == GC.KERNEL_OF[cs["fam"]], (cs["name"], gm.kernel_name)
        gm()
        torch.cuda.synchronize()
        if cs["fam"] == 10 and cs["tune"] and cs["tune"][1] % 100 >= 11:       # the tile height that was asked for
            assert lib.w2v2_gemm_f32_last_kernel() == (cs["tune"][1] % 100 - 10) * 10 + 2, cs["name"]
    finally:
        if tuner:
            tuner(old)
    return GC.judge(cs, p, c.cpu(), None if aux is None else aux.cpu())


def run_all(cases, twins=False, label=""):
    """Run the cases, print the parity lines, -> results by case name.  twins: the ring and the phased kernel forced on
    the same operands must agree bit for bit (the 128-row kernel too on the exact class, through the reference)."""
    worst, count, results, last = collections.defaultdict(float), collections.Counter(), {}, {}
    for cs in cases:
        r = run(cs)
        key = (cs["group"], f"{cs['ab']}>{cs['c']}", cs["fam"], cs["cls"])
        worst[key] = max(worst[key], r["ratio"])
        count[key] += 1
        results[cs["name"]] = r
        if twins and cs["tune"] and cs["tune"][0] == "kernel":
            ok = GC._operand_key(cs)
            if last.get("key") != ok:
                last = {"key": ok}
            last[cs["fam"]] = r
            if 2 in last and 4 in last:
                for what in ("c", "aux"):
                    if last[2][what] is not None:
                        assert torch.equal(GC._bits(last[2][what]), GC._bits(last[4][what])), (cs["name"], what, "ring != phased")
    for key in sorted(worst):
        group, types, fam, cls = key
        group += label
        if cls == "exact":
            print(f"gemm-parity: {group} {types} family {fam} exact: {count[key]} launches bit-equal to the reference")
        else:
            print(f"gemm-parity: {group} {types} family {fam} {cls}: {count[key]} launches, max error / bound {worst[key]:.3f}")
    return results


CTYPES = [(ab, c) for ab in GC.LP for c in (ab, "f32")]


@pytest.mark.parametrize("cls", ["exact", "real"])
@pytest.mark.parametrize("ab,c", CTYPES)
def test_gemm_lds_dma_families_over_tile_edges(ab, c, cls):
    """Families 1, 2 and 4 forced on the same operands: M over the 128- and 256-row tile edges, N over the 64-, 128- and
    256-column edges and the ragged widths, nk = 1..5.  A 16-bit C without whole lines must fall back from the phased
    kernel to the ring (the case table claims family 2 there and the launch asserts it)."""
    cases = GC.sweep_cases(ab, c, cls)
    assert {cs["fam"] for cs in cases} == {1, 2, 4}
    assert all(cs["fam"] == 2 for cs in cases if cs["tune"][1] == 4 and c != "f32" and cs["N"] % 64)
    run_all(cases, twins=True)


@pytest.mark.parametrize("ab,c", CTYPES)
def test_gemm_epilogue_kinds_on_every_lds_dma_family(ab, c):
    """Every epilogue kind at (391, 192, 192) and (257, 100, 128), with 16-byte rows of C and with an odd ldc."""
    run_all(GC.epilogue_cases(ab, c), twins=True)


@pytest.mark.parametrize("ab,c", CTYPES)
def test_gemm_descriptor_features(ab, c):
    """alpha != 1 with each epilogue, ldaux != ldc, aux == C in place, aux one element off its alignment, a bias slice
    from element 1, accumulate onto a non-zero C, split-K with the bias added once."""
    run_all(GC.feature_cases(ab, c), twins=True)


@pytest.mark.parametrize("ab,c", CTYPES)
def test_gemm_descriptor_features_register_staged(ab, c):
    """The same features on family 3 (K = 200 on the default route), K-contiguous and with A or B transposed: alpha with
    each epilogue, ldaux != ldc, aux == C, aux and bias off their alignment, accumulate onto an integer C."""
    cases = GC.feature_cases_regstage(ab, c)
    assert all(cs["fam"] == 3 and cs["tune"] is None and cs["K"] % 64 for cs in cases)
    for lay in GC.REGSTAGE_FEATURE_LAYOUTS:
        mine = [cs for cs in cases if (cs["ta"], cs["tb"]) == lay]
        assert len(mine) == len(GC.feature_options()) + (2 if c == "f32" else 0)
        assert sum(cs["accumulate"] for cs in mine) == (2 if c == "f32" else 0)
    run_all(cases, label=" register-staged")


@pytest.mark.parametrize("ab", GC.LP)
def test_gemm_128_row_kernel_with_128_column_tiles(ab):
    """Family 1 forced at a shape whose 128 x 128 tiles fill more than half of the CUs, so that the route leaves the
    128 x 64 tile every other family-1 case here takes: the instantiation the conv stack runs on."""
    n = cus()
    cases = GC.wide_cases(ab, n)
    for cs in cases:
        assert cs["fam"] == 1 and cs["N"] > 64 and -(-cs["M"] // 128) * -(-cs["N"] // 128) * 2 > n
    run_all(cases)


def test_gemm_descriptor_features_f32_lds_dma():
    cases = GC.feature_cases_f32()
    assert all(cs["fam"] == 10 for cs in cases)
    run_all(cases)


@pytest.mark.parametrize("ab,c", CTYPES)
def test_gemm_register_staged_layouts_and_k_tails(ab, c):
    run_all(GC.regstage_cases(ab, c))


@pytest.mark.parametrize("K", GC.ROUND_K)
@pytest.mark.parametrize("ab", GC.LP)
@pytest.mark.parametrize("family", [2, 4])
def test_gemm_persistent_rounds(family, ab, K):
    """More tiles than CUs: a partial second round with a ragged last M tile.  On the ring the 16-bit NONE / ADD / BIAS
    outputs leave their stores pending into the next tile (K = 192 and 256: the peeled rotation of three and four K
    steps; K = 64: the flush in one piece; K = 320: a fifth step behind the rotation) and a workgroup without a tile
    in the last round leaves the loop."""
    n = cus()
    cases = GC.round_cases(family, ab, K, n)
    M, N = GC.round_shape(family, n)
    tiles = -(-M // 256) * (N // (128 if family == 2 else 256))
    assert n < tiles < 2 * n and all(cs["fam"] == family for cs in cases)
    run_all(cases, label=f" K={K}")


@pytest.mark.parametrize("ab", GC.LP)
def test_gemm_segmented_a_on_lds_dma_families(ab):
    """The implicit convolution (a_seg) against conv1d in float64: tiles inside one segment, equal to one, across a
    segment boundary, and the ragged last tile, on families 1, 2 and 4."""
    cases = GC.conv_cases(ab)
    assert {cs["fam"] for cs in cases} == {1, 2, 4}
    run_all(cases, twins=True)


@pytest.mark.parametrize("ab", GC.LP)
def test_gemm_batched_with_group_bias_and_aux(ab):
    run_all(GC.batched_cases(ab))


@pytest.mark.parametrize("ab", GC.LP)
def test_gemm_two_term_weights_per_element(ab):
    """Integer hi and lo planes: a column below n_ext_from equals A hi^T exactly, the others A (hi + lo)^T, also where the
    double tiles are enumerated first over more than one round (gemm_cases.judge asserts both halves)."""
    run_all(GC.two_term_cases(ab, cus()))


@pytest.mark.parametrize("code", GC.F32_CODES)
def test_gemm_f32_tiles_and_layouts(code):
    """Families 9 and 10 under every tile code: the four layouts, ragged shapes, split-K 5 of K = 2000 bit for bit."""
    cases = GC.f32_cases(code)
    assert {cs["fam"] for cs in cases} == ({9} if code < 10 else {9, 10})
    run_all(cases, label=f" tile code {code}")
