"""GPU tests of every entry point of csrc/conv0.hip against the float64 references of tests/conv0_cases.py, at the edges
where these kernels can go wrong: one frame, a ragged frame tile, the first frame past a 128-frame chunk / a 5-chunk
workgroup / a 640-frame window-moment block, an idle fourth wave (C = 384), a second channel pass (C = 640, 320), the
eight-wave apply variant (C = 512), waveforms with a DC component, far below eps, loud and constant.  Outputs are judged
per frame and per channel, never by one whole-tensor norm; outputs and workspaces are pre-filled so that an element left
unwritten or written out of place shows.  Every test prints its figures (``conv0-parity:`` lines, collected by
tools/conv0_parity.py into profiles/conv0_parity.txt) before it asserts.  Bounds: see conv0_cases.py."""
import math

import pytest
import torch

import conv0_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SENTINEL = -768.0                 # exact in bf16 / fp16 / f32
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def say(line: str) -> None:
    print("conv0-parity: " + line)


def host(t: torch.Tensor) -> torch.Tensor:
    torch.cuda.synchronize()
    return t.detach().float().cpu().to(F64)


class Worst:
    """The measurement closest to (or furthest past) its bound."""

    def __init__(self):
        self.ratio, self.err, self.bound, self.item = -1.0, 0.0, 0.0, ""

    def add(self, err: float, bound: float, item: str) -> None:
        if not math.isfinite(err):
            err = math.inf
        ratio = 0.0 if err == 0 else (err / bound if bound > 0 else math.inf)
        if ratio > self.ratio:
            self.ratio, self.err, self.bound, self.item = ratio, err, bound, item

    def __str__(self):
        return f"{self.err:.2e} bound {self.bound:.2e} ({self.item})"

    @property
    def ok(self) -> bool:
        return self.ratio <= 1.0


def guarded(rows: int, C: int, dtype):
    """-> (whole buffer [rows + 2, C], the [rows, C] view between one sentinel row before and one after)."""
    buf = torch.full((rows + 2, C), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[1:rows + 1]


def guards_intact(buf: torch.Tensor) -> bool:
    torch.cuda.synchronize()
    return bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 1. statistics
def _stats(entry: str, ref):
    """Run one statistics entry on a NaN-filled workspace -> (mean, rstd) [B, C] float64."""
    o = ops()
    wav, w = ref.wav.to(DEV), ref.w.to(DEV)
    N = wav.shape[1]
    work = o.conv0_workspace(K.B, N, ref.C, ref.k, ref.stride, DEV).fill_(float("nan"))
    mr = work[work.numel() - K.B * ref.C * 2:]
    fn = o.lib().w2v2_conv0_stats_mfma if entry == "mfma" else o.lib().w2v2_conv0_stats
    rc = fn(wav.data_ptr(), w.data_ptr(), work.data_ptr(), mr.data_ptr(), K.B, N, ref.C, ref.k, ref.stride, K.EPS, o.stream())
    assert rc == 0, o.lib().w2v2_last_error()
    got = host(mr).view(K.B, ref.C, 2)
    return got[..., 0], got[..., 1]


@pytest.mark.parametrize("cls", K.CLASSES)
@pytest.mark.parametrize("C", K.STATS_C)
@pytest.mark.parametrize("entry", ["f32", "mfma"])
def test_stats_vs_float64(entry, C, cls):
    """w2v2_conv0_stats (the f32 route) and w2v2_conv0_stats_mfma (k = 10: the window-moment route where C % 128 == 0, the
    f32 route otherwise): {mean, rstd} per (b, c) within 2^-22 + 8 x the error of an ideal f32 statistics pass."""
    wm, wr = Worst(), Worst()
    for L in K.STATS_L:
        ref = K.forward_ref(cls, L, C)
        bm, br = K.stats_bounds(cls, L, C)
        e_mean, e_rstd = K.stats_errors(*_stats(entry, ref), ref)
        wm.add(e_mean, bm, f"L={L}")
        wr.add(e_rstd, br, f"L={L}")
    route = "window moments" if entry == "mfma" and C % 128 == 0 else "f32 sums"
    say(f"stats {entry} entry ({route}) C={C} {cls}: |d mean| * rstd {wm}; rel |d rstd| {wr}")
    assert wm.ok and wr.ok


@pytest.mark.parametrize("C", K.SPLIT_C)
def test_split_bf16_convolution_stats_vs_float64(C):
    """k = 8, stride 4 through w2v2_conv0_stats_mfma: the statistics of the split-bf16 matrix-core convolution, at the
    bounds of test_conv0_matrix_core_path.  L = 641 is the first chunk of a second 5-chunk workgroup."""
    wm, wr = Worst(), Worst()
    for L in K.STATS_L:
        ref = K.forward_ref("unit", L, C, K.SPLIT_K, K.SPLIT_STRIDE)
        mean, rstd = _stats("mfma", ref)
        ok = bool(torch.isfinite(mean).all()) and bool(torch.isfinite(rstd).all())
        wm.add(float((mean - ref.mean).abs().max()) if ok else math.inf,
               4 * 2.0 ** -16 * float(ref.u.abs().max()) / L ** 0.5, f"L={L}")
        wr.add(float(((rstd - ref.rstd).abs() / ref.rstd).max()) if ok else math.inf, 2e-5, f"L={L}")
    say(f"stats mfma entry (split-bf16 convolution, k=8) C={C} unit: |d mean| {wm}; rel |d rstd| {wr}")
    assert wm.ok and wr.ok


# ------------------------------------------------------------------------------------------------ 2. apply
def _apply(ref, dtype):
    o = ops()
    buf, rows = guarded(K.B * ref.L, ref.C, dtype)
    out = rows.view(K.B, ref.L, ref.C)
    work = o.conv0_workspace(K.B, ref.wav.shape[1], ref.C, ref.k, ref.stride, DEV).fill_(float("nan"))
    o.conv0_groupnorm_gelu(ref.wav.to(DEV), ref.w.to(DEV), ref.gamma.to(DEV), ref.beta.to(DEV), out, work, ref.k, ref.stride)
    return buf, out, work


@pytest.mark.parametrize("cls", K.APPLY_CLASSES)
@pytest.mark.parametrize("C", K.APPLY_C)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=NAME.get)
def test_apply_vs_float64_per_frame_and_per_channel(dtype, C, cls):
    """ops.conv0_groupnorm_gelu: every frame (over its channels) and every channel (over its frames) against float64.
    One frame has var = 0: rel-L2 against gelu(beta) is unbounded for any kernel, the absolute bound applies instead."""
    wf, wc, wa = Worst(), Worst(), Worst()
    intact = True
    for L in K.APPLY_L:
        ref = K.forward_ref(cls, L, C)
        buf, out, _ = _apply(ref, dtype)
        intact = intact and guards_intact(buf)
        got = host(out)
        if K.degenerate(ref):
            q = (got - ref.out).abs() / K.degenerate_abs_bound(ref, dtype)
            wa.add(float(q.max()) if bool(torch.isfinite(q).all()) else math.inf, 1.0, f"L={L}, |error| / absolute bound")
            continue
        bf, bc = K.apply_bounds(ref, dtype)
        for dim, bound, w in ((2, bf, wf), (1, bc, wc)):
            err, _ = K.sliced_rel_l2(got, ref.out, dim)
            i = int((err / bound).argmax())
            w.add(float(err.flatten()[i]), float(bound.flatten()[i]), f"L={L}")
    say(f"apply {NAME[dtype]} C={C} {cls}: per frame {wf}; per channel {wc}; var = 0: {wa}")
    assert intact, "a sentinel row next to the output was written"
    assert wf.ok and wc.ok and wa.ok


@pytest.mark.parametrize("C", K.APPLY_C)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=NAME.get)
def test_apply_constant_waveform_is_finite(dtype, C):
    intact = finite = True
    for L in K.APPLY_L:
        buf, out, _ = _apply(K.forward_ref("const", L, C), dtype)
        intact = intact and guards_intact(buf)
        finite = finite and bool(torch.isfinite(out.float()).all())
    say(f"apply {NAME[dtype]} C={C} const: finite {finite}, sentinel rows intact {intact}")
    assert intact and finite


# ------------------------------------------------------------------------------------------------ 3. backward
def _prefill(C: int, k: int):
    """Known non-zero contents of dw / dgamma / dbeta: small dyadic values, so that (result - prefill) loses nothing."""
    i = torch.arange(C * k, dtype=torch.float32)
    return ((i % 7 - 3) * 0.25).view(C, 1, k), ((i[:C] % 5 - 2) * 0.5), ((i[:C] % 3 - 1) * 0.25)


def _bwd_once(ref, dz, work, dtype):
    o = ops()
    g0 = _prefill(ref.C, ref.k)
    dw, dg, db = (t.clone().to(DEV) for t in g0)
    sums = torch.full((K.B, ref.C, 2), 123.0, device=DEV)
    o.conv0_bwd(ref.wav.to(DEV), ref.w.to(DEV), work, ref.gamma.to(DEV), ref.beta.to(DEV), dz.to(dtype).to(DEV).contiguous(),
                sums, dw, dg, db, ref.k, ref.stride)
    return [host(t) - g.to(F64) for t, g in zip((dw, dg, db), g0)]


@pytest.mark.parametrize("cls", K.BWD_CLASSES)
@pytest.mark.parametrize("C", K.BWD_C)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=NAME.get)
def test_conv0_bwd_vs_float64(dtype, C, cls):
    """ops.conv0_bwd on the forward's own {mean, rstd}: what it ADDS to dw / dgamma / dbeta against the closed float64
    formulas on the dtype-rounded dz; `sums` arrives dirty.  Run twice: the atomics promise no bit equality, the two runs
    are held to the same bounds against each other."""
    ww, wg, wb, rw, rg, rb = (Worst() for _ in range(6))
    for L in K.BWD_L:
        ref = K.forward_ref(cls, L, C)
        _, _, work = _apply(ref, dtype)
        dz = K.bwd_dz(L, C, dtype)
        dw_ref, dg_ref, db_ref, terms, _ = K.layer0_backward(ref, dz)
        (dw1, dg1, db1), (dw2, dg2, db2) = _bwd_once(ref, dz, work, dtype), _bwd_once(ref, dz, work, dtype)
        ww.add(K.sum_scale_error(dw1[:, 0], dw_ref, terms), K.BWD_TOL, f"L={L}")
        wg.add(K.rel_l2(dg1, dg_ref), K.BWD_TOL, f"L={L}")
        wb.add(K.rel_l2(db1, db_ref), K.BWD_TOL, f"L={L}")
        rw.add(K.sum_scale_error(dw2[:, 0], dw1[:, 0], terms), K.BWD_TOL, f"L={L}")
        rg.add(K.rel_l2(dg2, dg1), K.BWD_TOL, f"L={L}")
        rb.add(K.rel_l2(db2, db1), K.BWD_TOL, f"L={L}")
    say(f"bwd {NAME[dtype]} C={C} {cls}: dw /sum|terms| {ww}; dgamma {wg}; dbeta {wb}; "
        f"second run vs first: dw {rw.err:.2e} dgamma {rg.err:.2e} dbeta {rb.err:.2e}")
    assert all(w.ok for w in (ww, wg, wb, rw, rg, rb))


# ------------------------------------------------------------------------------------------------ 4. col2im
@pytest.mark.parametrize("k,stride", K.COL2IM_KS)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=NAME.get)
def test_col2im_is_the_exact_fold(dtype, k, stride):
    """Integer-valued columns: every sum is exact in all three dtypes, so the result is the float64 fold bit for bit; the
    last input row is covered by no frame and must come back 0 out of a NaN-filled dx."""
    bad = []
    for cin in K.COL2IM_CIN:
        for lout in K.COL2IM_LOUT:
            col, lin, fold = K.col2im_case(k, stride, cin, lout)
            dx = torch.full((K.B, lin, cin), float("nan"), dtype=dtype, device=DEV)
            ops().col2im(col.to(dtype).to(DEV), dx, K.B, lin, lout, cin, k, stride)
            if not torch.equal(host(dx), fold.to(dtype).to(F64)):
                bad.append((cin, lout))
    say(f"col2im {NAME[dtype]} k={k} stride={stride}: (bit-equal) {math.inf if bad else 0} over "
        f"{len(K.COL2IM_CIN) * len(K.COL2IM_LOUT)} shapes")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5. pack / unpack
@pytest.mark.parametrize("shape", K.PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_conv_weight_and_unpack_conv_grad_bit_equal(shape):
    """(512, 512, 5) is 1.3M elements: past the 4096 x 256 threads of the grid, the grid-stride loops loop."""
    o = ops()
    co, ci, k = shape
    w = K.rnd(co, ci, k, seed=21).float()
    res = {}
    for dtype in K.DTYPES:
        out = torch.full((co, k * ci), float("nan"), dtype=dtype, device=DEV)
        o.pack_conv_weight(w.to(DEV), out)
        torch.cuda.synchronize()
        res[NAME[dtype]] = torch.equal(out.cpu(), K.pack_ref(w).to(dtype))
    gp, g0 = K.rnd(co, k, ci, seed=22).float(), K.rnd(co, ci, k, seed=23).float()
    g = g0.clone().to(DEV)
    o.unpack_conv_grad(gp.to(DEV), g)
    torch.cuda.synchronize()
    res["unpack"] = torch.equal(g.cpu(), g0 + gp.permute(0, 2, 1))
    say(f"pack_conv_weight / unpack_conv_grad {shape}: (bit-equal) " + " ".join(f"{n} {0 if ok else math.inf}" for n, ok in res.items()))
    assert all(res.values()), res


# ------------------------------------------------------------------------------------------------ 6. layer-norm family
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("C", K.LN0_C)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=NAME.get)
def test_conv0_layernorm_gelu_forward_vs_float64(dtype, C, with_bias):
    """ops.conv0_layernorm_gelu: 111 frames are no multiple of a wave's eight; every frame against float64."""
    w_ = Worst()
    intact = True
    for cls in K.LN0_CLASSES:
        ref = K.ln0_ref(cls, C, with_bias)
        buf, rows = guarded(ref.B * ref.L, C, dtype)
        out = rows.view(ref.B, ref.L, C)
        ops().conv0_layernorm_gelu(ref.wav.to(DEV), ref.w.to(DEV), None if ref.bias is None else ref.bias.to(DEV),
                                   ref.gamma.to(DEV), ref.beta.to(DEV), out, K.K, K.STRIDE, K.EPS)
        intact = intact and guards_intact(buf)
        err, _ = K.sliced_rel_l2(host(out), ref.out, 2)
        w_.add(float(err.max()), K.tol_of(dtype), cls)
    say(f"conv0_layernorm_gelu fwd {NAME[dtype]} C={C} {'bias' if with_bias else 'no bias'}: per frame {w_}")
    assert intact, "a sentinel row next to the output was written"
    assert w_.ok


# ------------------------------------------------------------------------------------------------ 7. layernorm_gelu_fwd
@pytest.mark.parametrize("H", K.LNG_H)
@pytest.mark.parametrize("M", K.LNG_M)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=NAME.get)
def test_layernorm_gelu_fwd_vs_float64(dtype, M, H):
    x, gamma, beta, ref = K.ln_gelu_case(M, H, dtype)
    buf, y = guarded(M, H, dtype)
    ops().layernorm_gelu_fwd(x.to(dtype).to(DEV), gamma.to(DEV), beta.to(DEV), y, K.EPS)
    intact = guards_intact(buf)
    err, _ = K.sliced_rel_l2(host(y), ref, 1)
    w_ = Worst()
    w_.add(float(err.max()), K.tol_of(dtype), f"M={M}")
    say(f"layernorm_gelu_fwd {NAME[dtype]} M={M} H={H}: per row {w_}")
    assert intact and w_.ok
