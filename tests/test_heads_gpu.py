"""GPU tests of the loss-head kernels (csrc/heads.hip) called directly, and of heads.ClassifierHead, against the float64
references of tests/heads_cases.py at the branch edges: both sides of the hard-margin threshold and of the easy-margin
zero, label columns on the first / last thread and trip of the 1024-thread stride loops, arg-max ties across waves and
trips, every load path of row_invnorm, the grid-stride trip of normalize_bwd, the three-launch class-weight path and
the ragged chunk of the d(emb) products, the 64-lane / 256-thread edges of the BCE kernels.

Bounds.  f32 outputs of the row kernel: the bounds it has in test_surface_gpu.py (loss 2e-5 * max(1, |ref|), softmax
2e-6 absolute, gradients per-row rel-L2 1e-5); the f32 restatement of the kernel in tests/test_heads_cpu.py meets them on the same
inputs on the CPU (8.1e-7 / 3.6e-7 / 1.3e-6), so a miss here is the kernel's.  16-bit gradient outputs: the f32 launch rounded once (bitwise).  Head level:
the GEMM bounds of test_kernels_gpu._gemm_case (2e-5 rel-L2 in f32, 1.2e-2 with 16-bit operands and 16-bit dcos).
Lines that start with ``heads-parity:`` are the measured figures recorded in profiles/heads_parity.txt."""
import functools

import pytest
import torch

import heads_cases as HC
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SENT = -7.0                              # exactly representable in every dtype; no kernel here produces it
LOSS_TOL, SM_ATOL, GRAD_TOL = 2e-5, 2e-6, 1e-5
GEMM_TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2, torch.float16: 1.2e-2}


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def say(what, **figures):
    print("heads-parity: " + what + ": " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}"
                                                       for k, v in figures.items()))


def row_rel_l2(got, ref):
    """max over rows of |got_r - ref_r| / |ref_r| (float64, on the CPU)."""
    got, ref = got.detach().cpu().to(F64), ref.to(F64)
    if got.dim() == 1:
        got, ref = got[:, None], ref[:, None]
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------ a. the row kernel
@functools.lru_cache(maxsize=None)
def _row_ref(mode: int, C: int):
    """(case tensors on the CPU, float64 reference at loss_scale 1): computed once, shared, never modified."""
    margin, scale, easy = HC.ROW_MODES[mode]
    cos, label, inv_x, inv_w, ldc = HC.row_case(margin, C)
    return (cos, label, inv_x, inv_w, ldc), HC.aam_rows_ref(cos[:, :C], label, margin, scale, easy, None, inv_x, inv_w)


def _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, dtype, loss_scale=None, form="aam", earlier=None):
    """One launch into sentinel-filled buffers -> dict of device tensors.  form: "aam" (everything), "ce" (dcos_w only:
    dcos_x / inv_* / rowdot / colprod None), "eval" (dcos_w None: no gradient pointer at all, or, with ``earlier`` = the
    dict of an earlier launch, that launch's dcos_x / rowdot / colprod and inv_* handed in beside the None dcos_w)."""
    o = ops()
    B = cos.shape[0]
    f = lambda *shape, dt=F32: torch.full(shape, SENT, dtype=dt, device=DEV)
    out = {"softmax": f(B, ldc), "loss_rows": f(B), "correct": f(B), "dcos_w": f(B, ldc, dt=dtype),
           "dcos_x": f(B, ldc, dt=dtype), "rowdot": f(B), "colprod": f(B, C)}
    ls = None if loss_scale is None else torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV)
    a = form == "aam" or earlier is not None
    dw = None if form == "eval" else out["dcos_w"]
    gr = out if earlier is None else earlier
    o.aam_softmax_fwd_bwd(cos.to(DEV), label.to(DEV), out["softmax"], out["loss_rows"], dw,
                          gr["dcos_x"] if a else None, inv_x.to(DEV) if a else None, inv_w.to(DEV) if a else None,
                          gr["rowdot"] if a else None, gr["colprod"] if a else None, B, C, ldc, margin, scale, ls,
                          out["correct"], easy_margin=easy)
    torch.cuda.synchronize()
    return out


def _check_rows_f32(got, ref, C, ldc, k, tag, grads=("dcos_w", "dcos_x", "colprod", "rowdot")):
    """The f32 outputs of one launch against the float64 reference (k = the loss scale the gradients carry)."""
    R = HC.N_REGULAR
    lref = ref["loss_rows"]
    lerr = float(((got["loss_rows"].cpu().to(F64) - lref).abs() / lref.abs().clamp_min(1.0)).max())
    serr = float((got["softmax"][:, :C].cpu().to(F64) - ref["softmax"]).abs().max())
    gerr = {n: row_rel_l2(got[n][:R, :C] if got[n].dim() == 2 else got[n][:R], k * ref[n][:R]) for n in grads}
    say(tag, loss=lerr, loss_bound=LOSS_TOL, softmax=serr, softmax_bound=SM_ATOL,
        **{n: e for n, e in gerr.items()}, grad_bound=GRAD_TOL)
    assert lerr < LOSS_TOL and serr < SM_ATOL
    for n, e in gerr.items():
        assert e < GRAD_TOL, (n, e)
        assert torch.isfinite(got[n].float()[R:] if got[n].dim() == 1 else got[n].float()[R:, :C]).all(), n   # cos == +-1
    assert torch.equal(got["correct"].cpu().to(F64), ref["correct"])
    assert torch.equal(got["softmax"][:, C:], torch.full_like(got["softmax"][:, C:], SENT))


@pytest.mark.parametrize("loss_scale", [None, 8.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", HC.ROW_CLASSES)
@pytest.mark.parametrize("mode", range(len(HC.ROW_MODES)))
def test_aam_rows_vs_float64(mode, C, dtype, loss_scale):
    """w2v2_aam_softmax_fwd_bwd, every output of the full form, at label cosines on both sides of cos(pi - m) and of 0.
    The f32 outputs are held to the float64 reference; the 16-bit dcos_w / dcos_x must be the f32 launch's rounded once
    (the two template instantiations run the same f32 arithmetic and differ only in from_f32<T> at the store)."""
    margin, scale, easy = HC.ROW_MODES[mode]
    (cos, label, inv_x, inv_w, ldc), ref = _row_ref(mode, C)
    k = 1.0 if loss_scale is None else loss_scale
    tag = f"rows m={margin} s={scale} easy={int(easy)} C={C} {dtype} loss_scale={loss_scale}"
    got = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, dtype, loss_scale)
    pad = torch.full((cos.shape[0], ldc - C), SENT, dtype=dtype, device=DEV)
    assert torch.equal(got["dcos_w"][:, C:], pad) and torch.equal(got["dcos_x"][:, C:], pad)
    if dtype == F32:
        _check_rows_f32(got, ref, C, ldc, k, tag)
        return
    _check_rows_f32(got, ref, C, ldc, k, tag, grads=("colprod", "rowdot"))
    got32 = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, F32, loss_scale)
    _check_rows_f32(got32, ref, C, ldc, k, tag + " (its f32 launch)")
    for n in ("dcos_w", "dcos_x"):
        assert torch.equal(got[n][:, :C], got32[n][:, :C].to(dtype)), n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", range(len(HC.ROW_MODES)))
def test_aam_rows_optional_pointer_forms(mode, dtype):
    """CE form (dcos_w only) and eval form (dcos_w None) write what the full form writes and nothing else.  The eval
    form is launched twice: with no gradient pointer at all, and with the full launch's own dcos_x / rowdot / colprod
    handed in beside the None dcos_w -- those buffers must come back as the full launch left them."""
    margin, scale, easy = HC.ROW_MODES[mode]
    C = 1025
    (cos, label, inv_x, inv_w, ldc), ref = _row_ref(mode, C)
    full = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, dtype, 8.0)
    kept = {n: t.clone() for n, t in full.items()}
    ce = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, dtype, 8.0, form="ce")
    ev = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, dtype, 8.0, form="eval")
    ev2 = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, dtype, 8.0, form="eval", earlier=full)
    for got in (ce, ev, ev2):
        for n in ("softmax", "loss_rows", "correct"):
            assert torch.equal(got[n], full[n]), n
        for n in ("dcos_x", "rowdot", "colprod"):
            assert torch.equal(got[n], torch.full_like(got[n], SENT)), n
    assert torch.equal(ev["dcos_w"], torch.full_like(ev["dcos_w"], SENT))
    assert torch.equal(ev2["dcos_w"], torch.full_like(ev2["dcos_w"], SENT))
    for n in full:                       # what the earlier launch wrote is still there (ev2 was handed these buffers)
        assert torch.equal(full[n], kept[n]), n
    assert float(full["rowdot"][:HC.N_REGULAR].abs().min()) > 0 and float(full["colprod"][:, :C].abs().max()) > 0
    # dcos_w of the CE form is g itself (no inv_w): f32 against the reference, 16 bits = the f32 launch rounded once
    R = HC.N_REGULAR
    ce32 = ce if dtype == F32 else _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, F32, 8.0, form="ce")
    err = row_rel_l2(ce32["dcos_w"][:R, :C], 8.0 * ref["g"][:R])
    say(f"rows CE form m={margin} easy={int(easy)} C={C} {dtype}", g=err, grad_bound=GRAD_TOL)
    assert err < GRAD_TOL
    assert torch.equal(ce["dcos_w"][:, :C], ce32["dcos_w"][:, :C].to(dtype))
    assert torch.equal(ce["dcos_w"][:, C:], torch.full_like(ce["dcos_w"][:, C:], SENT))


def test_aam_rows_plain_mode_ignores_scale_and_loss_scale_spares_the_loss():
    mode, C = 3, 1025
    margin, _, easy = HC.ROW_MODES[mode]
    (cos, label, inv_x, inv_w, ldc), _ = _row_ref(mode, C)
    a = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, 30.0, easy, F32)
    b = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, 1.0, easy, F32)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    for mode in range(len(HC.ROW_MODES)):
        margin, scale, easy = HC.ROW_MODES[mode]
        (cos, label, inv_x, inv_w, ldc), _ = _row_ref(mode, C)
        one = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, F32)
        eight = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, F32, 8.0)
        for n in ("loss_rows", "softmax", "correct"):
            assert torch.equal(one[n], eight[n]), n
        for n in ("dcos_w", "dcos_x", "rowdot", "colprod"):       # a power of two: exact in f32
            assert torch.equal(one[n][..., :C] * 8.0 if one[n].dim() == 2 else one[n] * 8.0, eight[n][..., :C]), n
        assert float(one["dcos_w"][:HC.N_REGULAR, :C].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 3])
def test_aam_rows_bad_labels(mode, dtype):
    """Labels -1, C and 2**40: NaN loss row, exactly zero gradient rows, correct 0; the other rows as without them."""
    margin, scale, easy = HC.ROW_MODES[mode]
    C = 1025
    (cos, label, inv_x, inv_w, ldc), _ = _row_ref(mode, C)
    lab = label.clone()
    bad = [1, 4, 7]
    lab[1], lab[4], lab[7] = -1, C, 2 ** 40
    good = [i for i in range(lab.numel()) if i not in bad]
    a = _launch_rows(cos, label, inv_x, inv_w, C, ldc, margin, scale, easy, dtype)
    b = _launch_rows(cos, lab, inv_x, inv_w, C, ldc, margin, scale, easy, dtype)
    assert torch.isnan(b["loss_rows"][bad]).all() and float(b["correct"][bad].abs().max()) == 0.0
    for n in ("dcos_w", "dcos_x", "colprod"):
        assert float(b[n][bad][:, :C].float().abs().max()) == 0.0, n
    assert float(b["rowdot"][bad].abs().max()) == 0.0
    assert torch.isfinite(b["softmax"][:, :C]).all()
    for n in a:
        assert torch.equal(a[n][good], b[n][good]), n


def test_plain_rows_with_logits_of_plus_minus_80():
    """Plain CE on a row holding +80 and -80: the loss (up to 160) stays finite and matches float64; label on a -80
    column (loss ~ 160), on the +80 column (loss ~ 0, saturated softmax) and on an ordinary one."""
    C, ldc = 1025, 1040
    label = torch.tensor([5, 700, 1024, 9], dtype=torch.int64)
    cos = HC.plant_cosines(C, ldc, label, [-80.0, 80.0, 0.25, 0.1], seed=77)
    cos[0, 300], cos[1, 12], cos[2, 0], cos[2, 1023] = 80.0, -80.0, 80.0, -80.0
    ref = HC.aam_rows_ref(cos[:, :C], label, -1.0, 30.0, False)
    got = _launch_rows(cos, label, None, None, C, ldc, -1.0, 30.0, False, F32, form="ce")
    lref = ref["loss_rows"]
    lerr = float(((got["loss_rows"].cpu().to(F64) - lref).abs() / lref.abs().clamp_min(1.0)).max())
    serr = float((got["softmax"][:, :C].cpu().to(F64) - ref["softmax"]).abs().max())
    gerr = rel_l2(got["dcos_w"][:, :C].cpu(), ref["g"])
    say("rows plain +-80", loss=lerr, loss_bound=LOSS_TOL, softmax=serr, softmax_bound=SM_ATOL, g=gerr, grad_bound=GRAD_TOL)
    assert torch.isfinite(got["loss_rows"]).all() and float(lref.max()) > 159.0
    assert lerr < LOSS_TOL and serr < SM_ATOL and gerr < GRAD_TOL
    assert torch.equal(got["correct"].cpu().to(F64), ref["correct"])


# ------------------------------------------------------------------------------------------ b. arg-max ties
def test_correct_rows_takes_the_smallest_column_holding_the_maximum():
    """Plain mode (z = cos exactly).  Equal maxima in different waves (3, 70), in one thread's two trips (3, 1027) and
    on the trip boundary (1023, 1024): label on the smaller column -> 1, on the larger -> 0, elsewhere -> 0; a strict
    maximum under the label -> 1."""
    C, ldc = 1100, 1112
    rows = []                                        # (columns holding the maximum, label, expected)
    for lo, hi in ((3, 70), (3, 1027), (1023, 1024)):
        rows += [((lo, hi), lo, 1.0), ((lo, hi), hi, 0.0), ((lo, hi), 500, 0.0)]
    rows += [((70,), 70, 1.0), ((1027,), 1027, 1.0), ((1099,), 0, 0.0)]
    label = torch.tensor([r[1] for r in rows], dtype=torch.int64)
    g = torch.Generator().manual_seed(9)
    cos = torch.full((len(rows), ldc), float("nan"))
    cos[:, :C] = torch.rand(len(rows), C, generator=g) * 1.2 - 0.6
    for i, (cols, _, _) in enumerate(rows):
        for c in cols:
            cos[i, c] = 0.75
    ref = HC.aam_rows_ref(cos[:, :C], label, -1.0, 1.0, False)
    want = torch.tensor([r[2] for r in rows], dtype=F64)
    assert torch.equal(ref["correct"], want)
    got = _launch_rows(cos, label, None, None, C, ldc, -1.0, 1.0, False, F32, form="eval")
    assert got["correct"].cpu().to(F64).tolist() == want.tolist()


# ------------------------------------------------------------------------------------------ c. row_invnorm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", HC.INVNORM_ROWS)
def test_row_invnorm_every_load_path(rows, dtype):
    """1 / max(|x|, 1e-12) against float64 of the values read.  ld == cols, ld = cols + 4 (the float4 path where
    cols % 4 == 0) and ld = cols + 1 (scalar), for f32 also a base pointer one element off 16-byte alignment (scalar);
    the padding is NaN.  A zero row gives 1 / 1e-12f.  Bound: f32 sum of at most 257 squares, rel < 1e-6."""
    o = ops()
    worst = 0.0
    for cols in HC.INVNORM_COLS:
        g = torch.Generator().manual_seed(rows * 1000 + cols)
        vals = (torch.randn(rows, cols, generator=g) * 1.5).to(dtype)
        if rows >= 4:
            vals[2] = 0
        ref = HC.invnorm_ref(vals.float())
        for pad, off in ((0, 0), (4, 0), (1, 0)) + (((0, 1), (4, 1)) if dtype == F32 else ()):
            ld = cols + pad
            buf = torch.full((rows * ld + 4,), float("nan"), dtype=dtype, device=DEV)
            x = buf[off:off + rows * ld].view(rows, ld)
            x[:, :cols] = vals.to(DEV)
            assert x.data_ptr() % 16 == (4 * off if dtype == F32 else 0)
            inv = torch.full((rows + 1,), SENT, device=DEV)
            o.row_invnorm(x, inv, rows, cols, ld)
            torch.cuda.synchronize()
            got = inv[:rows].cpu().to(F64)
            err = float(((got - ref).abs() / ref)[ref < 1e11].max()) if bool((ref < 1e11).any()) else 0.0
            worst = max(worst, err)
            assert err < 1e-6, (cols, pad, off, err)
            assert float(inv[rows]) == SENT
            if rows >= 4:
                assert float(got[2]) == float(torch.tensor(1.0) / torch.tensor(1e-12)) and abs(float(got[2]) / 1e12 - 1) < 2e-7
    say(f"row_invnorm rows={rows} {dtype}", rel=worst, bound=1e-6)


# ------------------------------------------------------------------------------------------ d. normalize_bwd
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", HC.NORMBWD_SHAPES)
def test_normalize_bwd_vs_float64(rows, cols, dtype):
    """dx (+)= inv * (g - x * inv * dot) with x in three dtypes, ldx = cols and cols + 8 (NaN padding), written and
    added to a known dx.  (4100, 257) is more than 4096 x 256 elements: every thread takes a second grid trip."""
    o = ops()
    gen = torch.Generator().manual_seed(rows + cols)
    g = torch.randn(rows, cols, generator=gen)
    xv = (torch.randn(rows, cols, generator=gen) * 2.0).to(dtype)
    inv = torch.rand(rows, generator=gen) * 1.5 + 0.25
    dot = torch.randn(rows, generator=gen)
    pre = torch.randn(rows, cols, generator=gen)
    v = HC.normalize_bwd_ref(g, xv.float(), inv, dot)
    worst = 0.0
    for ldx in (cols, cols + 8):
        x = torch.full((rows, ldx), float("nan"), dtype=dtype, device=DEV)
        x[:, :cols] = xv.to(DEV)
        for add in (False, True):
            dx = torch.empty(rows * cols + 8, device=DEV)
            dx[:rows * cols] = pre.view(-1).to(DEV)
            dx[rows * cols:] = SENT
            o.normalize_bwd(g.to(DEV), x, inv.to(DEV), dot.to(DEV), dx, rows, cols, ldx=ldx, add_to=add)
            torch.cuda.synchronize()
            err = rel_l2(dx[:rows * cols].view(rows, cols).cpu(), v + pre.double() if add else v)
            worst = max(worst, err)
            assert err < 1e-6, (ldx, add, err)
            assert torch.equal(dx[rows * cols:], torch.full_like(dx[rows * cols:], SENT))
    say(f"normalize_bwd rows={rows} cols={cols} {dtype}", rel_l2=worst, bound=1e-6)


# ------------------------------------------------------------------------------------------ e. ClassifierHead
@functools.lru_cache(maxsize=None)
def _head_ref(kind, easy, shape, dtype):
    emb, W, bias, label, _ = HC.head_case(*shape)
    return (emb, W, bias, label), HC.head_ref(kind, emb, W, bias, label, dtype, HC.HEAD_MARGIN, HC.HEAD_SCALE, easy)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,E,C", HC.HEAD_SHAPES)
@pytest.mark.parametrize("kind,easy", [("aam", False), ("aam", True), ("ce", False)])
def test_classifier_head_vs_float64_oracle(kind, easy, B, E, C, dtype):
    """One ClassifierHead step, built the way AngularAdditiveMarginSoftMaxLoss._head builds it, on planted label cosines
    (margin 0.5: rows in the hard-margin fall-back and on both sides of 0 in every dtype).  (9, 20, 300) runs the
    three-launch dW path (E % 8 != 0); (66, 64, 600) and (3, 40, 4100) the ragged last chunk of the d(emb) products.
    w_grad / bias_grad start from a known tensor: AAM overwrites it, CE adds to it; a second step shows that nothing
    else accumulates."""
    from w2v2_speaker_amd.heads import ClassifierHead
    o = ops()
    (emb, W, bias, label), ref = _head_ref(kind, easy, (B, E, C), dtype)
    aam = kind == "aam"
    wm = W.to(DEV)
    wlp = wm if dtype == F32 else torch.empty(C, E, dtype=dtype, device=DEV)
    if wlp is not wm:
        o.cast(wm, wlp)
    gen = torch.Generator().manual_seed(C)
    w0, b0 = torch.randn(C, E, generator=gen) * 0.01, torch.randn(C, generator=gen) * 0.01
    w_grad, bias_grad = w0.to(DEV), None if aam else b0.to(DEV)
    head = ClassifierHead(kind, B, E, C, w_master=wm, w_operand=wlp, w_grad=w_grad, bias=None if aam else bias.to(DEV),
                          bias_grad=bias_grad, emb=torch.empty(B, E, device=DEV), act_dtype=dtype, train=True,
                          margin=HC.HEAD_MARGIN, scale=HC.HEAD_SCALE, easy_margin=easy)
    S = len(head.g_dx)
    assert head.fused_dw == (aam and E % 8 == 0) and S == (1 if C == 300 else 2) and head.ldc == HC.roundup8(C)
    tol = GEMM_TOL[dtype]
    lab = label.to(DEV)
    for step in (1, 2):
        head.emb.copy_(emb.to(DEV))
        loss, sm = head.forward_backward(lab)
        torch.cuda.synchronize()
        figs = {"loss": abs(float(loss) - float(ref["loss"])) / abs(float(ref["loss"])),
                "softmax": rel_l2(sm.cpu(), ref["softmax"]), "demb": rel_l2(head.demb.cpu(), ref["demb"]),
                "w_grad": rel_l2(w_grad.cpu().double() - (0 if aam else w0.double()), (1 if aam else step) * ref["w_grad"])}
        if not aam:
            figs["bias_grad"] = rel_l2(bias_grad.cpu().double() - b0.double(), step * ref["bias_grad"])
        say(f"head {kind} easy={int(easy)} B={B} E={E} C={C} {dtype} step {step}", **figs, bound=tol)
        for n, e in figs.items():
            assert e < tol, (n, e, step)
        want = (sm.argmax(dim=1) == lab).float()
        assert torch.equal(head.correct, want)
        assert float(head.softmax[:, C:].abs().max() if head.ldc > C else 0.0) == 0.0


# ------------------------------------------------------------------------------------------ f. the BCE head
def _launch_bce(emb, w, b, label, loss_scale, grads=True):
    o = ops()
    B, H = emb.shape
    f = lambda *shape: torch.full(shape, SENT, device=DEV)
    out = {"prob": f(B), "loss_rows": f(B), "dlogit": f(B), "demb": f(B, H), "dw": f(H + 1), "db": f(2)}
    ls = None if loss_scale is None else torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV)
    gr = [out[n] if grads else None for n in ("dlogit", "demb", "dw", "db")]
    o.bce_head_fwd_bwd(emb.to(DEV), w.to(DEV), b.to(DEV), label.to(DEV), out["prob"], out["loss_rows"], *gr, B, H, ls)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", HC.BCE_B)
@pytest.mark.parametrize("H", HC.BCE_H)
def test_bce_head_vs_float64(H, B):
    """w2v2_bce_head_fwd_bwd against float64 binary_cross_entropy_with_logits at H around the 64-lane stride of the row
    kernel and the 256-thread blocks of the weight-gradient kernel; logits +100 / -100 on their expensive side (loss
    100) and 0; with a loss scale; with a label 2 (NaN loss row, zero gradient).  Bounds: those of the golden test
    (prob 2e-6, dlogit 1e-7 * scale, rel-L2 1e-5); loss rows as the AAM rows (2e-5 * max(1, |ref|)); db, a sum of B
    signed terms, relative to |db| like demb and dw (1e-5)."""
    emb, w, b, label = HC.bce_case(B, H)
    if B >= 5:
        label[3] = 2
    for k in (None, 8.0):
        ref = HC.bce_ref(emb, w, b, label, k)
        got = _launch_bce(emb, w, b, label, k)
        kk = 1.0 if k is None else k
        ok = ~torch.isnan(ref["loss_rows"])
        lref = ref["loss_rows"][ok]
        figs = {"prob": float((got["prob"].cpu().double() - ref["prob"]).abs().max()),
                "loss": float(((got["loss_rows"].cpu().double()[ok] - lref).abs() / lref.abs().clamp_min(1.0)).max()),
                "dlogit": float((got["dlogit"].cpu().double() - ref["dlogit"]).abs().max()),
                "demb": rel_l2(got["demb"].cpu(), ref["demb"]), "dw": rel_l2(got["dw"][:H].cpu(), ref["dw"]),
                "db": abs(float(got["db"][0]) - float(ref["db"])) / abs(float(ref["db"]))}
        say(f"bce H={H} B={B} loss_scale={k}", prob=figs["prob"], prob_bound=2e-6, loss=figs["loss"], loss_bound=LOSS_TOL,
            dlogit=figs["dlogit"], dlogit_bound=1e-7 * kk, demb=figs["demb"], dw=figs["dw"], db=figs["db"], grad_bound=1e-5)
        assert figs["prob"] < 2e-6 and figs["loss"] < LOSS_TOL and figs["dlogit"] < 1e-7 * kk
        assert figs["demb"] < 1e-5 and figs["dw"] < 1e-5 and figs["db"] < 1e-5
        assert torch.isnan(got["loss_rows"].cpu()[~ok]).all() and int((~ok).sum()) == (1 if B >= 5 else 0)
        if B >= 5:
            assert float(got["dlogit"][3]) == 0.0 and float(got["demb"][3].abs().max()) == 0.0
        if B >= 2:
            assert abs(float(ref["loss_rows"][0]) - 100.0) < 1e-3 and abs(float(ref["loss_rows"][1]) - 100.0) < 1e-3
        assert float(got["dw"][H]) == SENT and float(got["db"][1]) == SENT
        ev = _launch_bce(emb, w, b, label, k, grads=False)
        assert torch.equal(ev["prob"], got["prob"])
        assert torch.equal(ev["loss_rows"].nan_to_num(-1.0), got["loss_rows"].nan_to_num(-1.0))
        for n in ("dlogit", "demb", "dw", "db"):
            assert torch.equal(ev[n], torch.full_like(ev[n], SENT)), n


def test_bce_head_refuses_a_mixed_set_of_gradient_pointers():
    """Gradient outputs come together: a mixed None set is refused (message from w2v2_last_error) before any launch."""
    o = ops()
    emb, w, b, label = HC.bce_case(5, 65)
    f = lambda *shape: torch.full(shape, SENT, device=DEV)
    prob, rows, dl, de, dw, db = f(5), f(5), f(5), f(5, 65), f(65), f(1)
    args = (emb.to(DEV), w.to(DEV), b.to(DEV), label.to(DEV), prob, rows)
    for gr in ((dl, None, None, None), (dl, de, dw, None), (None, de, dw, db), (dl, de, None, db)):
        with pytest.raises(RuntimeError, match="gradient outputs come together"):
            o.bce_head_fwd_bwd(*args, *gr, 5, 65)
    torch.cuda.synchronize()
    for t in (prob, rows, dl, de, dw, db):
        assert torch.equal(t, torch.full_like(t, SENT))
