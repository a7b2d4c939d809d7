"""GPU tests of the margin heads: w2v2_margin_softmax_fwd_bwd (csrc/margin_head.hip) called directly, heads.ClassifierHead
with sub-centres / the cosine margin / inter-top-k, and the plans, modules and trainers that pass the keywords through,
against the float64 references of tests/margin_head_cases.py.

Bounds: those of tests/test_heads_gpu.py.  f32 outputs of the row kernel: loss 2e-5 * max(1, |ref|), softmax 2e-6
absolute, gradients per-row rel-L2 1e-5 (the f32 restatement in tests/test_margin_head_cpu.py meets them on the same
inputs on the CPU, so a miss here is the kernel's); 16-bit gradient outputs: the f32 launch rounded once, bitwise; head
level: 2e-5 rel-L2 in f32, 1.2e-2 with 16-bit operands.  Rows whose label cosine is exactly +-1 are checked for
finiteness only.  Lines that start with ``margin-head-parity:`` are recorded in profiles/margin_head_parity.txt."""
import functools

import numpy as np
import pytest
import torch

import heads_cases as HC
import margin_head_cases as MC
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SENT = -7.0
LOSS_TOL, SM_ATOL, GRAD_TOL = 2e-5, 2e-6, 1e-5
GEMM_TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2, torch.float16: 1.2e-2}
GRADS = ("dcos_w", "dcos_x", "colprod", "rowdot")


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def say(what, **figures):
    print("margin-head-parity: " + what + ": " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}"
                                                             for k, v in figures.items()))


def row_rel_l2(got, ref):
    got, ref = got.detach().cpu().to(F64), ref.to(F64)
    if got.dim() == 1:
        got, ref = got[:, None], ref[:, None]
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------ a. the row kernel
@functools.lru_cache(maxsize=None)
def _row_ref(mode: int, C: int, K: int, n_top: int):
    """(case tensors on the CPU, float64 reference at loss_scale 1): computed once, shared, never modified."""
    mt, margin, scale, easy = MC.ROW_MODES[mode]
    cos, label, inv_x, inv_w, ld, tie = MC.row_case(margin, C, K, n_top)
    ref = MC.margin_rows_ref(cos[:, :C * K], label, C, K, mt, margin, scale, easy, n_top, MC.INTER_MARGIN, None, inv_x, inv_w)
    return (cos, label, inv_x, inv_w, ld, tie), ref


def _launch(cos, label, inv_x, inv_w, C, K, ld, mode, n_top, dtype, loss_scale=None, entry="margin"):
    """One launch into sentinel-filled buffers -> dict of device tensors (colprod: [B, C*K] in front of 8 guard floats)."""
    o = ops()
    mt, margin, scale, easy = MC.ROW_MODES[mode] if isinstance(mode, int) else mode
    B, Cn = cos.shape[0], C * K
    ldp = HC.roundup8(C) + 8 if entry == "margin" else ld
    f = lambda *shape, dt=F32: torch.full(shape, SENT, dtype=dt, device=DEV)
    out = {"softmax": f(B, ldp), "loss_rows": f(B), "correct": f(B), "dcos_w": f(B, ld, dt=dtype),
           "dcos_x": f(B, ld, dt=dtype), "rowdot": f(B), "colprod_raw": f(B * Cn + 8)}
    out["colprod"] = out["colprod_raw"][:B * Cn].view(B, Cn)
    ls = None if loss_scale is None else torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV)
    args = (cos.to(DEV), label.to(DEV), out["softmax"], out["loss_rows"], out["dcos_w"], out["dcos_x"], inv_x.to(DEV),
            inv_w.to(DEV), out["rowdot"], out["colprod"], B, C)
    if entry == "margin":
        o.margin_softmax_fwd_bwd(*args, K, ld, ldp, margin, scale, ls, out["correct"], easy_margin=easy, margin_type=mt,
                                 n_top=n_top, inter_margin=MC.INTER_MARGIN)
    else:
        o.aam_softmax_fwd_bwd(*args, ld, margin, scale, ls, out["correct"], easy_margin=easy)
    torch.cuda.synchronize()
    return out


def _check_guards(got, C, K, dtype):
    """Nothing outside [C*K) / [C) is written."""
    Cn = C * K
    for n in ("dcos_w", "dcos_x"):
        assert torch.equal(got[n][:, Cn:], torch.full_like(got[n][:, Cn:], SENT)), n
    assert got["softmax"].shape[1] > C and torch.equal(got["softmax"][:, C:], torch.full_like(got["softmax"][:, C:], SENT))
    assert torch.equal(got["colprod_raw"][-8:], torch.full_like(got["colprod_raw"][-8:], SENT))


def _check_f32(got, ref, C, K, k, tag, tie, grads=GRADS):
    """The f32 outputs of one launch against the float64 reference (k = the loss scale the gradients carry)."""
    R, Cn = MC.N_REGULAR, C * K
    lref = ref["loss_rows"]
    lerr = float(((got["loss_rows"].cpu().to(F64) - lref).abs() / lref.abs().clamp_min(1.0)).max())
    serr = float((got["softmax"][:, :C].cpu().to(F64) - ref["softmax"]).abs().max())
    gerr = {n: row_rel_l2(got[n][:R, :Cn] if got[n].dim() == 2 else got[n][:R], k * ref[n][:R]) for n in grads}
    say(tag, loss=lerr, loss_bound=LOSS_TOL, softmax=serr, softmax_bound=SM_ATOL, **gerr, grad_bound=GRAD_TOL)
    assert lerr < LOSS_TOL and serr < SM_ATOL
    for n, e in gerr.items():
        assert e < GRAD_TOL, (n, e)
        assert torch.isfinite(got[n].float()[R:] if got[n].dim() == 1 else got[n].float()[R:, :Cn]).all(), n   # cos == +-1
    assert torch.equal(got["correct"].cpu().to(F64), ref["correct"])
    # the gradient of a class sits on its first winning sub-centre; every other column holds an exact zero
    lose = ~MC.winner_mask(ref["kstar"], K)
    for n in grads:
        if got[n].dim() == 2:
            v = got[n][:, :Cn].float().cpu()
            assert float(v[lose].abs().max() if K > 1 else 0.0) == 0.0, n
            if n != "colprod":                   # (g * cos is zero on a label cosine of exactly 0)
                assert int((v[:R][~lose[:R]] != 0).sum()) == R * C, n
    if tie is not None and "colprod" in grads:
        # rank n_top was a tie of two classes: the smaller index carries the penalty (its own entry, to 1e-4), the
        # larger does not
        for c in tie:
            col = c * K + int(ref["kstar"][MC.TIE_ROW, c])
            a, b = float(got["colprod"][MC.TIE_ROW, col]), k * float(ref["colprod"][MC.TIE_ROW, col])
            assert abs(a - b) <= 1e-4 * abs(b), (c, a, b)
        assert bool(ref["sel"][MC.TIE_ROW, tie[0]]) and not bool(ref["sel"][MC.TIE_ROW, tie[1]])


@pytest.mark.parametrize("C,K", MC.ROW_SHAPES)
@pytest.mark.parametrize("mode", MC.GPU_ROW_MODES)
def test_margin_rows_vs_float64(mode, C, K):
    """Every output of the full form in f32, for every n_top and for loss_scale 1 and 1024 (a power of two: the
    gradients scale exactly, the loss, softmax and accuracy do not move)."""
    for n_top in MC.n_tops(C):
        (cos, label, inv_x, inv_w, ld, tie), ref = _row_ref(mode, C, K, n_top)
        tag = f"rows {MC.ROW_MODES[mode]} C={C} K={K} n_top={n_top}"
        one = _launch(cos, label, inv_x, inv_w, C, K, ld, mode, n_top, F32)
        _check_guards(one, C, K, F32)
        _check_f32(one, ref, C, K, 1.0, tag, tie)
        big = _launch(cos, label, inv_x, inv_w, C, K, ld, mode, n_top, F32, 1024.0)
        _check_guards(big, C, K, F32)
        for n in ("loss_rows", "softmax", "correct"):
            assert torch.equal(one[n], big[n]), n
        for n in GRADS:
            assert torch.equal(one[n] * 1024.0 if n == "rowdot" else one[n][:, :C * K] * 1024.0,
                               big[n] if n == "rowdot" else big[n][:, :C * K]), n


@pytest.mark.parametrize("C,K", MC.ROW_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES[1:])
def test_margin_rows_16_bit_outputs_are_the_f32_launch_rounded_once(dtype, C, K):
    for mode in MC.GPU_ROW_MODES:
        for n_top in MC.n_tops(C):
            (cos, label, inv_x, inv_w, ld, tie), ref = _row_ref(mode, C, K, n_top)
            got = _launch(cos, label, inv_x, inv_w, C, K, ld, mode, n_top, dtype, 1024.0)
            got32 = _launch(cos, label, inv_x, inv_w, C, K, ld, mode, n_top, F32, 1024.0)
            _check_guards(got, C, K, dtype)
            _check_f32(got, ref, C, K, 1024.0, f"rows {MC.ROW_MODES[mode]} C={C} K={K} n_top={n_top} {dtype}", tie,
                       grads=("colprod", "rowdot"))
            for n in ("dcos_w", "dcos_x"):
                assert torch.equal(got[n][:, :C * K], got32[n][:, :C * K].to(dtype)), n
            for n in ("softmax", "loss_rows", "correct", "colprod", "rowdot"):
                assert torch.equal(got[n], got32[n]), n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MC.GPU_ROW_MODES)
def test_margin_rows_one_label_out_of_range(mode, dtype):
    """A label of C: NaN loss row, exactly zero gradient row, correct 0; the other rows as without it."""
    C, K, n_top = 700, 3, 5
    (cos, label, inv_x, inv_w, ld, _), _ = _row_ref(mode, C, K, n_top)
    lab = label.clone()
    lab[5] = C
    good = [i for i in range(lab.numel()) if i != 5]
    a = _launch(cos, label, inv_x, inv_w, C, K, ld, mode, n_top, dtype)
    b = _launch(cos, lab, inv_x, inv_w, C, K, ld, mode, n_top, dtype)
    _check_guards(b, C, K, dtype)
    assert bool(torch.isnan(b["loss_rows"][5])) and float(b["correct"][5]) == 0.0 and float(b["rowdot"][5]) == 0.0
    for n in ("dcos_w", "dcos_x", "colprod"):
        assert float(b[n][5, :C * K].float().abs().max()) == 0.0, n
    assert torch.isfinite(b["softmax"][:, :C]).all()
    for n in ("softmax", "loss_rows", "correct") + GRADS:
        assert torch.equal(a[n][good], b[n][good]), n


def test_margin_rows_optional_pointers():
    """The evaluation form (no gradient pointer) writes the loss, softmax and accuracy of the full form and nothing else."""
    o = ops()
    C, K, n_top, mode = 700, 3, 5, 3
    (cos, label, inv_x, inv_w, ld, _), _ = _row_ref(mode, C, K, n_top)
    mt, margin, scale, easy = MC.ROW_MODES[mode]
    full = _launch(cos, label, inv_x, inv_w, C, K, ld, mode, n_top, F32)
    B, ldp = cos.shape[0], HC.roundup8(C) + 8
    sm, rows, corr = (torch.full(s, SENT, device=DEV) for s in ((B, ldp), (B,), (B,)))
    o.margin_softmax_fwd_bwd(cos.to(DEV), label.to(DEV), sm, rows, None, None, inv_x.to(DEV), inv_w.to(DEV), None, None, B,
                             C, K, ld, ldp, margin, scale, None, corr, margin_type=mt, n_top=n_top,
                             inter_margin=MC.INTER_MARGIN)
    torch.cuda.synchronize()
    assert torch.equal(sm, full["softmax"]) and torch.equal(rows, full["loss_rows"]) and torch.equal(corr, full["correct"])


# ------------------------------------------------------------------------------------------ b. the bitwise anchor
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", HC.ROW_CLASSES)
def test_one_centre_no_topk_arc_has_the_bits_of_the_aam_entry(C, dtype):
    """K = 1, n_top = 0, ARC: every output of the new entry equals w2v2_aam_softmax_fwd_bwd's bit for bit, on
    heads_cases.row_case for every angular mode."""
    for margin, scale, easy in HC.ROW_MODES:
        if margin < 0:
            continue
        cos, label, inv_x, inv_w, ldc = HC.row_case(margin, C)
        mode = ("arc", margin, scale, easy)
        new = _launch(cos, label, inv_x, inv_w, C, 1, ldc, mode, 0, dtype, 8.0)
        old = _launch(cos, label, inv_x, inv_w, C, 1, ldc, mode, 0, dtype, 8.0, entry="aam")
        for n in ("loss_rows", "correct", "rowdot", "colprod", "dcos_w", "dcos_x"):
            assert torch.equal(new[n], old[n]), (n, margin, easy)
        assert torch.equal(new["softmax"][:, :C], old["softmax"][:, :C])
        assert float(new["dcos_w"][:HC.N_REGULAR, :C].float().abs().max()) > 0


# ------------------------------------------------------------------------------------------ c. ClassifierHead
@functools.lru_cache(maxsize=None)
def _head_ref(shape, hmode, dtype):
    B, E, C, K = shape
    mt, easy, n_top = MC.HEAD_MODES[hmode]
    emb, W, label = MC.head_case(B, E, C, K)
    return (emb, W, label), MC.head_ref(emb, W, label, dtype, C, K, mt, MC.HEAD_MARGIN, MC.HEAD_SCALE, easy, n_top)


def _make_head(W, B, E, C, K, dtype, mt, easy, n_top, w_grad, margin=MC.HEAD_MARGIN):
    from w2v2_speaker_amd.heads import ClassifierHead
    o = ops()
    wm = W.to(DEV)
    wlp = wm if dtype == F32 else torch.empty(C * K, E, dtype=dtype, device=DEV)
    if wlp is not wm:
        o.cast(wm, wlp)
    return ClassifierHead("aam", B, E, C, w_master=wm, w_operand=wlp, w_grad=w_grad, emb=torch.empty(B, E, device=DEV),
                          act_dtype=dtype, train=True, margin=margin, scale=MC.HEAD_SCALE, easy_margin=easy,
                          sub_centers=K, margin_type=mt, inter_topk=n_top, inter_margin=MC.INTER_MARGIN)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,E,C,K", MC.HEAD_SHAPES)
@pytest.mark.parametrize("hmode", range(len(MC.HEAD_MODES)))
def test_margin_head_vs_float64_autograd(hmode, B, E, C, K, dtype):
    """One ClassifierHead step with sub-centres against float64 autograd from the embeddings, twice in a row (w_grad
    starts from a known tensor and is overwritten; nothing else accumulates).  The weight rows of sub-centres that win in
    no row of the batch carry only the F.normalize term of a zero gradient: exactly 0."""
    mt, easy, n_top = MC.HEAD_MODES[hmode]
    (emb, W, label), ref = _head_ref((B, E, C, K), hmode, dtype)
    gen = torch.Generator().manual_seed(C)
    w_grad = (torch.randn(C * K, E, generator=gen) * 0.01).to(DEV)
    head = _make_head(W, B, E, C, K, dtype, mt, easy, n_top, w_grad)
    assert head.margin_head and head.C == C and head.Cn == C * K and head.ldc == HC.roundup8(C * K)
    assert head.softmax.shape == (B, HC.roundup8(C)) and head.fused_dw == (E % 8 == 0)
    assert len(head.g_dx) == (2 if C * K >= 512 else 1)
    tol = GEMM_TOL[dtype]
    lab = label.to(DEV)
    never = ref["never"]
    for step in (1, 2):
        head.emb.copy_(emb.to(DEV))
        loss, sm = head.forward_backward(lab)
        torch.cuda.synchronize()
        assert sm.shape == (B, C)
        figs = {"loss": abs(float(loss) - float(ref["loss"])) / abs(float(ref["loss"])),
                "softmax": rel_l2(sm.cpu(), ref["softmax"]), "demb": rel_l2(head.demb.cpu(), ref["demb"]),
                "w_grad": rel_l2(w_grad.cpu(), ref["w_grad"])}
        say(f"head {mt} easy={int(easy)} n_top={n_top} B={B} E={E} C={C} K={K} {dtype} step {step}", **figs, bound=tol,
            never_winning_rows=int(never.sum()))
        for n, e in figs.items():
            assert e < tol, (n, e, step)
        assert int(never.sum()) > 0 or B > 20            # (66 rows: nearly every sub-centre wins somewhere)
        assert float(w_grad.cpu()[never].abs().max() if bool(never.any()) else 0.0) == 0.0
        assert float(ref["w_grad"][never].abs().max() if bool(never.any()) else 0.0) == 0.0
        assert torch.equal(head.correct, (sm.argmax(dim=1) == lab).float())


# ------------------------------------------------------------------------------------------ d. the default head
def _spy(monkeypatch):
    o = ops()
    calls = []
    for name in ("cast", "row_invnorm", "zero_ranges", "aam_softmax_fwd_bwd", "margin_softmax_fwd_bwd", "mean", "colsum",
                 "normalize_bwd", "aam_dw"):
        real = getattr(o, name)
        monkeypatch.setattr(o, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(real, name))
    return calls


def test_default_head_issues_the_calls_it_always_issued(monkeypatch):
    """A ClassifierHead built with the four keywords at their defaults (given or not) calls w2v2_aam_softmax_fwd_bwd in
    the sequence the head has always had and never the new entry; any non-default keyword swaps exactly that one call."""
    from w2v2_speaker_amd.heads import ClassifierHead
    B, E, C = 9, 24, 300
    emb, W, _, label, _ = HC.head_case(B, E, C)
    want = ["row_invnorm", "row_invnorm", "zero_ranges", "aam_softmax_fwd_bwd", "mean", "colsum", "normalize_bwd", "aam_dw"]
    out = []
    for kw in ({}, dict(sub_centers=1, margin_type="arc", inter_topk=0, inter_margin=0.3)):
        wm = W.to(DEV)
        head = ClassifierHead("aam", B, E, C, w_master=wm, w_operand=wm, w_grad=torch.zeros(C, E, device=DEV),
                              emb=emb.to(DEV), act_dtype=F32, train=True, margin=0.2, scale=30.0, **kw)
        assert not head.margin_head and head.softmax.shape == (B, head.ldc) and head.Cn == C
        calls = _spy(monkeypatch)
        loss, _ = head.forward_backward(label.to(DEV))
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert calls == want, calls
        out.append((float(loss), head.w_grad.clone(), head.demb.clone()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    wm = W.to(DEV)
    head = ClassifierHead("aam", B, E, C, w_master=wm, w_operand=wm, w_grad=torch.zeros(C, E, device=DEV), emb=emb.to(DEV),
                          act_dtype=F32, train=True, margin=0.2, scale=30.0, margin_type="cos")
    calls = _spy(monkeypatch)
    head.forward_backward(label.to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls == [c if c != "aam_softmax_fwd_bwd" else "margin_softmax_fwd_bwd" for c in want]
    with pytest.raises(ValueError):
        ClassifierHead("ce", B, E, C, w_master=wm, w_operand=wm, w_grad=None, bias=torch.zeros(C, device=DEV),
                       emb=emb.to(DEV), act_dtype=F32, train=False, sub_centers=2)


# ------------------------------------------------------------------------------------------ e. plans and modules
MARGIN_KW = dict(margin_type="cos", inter_topk=2, inter_margin=0.06)


def _standalone(plan_head, W0, emb, label):
    """A stand-alone ClassifierHead of the plan head's shape and keywords on the plan's embedding and the weights the
    step started from -> (loss, w_grad)."""
    h = plan_head
    w_grad = torch.full_like(W0, SENT)
    head = _make_head(W0.cpu(), h.B, h.E, h.C, h.K, F32, h.margin_type, h.easy_margin, h.inter_topk, w_grad, margin=h.margin)
    head.scale, head.inter_margin = h.scale, h.inter_margin
    head.emb.copy_(emb)
    loss, _ = head.forward_backward(label)
    torch.cuda.synchronize()
    return loss, w_grad


def test_wav2vec2_plan_trains_with_a_margin_head():
    from oracle import w2v2_oracle as O
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    cfg = W2V2Config.tiny()
    reg = Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                       hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)
    st = ParamStore(cfg, DEV, F32, head="aam", num_speakers=10, sub_centers=2)
    st.init_weights(11)
    with pytest.raises(ValueError, match="sub_centers"):
        Plan(st, 2, 4000, train=True, reg=reg, sub_centers=3)
    plan = Plan(st, 2, 4000, train=True, reg=reg, sub_centers=2, **MARGIN_KW)
    h = plan.head
    assert h.margin_head and (h.C, h.K, h.Cn, h.margin_type, h.inter_topk) == (10, 2, 20, "cos", 2)
    wav, label = O.synth_batch(2, 4000, 10, seed=5)
    W0, p0 = st.p("loss_fn.fc_weights").clone(), st.flat.clone()
    tr = SpeakerTrainer(st, plan, Constant(1e-3))
    loss, sm = tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=())
    torch.cuda.synchronize()
    assert sm.shape == (2, 10) and np.isfinite(float(loss))
    loss2, w_grad = _standalone(h, W0, plan.emb, label.to(DEV))
    assert float(loss) == float(loss2) and torch.equal(st.g("loss_fn.fc_weights"), w_grad)
    assert float(w_grad.abs().max()) > 0 and not torch.equal(st.flat, p0)
    assert not torch.equal(st.p("loss_fn.fc_weights"), W0)


def test_ecapa_plan_trains_with_a_margin_head():
    from w2v2_speaker_amd.ecapa import EcapaConfig, EcapaPlan, EcapaStore, EcapaTrainer
    from w2v2_speaker_amd.optim.schedule import Constant
    cfg = EcapaConfig.tiny()
    st = EcapaStore(cfg, DEV, F32, num_speakers=7, sub_centers=2)
    st.init_weights(3)
    plan = EcapaPlan(st, 4, 40, train=True, **MARGIN_KW)
    h = plan.head
    assert h.margin_head and (h.C, h.K, h.Cn) == (7, 2, 14)
    g = torch.Generator().manual_seed(1)
    feat, label = torch.randn(4, 40, cfg.input_mel_coefficients, generator=g).to(DEV), torch.randint(0, 7, (4,), generator=g).to(DEV)
    W0, p0 = st.p("loss_fn.fc_weights").clone(), st.flat.clone()
    tr = EcapaTrainer(st, plan, Constant(1e-3))
    loss, sm = tr.train_step(feat, label)
    torch.cuda.synchronize()
    assert sm.shape == (4, 7) and np.isfinite(float(loss))
    loss2, w_grad = _standalone(h, W0, plan.emb, label)
    assert float(loss) == float(loss2) and torch.equal(st.g("loss_fn.fc_weights"), w_grad)
    assert float(w_grad.abs().max()) > 0 and not torch.equal(st.flat, p0)


def _fc_module(**kw):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    tiny = W2V2Config.tiny()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: tiny)
    mcfg = Wav2vec2FCModuleConfig(reset_weights=True, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                  hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)
    try:
        return Wav2vec2FCModule.from_config(mcfg, num_speakers=10, device=DEV, act_dtype=F32, init_seed=5, max_lr=1e-3,
                                            max_steps=20, **kw)
    finally:
        W2V2Config.from_huggingface_id = orig


def test_modules_round_trip_their_state_and_follow_the_margin_schedule():
    from oracle import w2v2_oracle as O
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTDNNModuleConfig, EcapaTdnnModule
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    from w2v2_speaker_amd.optim.schedule import MarginSchedule
    mod = _fc_module(sub_centers=2, accumulate_grad_batches=2, **MARGIN_KW)
    sd = mod.state_dict()
    E = mod.store.embed_dim
    assert sd["loss_fn.fc_weights"].shape == (20, E) and mod.store.sub_centers == 2
    other = _fc_module(sub_centers=2, **MARGIN_KW)
    other.store.p("loss_fn.fc_weights").zero_()
    other.load_state_dict(sd)
    assert torch.equal(other.store.p("loss_fn.fc_weights").cpu(), sd["loss_fn.fc_weights"])
    with pytest.raises((ValueError, RuntimeError), match="20"):
        _fc_module().load_state_dict(sd)
    with pytest.raises(ValueError):
        _fc_module(loss="ce", sub_centers=2)
    # the margin follows the OPTIMISER step: constant within a window of two micro-batches
    mod.set_margin_schedule(MarginSchedule(0.4, initial=0.1, start_step=0, end_step=2))
    wav, label = O.synth_batch(4, 4000, 10, seed=3)
    batch = SpeakerClassificationDataBatch(4, list("abcd"), wav, label).to(DEV)
    mod.train()
    mod.on_train_start()
    seen = []
    for i in range(6):
        out = mod.training_step(batch, i)
        head = mod._plan(4, 4000, True).head
        seen.append(head.margin)
        assert head.margin_head and np.isfinite(float(out["loss"])) and out["prediction"].shape == (4, 10)
    torch.cuda.synchronize()
    assert seen == pytest.approx([0.1, 0.1, 0.25, 0.25, 0.4, 0.4], abs=1e-12) and mod.schedule_step == 3
    ecfg = EcapaTDNNModuleConfig(input_mel_coefficients=16, lin_neurons=24, channels=[64, 64, 64, 64, 192],
                                 attention_channels=16, res2net_scale=4, se_channels=16)
    em = EcapaTdnnModule.from_config(ecfg, num_speakers=5, device=DEV, act_dtype=F32, sub_centers=2, **MARGIN_KW)
    em.set_margin_schedule(MarginSchedule(0.3, initial=0.3))                # large-margin fine-tuning: a constant
    assert em.store.p("loss_fn.fc_weights").shape == (10, 24)
    g = torch.Generator().manual_seed(0)
    eb = SpeakerClassificationDataBatch(6, [str(i) for i in range(6)], torch.randn(6, 40, 16, generator=g),
                                        torch.randint(0, 5, (6,), generator=g))
    out = em.training_step(eb)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"])) and out["prediction"].shape == (6, 5)
    esd = em.state_dict()
    em2 = EcapaTdnnModule.from_config(ecfg, num_speakers=5, device=DEV, act_dtype=F32, sub_centers=2, **MARGIN_KW)
    em2.load_state_dict(esd)
    assert torch.equal(em2.store.p("loss_fn.fc_weights"), em.store.p("loss_fn.fc_weights"))


def test_argument_errors_raise_on_the_host_and_launch_nothing():
    o = ops()
    C, K = 5, 3
    (cos, label, inv_x, inv_w, ld, _), _ = _row_ref(0, C, K, 1)
    B, ldp = cos.shape[0], 16
    bufs = [torch.full(s, SENT, device=DEV) for s in ((B, ldp), (B,), (B, ld), (B, ld), (B,), (B, C * K), (B,))]
    sm, rows, dw, dx, rd, cp, corr = bufs
    base = (cos.to(DEV), label.to(DEV), sm, rows, dw, dx, inv_x.to(DEV), inv_w.to(DEV), rd, cp, B)
    for c, k, stride, n_top, im in ((C, K, ld, C, 0.06), (100, 1, 104, 17, 0.06), (C, 9, 48, 0, 0.06), (C, 0, ld, 0, 0.06),
                                    (C, K, ld, 1, -0.01), (C, K, C * K - 1, 1, 0.06)):
        with pytest.raises(ValueError):
            o.margin_softmax_fwd_bwd(*base, c, k, stride, ldp, 0.2, 30.0, None, corr, n_top=n_top, inter_margin=im)
    with pytest.raises(ValueError):
        o.margin_softmax_fwd_bwd(*base, C, K, ld, ldp, 0.2, 30.0, None, corr, margin_type="sphere")
    torch.cuda.synchronize()
    for t in bufs:
        assert torch.equal(t, torch.full_like(t, SENT))
    # the C entry refuses the same arguments itself (reached around the wrapper's check)
    from w2v2_speaker_amd import _lib
    lib = _lib.load()
    p = lambda t: t.data_ptr()
    for k, n_top, im in ((9, 0, 0.06), (K, C, 0.06), (K, 17, 0.06), (K, 1, -0.01)):
        rc = lib.w2v2_margin_softmax_fwd_bwd(p(base[0]), p(base[1]), p(sm), p(rows), p(dw), p(dx), p(base[6]), p(base[7]),
                                             p(rd), p(cp), B, C, k, ld if k <= K else 48, ldp, 0.2, 30.0, 0, 0, n_top, im,
                                             None, p(corr), o.dt(dw), o.stream())
        assert rc == -1
    torch.cuda.synchronize()
    for t in bufs:
        assert torch.equal(t, torch.full_like(t, SENT))
