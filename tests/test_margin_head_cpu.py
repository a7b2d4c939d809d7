"""CPU checks of what tests/test_margin_head_gpu.py stands on: the float64 references of tests/margin_head_cases.py fall
back to the golden-tied single-centre reference, the planted inputs reach what they are meant to reach, an f32
restatement of the kernel's arithmetic meets the GPU bounds on every row case; and the host-only parts of the margin
heads: MarginSchedule, the sub-centre shapes of the parameter stores, the host-side argument rules."""
import math

import pytest
import torch

import heads_cases as HC
import margin_head_cases as MC

F32, F64 = torch.float32, torch.float64
LOSS_TOL, SM_ATOL, GRAD_TOL = 2e-5, 2e-6, 1e-5         # the bounds of tests/test_heads_gpu.py


@pytest.mark.parametrize("margin,scale,easy", [m for m in HC.ROW_MODES if m[0] >= 0])
@pytest.mark.parametrize("C", HC.ROW_CLASSES)
def test_reference_with_one_centre_and_no_topk_is_the_aam_reference(margin, scale, easy, C):
    """K = 1, n_top = 0, ARC: margin_rows_ref equals heads_cases.aam_rows_ref (which test_heads_cpu.py ties to the
    golden-pinned oracle) on that file's own cases."""
    cos, label, inv_x, inv_w, _ = HC.row_case(margin, C)
    a = HC.aam_rows_ref(cos[:, :C], label, margin, scale, easy, 8.0, inv_x, inv_w)
    b = MC.margin_rows_ref(cos[:, :C], label, C, 1, "arc", margin, scale, easy, 0, 0.06, 8.0, inv_x, inv_w)
    R = HC.N_REGULAR
    for n in ("loss_rows", "softmax", "correct"):
        assert float((a[n] - b[n]).abs().max()) < 1e-12, n
    for n in ("g", "dcos_w", "dcos_x", "rowdot", "colprod"):
        assert float((a[n][:R] - b[n][:R]).abs().max()) < 1e-12, n


def test_reference_ties_and_selection():
    """First maximum among equal sub-centres takes the whole gradient; the stable sort gives equal negatives to the
    smaller class; the label column is never selected, also when it holds the row maximum."""
    cos = torch.tensor([[0.5, 0.5, 0.1,   0.2, 0.3, 0.3,   0.9, 0.1, 0.0,   0.3, 0.0, 0.3]], dtype=F32)
    label = torch.tensor([2])
    r = MC.margin_rows_ref(cos, label, 4, 3, "arc", 0.2, 30.0, False, 2, 0.06)
    assert r["kstar"].tolist() == [[0, 1, 0, 0]]
    # m = (0.5, 0.3, 0.9, 0.3): label 2 excluded, picks = class 0 then the tie 1 / 3 -> class 1
    assert r["sel"].tolist() == [[True, True, False, False]]
    win = MC.winner_mask(r["kstar"], 3)
    assert float(r["g"][~win].abs().max()) == 0.0 and float(r["g"][win].abs().min()) > 0.0
    r1 = MC.margin_rows_ref(cos, label, 4, 3, "cos", 0.2, 30.0, False, 1, 0.06)
    assert r1["sel"].tolist() == [[True, False, False, False]]


def test_reference_penalty_raises_the_selected_logits_only():
    """psi(m) > m for the selected classes (inter_margin in (0, pi/2), |m| < cos): their softmax grows, the loss grows."""
    cos, label, _, _, _, _ = MC.row_case(0.2, 700, 3, 5)
    a = MC.margin_rows_ref(cos[:, :2100], label, 700, 3, "arc", 0.2, 30.0, False, 0)
    b = MC.margin_rows_ref(cos[:, :2100], label, 700, 3, "arc", 0.2, 30.0, False, 5)
    assert int(b["sel"].sum()) == 5 * 12 and not bool(b["sel"][torch.arange(12), label].any())
    assert bool((b["loss_rows"] > a["loss_rows"]).all())


@pytest.mark.parametrize("C,K", MC.ROW_SHAPES)
def test_planted_rows_reach_what_they_plant(C, K):
    for n_top in MC.n_tops(C):
        cos, label, inv_x, inv_w, ld, tie = MC.row_case(0.2, C, K, n_top)
        Cn = C * K
        assert cos.shape == (12, ld) and ld == HC.roundup8(Cn) + 8 and torch.isnan(cos[:, Cn:]).all()
        assert float(cos[:, :Cn].abs().max()) <= 1.0
        r = MC.margin_rows_ref(cos[:, :Cn], label, C, K, "arc", 0.2, 30.0, False, n_top, 0.06, None, inv_x, inv_w)
        ar = torch.arange(12)
        # the label's class cosine is the planted one and its winner sits on b % K (a tie: the first)
        m = cos[:, :Cn].view(12, C, K).max(2).values
        assert torch.equal(m[ar, label].double(), torch.tensor(HC.label_cosines(0.2), dtype=F64).float().double())
        want_k = [(0 if (b == 0 and K >= 2) else b % K) for b in range(MC.N_REGULAR)]
        assert r["kstar"][ar, label][:MC.N_REGULAR].tolist() == want_k
        if K >= 2:
            y0 = int(label[0])
            assert cos[0, y0 * K] == cos[0, y0 * K + 1] and float(r["g"][0, y0 * K + 1]) == 0.0
            assert float(r["g"][0, y0 * K].abs()) > 0.0
        assert sorted(set(want_k)) == list(range(K))               # every position k wins in some row
        assert not bool(r["sel"][ar, label].any()) and int(r["sel"].sum()) == 12 * n_top
        assert bool((m[1].argmax() == label[1]) and (m[2].argmax() == label[2]))      # the label holds the row maximum
        if tie is not None:
            lo, hi = tie
            assert lo < hi and m[MC.TIE_ROW, lo] == m[MC.TIE_ROW, hi]
            assert bool(r["sel"][MC.TIE_ROW, lo]) and not bool(r["sel"][MC.TIE_ROW, hi])
        else:
            assert n_top == 0 or n_top == C - 1
        for n in ("dcos_w", "dcos_x", "rowdot", "colprod"):
            assert torch.isfinite(r[n][:MC.N_REGULAR]).all()
        if (C, K) == (700, 3):
            assert int(label[4]) == 341 and 341 * 3 <= 1023 < 1024 <= 341 * 3 + 2


def _rows_f32(cos, label, C, K, margin_type, margin, scale, easy, n_top, inter_margin):
    """The kernel's arithmetic restated in f32 torch, step for step (class maximum, label logit and dphi, the selection
    on the f32 class cosines, psi / dpsi, max, exp, the whole-row and the off-label sum, loss = (max + log sum) - z_y,
    label gradient -sum_off / sum where p_y > 1/2 else p_y - 1, the gradient on the winning column) -> (loss_rows,
    softmax, g [B, C*K]) in f32."""
    f = lambda v: torch.tensor(v, dtype=F32)
    c = cos.float()
    B = c.shape[0]
    ar = torch.arange(B)
    m, kstar = MC.class_cosines(c, C, K)
    cy = m[ar, label]
    sc = f(scale)
    if margin_type == "cos":
        zy, dphi = (cy - f(margin)) * sc, torch.ones(B)
    else:
        cos_m, sin_m = f(math.cos(margin)), f(math.sin(margin))
        th, mm = f(math.cos(math.pi - margin)), f(math.sin(math.pi - margin) * margin)
        sine = torch.sqrt((1.0 - cy * cy).clamp(0, 1))
        on = (cy > 0) if easy else (cy - th > 0)
        dphi = torch.where(on, cos_m + sin_m * cy / sine.clamp_min(1e-12), torch.ones(B))
        zy = torch.where(on, cy * cos_m - sine * sin_m, cy if easy else cy - mm) * sc
    sel = MC.select_topk(m, label, n_top)
    cos_i, sin_i = f(math.cos(inter_margin)), f(math.sin(inter_margin))
    sine = torch.sqrt((1.0 - m * m).clamp(0, 1))
    z = torch.where(sel, m * cos_i + sine * sin_i, m) * sc
    z[ar, label] = zy
    mx = z.max(dim=1).values
    e = torch.exp(z - mx[:, None])
    s = e.sum(dim=1)
    eo = e.clone()
    eo[ar, label] = 0.0
    inv = 1.0 / s
    p = e * inv[:, None]
    g = p * (1.0 / B) * sc * torch.where(sel, cos_i - sin_i * m / sine.clamp_min(1e-12), torch.ones_like(m))
    py = p[ar, label]
    g[ar, label] = torch.where(py > 0.5, -(eo.sum(dim=1) * inv), py - 1.0) * (1.0 / B) * sc * dphi
    full = torch.zeros(B, C, K).scatter_(2, kstar[:, :, None], g[:, :, None]).view(B, C * K)
    return (mx + torch.log(s)) - zy, p, full


def test_f32_restatement_of_the_margin_kernel_meets_the_gpu_bounds():
    """On every row case (all modes, shapes and n_top) f32 arithmetic in the kernel's order meets the bounds the device
    is held to, so a miss on the GPU is the kernel's, not the case's.  The worst figures are printed."""
    worst = [0.0, 0.0, 0.0]
    R = MC.N_REGULAR
    for mt, margin, scale, easy in MC.ROW_MODES:
        for C, K in MC.ROW_SHAPES:
            for n_top in MC.n_tops(C):
                cos, label, _, _, _, _ = MC.row_case(margin, C, K, n_top)
                cc = cos[:, :C * K]
                ref = MC.margin_rows_ref(cc, label, C, K, mt, margin, scale, easy, n_top, MC.INTER_MARGIN)
                loss, sm, g = _rows_f32(cc, label, C, K, mt, margin, scale, easy, n_top, MC.INTER_MARGIN)
                lerr = float(((loss.double() - ref["loss_rows"]).abs() / ref["loss_rows"].abs().clamp_min(1.0)).max())
                serr = float((sm.double() - ref["softmax"]).abs().max())
                gerr = float(((g.double() - ref["g"])[:R].norm(dim=1) / ref["g"][:R].norm(dim=1)).max())
                assert float(g[~MC.winner_mask(ref["kstar"], K)].abs().max() if K > 1 else 0.0) == 0.0
                worst = [max(a, b) for a, b in zip(worst, (lerr, serr, gerr))]
    print(f"margin-head-parity: f32 restatement of the margin kernel (CPU): loss {worst[0]:.3e}, loss_bound {LOSS_TOL:.3e}, "
          f"softmax {worst[1]:.3e}, softmax_bound {SM_ATOL:.3e}, g {worst[2]:.3e}, grad_bound {GRAD_TOL:.3e}")
    assert worst[0] < LOSS_TOL and worst[1] < SM_ATOL and worst[2] < GRAD_TOL


# ---------------------------------------------------------------------------------------------- margin schedule
def test_margin_schedule_end_points_clamping_and_modes():
    from w2v2_speaker_amd.optim.schedule import MarginSchedule
    lin = MarginSchedule(0.3, initial=0.1, start_step=10, end_step=30)
    assert [lin(s) for s in (0, 10)] == [0.1, 0.1] and lin(30) == pytest.approx(0.3, abs=1e-15)
    assert lin(1000) == pytest.approx(0.3, abs=1e-15) and lin(20) == pytest.approx(0.2, abs=1e-15)
    ex = MarginSchedule(0.2, start_step=0, end_step=100, mode="exp")
    assert ex(0) == 0.0 and ex(100) == pytest.approx(0.2, abs=1e-15) and ex(-5) == 0.0
    assert ex(500) == pytest.approx(0.2, abs=1e-15)
    assert ex(50) == pytest.approx(0.2 * (1 - 1000 ** -0.5) / (1 - 1e-3), abs=1e-15)
    assert all(ex(s) < ex(s + 1) for s in range(100)) and ex(50) > 0.2 * 0.5           # monotone; front-loaded
    const = MarginSchedule(0.5, initial=0.5, start_step=0, end_step=0)                 # large-margin fine-tuning
    assert const(0) == 0.5 and const(7) == 0.5
    for bad in (dict(mode="cosine"), dict(start_step=5, end_step=4)):
        with pytest.raises(ValueError):
            MarginSchedule(0.2, **{"end_step": 10, **bad})


# ---------------------------------------------------------------------------------------------- parameter stores
def test_param_store_sub_centres_shapes_and_state_dict_error():
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    one = ParamStore(cfg, "cpu", F32, head="aam", num_speakers=10)
    st = ParamStore(cfg, "cpu", F32, head="aam", num_speakers=10, sub_centers=3)
    E = one.p("loss_fn.fc_weights").shape[1]
    assert one.p("loss_fn.fc_weights").shape == (10, E) and st.p("loss_fn.fc_weights").shape == (30, E)
    assert st.num_speakers == 10 and st.sub_centers == 3 and one.sub_centers == 1
    st.init_weights(3)                  # xavier_normal_ over [30, E]: std = sqrt(2 / (30 + E))
    std = float(st.p("loss_fn.fc_weights").std())
    assert abs(std / math.sqrt(2.0 / (30 + E)) - 1.0) < 0.15
    sd = st.state_dict()
    assert sd["loss_fn.fc_weights"].shape == (30, E)
    st.load_state_dict(sd)
    with pytest.raises((ValueError, RuntimeError)) as err:
        one.load_state_dict(sd)
    assert f"(30, {E})" in str(err.value).replace("torch.Size", "").replace("[", "(").replace("]", ")") and \
        f"(10, {E})" in str(err.value).replace("torch.Size", "").replace("[", "(").replace("]", ")")
    with pytest.raises(ValueError):
        ParamStore(cfg, "cpu", F32, head="aam", num_speakers=10, sub_centers=9)
    with pytest.raises(ValueError):
        ParamStore(cfg, "cpu", F32, head="ce", num_speakers=10, sub_centers=2)


def test_ecapa_store_sub_centres_shapes():
    from w2v2_speaker_amd.ecapa import EcapaConfig, EcapaStore
    cfg = EcapaConfig.tiny()
    st = EcapaStore(cfg, "cpu", F32, num_speakers=7, sub_centers=2)
    assert st.p("loss_fn.fc_weights").shape == (14, cfg.lin_neurons) and st.num_speakers == 7 and st.sub_centers == 2


# ---------------------------------------------------------------------------------------------- host-side rules
def test_argument_rules_on_the_host():
    from w2v2_speaker_amd import ops
    assert ops.check_margin_head(100, 3, 5, 0.06, "cos") == ops.MARGIN_COS == 1
    assert ops.check_margin_head(5, 1, 4, 0.0, "arc") == ops.MARGIN_ARC == 0
    for C, K, n_top, im, mt in ((100, 9, 0, 0.06, "arc"), (100, 0, 0, 0.06, "arc"), (5, 1, 5, 0.06, "arc"),
                                (100, 1, 17, 0.06, "arc"), (100, 1, 1, -0.1, "arc"), (100, 1, 0, 0.06, "sphere")):
        with pytest.raises(ValueError):
            ops.check_margin_head(C, K, n_top, im, mt)


def test_symbol_declared_exported_and_wrapped_with_matching_signature():
    import ctypes
    import os
    import re
    from w2v2_speaker_amd import _build, _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "w2v2_hip.h")).read()
    name = "w2v2_margin_softmax_fwd_bwd"
    m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
    assert m and name in _lib._SIGS and name in _lib.EXPORTS and "margin_head.hip" in _build.SOURCES
    kinds = []
    for a in m.group(1).replace("\n", " ").split(","):
        t = a.strip().rsplit(" ", 1)[0].replace("const ", "")
        kinds.append(ctypes.c_void_p if "*" in a else {"int": ctypes.c_int32, "int64_t": ctypes.c_int64,
                                                        "float": ctypes.c_float}[t])
    res, args = _lib._SIGS[name]
    assert res is ctypes.c_int32 and list(args) == kinds
    assert "#define W2V2_MARGIN_ARC 0" in hdr and "#define W2V2_MARGIN_COS 1" in hdr
    assert hasattr(_lib.load(), name) and callable(ops.margin_softmax_fwd_bwd)


def test_loss_class_is_an_aam_loss_with_sub_centre_weights():
    from w2v2_speaker_amd.optim.loss import AngularAdditiveMarginSoftMaxLoss, SubCenterMarginSoftMaxLoss
    lf = SubCenterMarginSoftMaxLoss(24, 10, margin=0.2, scale=30, sub_centers=3, margin_type="cos", inter_topk=2,
                                    inter_margin=0.05, device="cpu")
    assert isinstance(lf, AngularAdditiveMarginSoftMaxLoss) and lf.fc_weights.shape == (30, 24)
    assert (lf.sub_centers, lf.margin_type, lf.inter_topk, lf.inter_margin) == (3, "cos", 2, 0.05)
    with pytest.raises(ValueError):
        SubCenterMarginSoftMaxLoss(24, 10, sub_centers=9, device="cpu")
    with pytest.raises(ValueError):
        SubCenterMarginSoftMaxLoss(24, 10, inter_topk=10, device="cpu")
