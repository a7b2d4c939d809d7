"""CPU checks of the float64 references and planted inputs in tests/heads_cases.py (what tests/test_heads_gpu.py compares
csrc/heads.hip against): the references reproduce the golden-pinned oracle, and the planted inputs reach every branch."""
import math

import pytest
import torch

import heads_cases as HC
from oracle import w2v2_oracle as O

F64 = torch.float64


def _random_head(B=6, E=24, C=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, E, generator=g, dtype=F64) * 2.0
    W = torch.randn(C, E, generator=g, dtype=F64)
    bias = torch.randn(C, generator=g, dtype=F64)
    label = torch.randint(0, C, (B,), generator=g)
    x[0] = -3.0 * W[label[0]] + 0.05 * x[0]          # one row in the hard-margin fall-back, one near cos = +1
    x[1] = 2.0 * W[label[1]] + 0.05 * x[1]
    return x, W, bias, label


@pytest.mark.parametrize("margin,scale,easy", [(0.2, 30.0, False), (0.3, 15.0, False), (0.5, 30.0, False),
                                               (0.2, 30.0, True), (0.5, 30.0, True)])
def test_rows_reference_reproduces_the_aam_oracle(margin, scale, easy):
    """aam_rows_ref on cos = normalize(x) @ normalize(W).T gives oracle.aam_softmax's loss, softmax, and -- pushed
    through the two F.normalize backwards with its own dcos / rowdot / colprod -- its dx and dW, to 1e-12."""
    x, W, _, label = _random_head()
    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    loss, sm = O.aam_softmax(xr, Wr, label, margin, scale, easy_margin=easy)
    loss.backward()
    inv_x, inv_w = 1.0 / x.norm(dim=1), 1.0 / W.norm(dim=1)
    cos = (x * inv_x[:, None]) @ (W * inv_w[:, None]).t()
    assert int((cos[torch.arange(6), label] - HC.threshold(margin) <= 0).sum()) >= 1
    r = HC.aam_rows_ref(cos, label, margin, scale, easy, inv_x=inv_x, inv_w=inv_w)
    assert abs(float(r["loss_rows"].mean()) - float(loss.detach())) < 1e-12
    assert float((r["softmax"] - sm.detach()).abs().max()) < 1e-12
    dx = HC.normalize_bwd_ref(r["dcos_w"] @ W, x, inv_x, r["rowdot"])
    dW = HC.normalize_bwd_ref(r["dcos_x"].t() @ x, W, inv_w, r["colprod"].sum(dim=0))
    assert float((dx - xr.grad).abs().max()) < 1e-12 and float((dW - Wr.grad).abs().max()) < 1e-12
    assert torch.equal(r["correct"], (sm.argmax(dim=1) == label).to(F64))
    # the head-level reference in f32 mode (nothing rounded) is the oracle
    h = HC.head_ref("aam", x, W, None, label, torch.float32, margin, scale, easy)
    assert abs(float(h["loss"]) - float(loss.detach())) < 1e-12 and float((h["softmax"] - sm.detach()).abs().max()) < 1e-12
    assert float((h["demb"] - xr.grad).abs().max()) < 1e-12 and float((h["w_grad"] - Wr.grad).abs().max()) < 1e-12


def test_rows_reference_reproduces_the_ce_oracle():
    """Plain mode (margin < 0, scale ignored) on logits = x W^T + b gives oracle.ce_head's loss, softmax and d/dlogits."""
    x, W, bias, label = _random_head(seed=1)
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, bias))
    loss, sm = O.ce_head(xr, Wr, br, label)
    loss.backward()
    logits = x @ W.t() + bias
    for scale in (30.0, 1.0):
        r = HC.aam_rows_ref(logits, label, -1.0, scale, False)
        assert abs(float(r["loss_rows"].mean()) - float(loss.detach())) < 1e-12
        assert float((r["softmax"] - sm.detach()).abs().max()) < 1e-12
        assert float((r["g"] @ W - xr.grad).abs().max()) < 1e-12
        assert float((r["g"].t() @ x - Wr.grad).abs().max()) < 1e-12
        assert float((r["g"].sum(dim=0) - br.grad).abs().max()) < 1e-12
    h = HC.head_ref("ce", x, W, bias, label, torch.float32)
    assert abs(float(h["loss"]) - float(loss.detach())) < 1e-12 and float((h["bias_grad"] - br.grad).abs().max()) < 1e-12


def test_rows_reference_bad_labels_and_loss_scale():
    x, W, _, label = _random_head(seed=2)
    cos = torch.nn.functional.normalize(x) @ torch.nn.functional.normalize(W).t()
    good = HC.aam_rows_ref(cos, label, 0.2, 30.0, False)
    lab = label.clone()
    lab[1], lab[3], lab[4] = -1, 11, 2 ** 40
    r = HC.aam_rows_ref(cos, lab, 0.2, 30.0, False, loss_scale=8.0)
    bad = torch.tensor([False, True, False, True, True, False])
    assert torch.isnan(r["loss_rows"][bad]).all() and torch.equal(r["loss_rows"][~bad], good["loss_rows"][~bad])
    assert float(r["g"][bad].abs().max()) == 0.0 and float(r["correct"][bad].abs().max()) == 0.0
    assert torch.allclose(r["g"][~bad], 8.0 * good["g"][~bad], rtol=1e-15, atol=0)


@pytest.mark.parametrize("margin,scale,easy", HC.ROW_MODES)
@pytest.mark.parametrize("C", HC.ROW_CLASSES)
def test_planted_cosines_reach_every_branch(margin, scale, easy, C):
    cos, label, inv_x, inv_w, ldc = HC.row_case(margin, C)
    assert cos.shape == (12, ldc) and ldc == HC.roundup8(C) + 8 and cos.dtype == torch.float32
    assert torch.isnan(cos[:, C:]).all() and float(cos[:, :C].abs().max()) <= 1.0
    assert label.tolist()[:4] == [0, C - 1, min(1023, C - 1), min(1024, C - 1)]
    cy = cos[torch.arange(12), label].double()[:HC.N_REGULAR]
    th = HC.threshold(margin if margin >= 0 else 0.2)
    # regular rows: 8 above th and 2 below it (-0.995 and th - 1e-3), none within 9e-4 of it; 4 above 0, 6 at or below it
    assert int((cy - th > 0).sum()) == 8 and int((cy - th <= 0).sum()) == 2 and float((cy - th).abs().min()) > 9e-4
    assert int((cy > 0).sum()) == 4 and int((cy <= 0).sum()) == 6
    assert float((cy[cy != 0]).abs().min()) > 9e-4
    assert cos[10, label[10]] == 1.0 and cos[11, label[11]] == -1.0
    off = cos[:, :C].clone()
    off[torch.arange(12), label] = 0.0
    assert float(off.abs().max()) <= 0.6
    r = HC.aam_rows_ref(cos[:, :C], label, margin, scale, easy, inv_x=inv_x, inv_w=inv_w)
    for k in ("loss_rows", "softmax"):
        assert torch.isfinite(r[k]).all()
    for k in ("dcos_w", "dcos_x", "rowdot", "colprod"):
        assert torch.isfinite(r[k][:HC.N_REGULAR]).all()
    assert float(r["loss_rows"].max()) < 60.0


@pytest.mark.parametrize("B,E,C", HC.HEAD_SHAPES)
def test_planted_embeddings_keep_their_branch_in_16_bits(B, E, C):
    """The planted label cosines are the targets (to f32 rounding); rounding emb and W to bf16 / fp16 (norms from the
    f32 masters, as the head does) moves them by at most 2 * 2^-9 + 2^-18 / 2 * 2^-12 + 2^-24 (each operand's relative
    rounding error, Cauchy-Schwarz), far less than the 0.03 by which every target clears cos(pi - 0.5) and 0."""
    emb, W, bias, label, targets = HC.head_case(B, E, C)
    t = torch.tensor(targets, dtype=F64)
    th = HC.threshold(HC.HEAD_MARGIN)
    assert float(torch.minimum((t - th).abs(), t.abs()).min()) >= 0.03 - 1e-12
    assert int((t - th <= 0).sum()) >= 1 and int((t - th > 0).sum()) >= 1 and int((t > 0).sum()) >= 1 and int((t <= 0).sum()) >= 1
    ar = torch.arange(B)
    c32 = HC.head_cosines(emb, W, torch.float32)[ar, label]
    assert float((c32 - t).abs().max()) < 1e-6
    lens = emb.double().norm(dim=1)
    assert float(lens.min()) >= 1.0 - 1e-6 and float(lens.max()) <= 4.0 + 1e-6
    for dtype, bound in ((torch.bfloat16, 2 * 2.0 ** -9 + 2.0 ** -18), (torch.float16, 2 * 2.0 ** -12 + 2.0 ** -24)):
        c16 = HC.head_cosines(emb, W, dtype)[ar, label]
        moved = float((c16 - t).abs().max())
        print(f"heads-parity: planted cosines B={B} E={E} C={C} {dtype}: moved by {moved:.3e} (bound {bound:.3e})")
        assert moved <= bound
        assert torch.equal(c16 - th > 0, t - th > 0) and torch.equal(c16 > 0, t > 0)
    # S / Kc / rest of the chunked d(emb) product and the dW path, as ClassifierHead derives them
    S = max(1, min(16, C // 256))
    Kc = (C // S) // 8 * 8 if S > 1 else C
    assert (E % 8 != 0, S, Kc, C - S * Kc) == {(9, 20, 300): (True, 1, 300, 0), (66, 64, 600): (False, 2, 296, 8),
                                               (3, 40, 4100): (False, 16, 256, 4)}[(B, E, C)]


def _rows_f32(cos, label, margin, scale, easy):
    """The row kernel's arithmetic restated in f32 torch, step for step (label logit and dphi, max, exp, the whole-row
    and the off-label sum, loss = (max + log sum) - z_y, label gradient -sum_off / sum where p_y > 1/2 else p_y - 1)
    -> (loss_rows, softmax, g) in f32."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    c = cos.float()
    B, C = c.shape
    ar = torch.arange(B)
    cy = c[ar, label]
    if margin < 0:
        zy, dphi, sc = cy, torch.ones(B), f(1.0)
    else:
        cos_m, sin_m = f(math.cos(margin)), f(math.sin(margin))
        th, mm = f(math.cos(math.pi - margin)), f(math.sin(math.pi - margin) * margin)
        sine = torch.sqrt((1.0 - cy * cy).clamp(0, 1))
        on = (cy > 0) if easy else (cy - th > 0)
        dphi = torch.where(on, cos_m + sin_m * cy / sine.clamp_min(1e-12), torch.ones(B))
        zy = torch.where(on, cy * cos_m - sine * sin_m, cy if easy else cy - mm) * f(scale)
        sc = f(scale)
    z = c * sc
    z[ar, label] = zy
    mx = z.max(dim=1).values
    e = torch.exp(z - mx[:, None])
    s = e.sum(dim=1)
    eo = e.clone()
    eo[ar, label] = 0.0
    inv = 1.0 / s
    p = e * inv[:, None]
    g = p * (1.0 / B) * sc
    py = p[ar, label]
    g[ar, label] = torch.where(py > 0.5, -(eo.sum(dim=1) * inv), py - 1.0) * (1.0 / B) * sc * dphi
    return (mx + torch.log(s)) - zy, p, g


def test_f32_restatement_of_the_row_kernel_meets_the_gpu_bounds():
    """What the bounds of tests/test_heads_gpu.py rest on: on the planted row cases, f32 arithmetic in the kernel's own
    order (with torch's exp / log in place of the device's fast ones) meets the bounds the device is held to -- loss
    2e-5 * max(1, |ref|), softmax 2e-6 absolute, gradient per-row rel-L2 1e-5 -- so the inputs are well posed: a device
    miss is the kernel's, not the case's.  The figures are printed (worst over all modes and class counts)."""
    worst = [0.0, 0.0, 0.0]
    R = HC.N_REGULAR
    for margin, scale, easy in HC.ROW_MODES:
        for C in HC.ROW_CLASSES:
            cos, label, _, _, _ = HC.row_case(margin, C)
            ref = HC.aam_rows_ref(cos[:, :C], label, margin, scale, easy)
            loss, sm, g = _rows_f32(cos[:, :C], label, margin, scale, easy)
            lerr = float(((loss.double() - ref["loss_rows"]).abs() / ref["loss_rows"].abs().clamp_min(1.0)).max())
            serr = float((sm.double() - ref["softmax"]).abs().max())
            gerr = float(((g.double() - ref["g"])[:R].norm(dim=1) / ref["g"][:R].norm(dim=1)).max())
            worst = [max(a, b) for a, b in zip(worst, (lerr, serr, gerr))]
    print(f"heads-parity: f32 restatement of the row kernel (CPU): loss {worst[0]:.3e}, loss_bound 2.000e-05, "
          f"softmax {worst[1]:.3e}, softmax_bound 2.000e-06, g {worst[2]:.3e}, grad_bound 1.000e-05")
    assert worst[0] < 2e-5 and worst[1] < 2e-6 and worst[2] < 1e-5
