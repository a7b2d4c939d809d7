"""Cases and float64 references for the loss-head kernels (csrc/heads.hip), shared by tests/test_heads_cpu.py,
tests/test_heads_gpu.py and tools/heads_parity.py.  No GPU and no ``ops`` import here: everything is plain torch on the
CPU in float64.

The references restate the formulas of ref: src/optim/loss/aam_softmax.py:50-74 and src/optim/loss/cross_entropy.py:27-31
on the COSINE matrix (the row kernel's own input), so that the row kernel can be tested without a GEMM in front of it;
tests/test_heads_cpu.py ties them to ``oracle.w2v2_oracle.aam_softmax`` / ``ce_head`` (which the goldens pin)."""
import math

import torch

F64 = torch.float64

# (margin, scale, easy_margin); margin < 0 is the plain cross-entropy mode of the row kernel (scale ignored, z = cos)
ROW_MODES = [(0.2, 30.0, False), (0.3, 15.0, False), (0.2, 30.0, True), (-1.0, 30.0, False)]
ROW_CLASSES = [5, 1024, 1025, 2500]     # one trip; exactly one trip of the 1024 threads; one column into the second; three trips
N_REGULAR = 10                          # rows 0 .. 9 are compared, rows 10 / 11 sit on cos == +1 / -1 (finiteness only)

HEAD_MARGIN, HEAD_SCALE = 0.5, 30.0
HEAD_TARGETS = [0.3, -0.95, -0.8, 0.9, 0.03, -0.03, 0.6, -0.5]
# (B, E, C): E % 8 != 0 -> three-launch dW path; S = 2, Kc = 296, rest = 8; S = 16, Kc = 256, rest = 4
HEAD_SHAPES = [(9, 20, 300), (66, 64, 600), (3, 40, 4100)]


def roundup8(n: int) -> int:
    return (n + 7) // 8 * 8


def threshold(margin: float) -> float:
    """th = cos(pi - m): at or below it the hard-margin head falls back to cos - sin(pi - m) * m."""
    return math.cos(math.pi - margin)


def label_cosines(margin: float):
    """The planted label cosines of the row cases: both sides of th, both sides of 0, near +-1, then +1 and -1 exactly.
    The plain mode (margin < 0) has no branch: it takes the list of margin 0.2."""
    th = threshold(margin if margin >= 0 else 0.2)
    return [0.3, 0.9, 0.995, -0.995, th + 1e-3, th - 1e-3, 1e-3, -1e-3, -0.5, 0.0, 1.0, -1.0]


def spread_labels(B: int, C: int) -> torch.Tensor:
    """Columns 0, C-1, 1023, 1024 (clamped to C-1: first / last thread of the first trip, first of the second), the
    rest spread over the row."""
    lab = [0, C - 1, min(1023, C - 1), min(1024, C - 1)] + [(977 * i + 13) % C for i in range(max(0, B - 4))]
    return torch.tensor(lab[:B], dtype=torch.int64)


def plant_cosines(C: int, ldc: int, label: torch.Tensor, label_cos, seed: int = 0) -> torch.Tensor:
    """[B, ldc] f32: off-label entries uniform in +-0.6, entry (b, label[b]) = label_cos[b], columns [C, ldc) NaN (the
    kernel must not read them)."""
    B = label.numel()
    g = torch.Generator().manual_seed(1000 + seed)
    cos = torch.full((B, ldc), float("nan"), dtype=torch.float32)
    cos[:, :C] = (torch.rand(B, C, generator=g, dtype=F64) * 1.2 - 0.6).float()
    cos[torch.arange(B), label] = torch.tensor(label_cos, dtype=F64).float()
    return cos


def row_case(margin: float, C: int, seed: int = 0):
    """-> (cos [12, ldc] f32, label [12], inv_x [12] f32, inv_w [C] f32, ldc) of one row-kernel case."""
    lc = label_cosines(margin)
    label = spread_labels(len(lc), C)
    ldc = roundup8(C) + 8
    cos = plant_cosines(C, ldc, label, lc, seed=seed + C)
    g = torch.Generator().manual_seed(2000 + seed + C)
    inv_x = (torch.rand(len(lc), generator=g) * 0.75 + 0.25).float()
    inv_w = (torch.rand(C, generator=g) * 1.5 + 0.5).float()
    return cos, label, inv_x, inv_w, ldc


def margin_logits(cos: torch.Tensor, label: torch.Tensor, margin: float, scale: float, easy_margin: bool) -> torch.Tensor:
    """z of ref: aam_softmax.py:57-68 from the cosine matrix (differentiable); margin < 0: z = cos."""
    if margin < 0:
        return cos
    cos_m, sin_m = math.cos(margin), math.sin(margin)
    th, mm = threshold(margin), math.sin(math.pi - margin) * margin
    sine = torch.sqrt((1.0 - cos * cos).clamp(0, 1))
    phi = cos * cos_m - sine * sin_m
    phi = torch.where(cos > 0, phi, cos) if easy_margin else torch.where((cos - th) > 0, phi, cos - mm)
    one_hot = torch.zeros_like(cos)
    one_hot.scatter_(1, label.view(-1, 1), 1)
    return (one_hot * phi + (1.0 - one_hot) * cos) * scale


def aam_rows_ref(cos, label, margin, scale, easy_margin, loss_scale=None, inv_x=None, inv_w=None):
    """float64 restatement of aam_row_kernel on the f32 cosine / logit matrix ``cos`` [B, C] it reads.  Returns a dict:
    loss_rows [B], softmax [B, C], g = d(mean loss)/dcos * loss_scale (autograd), dcos_w = g * inv_w[c],
    dcos_x = g * inv_x[b], rowdot[b] = sum_c g cos, colprod = g cos, correct[b] = (first arg-max of z == label).
    A label outside [0, C): NaN loss, zero gradients, correct 0 (and its softmax row is not defined here: NaN)."""
    B, C = cos.shape
    c = cos.to(F64).detach().clone().requires_grad_(True)
    bad = (label < 0) | (label >= C)
    lab = torch.where(bad, torch.zeros_like(label), label)
    z = margin_logits(c, lab, margin, scale, easy_margin)
    logp = torch.log_softmax(z, dim=1)
    rows = -logp.gather(1, lab.view(-1, 1)).view(-1)
    (rows * (~bad).to(F64)).sum().div(B).backward()          # the mean is over all B rows, bad ones add nothing
    g = c.grad * (1.0 if loss_scale is None else float(loss_scale))
    g[bad] = 0.0
    sm = torch.softmax(z.detach(), dim=1)
    sm[bad] = float("nan")
    cd = c.detach()
    first_max = (z.detach() == z.detach().max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)
    out = {"loss_rows": torch.where(bad, torch.full_like(rows, float("nan")), rows).detach(), "softmax": sm, "g": g,
           "dcos_w": g * inv_w.to(F64)[None, :] if inv_w is not None else g,
           "dcos_x": g * inv_x.to(F64)[:, None] if inv_x is not None else g,
           "rowdot": (g * cd).sum(dim=1), "colprod": g * cd,
           "correct": ((first_max == label) & ~bad).to(F64)}
    return out


# ---------------------------------------------------------------------------------------------- head-level cases
def plant_embeddings(W: torch.Tensor, label: torch.Tensor, targets, seed: int = 0) -> torch.Tensor:
    """emb[b] = len_b * (a w^ + sqrt(1 - a^2) r^), w^ = W[label[b]] / |W[label[b]]|, r^ a random unit vector orthogonal
    to w^, len_b uniform in [1, 4]: the label cosine of row b is a = targets[b] (f32 result, composed in float64)."""
    g = torch.Generator().manual_seed(3000 + seed)
    B, E = label.numel(), W.shape[1]
    wn = W.to(F64)[label]
    wn = wn / wn.norm(dim=1, keepdim=True)
    r = torch.randn(B, E, generator=g, dtype=F64)
    r = r - (r * wn).sum(dim=1, keepdim=True) * wn
    r = r / r.norm(dim=1, keepdim=True)
    a = torch.tensor(targets, dtype=F64).view(-1, 1)
    length = torch.rand(B, 1, generator=g, dtype=F64) * 3.0 + 1.0
    return (length * (a * wn + torch.sqrt(1.0 - a * a) * r)).float()


def head_case(B: int, E: int, C: int, seed: int = 0):
    """-> (emb [B, E] f32, W [C, E] f32, bias [C] f32, label [B], targets [B]) of one ClassifierHead case: class weights
    normal with the xavier deviation of the reference's init, label cosines planted on HEAD_TARGETS (cycled)."""
    g = torch.Generator().manual_seed(4000 + seed + C)
    W = (torch.randn(C, E, generator=g) * math.sqrt(2.0 / (C + E))).float()
    bias = (torch.randn(C, generator=g) * 0.5).float()
    label = spread_labels(B, C)
    targets = [HEAD_TARGETS[i % len(HEAD_TARGETS)] for i in range(B)]
    return plant_embeddings(W, label, targets, seed=seed + C), W, bias, label, targets


def _rounded_ste(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The value of ``t`` rounded to ``dtype`` with the gradient of ``t`` (the head rounds its GEMM operands and hands
    the gradient to the f32 masters unchanged)."""
    if dtype == torch.float32:
        return t
    return t + (t.detach().float().to(dtype).to(F64) - t.detach())


def head_cosines(emb, W, dtype) -> torch.Tensor:
    """What the head's cosine GEMM computes, in float64: operands rounded to ``dtype``, both norms from the f32 masters
    (differentiable wrt emb and W when they require grad)."""
    x, w = emb.to(F64) if emb.dtype != F64 else emb, W.to(F64) if W.dtype != F64 else W
    inv_x = 1.0 / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    inv_w = 1.0 / w.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return (_rounded_ste(x, dtype) @ _rounded_ste(w, dtype).t()) * inv_x * inv_w.t()


def head_ref(kind, emb, W, bias, label, dtype, margin=HEAD_MARGIN, scale=HEAD_SCALE, easy_margin=False):
    """float64 + autograd reference of one ClassifierHead step -> dict(loss, softmax, demb, w_grad, bias_grad).
    "ce": ``oracle.ce_head`` itself on the rounded operands.  "aam": the oracle's formula on head_cosines() -- for f32
    that IS ``oracle.aam_softmax`` (asserted to 1e-12 in tests/test_heads_cpu.py); for the 16-bit dtypes the oracle
    cannot be called as it stands because it would take the norms of the rounded operands, the head those of the masters."""
    from oracle import w2v2_oracle as O
    x = emb.to(F64).clone().requires_grad_(True)
    w = W.to(F64).clone().requires_grad_(True)
    out = {}
    if kind == "ce":
        b = bias.to(F64).clone().requires_grad_(True)
        loss, sm = O.ce_head(_rounded_ste(x, dtype), _rounded_ste(w, dtype), b, label)
        loss.backward()
        out["bias_grad"] = b.grad
    else:
        z = margin_logits(head_cosines(x, w, dtype), label, margin, scale, easy_margin)
        loss = -torch.log_softmax(z, dim=1).gather(1, label.view(-1, 1)).mean()
        sm = torch.softmax(z, dim=1)
        loss.backward()
    out.update(loss=loss.detach(), softmax=sm.detach(), demb=x.grad, w_grad=w.grad)
    return out


# ---------------------------------------------------------------------------------------------- the other kernels
INVNORM_ROWS = [1, 4, 5, 4099]
INVNORM_COLS = [1, 3, 63, 64, 65, 192, 257]
NORMBWD_SHAPES = [(1, 1), (7, 37), (66, 192), (4100, 257)]       # the last: > 4096 x 256 elements, a second grid trip
BCE_H = [1, 63, 64, 65, 257, 768]
BCE_B = [1, 5, 300]


def invnorm_ref(x_rounded: torch.Tensor) -> torch.Tensor:
    """1 / max(|x|, 1e-12) per row in float64 (F.normalize's eps) of the values the kernel reads."""
    return 1.0 / x_rounded.to(F64).norm(dim=1).clamp_min(1e-12)


def normalize_bwd_ref(g, x_rounded, inv, dot) -> torch.Tensor:
    """dx = inv * (g - x * inv * dot) per row, float64."""
    iv = inv.to(F64)[:, None]
    return iv * (g.to(F64) - x_rounded.to(F64) * iv * dot.to(F64)[:, None])


def bce_case(B: int, H: int, seed: int = 0):
    """-> (emb [B, H] f32, w [H] f32, b [1] f32, label [B] in {0, 1}); the first rows are built so that their logits are
    +100, -100 and 0 (saturated sigmoid on both sides, and the kink of the stable form), as far as B allows."""
    g = torch.Generator().manual_seed(5000 + seed + 7 * B + H)
    w = (torch.randn(H, generator=g) * 0.5).float()
    b = torch.tensor([0.25], dtype=torch.float32)
    emb = torch.randn(B, H, generator=g).float()
    wd = w.to(F64)
    for r, want in zip(range(B), (100.0, -100.0, 0.0)):
        e = emb[r].to(F64)
        e = e + (want - 0.25 - float(e @ wd)) * wd / float(wd @ wd)
        emb[r] = e.float()
    label = (torch.rand(B, generator=g) < 0.5).to(torch.int64)
    label[0] = 0                           # the saturated rows on their expensive side: loss = 100
    if B >= 2:
        label[1] = 1
    return emb, w, b, label


def bce_ref(emb, w, b, label, loss_scale=None):
    """float64 binary_cross_entropy_with_logits (mean over B) of Linear(H, 1), with autograd -> dict(prob, loss_rows,
    dlogit, demb, dw, db).  A label outside {0, 1}: NaN loss row, zero gradient."""
    import torch.nn.functional as F
    B = emb.shape[0]
    e = emb.to(F64).clone().requires_grad_(True)
    wv = w.to(F64).clone().requires_grad_(True)
    bv = b.to(F64).clone().requires_grad_(True)
    bad = (label != 0) & (label != 1)
    y = torch.where(bad, torch.zeros_like(label), label).to(F64)
    logit = e @ wv + bv
    logit.retain_grad()
    rows = F.binary_cross_entropy_with_logits(logit, y, reduction="none")
    ((rows * (~bad).to(F64)).sum() / B * (1.0 if loss_scale is None else float(loss_scale))).backward()
    return {"prob": torch.sigmoid(logit.detach()), "dlogit": logit.grad, "demb": e.grad, "dw": wv.grad, "db": bv.grad,
            "loss_rows": torch.where(bad, torch.full_like(rows, float("nan")), rows).detach()}
