"""Cases and float64 references for the margin heads (csrc/margin_head.hip, heads.ClassifierHead with sub-centres, the
cosine margin or inter-top-k), shared by tests/test_margin_head_cpu.py and tests/test_margin_head_gpu.py.  No GPU and no
``ops`` import here: plain torch on the CPU in float64.

The semantics are those written in include/w2v2_hip.h ("margin heads"); no reference file has such a head.  The
references take the class cosine by ``view(B, C, K).max(2)`` (autograd routes the gradient to the first maximum) and the
inter-top-k by a STABLE descending sort, so that ties resolve to the smaller index as the definition says."""
import math

import torch

import heads_cases as HC

F64 = torch.float64

# (margin_type, margin, scale, easy_margin)
ROW_MODES = [("arc", 0.2, 30.0, False), ("arc", 0.3, 15.0, False), ("arc", 0.2, 30.0, True), ("cos", 0.2, 30.0, False),
             ("cos", 0.35, 32.0, False)]
GPU_ROW_MODES = [0, 2, 3]                  # ARC hard, ARC easy, COS
# (C, K): one trip; sub-centres; exactly 1024 columns; one class into the second trip; class 341 straddles columns
# 1023 | 1024; three trips of the 1024 threads over the classes... (834, 3) = 2502 columns
ROW_SHAPES = [(5, 1), (5, 3), (512, 2), (1025, 1), (700, 3), (834, 3)]
MAX_TOPK = 16
INTER_MARGIN = 0.06
N_REGULAR = HC.N_REGULAR
TIE_ROW, TIE_VALUE = 3, 0.65               # the row whose rank-n_top negatives tie, on a value above the +-0.6 background

HEAD_MARGIN, HEAD_SCALE = 0.5, 30.0
# (B, E, C, K): E % 8 != 0 -> three-launch dW path; fused dW; 4110 columns = 16 chunks of 256 plus a ragged rest of 14
HEAD_SHAPES = [(9, 20, 100, 3), (66, 64, 200, 3), (3, 40, 1370, 3)]
# (margin_type, easy_margin, inter_topk)
HEAD_MODES = [("arc", False, 0), ("cos", False, 5), ("arc", True, 2)]


def n_tops(C: int):
    """{0, 1, min(5, C - 1), C - 1} with the last held to the entry's cap of 16 (C - 1 itself is legal at C = 5 only)."""
    return sorted({0, 1, min(5, C - 1), min(C - 1, MAX_TOPK)})


def row_case(margin: float, C: int, K: int, n_top: int, seed: int = 0):
    """-> (cos [12, ld] f32, label [12], inv_x [12] f32, inv_w [C*K] f32, ld) of one row-kernel case.  Background +-0.6
    in every column, NaN in [C*K, ld).  Row b's label class has its maximum, HC.label_cosines(margin)[b], on sub-centre
    b % K (every position k is a winner in some row) and its other sub-centres 0.25 .. 0.5 below it.  Planted beside:
      row 0: the label's sub-centres 0 and 1 hold the SAME value (K >= 2), and so do those of one negative class (0.55);
      rows 1, 2: the label class (0.9, 0.995) holds the row maximum -- it must never be selected;
      row TIE_ROW: n_top - 1 negatives at 0.7 + 0.01 i and two more, classes lo < hi, at exactly TIE_VALUE: rank n_top
        is a tie, lo is penalised and hi is not (where the row has n_top + 1 negatives)."""
    lc = HC.label_cosines(margin)
    B, Cn = len(lc), C * K
    label = HC.spread_labels(B, C)
    label[4] = 341 % C                                    # (700, 3): columns 1023 | 1024
    ld = HC.roundup8(Cn) + 8
    g = torch.Generator().manual_seed(7000 + seed + 13 * C + K)
    cos = torch.full((B, ld), float("nan"), dtype=torch.float32)
    cos[:, :Cn] = (torch.rand(B, Cn, generator=g, dtype=F64) * 1.2 - 0.6).float()

    def plant(b, c, kwin, value):
        low = torch.rand(K, generator=g, dtype=F64) * 0.25 + 0.25
        v = (value - low).clamp_min(-1.0)
        v[kwin] = value
        cos[b, c * K:(c + 1) * K] = v.float()

    for b in range(B):
        plant(b, int(label[b]), b % K, lc[b])
    if K >= 2:
        y0 = int(label[0])
        cos[0, y0 * K + 1] = cos[0, y0 * K]               # row 0 wins on k = 0: a two-way tie k = 0 / 1
        c = (y0 + 1) % C
        plant(0, c, 0, 0.55)
        cos[0, c * K + 1] = cos[0, c * K]
    y = int(label[TIE_ROW])
    neg = [c for c in range(C) if c != y]
    tie = None
    if n_top >= 1 and len(neg) >= n_top + 1:
        lo, hi = neg[1], neg[-1]
        for i, c in enumerate([c for c in neg if c not in (lo, hi)][:n_top - 1]):
            plant(TIE_ROW, c, i % K, 0.7 + 0.01 * i)
        plant(TIE_ROW, lo, (K - 1), TIE_VALUE)
        plant(TIE_ROW, hi, 0, TIE_VALUE)
        tie = (lo, hi)
    gen = torch.Generator().manual_seed(8000 + seed + C + K)
    inv_x = (torch.rand(B, generator=gen) * 0.75 + 0.25).float()
    inv_w = (torch.rand(Cn, generator=gen) * 1.5 + 0.5).float()
    return cos, label, inv_x, inv_w, ld, tie


def class_cosines(cos: torch.Tensor, C: int, K: int):
    """m [B, C] = max over the K adjacent sub-centre columns (differentiable: the gradient goes to the first maximum),
    kstar [B, C] = the smallest k that attains it."""
    B = cos.shape[0]
    v = cos.view(B, C, K)
    m = v.max(dim=2).values
    kstar = (v.detach() == m.detach()[:, :, None]).to(torch.int64).argmax(dim=2)
    # route the gradient through a gather at kstar (torch's max backward picks an index of its own on ties)
    return v.gather(2, kstar[:, :, None]).squeeze(2), kstar


def select_topk(m: torch.Tensor, label: torch.Tensor, n_top: int) -> torch.Tensor:
    """bool [B, C]: the n_top classes c != label with the largest m, ties to the smaller index (stable sort)."""
    sel = torch.zeros_like(m, dtype=torch.bool)
    if n_top == 0:
        return sel
    md = m.detach().clone()
    md.scatter_(1, label.view(-1, 1), float("-inf"))
    order = torch.sort(md, dim=1, descending=True, stable=True).indices[:, :n_top]
    sel.scatter_(1, order, True)
    return sel


def margin_logits(m, label, margin_type, margin, scale, easy_margin, n_top, inter_margin):
    """z [B, C] of the definition from the class cosines m (differentiable) and the selection mask."""
    one_hot = torch.zeros_like(m, dtype=torch.bool)
    one_hot.scatter_(1, label.view(-1, 1), True)
    sine = torch.sqrt((1.0 - m * m).clamp(0, 1))
    if margin_type == "cos":
        phi = m - margin
    else:
        cos_m, sin_m = math.cos(margin), math.sin(margin)
        th, mm = HC.threshold(margin), math.sin(math.pi - margin) * margin
        phi = m * cos_m - sine * sin_m
        phi = torch.where(m > 0, phi, m) if easy_margin else torch.where((m - th) > 0, phi, m - mm)
    sel = select_topk(m, label, n_top)
    psi = m * math.cos(inter_margin) + sine * math.sin(inter_margin)
    return torch.where(one_hot, phi, torch.where(sel, psi, m)) * scale, sel


def margin_rows_ref(cos, label, C, K, margin_type, margin, scale, easy_margin, n_top=0, inter_margin=INTER_MARGIN,
                    loss_scale=None, inv_x=None, inv_w=None):
    """float64 restatement of w2v2_margin_softmax_fwd_bwd on the f32 cosines ``cos`` [B, C*K].  Returns a dict:
    loss_rows [B], softmax [B, C], g [B, C*K] = d(mean loss)/dcos * loss_scale (autograd: zero off the winning
    sub-centres), dcos_w = g * inv_w[col], dcos_x = g * inv_x[b], rowdot, colprod = g * cos, correct, kstar, sel.
    A label outside [0, C): NaN loss, zero gradients, correct 0 (softmax row NaN: not defined here)."""
    B = cos.shape[0]
    c = cos.to(F64).detach().clone().requires_grad_(True)
    bad = (label < 0) | (label >= C)
    lab = torch.where(bad, torch.zeros_like(label), label)
    m, kstar = class_cosines(c, C, K)
    z, sel = margin_logits(m, lab, margin_type, margin, scale, easy_margin, n_top, inter_margin)
    rows = -torch.log_softmax(z, dim=1).gather(1, lab.view(-1, 1)).view(-1)
    (rows * (~bad).to(F64)).sum().div(B).backward()
    g = c.grad * (1.0 if loss_scale is None else float(loss_scale))
    g[bad] = 0.0
    sm = torch.softmax(z.detach(), dim=1)
    sm[bad] = float("nan")
    cd, zd = c.detach(), z.detach()
    first_max = (zd == zd.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)
    return {"loss_rows": torch.where(bad, torch.full_like(rows, float("nan")), rows).detach(), "softmax": sm, "g": g,
            "dcos_w": g * inv_w.to(F64)[None, :] if inv_w is not None else g,
            "dcos_x": g * inv_x.to(F64)[:, None] if inv_x is not None else g,
            "rowdot": (g * cd).sum(dim=1), "colprod": g * cd, "correct": ((first_max == label) & ~bad).to(F64),
            "kstar": kstar, "sel": sel}


def winner_mask(kstar: torch.Tensor, K: int) -> torch.Tensor:
    """bool [B, C*K]: the column c*K + kstar[b, c] of every class."""
    B, C = kstar.shape
    return torch.zeros(B, C, K, dtype=torch.bool).scatter_(2, kstar[:, :, None], True).view(B, C * K)


# ---------------------------------------------------------------------------------------------- head-level cases
def head_case(B: int, E: int, C: int, K: int, seed: int = 0):
    """-> (emb [B, E] f32, W [C*K, E] f32, label [B]): HC.head_case's construction over C*K weight rows; row b's cosine
    with sub-centre b % K of its label class is planted on HC.HEAD_TARGETS (the class cosine is then the larger of that
    and the other sub-centres' chance cosines)."""
    g = torch.Generator().manual_seed(9000 + seed + C * K)
    W = (torch.randn(C * K, E, generator=g) * math.sqrt(2.0 / (C * K + E))).float()
    label = HC.spread_labels(B, C)
    targets = [HC.HEAD_TARGETS[i % len(HC.HEAD_TARGETS)] for i in range(B)]
    rows = label * K + torch.arange(B) % K
    return HC.plant_embeddings(W, rows, targets, seed=seed + C * K), W, label


def head_ref(emb, W, label, dtype, C, K, margin_type, margin, scale, easy_margin, n_top, inter_margin=INTER_MARGIN):
    """float64 + autograd reference of one margin-head step from the embeddings -> dict(loss, softmax, demb, w_grad,
    never [C*K] bool = weight rows whose sub-centre wins in no row of the batch: their gradient is exactly zero)."""
    x = emb.to(F64).clone().requires_grad_(True)
    w = W.to(F64).clone().requires_grad_(True)
    m, kstar = class_cosines(HC.head_cosines(x, w, dtype), C, K)
    z, _ = margin_logits(m, label, margin_type, margin, scale, easy_margin, n_top, inter_margin)
    loss = -torch.log_softmax(z, dim=1).gather(1, label.view(-1, 1)).mean()
    loss.backward()
    return {"loss": loss.detach(), "softmax": torch.softmax(z.detach(), dim=1), "demb": x.grad, "w_grad": w.grad,
            "never": ~winner_mask(kstar, K).any(dim=0)}
