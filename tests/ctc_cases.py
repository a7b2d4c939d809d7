"""Cases and references of the CTC loss (csrc/ctc.hip), shared by tests/test_ctc_cpu.py, tests/test_ctc_gpu.py and
tools/ctc_bench.py.  No GPU and no ``ops`` import here: plain torch on the CPU.

``ctc_ref(..., dtype=F64)`` is the reference: torch's F.ctc_loss on log_softmax in float64 with autograd back to the
logits, i.e. ref: src/optim/loss/ctc_loss.py:36-58 (reduction "mean", zero_infinity) without its host copy;
tests/test_ctc_cpu.py ties it to goldens the reference's own class produced (tests/golden/g22_ctc.npz).  With
``dtype=F32`` it restates the kernel's arithmetic: the alpha / beta recursion over probabilities kept as (mantissa, int
exponent) pairs, beta without the emission of its own frame, the blank gradient from the two small sums.
``ref_f32_error`` is the error of torch's f32 CPU F.ctc_loss -- exactly what the reference runs -- against float64.

Bounds (loss: the project's f32 head bound; gradient: that bound or twice the reference's own f32 error on the same
inputs, whichever is larger -- two f32 evaluations of one recursion in different summation orders differ from each other
by about as much as each differs from float64)."""
import functools

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
LOSS_TOL, GRAD_TOL = 2e-5, 1e-5
MAX_TARGET = 31
LOG2E = 1.4426950408889634
ZERO_E = -(1 << 28)

# name -> (B, T, C incl. blank, target lengths, input lengths or None = T, blank bias, explicit targets or None,
#          utterances whose loss is infinite, ldc or None = C)
_SPECS = {
    # a single frame; an empty target
    "one_frame": (2, 1, 8, [1, 0], None, 0.0, None, (), None),
    # short inputs; the third has no frame for its label: loss row 0, gradient exactly 0
    "short_inputs": (3, 2, 5, [1, 1, 1], [2, 1, 0], 0.0, None, (2,), None),
    # repeated labels merge into one class column; [3, 3] needs 3 frames and has 2
    "repeats": (2, 5, 6, [3, 2], [5, 2], 0.0, [[1, 1, 2], [3, 3, 0]], (1,), None),
    # the full 63-state lattice
    "full_lattice": (3, 63, 8, [31, 31, 30], None, 0.0, None, (), None),
    # mixed lengths at the real frame count
    "mixed": (4, 149, 64, [31, 7, 1, 0], None, 0.0, None, (), None),
    "mixed_bias100": (4, 149, 64, [31, 7, 1, 0], None, 100.0, None, (), None),
    # C around the workgroup size (the scalar pass's trip count; 256 takes the 16-byte path) and around 4 x the workgroup
    # size (the 16-byte pass's trip count); 1021 in rows of 1024 whose padding holds NaN
    "c255": (2, 3, 255, [1, 1], None, 0.0, None, (), None),
    "c256": (2, 3, 256, [1, 1], None, 0.0, None, (), None),
    "c257": (2, 3, 257, [1, 1], None, 0.0, None, (), None),
    "c1023": (2, 3, 1023, [1, 1], None, 0.0, None, (), None),
    "c1024": (2, 3, 1024, [1, 1], None, 0.0, None, (), None),
    "c1025": (2, 3, 1025, [1, 1], None, 0.0, None, (), None),
    "c1021_nan_padding": (2, 3, 1021, [1, 1], None, 0.0, None, (), 1024),
    # the real head's rows (B = 8 keeps the float64 reference in seconds)
    "real": (8, 149, 5995, [1] * 8, None, 0.0, None, (), 6000),
    "real_bias100": (8, 149, 5995, [1] * 8, None, 100.0, None, (), 6000),
}
CASES = tuple(_SPECS)
SMALL_CASES = tuple(n for n in CASES if not n.startswith("real"))


def _nll(logits, targets, in_len, tgt_len, blank, dtype, zero_infinity, reduction):
    lp = F.log_softmax(logits.to(dtype), dim=2).transpose(0, 1)
    return F.ctc_loss(lp, targets, in_len.to(torch.int64), tgt_len.to(torch.int64), blank=blank, reduction=reduction,
                      zero_infinity=zero_infinity)


def torch_ctc(logits, targets, in_len, tgt_len, blank, dtype):
    """torch's CPU F.ctc_loss in ``dtype`` -> dict(loss_rows [B] = nll / max(L, 1), 0 where infinite; loss = their mean;
    grad [B, T, C] = d(loss)/d(logits); infinite [B] bool)."""
    x = logits.detach().to(dtype).requires_grad_(True)
    loss = _nll(x, targets, in_len, tgt_len, blank, dtype, True, "mean")
    loss.backward()
    with torch.no_grad():
        rows = _nll(x, targets, in_len, tgt_len, blank, dtype, False, "none")
        inf = torch.isinf(rows)
        rows = torch.where(inf, torch.zeros_like(rows), rows / tgt_len.clamp_min(1).to(dtype))
    return {"loss_rows": rows, "loss": loss.detach(), "grad": x.grad, "infinite": inf}


# ---------------------------------------------------------------------------------------- the kernel's arithmetic in f32
def _norm(v, e):
    m, k = torch.frexp(v)
    pos = v > 0
    return torch.where(pos, m, torch.zeros_like(m)), torch.where(pos, e + k, torch.full_like(e, ZERO_E))


def _sum3(a, b, c):
    em = torch.maximum(a[1], torch.maximum(b[1], c[1]))
    sh = lambda x: torch.ldexp(x[0], (x[1] - em).clamp_min(-200))
    return (sh(a) + sh(b)) + sh(c), em


def _shift(x, n):
    """lane s takes lane s - n (n > 0) or s + |n| (n < 0); lanes without a source take zero."""
    m, e = torch.zeros_like(x[0]), torch.full_like(x[1], ZERO_E)
    if n > 0:
        m[n:], e[n:] = x[0][:-n], x[1][:-n]
    else:
        m[:n], e[:n] = x[0][-n:], x[1][-n:]
    return m, e


def kernel_f32(logits, targets, in_len, tgt_len, blank):
    """What csrc/ctc.hip computes, operation for operation where it matters (the summation ORDER of the row sums and of
    the per-class posteriors is torch's, not the wavefront's)."""
    z = logits.to(F32)
    B, T, C = z.shape
    mx = z.max(-1).values
    ex = torch.exp(z - mx[..., None])
    # the off-blank mass against its own maximum, scaled once (under a blank bias of 100 its terms are denormals)
    zo = z.clone()
    zo[..., blank] = -float("inf")
    mxo = zo.max(-1).values
    sum_off = torch.exp(zo - mxo[..., None]).sum(-1) * torch.exp(mxo - mx) if C > 1 else torch.zeros_like(mx)
    total = sum_off + ex[..., blank]
    inv = 1.0 / total
    offm = sum_off * inv
    grad = torch.zeros(B, T, C, dtype=F32)
    rows = torch.zeros(B, dtype=F32)
    infinite = torch.zeros(B, dtype=torch.bool)
    one = lambda S, idx: (torch.zeros(S, dtype=F32).index_fill_(0, torch.tensor(idx), 0.5),
                          torch.full((S,), ZERO_E, dtype=torch.int32).index_fill_(0, torch.tensor(idx), 1))
    zero = lambda S: (torch.zeros(S, dtype=F32), torch.full((S,), ZERO_E, dtype=torch.int32))
    for b in range(B):
        L, Tb = int(tgt_len[b]), int(in_len[b])
        S = 2 * L + 1
        cls = torch.full((S,), blank, dtype=torch.int64)
        cls[1::2] = targets[b, :L]
        x = ((z[b, :Tb][:, cls].double() - mx[b, :Tb, None].double()) - torch.log(total[b, :Tb]).double()[:, None]) * LOG2E
        fl = torch.floor(x)
        pm, pe = torch.exp2((x - fl).to(F32)), fl.to(torch.int32)
        odd = (torch.arange(S) % 2) == 1
        skip_to = odd & (torch.arange(S) >= 3) & (cls != torch.roll(cls, 2))
        skip_from = torch.roll(skip_to, -2) & (torch.arange(S) + 2 < S)
        mask = lambda x, keep: (torch.where(keep, x[0], torch.zeros_like(x[0])),
                                torch.where(keep, x[1], torch.full_like(x[1], ZERO_E)))
        at, alpha = one(S, [0]), []
        for t in range(Tb):
            v, e = _sum3(at, _shift(at, 1), mask(_shift(at, 2), skip_to) if S > 2 else zero(S))
            at = _norm(v * pm[t], e + pe[t])
            alpha.append(at)
        fin = [i for i in (S - 1, S - 2) if i >= 0]
        pv = (at[0][fin[0]:fin[0] + 1], at[1][fin[0]:fin[0] + 1])
        pw = (at[0][fin[1]:fin[1] + 1], at[1][fin[1]:fin[1] + 1]) if len(fin) > 1 else zero(1)
        Pm, Pe = _norm(*_sum3(pv, pw, zero(1)))
        if not float(Pm) > 0:
            infinite[b] = True
            continue
        rows[b] = -(Pe.to(F32) * 0.69314718055994531 + torch.log(Pm))[0] / max(L, 1)
        bt = one(S, fin)
        k = 1.0 / (B * max(L, 1))
        for t in reversed(range(Tb)):
            a = alpha[t]
            e = (a[1] + bt[1] - Pe).clamp(-300, 300)
            gam = torch.where((a[0] > 0) & (bt[0] > 0), torch.ldexp(a[0] * bt[0] / Pm, e), torch.zeros(S))
            gb, gl = gam[0::2].sum(), gam[1::2].sum()
            p = ex[b, t] * inv[b, t]
            g = p.clone()
            for c in torch.unique(cls[1::2]).tolist():
                g[c] = p[c] - gam[1::2][cls[1::2] == c].sum()
            g[blank] = gl - offm[b, t] if p[blank] > 0.5 else p[blank] - gb
            grad[b, t] = g * k
            full = (bt[0] * pm[t], torch.where(bt[0] > 0, bt[1] + pe[t], torch.full_like(bt[1], ZERO_E)))
            bt = _norm(*_sum3(full, _shift(full, -1), mask(_shift(full, -2), skip_from) if S > 2 else zero(S)))
    return {"loss_rows": rows, "loss": rows.mean(), "grad": grad, "infinite": infinite}


def ctc_ref(logits, targets, in_len, tgt_len, blank=0, dtype=F64):
    """float64: the reference (torch's F.ctc_loss on log_softmax, autograd back to the logits).  float32: a restatement of
    the kernel's own arithmetic.  logits [B, T, C]; targets [B, Lmax] int64 (classes, blank excluded)."""
    if dtype == F64:
        return torch_ctc(logits, targets, in_len, tgt_len, blank, F64)
    return kernel_f32(logits, targets, in_len, tgt_len, blank)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(logits [B, T, C] f32, ldc, targets [B, Lmax] int64, in_len, tgt_len int32, blank, infinite (tuple), ref)."""
    B, T, C, tl, il, bias, tg, infinite, ldc = _SPECS[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 1000 * C + T)
    logits = torch.randn(B, T, C, generator=g, dtype=F64) * 1.5
    logits[..., 0] += bias
    Lmax = max(max(tl), 1)
    if tg is None:
        targets = torch.randint(1, C, (B, Lmax), generator=g)
    else:
        targets = torch.tensor(tg, dtype=torch.int64)
    for b, L in enumerate(tl):
        targets[b, L:] = 1          # the padding holds a valid class: nothing may depend on it
    c = {"name": name, "logits": logits.float(), "ldc": ldc or C, "targets": targets, "blank": 0, "infinite": infinite,
         "in_len": torch.tensor(il if il is not None else [T] * B, dtype=torch.int32),
         "tgt_len": torch.tensor(tl, dtype=torch.int32)}
    c["ref"] = ctc_ref(c["logits"], targets, c["in_len"], c["tgt_len"], 0, F64)
    got = tuple(i for i in range(B) if bool(c["ref"]["infinite"][i]))
    assert got == tuple(infinite), f"{name}: utterances {got} are infeasible in float64, {infinite} were meant to be"
    assert bool(torch.isfinite(c["ref"]["loss_rows"]).all())
    return c


def per_utterance_rel_l2(got, ref):
    """Largest rel-L2 over the utterances' [T, C] blocks (utterances whose reference gradient is zero are left out)."""
    got, ref = got.detach().cpu().to(F64), ref.to(F64)
    worst = 0.0
    for b in range(ref.shape[0]):
        n = float(ref[b].norm())
        if n > 0:
            worst = max(worst, float((got[b] - ref[b]).norm()) / n)
    return worst


@functools.lru_cache(maxsize=None)
def ref_f32_error(name):
    """Gradient error of torch's f32 CPU F.ctc_loss (the reference's arithmetic) against float64 on this case."""
    c = case(name)
    f32 = torch_ctc(c["logits"], c["targets"], c["in_len"], c["tgt_len"], c["blank"], F32)
    return per_utterance_rel_l2(f32["grad"], c["ref"]["grad"])


def grad_bound(name):
    return max(GRAD_TOL, 2.0 * ref_f32_error(name))


def errors(c, loss_rows, grad, k=1.0):
    """Measured figures of one evaluation against the case's float64 reference (k = what the gradient was scaled by):
    loss rows relative to max(1, |ref|), the gradient's largest per-utterance rel-L2, and whether everything that must be
    an exact zero is one (infeasible utterances, frames past an utterance's end)."""
    ref = c["ref"]
    lr = loss_rows.detach().cpu().to(F64)
    out = {"loss_rows": float(((lr - ref["loss_rows"]).abs() / ref["loss_rows"].abs().clamp_min(1)).max())}
    if grad is not None:
        gd = grad.detach().cpu().to(F64) / k
        out["grad"] = per_utterance_rel_l2(gd, ref["grad"])
        ok = True
        for b in range(gd.shape[0]):
            if b in c["infinite"]:
                ok = ok and bool((gd[b] == 0).all())
            ok = ok and bool((gd[b, int(c["in_len"][b]):] == 0).all())
        out["zeros_ok"] = ok
        live = [gd[b, :int(c["in_len"][b])].sum(-1).abs().max() for b in range(gd.shape[0])
                if b not in c["infinite"] and int(c["in_len"][b]) > 0]
        out["row_sum"] = float(torch.stack(live).max()) * float(gd.shape[0]) if live else 0.0
    return out


def within_bounds(name, e):
    return e["loss_rows"] < LOSS_TOL and e.get("grad", 0.0) <= grad_bound(name) and e.get("zeros_ok", True)
