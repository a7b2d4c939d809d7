"""Cases and references of the long-target CTC loss (csrc/ctc_long.hip), shared by tests/test_ctc_long_cpu.py,
tests/test_ctc_long_gpu.py and tools/ctc_long_bench.py.  Plain torch on the CPU; the only thing taken from the library
is the number of frames its lattice kernel stages in LDS per chunk (``ops.ctc_long_stage_frames``), around which the
``stage_*`` cases put their utterance lengths.

The reference is that of tests/ctc_cases.py: ``torch_ctc`` in float64 (torch's F.ctc_loss on log_softmax, autograd back to
the logits).  ``kernel_f32_pairs`` restates the kernel's arithmetic in f32 in the kernel's own layout: "thread" j owns the
pair (blank state 2j, label state 2j + 1), the label state of thread j - 1 is the one value that crosses threads forward,
the blank and label of thread j + 1 the two that cross backward; repeated labels are summed onto their class in ascending
order.  The bounds are the project's own (tests/ctc_cases.py): loss rows ``LOSS_TOL``; gradient, per-utterance rel-L2,
``max(GRAD_TOL, 2 x the error of torch's f32 CPU F.ctc_loss on the same inputs)``.

Spec: the nine fields of ``ctc_cases._SPECS`` -- (B, T, C incl. blank, target lengths, input lengths or None = T, blank
bias, explicit targets or None, utterances whose loss is infinite, ldc or None = C) -- and the blank (default 0).  A T
given as ("stage", W, k, d) is k x (frames staged per chunk at target width W) + d."""
import functools

import torch

import ctc_cases as CC
from ctc_cases import F32, F64, GRAD_TOL, LOG2E, LOSS_TOL, ZERO_E, errors, per_utterance_rel_l2, torch_ctc  # noqa: F401

MAX_TARGET = 1023
STAGE_W = 32          # the target width of the stage_* cases

_PAIRS = [[5, 5, 6, 6] * 15]          # A A B B A A ...: 60 labels, 30 of them repeats of their neighbour

_SPECS = {
    # the first two widths the short form refuses (65 and 67 states)
    "w32": (2, 70, 32, [32, 20], None, 0.0, None, (), None),
    "w33": (2, 72, 32, [33, 5], None, 0.0, None, (), None),
    # the wave edge of the pair layout (thread 63 | 64)
    "l63": (1, 136, 32, [63], None, 0.0, None, (), None),
    "l64": (1, 138, 32, [64], None, 0.0, None, (), None),
    "l65": (1, 140, 32, [65], None, 0.0, None, (), None),
    # workgroup-size steps: 256 | 512 threads, 512 | 1024 threads
    "l255": (1, 300, 32, [255], None, 0.0, None, (), None),
    "l256": (1, 301, 32, [256], None, 0.0, None, (), None),
    "l257": (1, 302, 32, [257], None, 0.0, None, (), None),
    "l511": (1, 580, 32, [511], None, 0.0, None, (), None),
    "l512": (1, 581, 32, [512], None, 0.0, None, (), None),
    # the full lattice: 2047 states, 1024 threads
    "l1023": (1, 1100, 32, [1023], None, 0.0, None, (), None),
    # mixed lengths in one batch; 32 labels in 20 frames and 1 label in 0 frames are infeasible
    "mixed_long": (4, 1100, 32, [1023, 32, 1, 0], [1100, 20, 0, 700], 0.0, None, (1, 2), None),
    # forty copies of one label need 79 frames
    "forty_same_79": (1, 79, 32, [40], None, 0.0, [[7] * 40], (), None),
    "forty_same_78": (1, 78, 32, [40], None, 0.0, [[7] * 40], (0,), None),
    # letter pairs: every second label repeats its neighbour, two classes carry 30 posteriors each
    "pairs": (1, 100, 32, [60], None, 0.0, _PAIRS, (), None),
    # T around the frames staged per LDS chunk, and two chunks plus one
    "stage_m1": (2, ("stage", STAGE_W, 1, -1), 32, [32, 9], None, 0.0, None, (), None),
    "stage_0": (2, ("stage", STAGE_W, 1, 0), 32, [32, 9], None, 0.0, None, (), None),
    "stage_p1": (2, ("stage", STAGE_W, 1, 1), 32, [32, 9], None, 0.0, None, (), None),
    "stage_2p1": (2, ("stage", STAGE_W, 2, 1), 32, [32, 9], None, 0.0, None, (), None),
    # the speech head's rows: C = 32 in rows of 32; C = 29 in rows of 32 whose padding holds NaN
    "c32": (2, 50, 32, [33, 12], None, 0.0, None, (), 32),
    "c29_nan_padding": (2, 50, 29, [33, 10], None, 0.0, None, (), 32),
    # the generic-C path under a wide target
    "c5995_wide": (2, 60, 5995, [40, 33], None, 0.0, None, (), 6000),
    "blank3": (2, 60, 32, [35, 3], None, 0.0, None, (), None, 3),
    # the reference's blank bias (what mixed_bias100 is to the short form)
    "wide_bias100": (4, 149, 64, [40, 7, 1, 0], None, 100.0, None, (), None),
}
CASES = tuple(_SPECS)


def stage_frames(width):
    from w2v2_speaker_amd import ops
    return ops.ctc_long_stage_frames(width)


# ---------------------------------------------------------------------------------------- the kernel's arithmetic in f32
def _mask(x, keep):
    return torch.where(keep, x[0], torch.zeros_like(x[0])), torch.where(keep, x[1], torch.full_like(x[1], ZERO_E))


def _zero(n):
    return torch.zeros(n, dtype=F32), torch.full((n,), ZERO_E, dtype=torch.int32)


def _one(n, idx):
    m, e = _zero(n)
    for i in idx:
        if 0 <= i < n:
            m[i], e[i] = 0.5, 1
    return m, e


def kernel_f32_pairs(logits, targets, in_len, tgt_len, blank):
    """What csrc/ctc_long.hip computes, in its pair layout (the summation ORDER of the row sums and of the two sums of
    posteriors over the states is torch's, not the workgroup's)."""
    z = logits.to(F32)
    B, T, C = z.shape
    mx = z.max(-1).values
    ex = torch.exp(z - mx[..., None])
    zo = z.clone()
    zo[..., blank] = -float("inf")
    mxo = zo.max(-1).values
    sum_off = torch.exp(zo - mxo[..., None]).sum(-1) * torch.exp(mxo - mx)
    total = sum_off + ex[..., blank]
    inv = 1.0 / total
    offm = sum_off * inv
    grad = torch.zeros(B, T, C, dtype=F32)
    rows = torch.zeros(B, dtype=F32)
    infinite = torch.zeros(B, dtype=torch.bool)
    for b in range(B):
        L, Tb = int(tgt_len[b]), int(in_len[b])
        n = L + 1                                   # thread j: blank 2j, label 2j + 1 (none in thread L)
        cls = targets[b, :L].to(torch.int64)
        slots = torch.cat([torch.tensor([blank]), cls])
        x = ((z[b, :Tb][:, slots].double() - mx[b, :Tb, None].double()) - torch.log(total[b, :Tb]).double()[:, None]) * LOG2E
        fl = torch.floor(x)
        pm, pe = torch.exp2((x - fl).to(F32)), fl.to(torch.int32)
        pml = torch.cat([pm[:, 1:], torch.ones(Tb, 1, dtype=F32)], 1)          # thread j's label slot (thread L: unused)
        pel = torch.cat([pe[:, 1:], torch.zeros(Tb, 1, dtype=torch.int32)], 1)
        j = torch.arange(n)
        live_l = j < L
        clsj = torch.cat([cls, torch.tensor([-1])])
        skip_to = (j >= 1) & live_l & (clsj != torch.roll(clsj, 1))
        skip_from = (j + 1 < L) & (torch.roll(clsj, -1) != clsj)
        ab, al = _one(n, [0]), _zero(n)
        alpha = []
        for t in range(Tb):
            pl = CC._shift(al, 1)
            vb = CC._sum3(ab, pl, _zero(n))
            vl = CC._sum3(al, ab, _mask(pl, skip_to))
            ab = CC._norm(vb[0] * pm[t, 0], vb[1] + pe[t, 0])
            al = _mask(CC._norm(vl[0] * pml[t], vl[1] + pel[t]), live_l)
            alpha.append((ab, al))
        fin_b = (ab[0][L:L + 1], ab[1][L:L + 1])
        fin_l = (al[0][L - 1:L], al[1][L - 1:L]) if L >= 1 else _zero(1)
        Pm, Pe = CC._norm(*CC._sum3(fin_b, fin_l, _zero(1)))
        if not float(Pm) > 0:
            infinite[b] = True
            continue
        rows[b] = -(Pe.to(F32) * 0.69314718055994531 + torch.log(Pm))[0] / max(L, 1)
        bb, bl = _one(n, [L]), _one(n, [L - 1])
        k = 1.0 / (B * max(L, 1))

        def post(a, bt):
            e = (a[1] + bt[1] - Pe).clamp(-300, 300)
            return torch.where((a[0] > 0) & (bt[0] > 0), torch.ldexp(a[0] * bt[0] / Pm, e), torch.zeros(n))

        for t in reversed(range(Tb)):
            gam_b, gam_l = post(alpha[t][0], bb), post(alpha[t][1], bl)
            gb, gl = gam_b.sum(), gam_l.sum()
            p = ex[b, t] * inv[b, t]
            occ = torch.zeros(C, dtype=F32).index_add_(0, cls, gam_l[:L])      # ascending label order per class
            g = p - occ
            g[blank] = gl - offm[b, t] if p[blank] > 0.5 else p[blank] - gb
            grad[b, t] = g * k
            fb = (bb[0] * pm[t, 0], torch.where(bb[0] > 0, bb[1] + pe[t, 0], torch.full_like(bb[1], ZERO_E)))
            fl_ = _mask((bl[0] * pml[t], torch.where(bl[0] > 0, bl[1] + pel[t], torch.full_like(bl[1], ZERO_E))), live_l)
            nb, nl = CC._shift(fb, -1), CC._shift(fl_, -1)
            bb = CC._norm(*CC._sum3(fb, fl_, _zero(n)))
            bl = _mask(CC._norm(*CC._sum3(fl_, nb, _mask(nl, skip_from))), live_l)
    return {"loss_rows": rows, "loss": rows.mean(), "grad": grad, "infinite": infinite}


def _frames(T):
    if isinstance(T, tuple):
        _, width, k, d = T
        return k * stage_frames(width) + d
    return T


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(logits [B, T, C] f32, ldc, targets [B, Lmax] int64, in_len, tgt_len int32, blank, infinite (tuple), ref)."""
    spec = _SPECS[name]
    B, T, C, tl, il, bias, tg, infinite, ldc = spec[:9]
    blank = spec[9] if len(spec) > 9 else 0
    T = _frames(T)
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 1000 * C + T)
    logits = torch.randn(B, T, C, generator=g, dtype=F64) * 1.5
    logits[..., blank] += bias
    Lmax = max(max(tl), 1)
    if tg is None:
        targets = torch.randint(0, C - 1, (B, Lmax), generator=g)
        targets = targets + (targets >= blank).to(torch.int64)            # every class but the blank
    else:
        targets = torch.tensor(tg, dtype=torch.int64)
    pad = 1 if blank != 1 else 2
    for b, L in enumerate(tl):
        targets[b, L:] = pad        # the padding holds a valid class: nothing may depend on it
    c = {"name": name, "logits": logits.float(), "ldc": ldc or C, "targets": targets, "blank": blank, "infinite": infinite,
         "in_len": torch.tensor(il if il is not None else [T] * B, dtype=torch.int32),
         "tgt_len": torch.tensor(tl, dtype=torch.int32)}
    c["ref"] = torch_ctc(c["logits"], targets, c["in_len"], c["tgt_len"], blank, F64)
    got = tuple(i for i in range(B) if bool(c["ref"]["infinite"][i]))
    assert got == tuple(infinite), f"{name}: utterances {got} are infeasible in float64, {infinite} were meant to be"
    assert bool(torch.isfinite(c["ref"]["loss_rows"]).all()) and bool(torch.isfinite(c["ref"]["grad"]).all())
    return c


@functools.lru_cache(maxsize=None)
def ref_f32_error(name):
    """Gradient error of torch's f32 CPU F.ctc_loss (the reference's arithmetic) against float64 on this case."""
    c = case(name)
    f32 = torch_ctc(c["logits"], c["targets"], c["in_len"], c["tgt_len"], c["blank"], F32)
    return per_utterance_rel_l2(f32["grad"], c["ref"]["grad"])


def grad_bound(name):
    return max(GRAD_TOL, 2.0 * ref_f32_error(name))


def within_bounds(name, e):
    return e["loss_rows"] < LOSS_TOL and e.get("grad", 0.0) <= grad_bound(name) and e.get("zeros_ok", True)
