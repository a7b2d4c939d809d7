"""Cases and the float64 reference of the triplet head (csrc/heads.hip triplet_row_kernel / triplet_grad_kernel), shared
by tests/test_triplet_cpu.py, tests/test_triplet_gpu.py and tools/triplet_bench.py.  No GPU and no ``ops`` import here:
plain torch on the CPU.

The reference restates ref: src/optim/loss/triplet_loss.py:21-107 -> F.triplet_margin_loss (p = 2, eps = 1e-6 added to
the difference, no swap, mean) with EXPLICIT positive / negative rows; tests/test_triplet_cpu.py ties it to the goldens
the reference itself produced (tests/golden/g21_triplet.npz).

Every case keeps |margin + d_ap - d_an| > HINGE_GAP for every row in float64: a hinge closer to zero than that may sit
on the other side in f32, and then loss and gradient differ by a whole row, not by rounding."""
import functools
import random

import torch

F32, F64 = torch.float32, torch.float64
EPS = 1e-6
HINGE_GAP = 1e-3
MARGINS = (1.0, 0.3)
# (B, E): smallest legal batch; a scalar tail of the 16-byte path; one wave; both sides of a 256-thread trip; several
# trips; the real head (66 utterances, mean+std of wav2vec2-base)
SHAPES = [(4, 1), (4, 5), (6, 64), (12, 255), (12, 256), (12, 257), (8, 3840), (66, 1536)]
LOSS_TOL, GRAD_TOL = 2e-5, 1e-5          # the bounds tests/test_heads_gpu.py holds the f32 head kernels to


def triplet_ref(emb, pos, neg, margin, coef=1.0, loss_scale=1.0, dtype=F64):
    """-> dict(d_ap, d_an, loss_rows, loss, active, demb) in ``dtype`` (float64: the reference; float32: a restatement of
    the kernel's arithmetic on the CPU).  demb = coef * loss_scale / B * d(sum of loss rows)/d(emb); a row is active
    when margin + d_ap - d_an >= 0 (torch's clamp_min backward)."""
    x = emb.to(dtype)
    pos, neg = torch.as_tensor(pos, dtype=torch.int64), torch.as_tensor(neg, dtype=torch.int64)
    B = x.shape[0]
    vap, van = x - x[pos] + EPS, x - x[neg] + EPS
    d_ap, d_an = vap.pow(2).sum(1).sqrt(), van.pow(2).sum(1).sqrt()
    v = margin + d_ap - d_an
    active = v >= 0
    g = torch.where(active, torch.full_like(v, coef * loss_scale / B), torch.zeros_like(v))
    unit = lambda vec, d: torch.where(d[:, None] > 0, vec / d[:, None].clamp_min(1e-300), torch.zeros_like(vec))
    uap, uan = unit(vap, d_ap) * g[:, None], unit(van, d_an) * g[:, None]
    demb = uap - uan
    demb.index_add_(0, pos, -uap)
    demb.index_add_(0, neg, uan)
    rows = v.clamp_min(0)
    return {"d_ap": d_ap, "d_an": d_an, "loss_rows": rows, "loss": rows.mean(), "active": active, "demb": demb, "v": v}


def draw(labels, rng):
    """One (pos, neg) per row with a private generator (the package's sample_triplets is tested on its own)."""
    pos, neg = [], []
    for i, l in enumerate(labels):
        pos.append(rng.choice([j for j, m in enumerate(labels) if m == l and j != i]))
        neg.append(rng.choice([j for j, m in enumerate(labels) if m != l]))
    return pos, neg


def speaker_embeddings(labels, E, seed, sep=0.7, spread=(0.2, 1.0)):
    """[B, E] f32: a centroid per speaker (pairwise distance ~ sep * sqrt(2)) plus per-row noise of a per-row size."""
    g = torch.Generator().manual_seed(seed)
    n_spk = max(labels) + 1
    cent = torch.randn(n_spk, E, generator=g, dtype=F64) * (sep / E ** 0.5)
    sigma = spread[0] + (spread[1] - spread[0]) * torch.rand(len(labels), 1, generator=g, dtype=F64)
    return (cent[torch.tensor(labels)] + torch.randn(len(labels), E, generator=g, dtype=F64) * sigma / E ** 0.5).float()


def check_gap(emb, pos, neg, margins=MARGINS):
    for m in margins:
        gap = float(triplet_ref(emb, pos, neg, m)["v"].abs().min())
        assert gap > HINGE_GAP, f"hinge {gap:.2e} from zero at margin {m}: choose another seed for this case"


@functools.lru_cache(maxsize=None)
def shape_case(B, E):
    """-> (emb [B, E] f32, pos, neg): B / 2 speakers with two rows each (B = 66: 22 speakers of three)."""
    per = 3 if B % 3 == 0 and B > 12 else 2
    labels = [i // per for i in range(B)]
    random.Random(B * 7919 + E).shuffle(labels)
    emb = speaker_embeddings(labels, E, B + E)
    pos, neg = draw(labels, random.Random(0))
    check_gap(emb, pos, neg)
    return emb, pos, neg


FAN_B, FAN_E = 12, 48
FAN_LABELS = [0] * 4 + [1] * 4 + [2] * 4


@functools.lru_cache(maxsize=None)
def fan_in_case():
    """Row 0 is the positive of every other anchor of its speaker (rows 1-3) and the negative of every anchor of the
    other speakers (rows 4-11): 11 terms land on it besides its own.  Row 11 is named by nobody.  At margin 1.0 every
    row is active, at 0.3 some are and some are not (asserted)."""
    pos = [1, 0, 0, 0, 5, 6, 7, 4, 9, 10, 8, 8]
    neg = [4, 5, 6, 7, 0, 0, 0, 0, 0, 0, 0, 0]
    assert 11 not in pos + neg and pos.count(0) == 3 and neg.count(0) == 8
    emb = speaker_embeddings(FAN_LABELS, FAN_E, 4242, sep=0.6, spread=(0.1, 1.2))
    check_gap(emb, pos, neg)
    a1, a3 = triplet_ref(emb, pos, neg, 1.0)["active"], triplet_ref(emb, pos, neg, 0.3)["active"]
    assert bool(a1.all()) and 0 < int(a3.sum()) < FAN_B
    return emb, pos, neg


@functools.lru_cache(maxsize=None)
def all_inactive_case():
    """Negatives far away (speaker centroids 50 apart): no row is active, the loss and the gradient are exact zeros."""
    emb = speaker_embeddings(FAN_LABELS, FAN_E, 77, sep=50.0)
    pos, neg = draw(FAN_LABELS, random.Random(5))
    assert not bool(triplet_ref(emb, pos, neg, 1.0)["active"].any())
    check_gap(emb, pos, neg)
    return emb, pos, neg


def errors(got, ref, k=1.0):
    """Measured figures of one launch against the float64 reference (k = what the gradient was scaled by): loss rows and
    mean relative to max(1, |ref|); d_ap, d_an and demb as the largest per-row rel-L2 (rows whose reference gradient is
    exactly zero must be exactly zero: reported as ``zero_rows_ok``)."""
    f = lambda t: t.detach().cpu().to(F64)
    out = {"loss_rows": float(((f(got["loss_rows"]) - ref["loss_rows"]).abs() / ref["loss_rows"].abs().clamp_min(1)).max())}
    if "loss" in got:
        out["loss"] = float((f(got["loss"]) - ref["loss"]).abs() / ref["loss"].abs().clamp_min(1))
    for n in ("d_ap", "d_an"):
        out[n] = float(((f(got[n]) - ref[n]).abs() / ref[n].abs().clamp_min(1e-300)).max())
    if got.get("demb") is not None:
        gd, rd = f(got["demb"]), k * ref["demb"]
        zero = rd.abs().sum(1) == 0
        out["zero_rows_ok"] = bool((gd[zero] == 0).all())
        nz = ~zero
        out["demb"] = float(((gd[nz] - rd[nz]).norm(dim=1) / rd[nz].norm(dim=1)).max()) if bool(nz.any()) else 0.0
    return out


def within_bounds(e):
    return (e["loss_rows"] < LOSS_TOL and e.get("loss", 0.0) < LOSS_TOL and e["d_ap"] < GRAD_TOL and e["d_an"] < GRAD_TOL
            and e.get("demb", 0.0) < GRAD_TOL and e.get("zero_rows_ok", True))


def sample_stream(make_sample, n_speakers, per_speaker, seq, seed):
    """The seeded sample stream of tests/golden/make_data_goldens.py (``stream``): speaker-grouped runs of ``seq`` samples,
    as the reference's shard writer lays them out.  ``make_sample``: the sample class (the reference's when the goldens
    are made, the package's when they are checked); this is the one copy both sides of the triplet goldens use."""
    rng = random.Random(seed)
    runs = [(spk, r) for spk in range(n_speakers) for r in range(per_speaker // seq)]
    rng.shuffle(runs)
    for spk, r in runs:
        for j in range(seq):
            yield make_sample(key=f"id{spk:03d}/vid{r:02d}/{j:05d}", ground_truth=spk,
                              network_input=torch.full((1, 8), float(spk * 1000 + r * 10 + j)), side_info=None)
