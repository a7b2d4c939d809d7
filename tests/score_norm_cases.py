"""Cases of the device score normalisation (csrc/score_norm.hip) with their float64 references and the HOST path's own
f32 result on the CPU.  No GPU and no ``ops`` import here.  The reference project has no score normalisation: the
definition is the one in include/w2v2_hip.h ("score normalisation") and the oracle is float64 numpy, below.

Bounds, by the rule of tests/scoring_cases.py:
  mu, sd            O(1) quantities: max(2 x the host f32 path's error against float64 on the same inputs, 2^-22).
  normalised score  divides by sd, so the floor is the propagated one, per trial, at the float64 values: with f = 2^-22,
                    floor_z = the mode's weight x sum over its sides of f (2 + |c - mu| / sd) / sd; the bound is
                    max(2 x the host error of the case, floor_z).
  topk_stats        on a given S has no product in front of it: the float64 result rounded to f32, within 2^-22 relative
                    to max(|mu|, sd).
  a priori          the accumulation order of an f32 product may put mu or sd of an end-to-end case outside the 2 x rule
                    (torch's CPU matmul is one f32 order, the MFMA another; neither is the better one).  That stage may
                    then take the a-priori bound of an f32 dot product of unit vectors, D 2^-24 (APRIORI); a test that
                    uses it says so in its printed line.
Data: a few cluster centres plus noise, so that the cohort cosines of a row have spread (sd between 0.008 and 0.26 on
these cases, host-path errors of 1e-8 to 2e-7 on mu and sd)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import scoring_cases as SC
from w2v2_speaker_amd.evaluation.speaker.cosine_distance import (CosineDistanceEvaluator, EmbeddingSample, center_batch,
                                                                 cohort_stats_host, length_norm_batch)

FLOOR = 2.0 ** -22
bound = SC.bound
padded = SC.padded
MODES = ("z", "t", "s")
MODE_WEIGHTS = {"z": (1.0, 0.0), "t": (0.0, 1.0), "s": (0.5, 0.5)}


def apriori(D: int) -> float:
    """|error| of an f32 dot product of two unit vectors of length D, whatever the order of the adds."""
    return D * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ float64 references
def cohort_cos_ref(bank, cohort, mean=None, std=None, length_norm=False):
    """Steps 1 and 2: S [N, M] float64."""
    u, c = SC.transform_ref(bank, mean, std, length_norm), SC.transform_ref(cohort, mean, std, length_norm)
    return (u @ c.T) / (np.maximum(np.linalg.norm(u, axis=1), 1e-8)[:, None] * np.maximum(np.linalg.norm(c, axis=1), 1e-8)[None, :])


def topk_stats_ref(S, K: int):
    """Step 3 per row in float64: the K largest values as a multiset (np.sort ties -0.0 with +0.0), their mean and unbiased
    std; a row with a NaN gives NaN."""
    S = np.asarray(S, dtype=np.float64)
    mu, sd = np.empty(S.shape[0]), np.empty(S.shape[0])
    for r, row in enumerate(S):
        if np.isnan(row).any():
            mu[r] = sd[r] = np.nan
            continue
        top = np.sort(row)[::-1][:K]
        mu[r], sd[r] = top.mean(), top.std(ddof=1)
    return mu, sd


def cohort_stats_ref(bank, cohort, K, mean=None, std=None, length_norm=False):
    return topk_stats_ref(cohort_cos_ref(bank, cohort, mean, std, length_norm), K)


def norm_scores_ref(cos, pairs, mu, sd, mode: str):
    """Step 4 in float64."""
    cos, mu, sd = (np.asarray(a, dtype=np.float64) for a in (cos, mu, sd))
    e, t = np.asarray(pairs).reshape(-1, 2).T
    ze, zt = (cos - mu[e]) / (sd[e] + 1e-12), (cos - mu[t]) / (sd[t] + 1e-12)
    we, wt = MODE_WEIGHTS[mode]
    return ze if mode == "z" else (zt if mode == "t" else we * ze + wt * zt)


def floor_z(cos, pairs, mu, sd, mode: str, f_stats: float = FLOOR):
    """The propagated floor of the normalised score, per trial, at the float64 values: z = (c - mu) / sd moves by
    (dc + dmu + |z| dsd) / sd; with dc = f = 2^-22 and dmu = dsd = ``f_stats`` that is (f + f_stats (1 + |z|)) / sd per
    side -- f (2 + |c - mu| / sd) / sd when the statistics keep the floor f, and the same expression with D 2^-24 in their
    place when the cohort product takes its a-priori bound."""
    cos, mu, sd = (np.asarray(a, dtype=np.float64) for a in (cos, mu, sd))
    e, t = np.asarray(pairs).reshape(-1, 2).T
    side = lambda i: (FLOOR + f_stats * (1.0 + np.abs(cos - mu[i]) / sd[i])) / sd[i]
    we, wt = MODE_WEIGHTS[mode]
    return we * side(e) + wt * side(t)


def segment_mean_ref(bank, labels):
    """float64 mean per label, labels in sorted order."""
    labels = np.asarray(labels)
    x = np.asarray(bank, dtype=np.float64)
    return np.stack([x[labels == s].mean(axis=0) for s in sorted(set(labels.tolist()))])


# ------------------------------------------------------------------------------------------------ the host f32 path
def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def host_cohort_stats(bank, cohort, K, mean=None, std=None, length_norm=False):
    """What the host evaluator computes for ``score_norm``: plain torch f32 on the CPU (matmul, topk, mean, std)."""
    b, c = _t(bank), _t(cohort)
    if mean is not None:
        b, c = center_batch(b, _t(mean), _t(std)), center_batch(c, _t(mean), _t(std))
    if length_norm:
        b, c = length_norm_batch(b), length_norm_batch(c)
    mu, sd = cohort_stats_host(b, c, K)
    return mu.numpy(), sd.numpy()


def host_norm_scores(bank, cohort, pairs, K, mode, mean=None, std=None, length_norm=False):
    """CosineDistanceEvaluator._compute_normalised_scores on the CPU."""
    ev = CosineDistanceEvaluator(mean is not None, length_norm, 0)
    if mean is not None:
        ev.mean, ev.std = _t(mean), _t(std)
    rows = [EmbeddingSample(str(i), _t(r)) for i, r in enumerate(bank)]
    sn = SimpleNamespace(cohort=_t(cohort), top_k=K, mode=mode)
    return np.array(ev._compute_normalised_scores([(rows[i], rows[j]) for i, j in np.asarray(pairs).reshape(-1, 2)], sn))


# ------------------------------------------------------------------------------------------------ data
def cluster_rows(rng, n: int, D: int, centres, noise: float = 0.9):
    """n rows around randomly chosen cluster centres: cosines against a cohort drawn the same way have spread."""
    pick = rng.integers(0, len(centres), n)
    return (centres[pick] + noise * rng.standard_normal((n, D))).astype(np.float32)


COHORT_SHAPES = ((7, 5, 4, 2), (67, 257, 192, 20), (33, 300, 1536, 300))      # (N, M, D, K)
MIDDLE = COHORT_SHAPES[1]
CENTRE_MODES = SC.PAIR_MODES                                                  # (centre, length norm)


@functools.lru_cache(maxsize=None)
def cohort_case(N: int, M: int, D: int, K: int, centre: bool = False, length_norm: bool = False):
    """-> dict: bank [N, D], cohort [M, D], mean / std (None without centring), the float64 mu / sd, the host f32 path's
    and the bounds."""
    rng = np.random.default_rng(7000 + 13 * N + D + 2 * int(centre) + int(length_norm))
    centres = rng.standard_normal((5, D)) + 0.3
    bank, cohort = cluster_rows(rng, N, D, centres), cluster_rows(rng, M, D, centres)
    mean = std = None
    if centre:
        m, s = SC.stats_ref(np.concatenate([bank, cohort]))
        mean, std = m.astype(np.float32), s.astype(np.float32)
    mu, sd = cohort_stats_ref(bank, cohort, K, mean, std, length_norm)
    hmu, hsd = host_cohort_stats(bank, cohort, K, mean, std, length_norm)
    return {"bank": bank, "cohort": cohort, "K": K, "mean": mean, "std": std, "length_norm": length_norm, "mu": mu, "sd": sd,
            "host_mu": hmu, "host_sd": hsd, "bound_mu": bound(np.abs(hmu - mu).max()), "bound_sd": bound(np.abs(hsd - sd).max()),
            "apriori": apriori(D)}


@functools.lru_cache(maxsize=None)
def trials_case(mode: str):
    """The middle cohort case with every pair of its first 12 rows as trials: float64 normalised scores, the host path's,
    and the per-trial bound."""
    N, M, D, K = MIDDLE
    c = cohort_case(N, M, D, K)
    pairs = np.array([(i, j) for i in range(12) for j in range(12) if i != j], dtype=np.int32)
    cos, _ = SC.score_pairs_ref(c["bank"], pairs)
    ref = norm_scores_ref(cos, pairs, c["mu"], c["sd"], mode)
    host = host_norm_scores(c["bank"], c["cohort"], pairs, K, mode)
    return {"case": c, "pairs": pairs, "cos": cos, "score": ref, "host_score": host,
            "bound": np.maximum(2.0 * np.abs(host - ref).max(), floor_z(cos, pairs, c["mu"], c["sd"], mode))}


# ------------------------------------------------------------------------------------------------ topk_stats on hand-made S
TOPK_M = (2, 5, 63, 64, 65, 255, 256, 257, 1025)


def topk_ks(M: int):
    return sorted({k for k in (2, 3, M - 1, M) if 2 <= k <= M})


SPECIAL_ROWS = ("all_equal", "three_values", "signed_zeros", "descending", "ascending", "plain")


def topk_rows(M: int, R: int, seed: int = 0):
    """R rows of M f32 values: the special rows in turn (row r is SPECIAL_ROWS[r % 6])."""
    rng = np.random.default_rng(9000 + 31 * M + R + seed)
    S = np.empty((R, M), dtype=np.float32)
    for r in range(R):
        kind = SPECIAL_ROWS[r % len(SPECIAL_ROWS)]
        if kind == "all_equal":
            S[r] = np.float32(0.3172)
        elif kind == "three_values":          # long tie groups: the K-th boundary falls inside one for most K
            S[r] = rng.choice(np.array([-0.25, 0.125, 0.7], dtype=np.float32), M)
        elif kind == "signed_zeros":
            S[r] = rng.choice(np.array([-0.0, 0.0, -0.5, 0.5], dtype=np.float32), M)
            S[r, :2] = (-0.0, 0.0)
        elif kind == "descending":
            S[r] = np.linspace(0.9, -0.9, M, dtype=np.float32)
        elif kind == "ascending":
            S[r] = np.linspace(-0.9, 0.9, M, dtype=np.float32)
        else:
            S[r] = (0.2 + 0.15 * rng.standard_normal(M)).astype(np.float32)
    return S


def topk_within(mu, sd, ref_mu, ref_sd):
    """max over rows of the error against the float64 result rounded to f32, relative to max(|mu|, sd)."""
    scale = np.maximum(np.abs(ref_mu), ref_sd)
    scale = np.where(scale > 0, scale, 1.0)
    em = np.abs(mu.astype(np.float64) - ref_mu.astype(np.float32).astype(np.float64)) / scale
    es = np.abs(sd.astype(np.float64) - ref_sd.astype(np.float32).astype(np.float64)) / scale
    return float(em.max()), float(es.max())


# ------------------------------------------------------------------------------------------------ the g12 trial set
G12_TOP_K = 4


@functools.lru_cache(maxsize=None)
def g12_norm_case(mode: str = "s"):
    """The 496 trials of g12 normalised with the speaker-mean cohort of the same 32 rows: float64, host f32, bound.
    An ill-conditioned case on purpose (it is the reference evaluator's own embeddings): every cohort cosine lies in
    [0.9966, 0.9993], sd in [5.1e-4, 1.2e-3], so one ulp of a cosine (6e-8) moves a score by up to 1e-3.  ``bound`` is the
    2 x rule; ``bound_apriori`` lets the statistics take the a-priori bound of the f32 product, D 2^-24."""
    g = SC.g12()
    bank, speaker = g["embedding"], g["speaker"]
    pairs = g["trials"][:, 1:].astype(np.int32)
    cohort64 = segment_mean_ref(bank, speaker)
    cohort = cohort64.astype(np.float32)
    K = min(G12_TOP_K, cohort.shape[0])
    mu, sd = cohort_stats_ref(bank, cohort, K)
    cos, _ = SC.score_pairs_ref(bank, pairs)
    ref = norm_scores_ref(cos, pairs, mu, sd, mode)
    host = host_norm_scores(bank, cohort, pairs, K, mode)
    hmu, hsd = host_cohort_stats(bank, cohort, K)
    host2 = 2.0 * np.abs(host - ref).max()
    return {"bank": bank, "speaker": speaker, "pairs": pairs, "gt": g["trials"][:, 0].tolist(), "cohort": cohort,
            "cohort64": cohort64, "K": K, "mode": mode, "mu": mu, "sd": sd, "score": ref, "host_score": host,
            "bound_mu": bound(np.abs(hmu - mu).max()), "bound_sd": bound(np.abs(hsd - sd).max()), "apriori": apriori(bank.shape[1]),
            "bound": np.maximum(host2, floor_z(cos, pairs, mu, sd, mode)),
            "bound_apriori": np.maximum(host2, floor_z(cos, pairs, mu, sd, mode, apriori(bank.shape[1])))}
