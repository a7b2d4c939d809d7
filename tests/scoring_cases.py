"""Cases of the device trial scoring (csrc/score.hip) with their float64 references and, per case, the HOST evaluator's
own f32 result on the CPU.  No GPU and no ``ops`` import here: test_scoring_cpu.py pins the references to what the
reference evaluator produced (tests/golden/g12_eer.npz), test_scoring_gpu.py holds the kernels to them.

The bound, per case and quantity: 2 x the error of the host f32 path against float64 on the same inputs, with a floor of
2^-22.  The scores are O(1): 2^-22 is 2 ulp at 1.0 for the quotient and the same for the stored result, and the floor
keeps the bound from being zero where torch happens to be exact; the factor 2 is the margin the wav2spk and x-vector
tests give over torch-f32's own error.  Mean and std take the same rule relative to the per-dimension float64 std; a
dimension whose float64 std is 0 has no scale to be relative to and must come out exact (mean = the constant, std = 0).

Shapes: the smallest at which each kernel can go wrong (one 16-byte vector; a wave trip of 256 features minus a vector,
exact, plus a vector; the four-trial workgroup of score_pairs and its neighbours; the 128-row chunk of embed_stats and
its neighbours; one row per wave and fewer rows than waves in score_frame_sets)."""
import functools
import os

import numpy as np
import torch

from w2v2_speaker_amd.evaluation.speaker.cosine_distance import (CosineDistanceEvaluator, EmbeddingSample, EvaluationPair,
                                                                 compute_mean_std_batch)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 2.0 ** -22


def bound(host_err: float) -> float:
    return max(2.0 * float(host_err), FLOOR)


def padded(a: np.ndarray, gap: int) -> np.ndarray:
    """[rows, D] -> [rows, D + gap] with NaN in the gap: a kernel that reads past D poisons its result."""
    out = np.full((a.shape[0], a.shape[1] + gap), np.nan, dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


# ------------------------------------------------------------------------------------------------ float64 references
def stats_ref(bank):
    x = np.asarray(bank, dtype=np.float64)
    return x.mean(axis=0), x.std(axis=0, ddof=1)


def transform_ref(x, mean, std, length_norm):
    """float64 of the evaluator's centre_batch / length_norm_batch on f32 inputs (the statistics are inputs as well)."""
    x = np.asarray(x, dtype=np.float64)
    if mean is not None:
        x = (x - np.asarray(mean, dtype=np.float64)) / (np.asarray(std, dtype=np.float64) + 1e-12)
    if length_norm:
        x = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return x


def cos_ref(a, b):
    """torch's cosine_similarity in float64: each norm clamped at 1e-8 on its own."""
    return (a * b).sum(-1) / (np.maximum(np.linalg.norm(a, axis=-1), 1e-8) * np.maximum(np.linalg.norm(b, axis=-1), 1e-8))


def to_score(cos):
    return np.clip((np.asarray(cos, dtype=np.float64) + 1) / 2, 0, 1)        # ref: speaker_recognition_evaluator.py:81


def score_pairs_ref(bank, pairs, mean=None, std=None, length_norm=False):
    u = transform_ref(bank, mean, std, length_norm)
    pairs = np.asarray(pairs).reshape(-1, 2)
    cos = cos_ref(u[pairs[:, 0]], u[pairs[:, 1]])
    return cos, to_score(cos)


def frame_sets_ref(frames, sel, counts):
    """The PAIRWISE form, as the evaluator computes it: the mean over all (i, j) of cos(l_i, r_j)."""
    x = np.asarray(frames, dtype=np.float64)
    cos = np.array([cos_ref(x[s[0, :c[0]]][:, None, :], x[s[1, :c[1]]][None, :, :]).mean() for s, c in zip(sel, counts)])
    return cos, to_score(cos)


def frame_sets_separated_ref(frames, sel, counts):
    """The SEPARATED form the kernel uses: < mean_i l_i / max(|l_i|, 1e-8), mean_j r_j / max(|r_j|, 1e-8) >."""
    x = np.asarray(frames, dtype=np.float64)
    xn = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-8)
    return np.array([float(xn[s[0, :c[0]]].mean(0) @ xn[s[1, :c[1]]].mean(0)) for s, c in zip(sel, counts)])


# ------------------------------------------------------------------------------------------------ the host f32 path
def host_stats(bank):
    mean, std = compute_mean_std_batch(torch.from_numpy(np.ascontiguousarray(bank)))
    return mean.numpy(), std.numpy()


def host_pairs(bank, pairs, mean=None, std=None, length_norm=False):
    """CosineDistanceEvaluator._compute_prediction_scores on the CPU -> (cos, score) as ``evaluate`` forms them."""
    ev = CosineDistanceEvaluator(mean is not None, length_norm, 0)
    if mean is not None:
        ev.mean, ev.std = torch.from_numpy(np.ascontiguousarray(mean)), torch.from_numpy(np.ascontiguousarray(std))
    rows = [EmbeddingSample(str(i), torch.from_numpy(np.ascontiguousarray(r))) for i, r in enumerate(bank)]
    cos = np.array(ev._compute_prediction_scores([(rows[i], rows[j]) for i, j in np.asarray(pairs).reshape(-1, 2)]))
    return cos, to_score(cos)


def host_frame_sets(frames, sel, counts):
    """The arithmetic of compute_non_pooled_cosine_scores on frames already drawn (its own draw is random.sample)."""
    x = torch.from_numpy(np.ascontiguousarray(frames))
    out = []
    for s, c in zip(sel, counts):
        left, right = x[torch.as_tensor(s[0, :c[0]].astype(np.int64))], x[torch.as_tensor(s[1, :c[1]].astype(np.int64))]
        n1, n2, d = left.shape[0], right.shape[0], left.shape[1]
        sc = torch.nn.functional.cosine_similarity(left[:, None, :].expand(n1, n2, d).reshape(n1 * n2, d),
                                                   right[None, :, :].expand(n1, n2, d).reshape(n1 * n2, d), dim=1, eps=1e-8)
        out.append(torch.mean(sc).numpy().tolist())
    cos = np.array(out)
    return cos, to_score(cos)


# ------------------------------------------------------------------------------------------------ score_pairs cases
PAIR_DIMS = (4, 252, 256, 260, 1536)
PAIR_MODES = ((False, False), (True, False), (False, True), (True, True))      # (centre, length norm)
ZERO_ROW, TINY_ROW, BIG_ROW, MEAN_ROW = 2, 3, 4, 5
# i == j, the zero row, the tiny row, the scaled row, the row that equals the mean in one dimension, and plain ones
PAIR_LIST = ((0, 1), (1, 1), (ZERO_ROW, 0), (TINY_ROW, 6), (BIG_ROW, 7), (MEAN_ROW, 0), (7, 6), (TINY_ROW, ZERO_ROW),
             (BIG_ROW, BIG_ROW))
PAIR_COUNTS = (1, 3, 4, 5)       # around the four-trial workgroup (the full list has nine: three workgroups)


@functools.lru_cache(maxsize=None)
def pairs_case(D: int, centre: bool, length_norm: bool):
    """-> dict: bank [8, D] f32, ld_bank [8, D + 4] with NaN behind every row, pairs, mean / std (None without centring),
    the float64 reference and the host f32 result."""
    rng = np.random.default_rng(1000 + D)
    bank = rng.standard_normal((8, D)).astype(np.float32) + np.float32(0.5)
    bank[ZERO_ROW] = 0
    bank[TINY_ROW] *= np.float32(1e-10) / np.float32(np.linalg.norm(bank[TINY_ROW].astype(np.float64)))
    bank[BIG_ROW] *= np.float32(1e3)
    mean = std = None
    if centre:
        m, s = stats_ref(bank[[0, 1, 5, 6, 7]])
        mean, std = m.astype(np.float32), s.astype(np.float32)
        bank[:, 0] = mean[0]                     # a dimension every row shares: its std is exactly 0
        std[0] = 0
        bank[MEAN_ROW, D - 1] = mean[D - 1]      # one row equal to the mean in a dimension with spread
    pairs = np.array(PAIR_LIST, dtype=np.int32)
    cos, score = score_pairs_ref(bank, pairs, mean, std, length_norm)
    hcos, hscore = host_pairs(bank, pairs, mean, std, length_norm)
    return {"bank": bank, "ld_bank": padded(bank, 4), "pairs": pairs, "mean": mean, "std": std, "length_norm": length_norm,
            "cos": cos, "score": score, "host_cos": hcos, "host_score": hscore,
            "bound_cos": bound(np.abs(hcos - cos).max()), "bound_score": bound(np.abs(hscore - score).max())}


@functools.lru_cache(maxsize=None)
def two_row_case():
    """N = 2: the smallest bank."""
    bank = np.array([[1, 2, 3, 4], [-2, 0.5, 1, 3]], dtype=np.float32)
    pairs = np.array([(0, 1), (1, 0), (1, 1)], dtype=np.int32)
    cos, score = score_pairs_ref(bank, pairs)
    hcos, hscore = host_pairs(bank, pairs)
    return {"bank": bank, "pairs": pairs, "cos": cos, "score": score,
            "bound_cos": bound(np.abs(hcos - cos).max()), "bound_score": bound(np.abs(hscore - score).max())}


# ------------------------------------------------------------------------------------------------ embed_stats cases
STATS_ROWS = (3, 128, 129, 257, 2177)     # 2177 = 18 chunks: the fold's runs hold two chunks each, the last chunk one row
STATS_DIMS = (4, 260)
OFFSET_DIM, CONST_DIM = 0, 1


def stats_err(got_mean, got_std, ref_mean, ref_std):
    """(max |mean error| / std, max |std error| / std) over the dimensions that have a spread."""
    on = ref_std > 0
    return (float((np.abs(np.asarray(got_mean, np.float64) - ref_mean)[on] / ref_std[on]).max()),
            float((np.abs(np.asarray(got_std, np.float64) - ref_std)[on] / ref_std[on]).max()))


@functools.lru_cache(maxsize=None)
def stats_case(N: int, D: int):
    rng = np.random.default_rng(2000 + 7 * N + D)
    bank = (rng.standard_normal((N, D)) * rng.uniform(0.1, 3.0, D) + rng.uniform(-2, 2, D)).astype(np.float32)
    bank[:, OFFSET_DIM] = (1e3 + 1e-2 * rng.standard_normal(N)).astype(np.float32)      # mean 1e3, std 1e-2
    bank[:, CONST_DIM] = np.float32(0.37)                                               # std exactly 0
    mean, std = stats_ref(bank)
    assert std[CONST_DIM] == 0 and mean[CONST_DIM] == float(np.float32(0.37)) and (np.delete(std, CONST_DIM) > 0).all()
    hm, hs = host_stats(bank)
    em, es = stats_err(hm, hs, mean, std)
    return {"bank": bank, "ld_bank": padded(bank, 4), "mean": mean, "std": std, "bound_mean": bound(em), "bound_std": bound(es)}


# ------------------------------------------------------------------------------------------------ score_frame_sets cases
FRAME_DIMS = (4, 260, 768)
FRAME_COUNTS = ((1, 1), (3, 1), (7, 50), (50, 50))
FRAME_ROWS, FRAME_W, ZERO_FRAME = 120, 50, 5


@functools.lru_cache(maxsize=None)
def frames_case(D: int):
    """One trial per entry of FRAME_COUNTS over a 120-row frame bank; the (7, 50) trial selects the all-zero frame and the
    bank's last row, the (50, 50) trial the last row as well."""
    rng = np.random.default_rng(3000 + D)
    frames = rng.standard_normal((FRAME_ROWS, D)).astype(np.float32) + np.float32(0.3)
    frames[ZERO_FRAME] = 0
    sel = np.zeros((len(FRAME_COUNTS), 2, FRAME_W), dtype=np.int32)
    counts = np.array(FRAME_COUNTS, dtype=np.int32)
    for t, c in enumerate(FRAME_COUNTS):
        for side in (0, 1):
            sel[t, side, :c[side]] = rng.choice(FRAME_ROWS, c[side], replace=False)
    sel[2, 0, :2] = (ZERO_FRAME, FRAME_ROWS - 1)
    sel[2, 0, 2:7] = (10, 11, 12, 13, 14)
    if FRAME_ROWS - 1 not in sel[3, 1]:
        sel[3, 1, 49] = FRAME_ROWS - 1
    cos, score = frame_sets_ref(frames, sel, counts)
    hcos, hscore = host_frame_sets(frames, sel, counts)
    return {"frames": frames, "ld_frames": padded(frames, 4), "sel": sel, "counts": counts, "cos": cos, "score": score,
            "bound_cos": bound(np.abs(hcos - cos).max()), "bound_score": bound(np.abs(hscore - score).max())}


def clamp_case():
    """7 x 5 rows with an all-zero row and a row of norm 1e-10: where the separated form would differ from the pairwise
    one if torch clamped the PRODUCT of the norms."""
    rng = np.random.default_rng(77)
    frames = rng.standard_normal((12, 16)).astype(np.float32)
    frames[1] = 0
    frames[8] *= np.float32(1e-10) / np.float32(np.linalg.norm(frames[8].astype(np.float64)))
    sel = np.zeros((1, 2, 7), dtype=np.int32)
    sel[0, 0] = np.arange(7)
    sel[0, 1, :5] = np.arange(7, 12)
    return frames, sel, np.array([[7, 5]], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the g12 trial set
def g12():
    return np.load(os.path.join(GOLDEN, "g12_eer.npz"))


G12_BRANCHES = {"": (False, False), "_c": (True, False), "_cl": (True, True), "_l": (False, True)}


@functools.lru_cache(maxsize=None)
def g12_case(tag: str):
    """The reference evaluator's branch ``tag`` on the 496 trials of g12: float64 reference, host f32 result, bound."""
    g = g12()
    centre, ln = G12_BRANCHES[tag]
    bank = g["embedding"]
    pairs = g["trials"][:, 1:].astype(np.int32)
    mean, std = (g["fit_mean"], g["fit_std"]) if centre else (None, None)
    cos, score = score_pairs_ref(bank, pairs, mean, std, ln)
    _, hscore = host_pairs(bank, pairs, mean, std, ln)
    return {"bank": bank, "pairs": pairs, "gt": g["trials"][:, 0].tolist(), "mean": mean, "std": std, "length_norm": ln,
            "score": score, "host_score": hscore, "bound_score": bound(np.abs(hscore - score).max())}


def g12_frames():
    """The six 2-D embeddings of g12 as one ragged frame bank -> (frames [sum T, 64], offsets [7], trials [15, 3])."""
    g = g12()
    embs = [g[f"nonpooled_emb{i}"] for i in range(6)]
    return np.concatenate(embs), np.concatenate([[0], np.cumsum([e.shape[0] for e in embs])]), g["nonpooled_trials"]


# ------------------------------------------------------------------------------------------------ a set whose EER cannot flip
def separated_set():
    """32 utterances of 8 speakers, D = 64, all 496 pairs, for the EER of the PLAIN branch (on g12 that branch's smallest
    target / non-target score gap is 8.9e-8: a last-bit difference may swap a pair).  Here no target score lies within
    4 x the bound of a non-target score in float64, so neither an f32 host path nor the device within the bound can
    change the ROC; the classes still overlap, so the EER is not trivially 0."""
    rng = np.random.default_rng(4242)
    centres = rng.standard_normal((8, 64))
    spk = np.repeat(np.arange(8), 4)
    bank = (centres[spk] + 1.6 * rng.standard_normal((32, 64))).astype(np.float32)
    trials = [(int(spk[i] == spk[j]), i, j) for i in range(32) for j in range(i + 1, 32)]
    pairs = np.array([t[1:] for t in trials], dtype=np.int32)
    gt = np.array([t[0] for t in trials])
    _, score = score_pairs_ref(bank, pairs)
    _, hscore = host_pairs(bank, pairs)
    b = bound(np.abs(hscore - score).max())
    gap = np.abs(score[gt == 1][:, None] - score[gt == 0][None, :]).min()
    assert gap > 4 * b, (gap, b)
    assert score[gt == 1].min() < score[gt == 0].max()          # overlapping classes: an EER that can move
    keys = [f"utt{i:02d}" for i in range(32)]
    return {"bank": bank, "keys": keys, "pairs": pairs, "gt": gt.tolist(), "score": score, "bound_score": b,
            "eval_pairs": [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]}
