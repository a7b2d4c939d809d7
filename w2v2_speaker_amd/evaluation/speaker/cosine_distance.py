"""Mirror of ref: src/evaluation/speaker/{speaker_recognition_evaluator,cosine_distance}.py: trial scoring by
cosine similarity, ``(s+1)/2`` clipped to [0,1] (evaluator.py:81), then EER / minDCF."""
from __future__ import annotations

import random
from dataclasses import dataclass
from typing import List, Tuple, Union
from warnings import warn

import numpy as np
import torch


@dataclass
class EvaluationPair:
    same_speaker: bool
    sample1_id: str
    sample2_id: str


@dataclass
class EmbeddingSample:
    sample_id: str
    embedding: Union[torch.Tensor, List[torch.Tensor]]


def compute_mean_std_batch(all_tensors: torch.Tensor):
    """ref: speaker_recognition_evaluator.py:154-159 -- per-dimension mean and UNBIASED std over [NUM_SAMPLES, EMBEDDING_SIZE]."""
    std, mean = torch.std_mean(all_tensors, dim=0)
    return mean, std


def center_batch(embedding_tensor: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """ref: speaker_recognition_evaluator.py:162-167 -- despite the name this is a per-dimension z-score:
    the reference divides by ``std + 1e-12`` as well as subtracting the mean."""
    return (embedding_tensor - mean) / (std + 1e-12)


def length_norm_batch(embedding_tensor: torch.Tensor) -> torch.Tensor:
    """ref: speaker_recognition_evaluator.py:170-172."""
    return torch.nn.functional.normalize(embedding_tensor, dim=1)


def compute_cosine_scores(left_samples: torch.Tensor, right_samples: torch.Tensor) -> List[float]:
    """ref: cosine_distance.py:235-241 (``torch.nn.CosineSimilarity()``: dim 1, eps 1e-8)."""
    return torch.nn.functional.cosine_similarity(left_samples, right_samples, dim=1, eps=1e-8) \
        .detach().cpu().numpy().tolist()


def compute_non_pooled_cosine_scores(left_tensor: torch.Tensor, right_tensor: torch.Tensor) -> float:
    """ref: cosine_distance.py:203-232 -- a sample whose embedding is 2-D ([frames, features], the ``NoPooling`` head):
    at most 50 frames per side, drawn with the GLOBAL ``random`` module (left side first, so a caller that seeds
    ``random`` sees the reference's draws), and the score is the mean of all pairwise frame cosines.  Element (i, j) of
    the broadcast below is element ``i * p2 + j`` of the reference's repeat_interleave / repeat pair, so the mean runs
    over the same values in the same order."""
    p1, p2 = left_tensor.shape[0], right_tensor.shape[0]
    left = left_tensor[random.sample(range(p1), min(50, p1)), :]
    right = right_tensor[random.sample(range(p2), min(50, p2)), :]
    with torch.no_grad():
        n1, n2, d = left.shape[0], right.shape[0], left.shape[1]
        score = torch.nn.functional.cosine_similarity(
            left[:, None, :].expand(n1, n2, d).reshape(n1 * n2, d),
            right[None, :, :].expand(n1, n2, d).reshape(n1 * n2, d), dim=1, eps=1e-8)
    return torch.mean(score).detach().cpu().numpy().tolist()


def cohort_stats_host(bank: torch.Tensor, cohort: torch.Tensor, top_k: int):
    """The cohort statistics of score normalisation in plain torch on the tensors' own device (f32 on the CPU for the host
    evaluator): every row of the already transformed ``bank`` [N, D] against every row of the transformed ``cohort``
    [M, D] as torch's cosine_similarity forms it (each norm clamped at 1e-8 on its own), then the mean and the unbiased std
    of the ``top_k`` largest cosines of each row -> (mu [N], sd [N]).  The definition: include/w2v2_hip.h, "score
    normalisation"; the reference project has no such stage."""
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 2 <= top_k <= cohort.shape[0]:
        raise ValueError(f"score_norm: top_k = {top_k!r} outside [2, M = {cohort.shape[0]}]")
    un = bank / torch.linalg.vector_norm(bank, dim=1, keepdim=True).clamp_min(1e-8)
    cn = cohort / torch.linalg.vector_norm(cohort, dim=1, keepdim=True).clamp_min(1e-8)
    top = torch.topk(torch.matmul(un, cn.t()), top_k, dim=1).values
    return top.mean(dim=1), top.std(dim=1)


def normalise_scores(cos: torch.Tensor, mu_e, sd_e, mu_t, sd_t, mode: str) -> torch.Tensor:
    """z_e = (c - mu_e) / (sd_e + 1e-12), z_t likewise; "z" -> z_e, "t" -> z_t, "s" -> (z_e + z_t) / 2."""
    if mode not in ("z", "t", "s"):
        raise ValueError(f"score_norm: mode={mode!r}: 'z', 't' or 's'")
    ze, zt = (cos - mu_e) / (sd_e + 1e-12), (cos - mu_t) / (sd_t + 1e-12)
    return ze if mode == "z" else (zt if mode == "t" else (ze + zt) / 2)


def resolve_trials(pairs: List[EvaluationPair], keys):
    """The trial list against the sample ids (``keys[r]`` names row r; ref: speaker_recognition_evaluator.py:45-72) ->
    (ground_truth, rows, missing): the 0 / 1 list and the (row of sample1, row of sample2) list of the trials, and None -- or,
    from the first trial that names an id the keys do not hold, that trial's two ids.  Duplicate keys raise.  Every
    evaluator's ``evaluate`` and device_scoring.TrialIndex resolve with this."""
    row_of = {}
    for r, k in enumerate(keys):
        if k in row_of:
            raise ValueError(f"duplicate key {k}")
        row_of[k] = r
    gt, rows = [], []
    for pair in pairs:
        if pair.sample1_id not in row_of or pair.sample2_id not in row_of:
            return gt, rows, (pair.sample1_id, pair.sample2_id)
        gt.append(1 if pair.same_speaker else 0)
        rows.append((row_of[pair.sample1_id], row_of[pair.sample2_id]))
    return gt, rows, None


def missing_pair_answer(missing: Tuple[str, str]) -> dict:
    """What the reference answers to a trial whose sample is missing: a warning (in the caller's name) and -1 throughout."""
    warn(f"{missing[0]} or {missing[1]} not in sample_map", stacklevel=2)
    return {"eer": -1, "eer_threshold": -1, "mdc": -1, "mdc_threshold": -1}


class CosineDistanceEvaluator:
    """ref: cosine_distance.py:66-201.  Defaults = config/evaluator/cosine_distance.yaml (no centering, no length
    norm, max_num_training_samples 0); the non-default branches follow the reference as well: centering is
    ``(x - mean) / (std + 1e-12)`` with the statistics of ``fit_parameters``, then optional length norm, then the
    cosine; 2-D embeddings take the non-pooled scoring (no centering / length norm there, as in the reference)."""

    def __init__(self, center_before_scoring: bool = False, length_norm_before_scoring: bool = False,
                 max_num_training_samples: int = 0):
        self.center_before_scoring = center_before_scoring
        self.length_norm_before_scoring = length_norm_before_scoring
        self.max_num_training_samples = max_num_training_samples
        self.mean = None
        self.std = None

    def _using_parameters(self) -> bool:
        return self.center_before_scoring

    def fit_parameters(self, embedding_tensors: List[torch.Tensor], _label_tensors=None):
        if not self._using_parameters():
            return
        if len(embedding_tensors) <= 2:
            raise ValueError("mean/std calculation requires more than 2 samples")
        self.mean, self.std = compute_mean_std_batch(torch.stack(embedding_tensors, dim=0))

    def reset_parameters(self):
        """ref: cosine_distance.py:99-104."""
        if not self._using_parameters():
            return
        self.mean = None
        self.std = None

    def _transform_pairs_to_tensor(self, pairs: List[Tuple[EmbeddingSample, EmbeddingSample]]):
        """ref: speaker_recognition_evaluator.py:123-137."""
        return (torch.stack([torch.as_tensor(a.embedding) for a, _ in pairs]),
                torch.stack([torch.as_tensor(b.embedding) for _, b in pairs]))

    def _compute_prediction_scores(self, pairs: List[Tuple[EmbeddingSample, EmbeddingSample]]) -> List[float]:
        first = pairs[0][0].embedding
        if isinstance(first, list):                     # ref: cosine_distance.py:110-112 (ensemble of layers)
            return self._compute_ensemble_prediction_scores(pairs)
        if len(first.shape) == 2:                       # ref: cosine_distance.py:114-116 (non-pooled embeddings)
            return self._compute_non_pooled_prediction_scored(pairs)
        left, right = self._transform_pairs_to_tensor(pairs)
        if self.center_before_scoring:
            if self.mean is None or self.std is None:   # the reference dies on ``tensor - None`` here; say why
                raise TypeError("center_before_scoring=True but fit_parameters() has not been called "
                                "(mean / std are None)")
            left = center_batch(left, self.mean, self.std)
            right = center_batch(right, self.mean, self.std)
        if self.length_norm_before_scoring:
            left = length_norm_batch(left)
            right = length_norm_batch(right)
        return compute_cosine_scores(left, right)

    def _compute_non_pooled_prediction_scored(self, pairs: List[Tuple[EmbeddingSample, EmbeddingSample]]) -> List[float]:
        """ref: cosine_distance.py:187-200 (name kept, typo included: callers may reach for it)."""
        return [compute_non_pooled_cosine_scores(a.embedding, b.embedding) for a, b in pairs]

    def _compute_ensemble_prediction_scores(self, pairs: List[Tuple[EmbeddingSample, EmbeddingSample]]) -> List[float]:
        """ref: cosine_distance.py:134-185 -- every sample carries a LIST of embeddings (one per hidden state,
        Wav2vec2FCModule.compute_ensemble_embedding); the score of a pair is the mean of the per-member scores."""
        n = len(pairs[0][0].embedding)
        for s1, s2 in pairs:
            if not isinstance(s1.embedding, list) or not isinstance(s2.embedding, list):
                raise ValueError("not every embedding sample is an ensemble")
            if len(s1.embedding) != n or len(s2.embedding) != n:
                raise ValueError(f"expected each list to have len num_ensembles={n}")
        member_scores = [self._compute_prediction_scores(
            [(EmbeddingSample(sample_id=a.sample_id, embedding=a.embedding[i]),
              EmbeddingSample(sample_id=b.sample_id, embedding=b.embedding[i])) for a, b in pairs]) for i in range(n)]
        combined = []
        for idx in range(len(pairs)):
            score = 0
            for i in range(n):                       # same accumulation order as the reference
                score += member_scores[i][idx] * (1 / n)
            combined.append(score)
        return combined

    def _compute_normalised_scores(self, pairs: List[Tuple[EmbeddingSample, EmbeddingSample]], score_norm) -> List[float]:
        """The score-normalised form of ``_compute_prediction_scores`` in plain torch f32 on the CPU (matmul, topk, mean,
        std): ``score_norm`` carries ``cohort`` [M, D], ``top_k`` and ``mode`` (device_scoring.ScoreNorm).  Pooled
        embeddings only.  The cohort takes the evaluator's centring / length norm, as the embeddings do."""
        first = pairs[0][0].embedding
        if isinstance(first, list):
            raise NotImplementedError("score_norm takes one embedding per sample: a normalised ensemble score is not defined")
        if len(first.shape) == 2:
            raise NotImplementedError("score_norm takes pooled embeddings: a frame set has no single cohort cosine")
        rows, order = {}, []
        for a, b in pairs:
            for smp in (a, b):
                if id(smp) not in rows:
                    rows[id(smp)] = len(order)
                    order.append(smp)
        bank = torch.stack([torch.as_tensor(s.embedding) for s in order]).float()
        cohort = torch.as_tensor(score_norm.cohort).detach().to("cpu", torch.float32)
        if self.center_before_scoring:
            if self.mean is None or self.std is None:
                raise TypeError("center_before_scoring=True but fit_parameters() has not been called "
                                "(mean / std are None)")
            bank = center_batch(bank, self.mean, self.std)
            cohort = center_batch(cohort, self.mean, self.std)
        if self.length_norm_before_scoring:
            bank = length_norm_batch(bank)
            cohort = length_norm_batch(cohort)
        mu, sd = cohort_stats_host(bank, cohort, score_norm.top_k)
        e = torch.tensor([rows[id(a)] for a, _ in pairs])
        t = torch.tensor([rows[id(b)] for _, b in pairs])
        cos = torch.nn.functional.cosine_similarity(bank[e], bank[t], dim=1, eps=1e-8)
        return normalise_scores(cos, mu[e], sd[e], mu[t], sd[t], score_norm.mode).detach().cpu().numpy().tolist()

    def _host_member_rows(self, pp, n: int) -> np.ndarray:
        """The metric scores of every member of an ensemble on the host, float64 [n, P]: what a fusion takes."""
        first = pp[0][0].embedding
        if not isinstance(first, list) or len(first) != n:
            raise ValueError(f"calibration: fitted on {n} systems: every sample carries a list of {n} embeddings")
        rows = [self._compute_prediction_scores(
            [(EmbeddingSample(sample_id=a.sample_id, embedding=a.embedding[i]),
              EmbeddingSample(sample_id=b.sample_id, embedding=b.embedding[i])) for a, b in pp]) for i in range(n)]
        return np.clip((np.array(rows, dtype=np.float64) + 1) / 2, 0, 1)

    def evaluate(self, pairs: List[EvaluationPair], samples: List[EmbeddingSample], score_norm=None, calibration=None,
                 llr_metrics: bool = False):
        """``score_norm`` (device_scoring.ScoreNorm, default None: the reference's evaluation, unchanged): the trial scores
        are normalised with its cohort first; they are then unbounded and go to the metrics as they are, NOT through
        ``(s+1)/2`` and the clip.  ``calibration`` (calibration.ScoreCalibration, fitted; default None): the scores that go
        to the metrics are the calibrated llrs of those scores (float64 numpy here), unbounded, and the dict gains cllr,
        act_dcf, act_p_miss and act_p_fa; a K-system calibration fuses the K members of an ensemble.
        ``llr_metrics=True`` without a calibration adds the same four keys for the scores as they are."""
        from .device_scoring import host_llr_metrics, host_metrics
        samples = list(samples)
        gt, rows, missing = resolve_trials(pairs, [s.sample_id for s in samples])
        if missing is not None:
            return missing_pair_answer(missing)
        pp = [(samples[a], samples[b]) for a, b in rows]
        if calibration is not None and calibration.num_systems != 1:
            scores = calibration.apply(self._host_member_rows(pp, calibration.num_systems)).tolist()
        elif score_norm is not None:
            scores = self._compute_normalised_scores(pp, score_norm)
        else:
            scores = np.clip((np.array(self._compute_prediction_scores(pp)) + 1) / 2, 0, 1).tolist()
        if calibration is not None or llr_metrics:
            if calibration is not None and calibration.num_systems == 1:
                scores = calibration.apply(np.asarray(scores, dtype=np.float64)).tolist()
            return host_llr_metrics(gt, scores, calibration)
        return host_metrics(gt, scores)

    # ------------------------------------------------------------------ the same evaluation over a bank on the device
    def fit_parameters_bank(self, bank: torch.Tensor):
        """``fit_parameters`` for embeddings that are rows of a device ``[N, D]`` bank: mean / std by w2v2_embed_stats,
        kept on the device."""
        if not self._using_parameters():
            return
        if bank.shape[0] <= 2:
            raise ValueError("mean/std calculation requires more than 2 samples")
        from ... import ops
        self.mean, self.std = ops.embed_stats(bank)

    def evaluate_bank(self, pairs: List[EvaluationPair], keys: List[str], bank, frame_offsets=None):
        """``evaluate`` without the embeddings leaving the device: ``bank`` is an ``[N, D]`` device tensor whose row r is
        the embedding of ``keys[r]``, a list of such tensors (an ensemble), or -- with ``frame_offsets`` [N + 1] -- a ragged
        ``[sum T, D]`` frame bank (the non-pooled form; no centring / length norm there, as in the reference).  Scores are
        computed by the kernels of csrc/score.hip and one array of P (ensemble of n: n * P) floats is copied to the host;
        EER / minDCF as in ``evaluate``.  ``last_bank_scoring`` keeps the scores and the copy's size.  (The form that can
        leave the metrics on the device as well, and that takes ``score_norm``: ``evaluate_bank_metrics``.)"""
        return self.evaluate_bank_metrics(pairs, keys, bank, frame_offsets, metrics="host")

    def _metric_scores_device(self, bank: torch.Tensor, index, score_norm=None) -> torch.Tensor:
        """The scores the metrics would see for one pooled bank, float32 [P] on the device (ScoreCalibration.fit_bank)."""
        from .device_scoring import score_trials_device
        if self.center_before_scoring and (self.mean is None or self.std is None):
            raise TypeError("center_before_scoring=True but fit_parameters() has not been called "
                            "(mean / std are None)")
        centre = self.center_before_scoring
        return score_trials_device(bank, index, mean=self.mean if centre else None, std=self.std if centre else None,
                                   length_norm=self.length_norm_before_scoring, keep_on_device=True,
                                   **({} if score_norm is None else {"score_norm": score_norm})).device_scores

    def evaluate_bank_metrics(self, pairs: List[EvaluationPair], keys: List[str], bank, frame_offsets=None,
                              metrics: str = "host", score_norm=None, calibration=None, llr_metrics: bool = False):
        """``evaluate_bank`` with the choice of where ROC / EER / minDCF are computed.  ``metrics="host"``: exactly
        ``evaluate_bank``.  ``metrics="device"`` (one bank or a frame bank): the scores stay on the device too, the metrics
        are computed there (csrc/metrics.hip, device_scoring.metrics_device) and eight doubles cross;
        ``last_bank_scoring`` then has ``scores`` None and ``host_copy_floats`` 0, and ``last_bank_metrics`` says which
        path answered.  An ensemble's members are combined on the host, so ``metrics="device"`` raises
        NotImplementedError for one; any other value of ``metrics`` raises ValueError.  ``score_norm``
        (device_scoring.ScoreNorm; one pooled bank only, anything else raises NotImplementedError): the scores are
        normalised on the device with its cohort (csrc/score_norm.hip) before they cross or reach the metrics; they are
        unbounded, not mapped to [0, 1].  ``calibration`` (calibration.ScoreCalibration, fitted; default None: all of the
        above, unchanged): the scores become calibrated llrs on the device (csrc/calibration.hip) before they cross or reach
        the metrics, and the dict gains cllr, act_dcf, act_p_miss and act_p_fa (ops.llr_metrics with ``metrics="device"``,
        still eight doubles in one copy).  A list of n banks with an n-system calibration is fused on the device:
        ``metrics="device"`` works for it, and P floats cross with ``metrics="host"``, not n * P.  ``llr_metrics=True``
        without a calibration adds the four keys for the scores as they are."""
        from .device_scoring import TrialIndex, check_metrics_choice, finish_bank_metrics, score_trials_device
        check_metrics_choice(metrics)
        if metrics == "device" and isinstance(bank, (list, tuple)) and calibration is None:
            raise NotImplementedError("metrics='device' takes one bank: the members of an ensemble are combined on the host "
                                      "in the reference's Python-float order")
        index = TrialIndex(pairs, keys)
        if index.missing is not None:
            return missing_pair_answer(index.missing)
        centre = self.center_before_scoring and frame_offsets is None
        if centre and (self.mean is None or self.std is None):
            raise TypeError("center_before_scoring=True but fit_parameters() has not been called "
                            "(mean / std are None)")
        self.last_bank_scoring = score_trials_device(
            bank, index, mean=self.mean if centre else None, std=self.std if centre else None,
            length_norm=self.length_norm_before_scoring and frame_offsets is None, frame_offsets=frame_offsets,
            keep_on_device=metrics == "device", **({} if score_norm is None else {"score_norm": score_norm}),
            **({} if calibration is None else {"calibration": calibration}))
        return finish_bank_metrics(self, index, metrics, calibration, calibration is not None or llr_metrics)
