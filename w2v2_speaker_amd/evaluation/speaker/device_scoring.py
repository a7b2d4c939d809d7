"""Trial scoring on the device (csrc/score.hip): what ``CosineDistanceEvaluator.evaluate_bank`` runs.

The host evaluator (cosine_distance.py, a mirror of the reference) gathers a left and a right ``[P, D]`` tensor on the
host from one ``EmbeddingSample`` object per utterance.  Here the embeddings stay where the forward left them -- one
``[N, D]`` bank on the device -- the trial list becomes one ``[P, 2]`` int32 table of bank rows, built and checked once on
the host, and ``P`` scores come back in one copy.  ROC / EER / minDCF run on the host (eval_metrics.py) by default;
``metrics_device`` computes them where the scores are (csrc/metrics.hip) and copies eight doubles instead."""
from __future__ import annotations

import random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ... import ops
from ...eval_metrics import calculate_eer, calculate_mdc
from .cosine_distance import resolve_trials

FRAME_CAP = 50      # frames per side of a non-pooled trial (ref: cosine_distance.py:203-232)


def _upload(a: np.ndarray, device) -> torch.Tensor:
    """Host array -> device tensor through pinned memory (one asynchronous copy on the current stream)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if torch.device(device).type == "cuda":
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


class TrialIndex:
    """A trial list as bank rows.  ``keys[r]`` is the sample id of bank row ``r``; ``pairs`` are the evaluator's
    ``EvaluationPair``s.  ``table`` is the int32 ``[P, 2]`` array of (row of sample1, row of sample2), ``ground_truth`` the
    0 / 1 list of ``evaluate``.  A pair that names a key the bank does not hold leaves ``table`` None and ``missing`` set to
    the two ids (``evaluate`` answers that with a warning and a dict of -1).  Duplicate keys raise, as in ``evaluate``."""

    def __init__(self, pairs, keys: Sequence[str]):
        keys = list(keys)
        self.num_rows = len(keys)
        self.ground_truth, rows, self.missing = resolve_trials(pairs, keys)
        self.table = None if self.missing else self._checked(rows, self.num_rows)
        self._device_table = None
        self._device_labels = None

    @classmethod
    def from_rows(cls, rows, ground_truth: Sequence[int], num_rows: int) -> "TrialIndex":
        """From row numbers directly (a caller that has no string keys); an index outside [0, num_rows) raises."""
        self = cls.__new__(cls)
        self.num_rows, self.missing = int(num_rows), None
        self.ground_truth = [int(g) for g in ground_truth]
        self.table = cls._checked(rows, self.num_rows)
        if len(self.ground_truth) != len(self.table):
            raise ValueError("one ground-truth label per trial")
        self._device_table = None
        self._device_labels = None
        return self

    @staticmethod
    def _checked(rows, num_rows: int) -> np.ndarray:
        t = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
        if t.shape[0] == 0:
            raise ValueError("empty trial list")
        if num_rows > np.iinfo(np.int32).max:
            raise ValueError(f"{num_rows} bank rows do not fit the int32 trial table")
        if t.min() < 0 or t.max() >= num_rows:
            bad = int(np.argmax((t < 0).any(1) | (t >= num_rows).any(1)))
            raise ValueError(f"trial {bad} names row {tuple(int(v) for v in t[bad])} outside [0, {num_rows})")
        return t.astype(np.int32)

    def __len__(self) -> int:
        return 0 if self.table is None else self.table.shape[0]

    def device_table(self, device) -> torch.Tensor:
        """The table on ``device``, uploaded once."""
        if self.table is None:
            raise ValueError(f"{self.missing[0]} or {self.missing[1]} not in the bank")
        if self._device_table is None or self._device_table.device != torch.device(device):
            self._device_table = _upload(self.table, device)
        return self._device_table

    def device_labels(self, device) -> torch.Tensor:
        """``ground_truth`` as uint8 [P] on ``device``, uploaded once."""
        if self.table is None:
            raise ValueError(f"{self.missing[0]} or {self.missing[1]} not in the bank")
        if self._device_labels is None or self._device_labels.device != torch.device(device):
            self._device_labels = _upload(np.asarray(self.ground_truth, dtype=np.uint8), device)
        return self._device_labels


def draw_frame_sets(frame_counts: Sequence[int], trial_index: TrialIndex, cap: int = FRAME_CAP):
    """The frame draws of the non-pooled score, as the host evaluator makes them (compute_non_pooled_cosine_scores): per
    trial, left side then right side, ``random.sample(range(p), min(cap, p))`` on the GLOBAL ``random`` -- a caller who
    seeds it gets the reference's draws.  ``frame_counts[r]`` = frames of utterance ``r``, whose frames are rows
    ``offset[r] .. offset[r] + p`` of the ragged frame bank.  -> (sel int32 [P, 2, cap] absolute row numbers, unused slots
    0; counts int32 [P, 2])."""
    if not 1 <= cap <= ops.FRAME_SET_MAX_W:
        raise ValueError(f"cap = {cap} outside [1, {ops.FRAME_SET_MAX_W}]")
    counts_in = np.asarray(frame_counts, dtype=np.int64)
    if counts_in.shape != (trial_index.num_rows,) or (counts_in < 1).any():
        raise ValueError("one positive frame count per bank utterance")
    offsets = np.concatenate([[0], np.cumsum(counts_in)])
    if offsets[-1] > np.iinfo(np.int32).max:
        raise ValueError(f"{int(offsets[-1])} frame rows do not fit the int32 selection table")
    if trial_index.table is None:
        raise ValueError(f"{trial_index.missing[0]} or {trial_index.missing[1]} not in the bank")
    P = len(trial_index)
    sel = np.zeros((P, 2, cap), dtype=np.int32)
    counts = np.zeros((P, 2), dtype=np.int32)
    for t, (l, r) in enumerate(trial_index.table.tolist()):
        for side, u in ((0, l), (1, r)):
            p = int(counts_in[u])
            drawn = random.sample(range(p), min(cap, p))
            counts[t, side] = len(drawn)
            sel[t, side, :len(drawn)] = offsets[u] + np.asarray(drawn, dtype=np.int64)
    return sel, counts


SCORE_NORM_MODES = ("z", "t", "s")


class ScoreNorm:
    """Adaptive score normalisation of a trial list with a cohort (include/w2v2_hip.h, "score normalisation"): ``cohort``
    an ``[M, D]`` float32 tensor of impostor embeddings (speaker_mean_cohort builds one), ``top_k`` the K largest cohort
    cosines of each side that give its mean and std (``top_k = M``: the non-adaptive norm), ``mode`` "z" (the enrolment
    side), "t" (the test side) or "s" (the mean of both).  The normalised score is unbounded: it is NOT mapped through
    ``(x + 1) / 2`` and not clipped.  The cohort goes through the evaluator's own centring / length norm, as the bank does."""

    def __init__(self, cohort: torch.Tensor, top_k: int, mode: str = "s"):
        if mode not in SCORE_NORM_MODES:
            raise ValueError(f"ScoreNorm: mode={mode!r}: 'z', 't' or 's'")
        if not isinstance(cohort, torch.Tensor) or cohort.dim() != 2 or cohort.shape[0] < 2:
            raise ValueError("ScoreNorm: cohort is an [M, D] tensor, M >= 2")
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 2 <= top_k <= cohort.shape[0]:
            raise ValueError(f"ScoreNorm: top_k = {top_k!r} outside [2, M = {cohort.shape[0]}]")
        self.cohort, self.top_k, self.mode = cohort, top_k, mode


def speaker_mean_cohort(bank: torch.Tensor, labels: Sequence) -> torch.Tensor:
    """The usual cohort: one mean embedding per speaker of ``bank`` [N, D] (a device tensor of training embeddings;
    ``labels[r]`` = the speaker of row r, any hashable) -> [S, D] on the device, speakers in sorted label order
    (w2v2_segment_mean).  The grouping -- a stable order of the rows by speaker and the segment offsets -- is built on the
    host from the labels; every speaker named has at least one row by construction."""
    labels = list(labels)
    if not isinstance(bank, torch.Tensor) or bank.dim() != 2 or len(labels) != bank.shape[0] or not labels:
        raise ValueError("speaker_mean_cohort: one label per bank row")
    if len(labels) > np.iinfo(np.int32).max:
        raise ValueError(f"{len(labels)} bank rows do not fit the int32 order table")
    speakers = sorted(set(labels))
    index = {s: i for i, s in enumerate(speakers)}
    ids = np.fromiter((index[l] for l in labels), dtype=np.int64, count=len(labels))
    order = np.argsort(ids, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=len(speakers)))]).astype(np.int32)
    return ops.segment_mean(bank, _upload(order, bank.device), _upload(offsets, bank.device))


@dataclass
class DeviceScores:
    """What score_trials_device hands back: ``scores`` float64 [P] in [0, 1] (what ``evaluate`` feeds the metrics; with
    ``score_norm`` the normalised scores, unbounded),
    ``host_copy_floats`` the number of floats that crossed to the host (P, or n * P for an ensemble of n),
    ``bank_floats`` the elements of the bank(s) that stayed on the device.  With ``keep_on_device`` the scores did not
    cross: ``scores`` is None, ``host_copy_floats`` 0 and ``device_scores`` the float32 [P] tensor the kernel wrote."""
    scores: Optional[np.ndarray]
    host_copy_floats: int
    bank_floats: int
    device_scores: Optional[torch.Tensor] = None


def score_trials_device(bank: Union[torch.Tensor, Sequence[torch.Tensor]], trial_index: TrialIndex, *, mean=None, std=None,
                        length_norm: bool = False, frame_offsets=None, cap: int = FRAME_CAP,
                        keep_on_device: bool = False, score_norm: Optional[ScoreNorm] = None,
                        calibration=None) -> DeviceScores:
    """Score ``trial_index`` over ``bank`` on the device.  bank: an ``[N, D]`` device tensor; a list of those (an
    ensemble: every member scored into one ``[n, P]`` buffer, combined on the host in the reference's order
    ``score += s_i * (1 / n)`` as Python floats, ref: cosine_distance.py:172-181); or, with ``frame_offsets`` ([N + 1],
    utterance r = rows frame_offsets[r] .. frame_offsets[r + 1]), a ragged ``[sum T, D]`` frame bank scored as the
    non-pooled form (frames drawn by draw_frame_sets from the global ``random``; no centring, no length norm, as in the
    reference).  One device -> host copy; none with ``keep_on_device`` (one bank or a frame bank: the scores stay
    where ``metrics_device`` reads them; an ensemble is combined on the host and cannot stay).  ``score_norm`` (one pooled
    bank only): the scores are the normalised ones (ops.cohort_stats + ops.score_pairs_norm), computed where the bank is.
    ``calibration`` (calibration.ScoreCalibration, fitted; default None: everything above, unchanged): the scores are the
    calibrated llrs ``a_0 + sum_k a_k s_k`` of the members' metric scores, computed on the device (ops.calib_apply), unbounded
    and not mapped again.  A list of n banks with an n-system calibration is FUSED there: ``keep_on_device`` works and P
    floats cross otherwise, not n * P."""
    members = list(bank) if isinstance(bank, (list, tuple)) else [bank]
    if not members or not all(isinstance(b, torch.Tensor) for b in members):
        raise ValueError("bank is a device tensor or a non-empty list of them")
    if score_norm is not None and len(members) != 1:
        raise NotImplementedError("score_norm takes one bank: the members of an ensemble are combined on the host, and a "
                                  "normalised ensemble score is not defined")
    if score_norm is not None and frame_offsets is not None:
        raise NotImplementedError("score_norm takes pooled embeddings: a frame bank has no single cohort cosine per "
                                  "utterance")
    dev = members[0].device
    P = len(trial_index)
    if keep_on_device and len(members) != 1 and calibration is None:
        raise NotImplementedError("keep_on_device: the members of an ensemble are combined on the host in the reference's "
                                  "Python-float order")
    if frame_offsets is not None:
        if len(members) != 1:
            raise ValueError("a frame bank is one tensor")
        off = np.asarray(torch.as_tensor(frame_offsets).cpu() if isinstance(frame_offsets, torch.Tensor) else frame_offsets,
                         dtype=np.int64)
        if off.shape != (trial_index.num_rows + 1,) or off[0] != 0 or off[-1] != members[0].shape[0]:
            raise ValueError(f"frame_offsets is [N + 1] = [{trial_index.num_rows + 1}], from 0 to the rows of the frame bank")
        sel, counts = draw_frame_sets(np.diff(off), trial_index, cap)
        _, score = ops.score_frame_sets(members[0], _upload(sel, dev), _upload(counts, dev))
        if calibration is not None:
            return calibrated_scores(score.unsqueeze(0), calibration, keep_on_device, members[0].numel())
        if keep_on_device:
            return DeviceScores(None, 0, members[0].numel(), score)
        host = score.cpu().numpy()
        return DeviceScores(host.astype(np.float64), host.size, members[0].numel())
    table = trial_index.device_table(dev)
    for b in members:
        if b.dim() != 2 or b.shape[0] != trial_index.num_rows:
            raise ValueError(f"bank of shape {tuple(b.shape)}: expected [{trial_index.num_rows}, D]")
    mean = None if mean is None else mean.to(dev, torch.float32).contiguous()
    std = None if std is None else std.to(dev, torch.float32).contiguous()
    n = len(members)
    cos = torch.empty(n, P, dtype=torch.float32, device=dev)
    score = torch.empty(n, P, dtype=torch.float32, device=dev)
    for i, b in enumerate(members):
        ops.score_pairs(b, table, mean, std, length_norm, cos[i], score[i])
    bank_floats = sum(b.numel() for b in members)
    if score_norm is not None:
        cohort = score_norm.cohort.to(dev, torch.float32).contiguous()
        mu, sd = ops.cohort_stats(members[0], cohort, score_norm.top_k, mean, std, length_norm)
        normed = ops.score_pairs_norm(cos[0], table, mu, sd, score_norm.mode)
        if calibration is not None:
            return calibrated_scores(normed.unsqueeze(0), calibration, keep_on_device, bank_floats)
        if keep_on_device:
            return DeviceScores(None, 0, bank_floats, normed)
        host = normed.cpu().numpy()
        return DeviceScores(host.astype(np.float64), host.size, bank_floats)
    if calibration is not None:
        return calibrated_scores(score, calibration, keep_on_device, bank_floats)
    if n == 1 and keep_on_device:
        return DeviceScores(None, 0, bank_floats, score[0])
    if n == 1:
        host = score[0].cpu().numpy()
        return DeviceScores(host.astype(np.float64), host.size, bank_floats)
    host = cos.cpu().numpy()
    member_scores = host.tolist()
    combined = []
    for idx in range(P):
        s = 0
        for i in range(n):                           # same accumulation order as the reference
            s += member_scores[i][idx] * (1 / n)
        combined.append(s)
    return DeviceScores(np.clip((np.array(combined) + 1) / 2, 0, 1), host.size, bank_floats)


def calibrated_scores(rows: torch.Tensor, calibration, keep_on_device: bool, bank_floats: int) -> DeviceScores:
    """The members' metric scores ``rows`` (float32 [K, P] on the device) through a fitted calibration -> the llrs as a
    DeviceScores: on the device with ``keep_on_device``, else one copy of P floats."""
    llr = calibration.apply(rows)
    if keep_on_device:
        return DeviceScores(None, 0, bank_floats, llr)
    host = llr.cpu().numpy()
    return DeviceScores(host.astype(np.float64), host.size, bank_floats)


LLR_KEYS = ("cllr", "act_dcf", "act_p_miss", "act_p_fa")
DEFAULT_POINT = (1, 1, 0.05)        # c_miss, c_fa, p_target of calculate_mdc's defaults: llr_metrics=True without a calibration


def operating_point(calibration) -> Tuple[float, float, float]:
    return DEFAULT_POINT if calibration is None else (calibration.c_miss, calibration.c_fa, calibration.p_target)


def host_llr_metrics(ground_truth: Sequence[int], llr: Sequence[float], calibration=None) -> dict:
    """``host_metrics`` of llrs plus cllr / act_dcf / act_p_miss / act_p_fa at the calibration's operating point (float64
    numpy, calibration.llr_metrics_numpy)."""
    from .calibration import llr_metrics_numpy
    res = host_metrics(ground_truth, llr)
    m = llr_metrics_numpy(llr, ground_truth, *operating_point(calibration))
    res.update({k: m[k] for k in LLR_KEYS})
    return res


def host_metrics(ground_truth: Sequence[int], scores: Sequence[float]) -> dict:
    """EER / minDCF as ``CosineDistanceEvaluator.evaluate`` computes them from Python lists, with its fallbacks."""
    try:
        eer, eer_threshold = calculate_eer(ground_truth, scores, pos_label=1)
    except (ValueError, ZeroDivisionError) as e:       # reference falls back to a very bad score
        print(f"EER calculation had {e}")
        eer, eer_threshold = 1, 1337
    try:
        mdc, mdc_threshold = calculate_mdc(ground_truth, scores)
    except (ValueError, ZeroDivisionError) as e:
        print(f"mdc calculation had {e}")
        mdc, mdc_threshold = 1, 1337
    return {"eer": eer, "eer_threshold": eer_threshold, "mdc": mdc, "mdc_threshold": mdc_threshold}


@dataclass
class DeviceMetrics:
    """What metrics_device did: ``path`` "device" or "host" (one class only, or NaN scores: the host's answer by
    construction), ``host_copy_floats`` the scores that crossed (0 on the device path), ``host_copy_doubles`` the eight
    doubles of w2v2_trial_metrics (0 when nothing was launched), ``fields`` those eight by name."""
    path: str
    host_copy_floats: int
    host_copy_doubles: int
    fields: Optional[dict] = None


def _host_scores(score: torch.Tensor) -> List[float]:
    """The device scores as the list ``evaluate_bank`` feeds the host metrics (float64 of the float32 scores)."""
    return score.cpu().numpy().astype(np.float64).tolist()


def metrics_device(score: torch.Tensor, trial_index: TrialIndex, *, workspace=None, record: Optional[list] = None) -> dict:
    """EER / minDCF of the device scores ``score`` (float32 [P], as score_trials_device(keep_on_device=True) leaves
    them) against ``trial_index.ground_truth`` -> the dict of ``evaluate``.  One device -> host copy of eight doubles.
    Two cases take exactly the host path of ``evaluate_bank``, so their answers (the ``1, 1337`` fallbacks included) are
    the host's: a list with one class only (known before any launch; nothing is launched) and NaN among the scores
    (``n_nan > 0``: the scores are then copied).  ``record``: a list that receives one DeviceMetrics."""
    gt = trial_index.ground_truth
    if not isinstance(score, torch.Tensor) or score.dim() != 1 or score.numel() != len(trial_index):
        raise ValueError(f"metrics_device: one score per trial ({len(trial_index)})")
    n_pos = sum(gt)
    if n_pos == 0 or n_pos == len(gt):
        if record is not None:
            record.append(DeviceMetrics("host", score.numel(), 0))
        return host_metrics(gt, _host_scores(score))
    out = ops.trial_metrics(score, trial_index.device_labels(score.device), workspace=workspace).cpu().tolist()
    fields = dict(zip(ops.TRIAL_METRICS_FIELDS, out))
    if fields["n_nan"] > 0:
        if record is not None:
            record.append(DeviceMetrics("host", score.numel(), 8, fields))
        return host_metrics(gt, _host_scores(score))
    if record is not None:
        record.append(DeviceMetrics("device", 0, 8, fields))
    return {k: fields[k] for k in ("eer", "eer_threshold", "mdc", "mdc_threshold")}


def metrics_device_llr(score: torch.Tensor, trial_index: TrialIndex, calibration=None, *, record: Optional[list] = None) -> dict:
    """``metrics_device`` for llrs (calibrated scores, or raw ones under ``llr_metrics=True``): EER / minDCF by
    ops.trial_metrics and Cllr / actDCF at the calibration's operating point by ops.llr_metrics, both where the llrs are ->
    the dict of ``evaluate`` with cllr, act_dcf, act_p_miss and act_p_fa added.  ONE device -> host copy of eight doubles:
    the eight values of the dict.  The two cases of metrics_device take the host path here as well: a list of one class
    (nothing is launched) and NaN among the llrs (then, and only then, cllr is NaN: the llrs are copied and the host
    answers).  ``record`` receives one DeviceMetrics whose ``fields`` are the eight values by name."""
    gt = trial_index.ground_truth
    if not isinstance(score, torch.Tensor) or score.dim() != 1 or score.numel() != len(trial_index):
        raise ValueError(f"metrics_device_llr: one llr per trial ({len(trial_index)})")
    n_pos = sum(gt)
    if n_pos == 0 or n_pos == len(gt):
        if record is not None:
            record.append(DeviceMetrics("host", score.numel(), 0))
        return host_llr_metrics(gt, _host_scores(score), calibration)
    labels = trial_index.device_labels(score.device)
    both = torch.empty(16, dtype=torch.float64, device=score.device)
    ops.trial_metrics(score, labels, out=both[:8])
    ops.llr_metrics(score, labels, *operating_point(calibration), out=both[8:])
    names = ("eer", "eer_threshold", "mdc", "mdc_threshold") + LLR_KEYS
    fields = dict(zip(names, torch.cat([both[0:4], both[8:9], both[11:14]]).cpu().tolist()))
    if fields["cllr"] != fields["cllr"]:
        if record is not None:
            record.append(DeviceMetrics("host", score.numel(), 8, fields))
        return host_llr_metrics(gt, _host_scores(score), calibration)
    if record is not None:
        record.append(DeviceMetrics("device", 0, 8, fields))
    return dict(fields)


def check_metrics_choice(metrics) -> None:              # the first check of every evaluate_bank_metrics
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics={metrics!r}: 'host' or 'device'")


def finish_bank_metrics(evaluator, index: TrialIndex, metrics: str, calibration, llrs: bool) -> dict:
    """What every evaluator's evaluate_bank_metrics does behind ``evaluator.last_bank_scoring``: the host or the device
    metrics, with the four llr keys when the scores are llrs (``llrs``: a calibration, or llr_metrics=True)."""
    rec = evaluator.last_bank_scoring
    if metrics == "device":
        record = []
        res = metrics_device_llr(rec.device_scores, index, calibration, record=record) if llrs \
            else metrics_device(rec.device_scores, index, record=record)
        evaluator.last_bank_metrics = record[0]
        rec.host_copy_floats = record[0].host_copy_floats          # (the host path copied them after all)
        return res
    if llrs:
        return host_llr_metrics(index.ground_truth, rec.scores.tolist(), calibration)
    return host_metrics(index.ground_truth, rec.scores.tolist())
