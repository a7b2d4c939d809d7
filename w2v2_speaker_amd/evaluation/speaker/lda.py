"""The LDA scoring back-end (ref: src/evaluation/speaker/lda.py, config/evaluator/lda.yaml): a fitted projection to a
latent space, centring and length norm there, then the cosine.

The reference's class cannot run as shipped (its base-class constructor lacks the keyword it is given, and it fits
``PCA(n_components=200, whiten=True)`` whatever ``num_pca_components`` says), so the definition is the "scoring back-ends"
block of include/w2v2_hip.h; the reference's constructor keywords and its chain -- projection, centring, length norm,
score -- are kept.  ``projection="pca"`` is what the reference really fits (whitening PCA); ``projection="lda"`` is the
discriminant projection its name promises.

``fit_parameters`` sums the statistics in float64 on the host; ``fit_parameters_bank`` sums them on the device
(ops.segment_mean, ops.embed_stats, ops.class_scatter); both hand them to the solvers of backend.py.  ``evaluate`` scores in
plain torch f32 on the CPU, ``evaluate_bank`` / ``evaluate_bank_metrics`` on the device, as the cosine evaluator's do."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import backend
from .cosine_distance import (EmbeddingSample, EvaluationPair, center_batch, cohort_stats_host, length_norm_batch,
                              missing_pair_answer, normalise_scores, resolve_trials)


class LatentBackendEvaluator:
    """What the LDA and the PLDA evaluator share: steps 1-3 of the definition (class statistics, projection, latent
    mean / std), the model's host and device copies, and the plumbing of ``evaluate`` / ``evaluate_bank_metrics``.  A
    subclass says how a fitted latent bank is scored (``_host_scores``, ``_device_scores``)."""

    name = "back-end"
    clip_scores = True                      # (s + 1) / 2 clipped to [0, 1] before the metrics (the cosine back-ends)

    def _init_latent(self, num_components: int, projection: str, max_training_batches_to_fit: int,
                     center_before_fit: bool = False) -> None:
        if projection not in backend.PROJECTIONS:
            raise ValueError(f"projection={projection!r}: 'pca' or 'lda'")
        if isinstance(num_components, bool) or not isinstance(num_components, int) or num_components < 1:
            raise ValueError(f"{self.name}: {num_components!r} components: a positive integer")
        self.projection = projection
        self._num_components = num_components
        self._center_before_fit = bool(center_before_fit)
        self.max_training_batches_to_fit = max_training_batches_to_fit
        self.max_num_training_samples = max_training_batches_to_fit       # the name the cosine evaluator uses
        self.last_bank_scoring = None
        self.last_bank_metrics = None
        self._clear()

    def _clear(self) -> None:
        self._proj_w = None                 # f32 [R4, D] on the host, zero rows behind R: y = W x + b
        self._proj_b = None                 # f32 [R4]
        self._mean = None                   # f32 [R4]: latent mean / std of the training rows (pad columns 0)
        self._std = None
        self._on_device = {}

    def reset_parameters(self):
        self._clear()

    # ------------------------------------------------------------------ the fit
    def _latent_flags(self):
        """(centre, length_norm) of step 3."""
        return True, True

    def _gather(self, embedding_tensors, label_tensors):
        if isinstance(embedding_tensors, (list, tuple)):
            X = torch.cat([torch.as_tensor(e) for e in embedding_tensors])
        else:
            X = torch.as_tensor(embedding_tensors)
        labels = label_tensors
        if isinstance(labels, (list, tuple)) and len(labels) and isinstance(labels[0], torch.Tensor):
            labels = torch.cat([l.reshape(-1) for l in labels])
        if X.dim() != 2:
            raise ValueError(f"{self.name}: the training embeddings concatenate to [N, D] (got {tuple(X.shape)})")
        ids, C = backend.label_ids(labels)
        if len(ids) != X.shape[0]:
            raise ValueError(f"{self.name}: {len(ids)} labels for {X.shape[0]} embeddings")
        return X, ids, C

    def _check_classes(self, N: int, C: int) -> None:
        if C < 2:
            raise ValueError(f"{self.name}: {C} class(es): at least 2 speakers are needed")

    def _store_projection(self, P: torch.Tensor, mu0: torch.Tensor, pre=None) -> None:
        """y = P (x' - mu0) with x' = (x - m) / (s + 1e-12) when the fit z-scored its rows (pre = (m, s)), folded into one
        weight and one bias."""
        R, D = P.shape
        if pre is not None:
            m, s = (v.to(torch.float64) for v in pre)
            W = P / (s + 1e-12)
            b = -(W @ m) - P @ mu0
        else:
            W, b = P, -(P @ mu0)
        R4 = backend.pad4(R)
        self._proj_w = backend.padded_rows(W, R4, D)
        self._proj_b = backend.padded_rows(b[None, :], 1, R4)[0].contiguous()

    def fit_parameters(self, embedding_tensors: List[torch.Tensor], label_tensors: List[torch.Tensor]):
        """ref: lda.py:55-80 / plda.py:52-117 -- ``t.cat`` of both lists; the statistics in float64 on the host."""
        X, ids, C = self._gather(embedding_tensors, label_tensors)
        self._check_classes(X.shape[0], C)
        self._clear()
        X = X.detach().to("cpu", torch.float64)
        pre = None
        if self._center_before_fit:
            s, m = torch.std_mean(X.to(torch.float32), dim=0)
            pre = (m, s)
            X = (X - m.to(torch.float64)) / (s.to(torch.float64) + 1e-12)
        stats = backend.class_statistics_host(X, ids, C)
        P = backend.solve_projection(stats, self._num_components, self.projection)
        self._store_projection(P, stats.mu0, pre)
        Y = (X - stats.mu0) @ P.T
        std, mean = torch.std_mean(Y, dim=0)
        R4 = self._proj_w.shape[0]
        self._mean = backend.padded_rows(mean[None, :], 1, R4)[0].contiguous()
        self._std = backend.padded_rows(std[None, :], 1, R4)[0].contiguous()
        self._fit_latent_host(Y, mean, std, ids, C)

    def _fit_latent_host(self, Y, mean, std, ids, C) -> None:
        pass

    def fit_parameters_bank(self, bank: torch.Tensor, labels: Sequence):
        """``fit_parameters`` for embeddings that are rows of a device ``[N, D]`` f32 bank, ``labels[r]`` the speaker of row
        r: class means, global mean, the two scatter matrices, the projection of the bank and its latent statistics are
        computed on the device; two [D, D] float64 matrices cross for the eigen-solves."""
        from ... import ops
        from .device_scoring import _upload
        N, D, _ = ops._bank(bank, f"{self.name} fit")
        ids, C = backend.label_ids(labels)
        if len(ids) != N:
            raise ValueError(f"{self.name}: {len(ids)} labels for {N} bank rows")
        self._check_classes(N, C)
        self._clear()
        dev, raw = bank.device, bank
        pre = None
        if self._center_before_fit:
            m, s = ops.embed_stats(bank)
            bank, _ = ops.rows_transform(bank, m, s)
            pre = (m.cpu(), s.cpu())
        order, offsets, counts = backend.segments(ids, C)
        groups = {"seg_id": _upload(ids.astype(np.int32), dev), "order": _upload(order, dev), "offsets": _upload(offsets, dev),
                  "sqrt_n": _upload(np.sqrt(counts.astype(np.float64)).astype(np.float32), dev), "counts": counts}
        means = ops.segment_mean(bank, groups["order"], groups["offsets"])
        mu0, _ = ops.embed_stats(bank)
        Sw = ops.class_scatter(bank, groups["seg_id"], means)
        Sb = ops.class_scatter(means, None, mu0.view(1, D), row_weight=groups["sqrt_n"])
        stats = backend.ClassStatistics(torch.from_numpy(counts.astype(np.float64)), means.cpu().to(torch.float64),
                                        mu0.cpu().to(torch.float64), backend._sym(Sw.cpu()), backend._sym(Sb.cpu()))
        P = backend.solve_projection(stats, self._num_components, self.projection)
        self._store_projection(P, stats.mu0, pre)
        Y = self._project(raw)                              # (the stored projection takes the raw rows)
        mean, std = ops.embed_stats(Y)
        self._mean, self._std = mean.cpu(), std.cpu()
        self._on_device = {}                                # (the device copy was made without them)
        self._fit_latent_bank(Y, groups, C)

    def _fit_latent_bank(self, Y, groups, C) -> None:
        pass

    # ------------------------------------------------------------------ the model, where it is needed
    def _require_fit(self) -> None:
        if self._proj_w is None:
            raise ValueError(f"{self.name}: fit_parameters() / fit_parameters_bank() has not been called")

    def _model_tensors(self) -> dict:
        return {"w": self._proj_w, "b": self._proj_b, "mean": self._mean, "std": self._std}

    def _device_model(self, device) -> dict:
        key = str(torch.device(device))
        if key not in self._on_device:
            self._on_device[key] = {k: v.to(device).contiguous() for k, v in self._model_tensors().items() if v is not None}
        return self._on_device[key]

    def _project(self, bank: torch.Tensor, which: str = "") -> torch.Tensor:
        """rows [N, K] -> rows W^T + b [N, R4] on the device: one exact-f32 GEMM with the bias epilogue."""
        from ... import ops
        m = self._device_model(bank.device)
        w, b = m[which + "w"], m[which + "b"]
        N, K, ld = ops._bank(bank, f"{self.name} projection")
        if K != w.shape[1]:
            raise ValueError(f"{self.name}: the bank has D = {K}, the fitted model D = {w.shape[1]}")
        out = torch.empty(N, w.shape[0], dtype=torch.float32, device=bank.device)
        ops.Gemm(N, w.shape[0], K, bank, w, out, lda=ld, ldb=K, ldc=w.shape[0], epilogue=ops.EPI_BIAS, bias=b)()
        return out

    # ------------------------------------------------------------------ scoring
    def _host_latent(self, bank: torch.Tensor) -> torch.Tensor:
        """Steps 2 and 3 of the fitted model on host rows [n, D], in f32."""
        if bank.shape[1] != self._proj_w.shape[1]:
            raise ValueError(f"{self.name}: the embeddings have D = {bank.shape[1]}, the fitted model D = {self._proj_w.shape[1]}")
        y = bank @ self._proj_w.T + self._proj_b
        centre, length_norm = self._latent_flags()
        if centre:
            y = center_batch(y, self._mean, self._std)
        if length_norm:
            y = length_norm_batch(y)
        return y

    def _host_scores(self, latent: torch.Tensor, e: torch.Tensor, t: torch.Tensor, score_norm) -> torch.Tensor:
        raise NotImplementedError

    def _device_scores(self, bank: torch.Tensor, index, keep_on_device: bool, score_norm):
        raise NotImplementedError

    def evaluate(self, pairs: List[EvaluationPair], samples: List[EmbeddingSample], score_norm=None, calibration=None,
                 llr_metrics: bool = False):
        """ref: speaker_recognition_evaluator.py:45-101 with the fitted model in plain torch f32 on the CPU.
        ``calibration`` / ``llr_metrics``: as on CosineDistanceEvaluator.evaluate (one system)."""
        self._require_fit()
        from .device_scoring import host_llr_metrics, host_metrics
        samples = list(samples)
        gt, trials, missing = resolve_trials(pairs, [s.sample_id for s in samples])
        if missing is not None:
            return missing_pair_answer(missing)
        rows, e, t = [s.embedding for s in samples], [a for a, _ in trials], [b for _, b in trials]
        if any(isinstance(r, (list, tuple)) for r in rows):
            raise NotImplementedError(f"{self.name}: one embedding per sample: an ensemble has no fitted back-end")
        if any(torch.as_tensor(r).dim() != 1 for r in rows):
            raise NotImplementedError(f"{self.name}: pooled embeddings only: a frame set has no fitted back-end")
        bank = torch.stack([torch.as_tensor(r) for r in rows]).detach().to("cpu", torch.float32)
        with torch.no_grad():
            scores = self._host_scores(self._host_latent(bank), torch.tensor(e), torch.tensor(t), score_norm)
        scores = scores.numpy().astype(np.float64)
        if self.clip_scores and score_norm is None:
            scores = np.clip((scores + 1) / 2, 0, 1)
        if calibration is not None:
            scores = calibration.apply(scores)
        if calibration is not None or llr_metrics:
            return host_llr_metrics(gt, scores.tolist(), calibration)
        return host_metrics(gt, scores.tolist())

    def evaluate_bank(self, pairs: List[EvaluationPair], keys: List[str], bank, frame_offsets=None):
        return self.evaluate_bank_metrics(pairs, keys, bank, frame_offsets, metrics="host")

    def _metric_scores_device(self, bank: torch.Tensor, index, score_norm=None) -> torch.Tensor:
        """The scores the metrics would see for one bank, float32 [P] on the device (ScoreCalibration.fit_bank)."""
        self._require_fit()
        return self._device_scores(bank, index, True, score_norm).device_scores

    def evaluate_bank_metrics(self, pairs: List[EvaluationPair], keys: List[str], bank, frame_offsets=None,
                              metrics: str = "host", score_norm=None, calibration=None, llr_metrics: bool = False):
        """``evaluate`` without the embeddings leaving the device, as CosineDistanceEvaluator.evaluate_bank_metrics:
        ``bank`` is an ``[N, D]`` f32 device tensor whose row r is the embedding of ``keys[r]``.  ``metrics="device"``
        leaves the scores on the device and computes EER / minDCF there.  ``last_bank_scoring`` / ``last_bank_metrics``
        as on the cosine evaluator.  ``calibration`` (one system) / ``llr_metrics``: as there -- the scores become
        calibrated llrs on the device and the dict gains cllr, act_dcf, act_p_miss and act_p_fa."""
        from .device_scoring import TrialIndex, calibrated_scores, check_metrics_choice, finish_bank_metrics
        check_metrics_choice(metrics)
        if isinstance(bank, (list, tuple)):
            raise NotImplementedError(f"{self.name}: one bank: an ensemble has no fitted back-end")
        if frame_offsets is not None:
            raise NotImplementedError(f"{self.name}: pooled embeddings only: a frame bank has no fitted back-end")
        self._require_fit()
        index = TrialIndex(pairs, keys)
        if index.missing is not None:
            return missing_pair_answer(index.missing)
        if not isinstance(bank, torch.Tensor) or bank.dim() != 2 or bank.shape[0] != index.num_rows:
            raise ValueError(f"bank of shape {tuple(getattr(bank, 'shape', ()))}: expected [{index.num_rows}, D]")
        if calibration is None:
            self.last_bank_scoring = self._device_scores(bank, index, metrics == "device", score_norm)
        else:
            raw = self._device_scores(bank, index, True, score_norm)
            self.last_bank_scoring = calibrated_scores(raw.device_scores.unsqueeze(0), calibration, metrics == "device",
                                                       raw.bank_floats)
        return finish_bank_metrics(self, index, metrics, calibration, calibration is not None or llr_metrics)


class LDAEvaluator(LatentBackendEvaluator):
    """ref: lda.py:31-107 with the reference's keywords (config/evaluator/lda.yaml).  ``num_pca_components`` is honoured
    (the reference hard-codes 200).  ``center_before_fit_training_batches``: the training rows are z-scored before the
    fit, as in the reference; the same z-score is then part of the model and applied to the rows that are scored (the
    reference forgets it there).  ``center_before_scoring`` / ``length_norm_before_scoring`` act in the latent space."""

    name = "lda"

    def __init__(self, center_before_scoring: bool, length_norm_before_scoring: bool, max_training_batches_to_fit: int,
                 num_pca_components: int, center_before_fit_training_batches: bool, projection: str = "pca"):
        self.center_before_scoring = center_before_scoring
        self.length_norm_before_scoring = length_norm_before_scoring
        self.num_pca_components = num_pca_components
        self.center_before_fit_training_batches = center_before_fit_training_batches
        self._init_latent(num_pca_components, projection, max_training_batches_to_fit, center_before_fit_training_batches)

    def _latent_flags(self):
        return bool(self.center_before_scoring), bool(self.length_norm_before_scoring)

    def _host_scores(self, latent, e, t, score_norm):
        cos = torch.nn.functional.cosine_similarity(latent[e], latent[t], dim=1, eps=1e-8)
        if score_norm is None:
            return cos
        cohort = self._host_latent(torch.as_tensor(score_norm.cohort).detach().to("cpu", torch.float32))
        mu, sd = cohort_stats_host(latent, cohort, score_norm.top_k)
        return normalise_scores(cos, mu[e], sd[e], mu[t], sd[t], score_norm.mode)

    def _device_scores(self, bank, index, keep_on_device, score_norm):
        from .device_scoring import ScoreNorm, score_trials_device
        centre, length_norm = self._latent_flags()
        m = self._device_model(bank.device)
        extra = {}
        if score_norm is not None:                          # the cohort goes through the same projection
            cohort = self._project(score_norm.cohort.to(bank.device, torch.float32).contiguous())
            extra["score_norm"] = ScoreNorm(cohort, score_norm.top_k, score_norm.mode)
        return score_trials_device(self._project(bank.detach()), index, mean=m["mean"] if centre else None,
                                   std=m["std"] if centre else None, length_norm=length_norm,
                                   keep_on_device=keep_on_device, **extra)
