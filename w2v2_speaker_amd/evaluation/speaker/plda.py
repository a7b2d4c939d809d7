"""The PLDA scoring back-end (ref: src/evaluation/speaker/plda.py, config/evaluator/plda.yaml): a fitted projection,
centring and length norm in the latent space, then the log-likelihood ratio of a two-covariance PLDA model.

The reference's class needs ``bob.learn.em`` and scores with ``10 ** llr`` pushed through ``(s + 1) / 2`` and a clip; the
definition here is the "scoring back-ends" block of include/w2v2_hip.h: the two-covariance model fitted by EM over
class-level statistics (backend.plda_em), diagonalised, and scored in closed form.  The score is the llr itself,
unbounded; it goes to the metrics as it is."""
from __future__ import annotations

import numpy as np
import torch

from . import backend
from .lda import LatentBackendEvaluator


class PLDAEvaluator(LatentBackendEvaluator):
    """ref: plda.py:28-50 with the reference's keywords.  ``num_lda_pca_components`` = R of the projection,
    ``num_plda_pca_components`` = Q <= R dimensions of the diagonalised model that are scored, ``max_iterations`` EM
    steps."""

    name = "plda"
    clip_scores = False

    def __init__(self, num_lda_pca_components: int, num_plda_pca_components: int, max_iterations: int,
                 max_training_batches_to_fit: int, projection: str = "pca"):
        self.num_lda_pca_components = num_lda_pca_components
        self.num_plda_pca_components = num_plda_pca_components
        self.max_iterations = max_iterations
        self._init_latent(num_lda_pca_components, projection, max_training_batches_to_fit)
        if isinstance(num_plda_pca_components, bool) or not isinstance(num_plda_pca_components, int) \
                or not 1 <= num_plda_pca_components <= num_lda_pca_components:
            raise ValueError(f"plda: num_plda_pca_components = {num_plda_pca_components!r} outside "
                             f"[1, num_lda_pca_components = {num_lda_pca_components}]")
        if isinstance(max_iterations, bool) or not isinstance(max_iterations, int) or max_iterations < 0:
            raise ValueError(f"plda: max_iterations = {max_iterations!r}: a non-negative integer")

    def _clear(self) -> None:
        super()._clear()
        self._diag_w = None                 # f32 [Q4, R4]: u = A z + b2, zero rows / columns in the pads
        self._diag_b = None                 # f32 [Q4]
        self._p = None                      # f64 [Q4], zero in the pad
        self._q = None
        self._k = None
        self.psi = None                     # f64 [Q]: the between-class variances of the scored dimensions

    def _check_classes(self, N: int, C: int) -> None:
        super()._check_classes(N, C)
        if N <= C:
            raise ValueError(f"plda: N = {N} rows of C = {C} classes leave no within-class scatter")

    def _store_plda(self, counts, means, mu, Sw) -> None:
        R, Q = self._num_components, self.num_plda_pca_components
        A, psi, p, q, k = backend.solve_plda(counts, means[:, :R], mu[:R], Sw[:R, :R], Q, self.max_iterations)
        R4, Q4 = backend.pad4(R), backend.pad4(Q)
        self._diag_w = backend.padded_rows(A, Q4, R4)
        self._diag_b = backend.padded_rows(-(A @ mu[:R])[None, :], 1, Q4)[0].contiguous()
        self._p = torch.zeros(Q4, dtype=torch.float64)
        self._q = torch.zeros(Q4, dtype=torch.float64)
        self._p[:Q], self._q[:Q] = p, q
        self._k, self.psi = k, psi
        self._on_device = {}

    def _fit_latent_host(self, Y, mean, std, ids, C) -> None:
        Z = torch.nn.functional.normalize((Y - mean) / (std + 1e-12), dim=1)
        stats = backend.class_statistics_host(Z, ids, C)
        self._store_plda(stats.counts, stats.means, stats.mu0, stats.Sw)

    def _fit_latent_bank(self, Y, groups, C) -> None:
        from ... import ops
        m = self._device_model(Y.device)
        Z, _ = ops.rows_transform(Y, m["mean"], m["std"], True)
        means = ops.segment_mean(Z, groups["order"], groups["offsets"])
        mu, _ = ops.embed_stats(Z)
        Sw = ops.class_scatter(Z, groups["seg_id"], means)
        self._store_plda(torch.from_numpy(groups["counts"].astype(np.float64)), means.cpu().to(torch.float64),
                         mu.cpu().to(torch.float64), backend._sym(Sw.cpu()))

    def _require_fit(self) -> None:
        super()._require_fit()
        if self._diag_w is None:
            raise ValueError("plda: fit_parameters() / fit_parameters_bank() has not been called")

    def _model_tensors(self) -> dict:
        out = super()._model_tensors()
        if self._diag_w is not None:
            out.update({"diag_w": self._diag_w, "diag_b": self._diag_b, "p": self._p, "q": self._q})
        return out

    def _host_scores(self, latent, e, t, score_norm):
        if score_norm is not None:
            raise NotImplementedError("plda: score normalisation of PLDA scores is not built")
        u = latent @ self._diag_w.T + self._diag_b
        p, q = self._p.to(torch.float32), self._q.to(torch.float32)
        ue, ut = u[e], u[t]
        return self._k + (ue * ut * p).sum(dim=1) - ((ue * ue + ut * ut) * q).sum(dim=1)

    def _device_scores(self, bank, index, keep_on_device, score_norm):
        from ... import ops
        from .device_scoring import DeviceScores
        if score_norm is not None:
            raise NotImplementedError("plda: score normalisation of PLDA scores is not built")
        m = self._device_model(bank.device)
        Z, _ = ops.rows_transform(self._project(bank.detach()), m["mean"], m["std"], True)
        llr = ops.plda_score_pairs(self._project(Z, "diag_"), index.device_table(bank.device), m["p"], m["q"], self._k)
        if keep_on_device:
            return DeviceScores(None, 0, bank.numel(), llr)
        host = llr.cpu().numpy()
        return DeviceScores(host.astype(np.float64), host.size, bank.numel())
