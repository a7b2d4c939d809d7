"""The host side of the LDA / PLDA scoring back-ends: dense float64 linear algebra on D x D and C x R data.

The definition is the "scoring back-ends" block of include/w2v2_hip.h.  Everything that is O(N) in the training bank or
O(P) in the trial list runs on the device (ops.class_scatter, ops.Gemm, ops.plda_score_pairs); what is left -- the
symmetric eigen-solves and the EM over class-level sufficient statistics -- is here, in float64 on the CPU.  The host fit
(``fit_parameters``) and the device fit (``fit_parameters_bank``) of the evaluators call the same solvers: they differ
only in who summed the statistics."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

EIG_FLOOR = 1e-10           # a kept eigenvalue <= EIG_FLOOR * lambda_max is a singular covariance
PROJECTIONS = ("pca", "lda")


def label_ids(labels: Sequence) -> Tuple[np.ndarray, int]:
    """One speaker label per row (host integers, tensors of them, or any hashable) -> (ids int64 [N] in 0 .. C-1, C),
    speakers in sorted label order (as device_scoring.speaker_mean_cohort maps them)."""
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().reshape(-1).tolist()
    elif isinstance(labels, np.ndarray):
        labels = labels.reshape(-1).tolist()
    labels = [l.item() if isinstance(l, (torch.Tensor, np.generic)) else l for l in labels]
    if not labels:
        raise ValueError("back-end fit: no labels")
    index = {s: i for i, s in enumerate(sorted(set(labels)))}
    return np.fromiter((index[l] for l in labels), dtype=np.int64, count=len(labels)), len(index)


def segments(ids: np.ndarray, C: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(order int32 [N]: the rows grouped by class, stable; offsets int32 [C + 1]; counts int64 [C])."""
    if len(ids) > np.iinfo(np.int32).max:
        raise ValueError(f"{len(ids)} bank rows do not fit the int32 order table")
    counts = np.bincount(ids, minlength=C)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return order, offsets, counts


def _sym(S) -> torch.Tensor:
    S = torch.as_tensor(S, dtype=torch.float64, device="cpu")
    return (S + S.T) / 2


@dataclass
class ClassStatistics:
    """Step 1: counts [C], class means [C, D], global mean [D], S_w and S_b [D, D]; float64 on the host."""
    counts: torch.Tensor
    means: torch.Tensor
    mu0: torch.Tensor
    Sw: torch.Tensor
    Sb: torch.Tensor

    @property
    def N(self) -> int:
        return int(self.counts.sum())

    @property
    def C(self) -> int:
        return int(self.counts.numel())


def class_statistics_host(X, ids: np.ndarray, C: int) -> ClassStatistics:
    """Step 1 in float64 on the host: X [N, D] (any float dtype), ids int64 [N] in 0 .. C-1."""
    X = torch.as_tensor(X).detach().to("cpu", torch.float64)
    idt = torch.from_numpy(np.asarray(ids, dtype=np.int64))
    counts = torch.bincount(idt, minlength=C).to(torch.float64)
    means = torch.zeros(C, X.shape[1], dtype=torch.float64).index_add_(0, idt, X) / counts[:, None]
    mu0 = X.mean(dim=0)
    Xc = X - means[idt]
    Mc = (means - mu0) * counts.sqrt()[:, None]
    return ClassStatistics(counts, means, mu0, _sym(Xc.T @ Xc), _sym(Mc.T @ Mc))


def _top_eigen(S: torch.Tensor, R: int, what: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """The R largest eigenpairs of the symmetric S, descending; a kept eigenvalue at or below the floor raises."""
    lam, V = torch.linalg.eigh(S)
    lam, V = lam.flip(0)[:R], V.flip(1)[:, :R]
    if not bool(lam[0] > 0) or bool(lam[-1] <= EIG_FLOOR * lam[0]):
        raise ValueError(f"{what}: singular covariance (eigenvalue {float(lam[-1]):.3e} of the {R} kept against the largest "
                         f"{float(lam[0]):.3e}): reduce the number of components")
    return lam, V


def _check_rank(R, limit: int, what: str) -> int:
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= limit:
        raise ValueError(f"{what}: {R!r} components outside [1, {limit}]")
    return int(R)


def pca_projection(St, N: int, R: int) -> torch.Tensor:
    """Whitening PCA: the top-R eigenpairs (lambda, v) of S_t / (N - 1) -> P [R, D] with rows v / sqrt(lambda)."""
    St = _sym(St)
    R = _check_rank(R, min(St.shape[0], N - 1), "pca projection")
    lam, V = _top_eigen(St / (N - 1), R, "pca projection")
    return (V / lam.sqrt()).T.contiguous()


def lda_projection(Sw, Sb, N: int, C: int, R: int) -> torch.Tensor:
    """Whiten S_w / (N - C), then the top-R eigenvectors of the whitened S_b / (C - 1) -> P [R, D]; P S_w P^T / (N - C)
    is the identity."""
    Sw, Sb = _sym(Sw), _sym(Sb)
    D = Sw.shape[0]
    if N <= C:
        raise ValueError(f"lda projection: N = {N} rows of C = {C} classes leave no within-class scatter")
    R = _check_rank(R, min(D, C - 1), "lda projection")
    lam, V = _top_eigen(Sw / (N - C), D, "lda projection (within-class covariance)")
    T = (V / lam.sqrt()).T                                  # T (S_w / (N - C)) T^T = I
    lam_b, U = _top_eigen(_sym(T @ (Sb / (C - 1)) @ T.T), R, "lda projection (between-class covariance)")
    return (U.T @ T).contiguous()


def solve_projection(stats: ClassStatistics, R: int, projection: str) -> torch.Tensor:
    """Step 2, the one entry both fits call -> P [R, D] float64."""
    if projection not in PROJECTIONS:
        raise ValueError(f"projection={projection!r}: 'pca' or 'lda'")
    if stats.C < 2:
        raise ValueError(f"back-end fit: {stats.C} class(es): at least 2 speakers are needed")
    if projection == "pca":
        return pca_projection(stats.Sw + stats.Sb, stats.N, R)
    return lda_projection(stats.Sw, stats.Sb, stats.N, stats.C, R)


def plda_em(counts, means, mu, Sw, max_iterations: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two-covariance EM of step 4 over class-level statistics: counts [C], class means [C, R], mu [R], S_w [R, R] ->
    (B, W) float64.  Phi depends on n_c alone, so the classes are grouped by their count; the outer-product sums are
    matrix products.  With M = W + n B:  Phi = W M^-1 B  and  Phi n W^-1 = n B M^-1  (no inverse of B or W is formed)."""
    counts = torch.as_tensor(counts, dtype=torch.float64, device="cpu")
    means = torch.as_tensor(means, dtype=torch.float64, device="cpu")
    mu = torch.as_tensor(mu, dtype=torch.float64, device="cpu")
    Sw = _sym(Sw)
    C, N = counts.numel(), float(counts.sum())
    if C < 2:
        raise ValueError(f"plda: {C} class(es): at least 2 speakers are needed")
    if N <= C:
        raise ValueError(f"plda: N = {int(N)} rows of C = {C} classes leave no within-class scatter")
    dev = means - mu
    W = Sw / N
    B = _sym(dev.T @ dev / C)
    sizes, group = torch.unique(counts, return_inverse=True)
    for _ in range(int(max_iterations)):
        yhat = torch.empty_like(dev)
        phi_b = torch.zeros_like(B)                         # sum_c Phi_c
        phi_w = torch.zeros_like(B)                         # sum_c n_c Phi_c
        for g, n in enumerate(sizes.tolist()):
            rows = (group == g).nonzero().reshape(-1)
            try:
                K = torch.linalg.solve(W + n * B, B)        # M^-1 B
            except RuntimeError as e:
                raise ValueError(f"plda: singular covariance in the E-step ({e}): reduce the number of components") from e
            phi = _sym(W @ K)
            yhat[rows] = n * (dev[rows] @ K)                # rows: (n B M^-1 d)^T = n d^T M^-1 B
            phi_b += len(rows) * phi
            phi_w += len(rows) * n * phi
        res = (dev - yhat) * counts.sqrt()[:, None]
        B = _sym((phi_b + yhat.T @ yhat) / C)
        W = _sym((Sw + res.T @ res + phi_w) / N)
    return B, W


def plda_diagonalise(B, W, Q: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A with A W A^T = I and A B A^T = diag(psi), psi descending -> (A [Q, R], psi [Q]): the first Q rows (all R by
    default).  A singular W raises."""
    B, W = _sym(B), _sym(W)
    R = W.shape[0]
    Q = R if Q is None else _check_rank(Q, R, "plda components")
    lam, V = _top_eigen(W, R, "plda (within-class covariance)")
    T = (V / lam.sqrt()).T
    psi, U = torch.linalg.eigh(_sym(T @ B @ T.T))
    psi, U = psi.flip(0), U.flip(1)
    return (U.T @ T)[:Q].contiguous(), psi[:Q].clamp_min(0.0).contiguous()


def plda_coefficients(psi) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """(p [Q], q [Q], k) of the closed-form llr from the between-class variances psi of the diagonalised model."""
    psi = torch.as_tensor(psi, dtype=torch.float64, device="cpu")
    p = psi / (2 * psi + 1)
    q = psi * psi / (2 * (psi + 1) * (2 * psi + 1))
    k = float((torch.log1p(psi) - 0.5 * torch.log1p(2 * psi)).sum())
    return p, q, k


def solve_plda(counts, means, mu, Sw, Q: int, max_iterations: int):
    """Step 4 on the host, the one entry both fits call -> (A [Q, R], psi [Q], p [Q], q [Q], k)."""
    B, W = plda_em(counts, means, mu, Sw, max_iterations)
    A, psi = plda_diagonalise(B, W, Q)
    p, q, k = plda_coefficients(psi)
    return A, psi, p, q, k


def pad4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


def padded_rows(M: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """M [r, c] float64 -> float32 [rows, cols] with zeros behind it (the GEMM operand of a projection)."""
    out = torch.zeros(rows, cols, dtype=torch.float32)
    out[:M.shape[0], :M.shape[1]] = M.to(torch.float32)
    return out
