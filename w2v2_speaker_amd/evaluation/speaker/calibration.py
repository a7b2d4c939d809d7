"""Score calibration and linear fusion: trial scores -> log-likelihood ratios, and Cllr / actDCF of the result.

The definition is the "score calibration" block of include/w2v2_hip.h (the reference project has no calibration): a
prior-weighted logistic regression of K systems' scores on standardised features, fitted by Newton steps with step
halving, mapped back to ``llr = a_0 + sum_k a_k s_k``.  K = 1 calibrates one system, K > 1 fuses several.  Device tensors
take the kernels of csrc/calibration.hip (ops.calib_fit / calib_apply / llr_metrics: the whole fit is enqueued at once and
its state lives in one f64 record on the device); CPU tensors and arrays take the same definition in float64 numpy, which
is also what the evaluators' host path (``evaluate(..., calibration=)``) uses."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from ...ops import cost_checks as check_costs       # one statement of calculate_mdc's conditions, the wrappers' own

MAX_SYSTEMS = 8
DEC_STOP = 1e-12
STEP_MIN = 2.0 ** -20
LLR_KEYS = ("cllr", "act_dcf", "act_p_miss", "act_p_fa")
STATUS_CAUSE = {
    0: "not converged after {rounds} rounds (max_iter={max_iter}): development scores that a threshold separates have no "
       "finite optimum -- fit with ridge > 0, or raise max_iter",
    2: "the fit failed: {detail}",
    3: "the step fell below 2^-20 without a decrease of the objective after {rounds} rounds",
}


class CalibrationError(ValueError):
    """A fit that did not end with status 1 (converged); ``status`` and ``fields`` keep what the record said."""

    def __init__(self, message: str, status: int, fields: Optional[dict] = None):
        super().__init__(message)
        self.status, self.fields = status, fields


def effective_prior(c_miss, c_fa, p_target) -> float:
    t = float(p_target) * float(c_miss)
    return t / (t + (1.0 - float(p_target)) * float(c_fa))


def bayes_threshold(c_miss, c_fa, p_target) -> float:
    """theta = -log(pi / (1 - pi)); +inf / -inf at an effective prior of 0 / 1."""
    pi = effective_prior(c_miss, c_fa, p_target)
    if pi <= 0.0:
        return math.inf
    if pi >= 1.0:
        return -math.inf
    return -math.log(pi / (1.0 - pi))


# ------------------------------------------------------------------------------------------------ the definition in numpy
def _sigmoid_pair(z: np.ndarray):
    """(sigma(z), sigma(-z), log1p(exp(-|z|))) from one exponential, each quotient safe from overflow."""
    e = np.exp(-np.abs(z))
    inv = 1.0 / (1.0 + e)
    big, small = inv, e * inv
    pos = z >= 0
    return np.where(pos, big, small), np.where(pos, small, big), np.log1p(e)


def statistics_numpy(X: np.ndarray, y: np.ndarray, w: np.ndarray, pi: float, ridge: float = 0.0):
    """Step 2 on standardised features X [P, K + 1] (column 0 all ones), labels y (bool [P]) -> (J, g, H) float64."""
    tau = math.log(pi / (1.0 - pi))
    c = np.where(y, pi / y.sum(), (1.0 - pi) / (~y).sum())
    z = X @ w + tau
    p, q, lp = _sigmoid_pair(z)
    J = float(np.sum(c * (np.maximum(np.where(y, -z, z), 0.0) + lp)) + 0.5 * ridge * np.sum(w[1:] ** 2))
    g = X.T @ (c * np.where(y, -q, p))
    H = (X * (c * p * q)[:, None]).T @ X
    g[1:] += ridge * w[1:]
    H[np.arange(1, len(w)), np.arange(1, len(w))] += ridge
    return J, g, H


def fit_numpy(scores, labels, c_miss=1, c_fa=1, p_target=0.05, ridge=0.0, max_iter=32) -> dict:
    """Steps 1-4 in float64 numpy: scores [K, P] (or [P]), labels [P] of 0 / 1 -> the fields of the device record (status,
    rounds, K, J, decrement, n_tar, n_non, n_nan, w, mean, sd, r, a, g, H) as a dict."""
    S = np.atleast_2d(np.asarray(scores, dtype=np.float64))
    y = np.asarray(labels).reshape(-1) != 0
    K, P = S.shape
    n_tar, n_nan = int(y.sum()), int(np.isnan(S).any(axis=0).sum())
    out = {"status": 0, "rounds": 0, "K": K, "J": math.inf, "decrement": 0.0, "n_tar": n_tar, "n_non": P - n_tar,
           "n_nan": n_nan, "w": [0.0] * (K + 1), "a": [0.0] * (K + 1), "mean": [0.0] * K, "sd": [0.0] * K, "r": [0.0] * K}
    if n_nan or n_tar == 0 or n_tar == P:
        out["status"] = 2
        return out
    with np.errstate(all="ignore"):
        m = S.sum(axis=1) / P
        sd = np.sqrt(((S - m[:, None]) ** 2).sum(axis=1) / (P - 1))
        r = 1.0 / sd
    out.update(mean=m.tolist(), sd=sd.tolist(), r=r.tolist())
    if not (np.all(sd > 0) and np.all(np.isfinite(sd)) and np.all(np.isfinite(r))):
        out["status"] = 2
        return out
    X = np.concatenate([np.ones((P, 1)), ((S - m[:, None]) * r[:, None]).T], axis=1)
    pi = effective_prior(c_miss, c_fa, p_target)
    w = np.zeros(K + 1)
    wt, d, step, J_acc = w.copy(), np.zeros(K + 1), 1.0, math.inf
    for rounds in range(1, int(max_iter) + 1):
        out["rounds"] = rounds
        with np.errstate(all="ignore"):
            J, g, H = statistics_numpy(X, y, wt, pi, ridge)
        if not (np.isfinite(J) and np.all(np.isfinite(g)) and np.all(np.isfinite(H))):
            out["status"] = 2
            break
        if rounds > 1 and J > J_acc:
            step *= 0.5
            if step < STEP_MIN:
                out["status"] = 3
                break
            wt = w - step * d
            continue
        w, J_acc = wt.copy(), J
        out.update(J=J, g=g.tolist(), H=H.tolist())
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            out["status"] = 2
            break
        d = np.linalg.solve(L.T, np.linalg.solve(L, g))
        dec = float(g @ d) / 2
        out["decrement"] = dec
        if not np.isfinite(dec):
            out["status"] = 2
            break
        c_min = min(pi / n_tar, (1.0 - pi) / (P - n_tar))
        separated = ridge == 0 and J < c_min * math.log(2.0)   # every trial on its right side: no finite optimum
        if dec < DEC_STOP and not separated:
            out["status"] = 1
            break
        step, wt = 1.0, w - d
    a = w[1:] * r
    out.update(w=w.tolist(), a=[float(w[0] - np.sum(a * m))] + a.tolist())
    return out


def apply_numpy(scores, a: Sequence[float]) -> np.ndarray:
    """Step 5 in float64: scores [K, P] (or [P]) -> llr float64 [P] (NOT rounded to f32)."""
    S = np.atleast_2d(np.asarray(scores, dtype=np.float64))
    llr = np.full(S.shape[1], float(a[0]))
    for k in range(S.shape[0]):
        llr = llr + float(a[k + 1]) * S[k]
    return llr


def llr_metrics_numpy(llr, labels, c_miss=1, c_fa=1, p_target=0.05) -> dict:
    """Step 6 in float64 numpy -> the eight outputs of w2v2_llr_metrics by name."""
    check_costs(c_miss, c_fa, p_target)
    z = np.asarray(llr, dtype=np.float64).reshape(-1)
    y = np.asarray(labels).reshape(-1) != 0
    theta = bayes_threshold(c_miss, c_fa, p_target)
    nan = np.isnan(z)
    with np.errstate(all="ignore"):
        sp = np.maximum(np.where(y, -z, z), 0.0) + np.log1p(np.exp(-np.abs(z)))
        n_tar, n_non = float(y.sum()), float((~y).sum())
        cllr_tar = float(np.sum(sp[y]) / n_tar / math.log(2.0)) if n_tar else math.nan
        cllr_non = float(np.sum(sp[~y]) / n_non / math.log(2.0)) if n_non else math.nan
        p_miss = float(np.sum(y & (z < theta))) / n_tar if n_tar else math.nan
        p_fa = float(np.sum(~y & (z >= theta))) / n_non if n_non else math.nan
    c_det = c_miss * p_miss * p_target + c_fa * p_fa * (1 - p_target)
    c_def = min(c_miss * p_target, c_fa * (1 - p_target))
    with np.errstate(all="ignore"):
        act = float(np.float64(c_det) / np.float64(c_def))
    return {"cllr": 0.5 * (cllr_tar + cllr_non), "cllr_tar": cllr_tar, "cllr_non": cllr_non, "act_dcf": act,
            "act_p_miss": p_miss, "act_p_fa": p_fa, "n_pos": n_tar, "n_nan": float(nan.sum())}


# ------------------------------------------------------------------------------------------------ the user's side
class ScoreCalibration:
    """``fit_scores`` / ``fit_bank`` fit the affine map, ``apply`` maps scores to llrs.  ``p_target``, ``c_miss``, ``c_fa``
    give the operating point the fit is weighted for and the Bayes threshold of actDCF; ``ridge`` >= 0 penalises the
    slopes (not the offset) of the standardised features.  Nothing here is a default of any evaluator."""

    def __init__(self, p_target: float = 0.05, c_miss: float = 1, c_fa: float = 1, max_iter: int = 32, ridge: float = 0.0):
        check_costs(c_miss, c_fa, p_target, open_prior=True)
        if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not 1 <= max_iter <= 4096:
            raise ValueError(f"max_iter = {max_iter!r} outside [1, 4096]")
        if not (isinstance(ridge, (int, float)) and 0 <= ridge < math.inf):
            raise ValueError(f"ridge = {ridge!r} must be a finite number >= 0")
        self.p_target, self.c_miss, self.c_fa, self.max_iter, self.ridge = p_target, c_miss, c_fa, max_iter, float(ridge)
        self.record = None                   # the f64 record on the device (device fits only)
        self._fields = None                  # its one host copy, or the numpy fit's dict
        self.num_systems = None
        self.last_fit_scoring = None         # fit_bank: the DeviceScores of the members

    # ------------------------------------------------------------------ fitting
    def fit_scores(self, scores, labels) -> "ScoreCalibration":
        """scores [K, P] (or [P]: one system), labels [P] of 0 / 1.  Device tensors: the kernels (the scores are used as
        float32, the labels as uint8; one copy of the record crosses, to check the status).  CPU tensors / arrays: float64
        numpy.  Raises CalibrationError unless the fit converged."""
        if isinstance(scores, torch.Tensor) and scores.is_cuda:
            from ... import ops
            labels = torch.as_tensor(labels)
            if labels.dtype != torch.uint8:
                labels = (labels != 0).to(torch.uint8)
            labels = labels.to(scores.device).reshape(-1).contiguous()
            s = scores.detach()
            if s.dtype != torch.float32:
                s = s.float()
            if s.stride(-1) != 1:
                s = s.contiguous()
            self.record = ops.calib_fit(s, labels, self.c_miss, self.c_fa, self.p_target, self.ridge, self.max_iter)
            self._fields = ops.calib_record_fields(self.record)
        else:
            s = scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
            l = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
            if s.ndim not in (1, 2) or not 1 <= np.atleast_2d(s).shape[0] <= MAX_SYSTEMS or np.atleast_2d(s).shape[1] < 1:
                raise ValueError(f"scores is [K, P] (or [P]) with 1 <= K <= {MAX_SYSTEMS} systems and P >= 1 trials")
            if l.reshape(-1).shape[0] != np.atleast_2d(s).shape[1]:
                raise ValueError(f"one label per trial (P = {np.atleast_2d(s).shape[1]})")
            self.record = None
            self._fields = fit_numpy(s, l, self.c_miss, self.c_fa, self.p_target, self.ridge, self.max_iter)
        self.num_systems = self._fields["K"]
        self._raise_unless_converged()
        return self

    def _raise_unless_converged(self) -> None:
        f = self._fields
        st = f["status"]
        if st == 1:
            return
        detail = ""
        if st == 2:
            if f["n_nan"] > 0:
                detail = f"{int(f['n_nan'])} trial(s) with a NaN score"
            elif f["n_tar"] == 0 or f["n_non"] == 0:
                detail = "one class is absent from the development trials"
            elif not all(v > 0 and math.isfinite(v) and math.isfinite(1 / v) for v in f["sd"]):
                k = [i for i, v in enumerate(f["sd"]) if not (v > 0 and math.isfinite(v))]
                detail = f"system(s) {k} have a constant (sd = 0) or non-finite score"
            else:
                detail = "the Hessian is not positive definite or a sum is not finite (collinear systems? try ridge > 0)"
        msg = STATUS_CAUSE.get(st, "status {status}").format(rounds=f["rounds"], max_iter=self.max_iter, detail=detail, status=st)
        raise CalibrationError(f"calibration: {msg}", st, f)

    def fit_bank(self, evaluator, pairs, keys, bank, score_norm=None) -> "ScoreCalibration":
        """Score a development trial list with ``evaluator`` (cosine, LDA or PLDA) on the device and fit on those scores,
        which never leave it.  ``bank``: an [N, D] device tensor, or a list of K of them (K systems: a fusion).  The scores
        are what the evaluator's metrics would see without a calibration (the cosine back-ends' (s + 1) / 2, the PLDA llr,
        the normalised score with ``score_norm``)."""
        from .device_scoring import TrialIndex
        index = TrialIndex(pairs, keys)
        if index.missing is not None:
            raise ValueError(f"{index.missing[0]} or {index.missing[1]} not in the bank")
        members = list(bank) if isinstance(bank, (list, tuple)) else [bank]
        S = member_scores_device(evaluator, members, index, score_norm)
        return self.fit_scores(S, index.device_labels(S.device))

    # ------------------------------------------------------------------ the fitted map
    @property
    def status(self) -> int:
        self._require_fit()
        return self._fields["status"]

    @property
    def fields(self) -> dict:
        self._require_fit()
        return self._fields

    @property
    def weights(self) -> np.ndarray:
        """(a_0, a_1 .. a_K) float64: llr = a_0 + sum_k a_k s_k."""
        self._require_fit()
        return np.asarray(self._fields["a"], dtype=np.float64)

    def _require_fit(self) -> None:
        if self._fields is None:
            raise ValueError("calibration: fit_scores() / fit_bank() has not been called")

    def _device_map(self, device) -> torch.Tensor:
        if self.record is not None and self.record.device == torch.device(device):
            return self.record
        return torch.from_numpy(self.weights).to(device)

    def apply(self, scores):
        """scores [K, P] (or [P] for K = 1) -> llr [P]: a device tensor gives a float32 device tensor (ops.calib_apply, the
        map read on the device); a CPU tensor or an array gives float64 numpy."""
        self._require_fit()
        if isinstance(scores, torch.Tensor) and scores.is_cuda:
            from ... import ops
            s = scores.detach()
            if s.dtype != torch.float32:
                s = s.float()
            if s.stride(-1) != 1:
                s = s.contiguous()
            if (1 if s.dim() == 1 else s.shape[0]) != self.num_systems:
                raise ValueError(f"calibration: fitted on {self.num_systems} system(s)")
            return ops.calib_apply(s, self._device_map(s.device))
        s = scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
        if np.atleast_2d(s).shape[0] != self.num_systems:
            raise ValueError(f"calibration: fitted on {self.num_systems} system(s)")
        return apply_numpy(s, self.weights)

    def llr_metrics_host(self, llr, labels) -> dict:
        """cllr / act_dcf / act_p_miss / act_p_fa of host llrs at this calibration's operating point."""
        m = llr_metrics_numpy(llr, labels, self.c_miss, self.c_fa, self.p_target)
        return {k: m[k] for k in LLR_KEYS}


def member_scores_device(evaluator, members, index, score_norm=None) -> torch.Tensor:
    """The uncalibrated metric scores of every member bank, on the device: float32 [K, P]."""
    if not 1 <= len(members) <= MAX_SYSTEMS:
        raise ValueError(f"calibration: {len(members)} systems outside [1, {MAX_SYSTEMS}]")
    rows = [evaluator._metric_scores_device(b, index, score_norm) for b in members]
    if len(rows) == 1:
        return rows[0].unsqueeze(0)
    return torch.stack(rows)


def llr_keys_device(llr: torch.Tensor, index, c_miss=1, c_fa=1, p_target=0.05, record: Optional[list] = None) -> dict:
    """cllr / act_dcf / act_p_miss / act_p_fa of device llrs: ops.llr_metrics and one copy of eight doubles."""
    from ... import ops
    out = ops.llr_metrics(llr, index.device_labels(llr.device), c_miss, c_fa, p_target).cpu().tolist()
    fields = dict(zip(ops.LLR_METRICS_FIELDS, out))
    if record is not None:
        record.append(fields)
    return {k: fields[k] for k in LLR_KEYS}
