"""Cases of the score calibration (csrc/calibration.hip, evaluation/speaker/calibration.py) with their float64 oracle.  No
GPU and no ``ops`` import here: test_calibration_cpu.py holds the oracle to scipy and the numpy path of ScoreCalibration to
the oracle, test_calibration_gpu.py holds the kernels to the oracle.

The oracle is the "score calibration" block of include/w2v2_hip.h written independently of the package in float64 numpy:
``moments`` / ``features`` (step 1), ``stats`` (step 2, with the sum of the magnitudes of every output's terms for the
kernel's bound), ``newton`` (a plain damped Newton iteration: no status codes, no record), ``decrement`` (the stop
quantity g.H^-1 g / 2 at any point), ``affine`` (step 4), ``apply_ref`` (step 5 with the f32 rounding-boundary test) and
``llr_metrics_ref`` (step 6).

Bounds:
  statistics   1e-12 * sum_i |term_i| per output (J, every g_k, every H_kl): 2^-53 = 1.1e-16, so this leaves room for a
               sequential chain of a few thousand additions and a few ulp per transcendental.
  fit          the ORACLE's decrement at the device's weights <= 1e-10: the stop rule's 1e-12 plus the statistics bound.
  moments      mean: 1e-12 * mean |s|; sd: 1e-12 relative (a sum of non-negative terms, its first-order dependence on the
               mean vanishes); affine map: 1e-11 relative to sum_k |a_k m_k| + |w_0| (exact formulas of rounded inputs).
  apply        equal bits away from an f32 rounding boundary, one f32 ulp at one; no committed input is at one.
  llr metrics  counts and the three actual-cost figures exact; cllr 1e-12 relative.

Every fitted case is non-separable by construction, and ``fitted_cases`` asserts it with a linear programme: no w != 0 has
y_i w.x_i >= 0 for every trial (neither complete nor quasi-complete separation), so the optimum is finite."""
import functools
import math

import numpy as np

STAT_REL = 1e-12
FIT_DECREMENT = 1e-10
CLLR_REL = 1e-12
PRIORS = (0.01, 0.05, 0.5)
SYSTEMS = (1, 2, 3, 8)
PAD = 12


def sizes(tile: int):
    return (2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5)


def effective_prior(p_target, c_miss=1.0, c_fa=1.0):
    return p_target * c_miss / (p_target * c_miss + (1.0 - p_target) * c_fa)


def theta_of(p_target, c_miss=1.0, c_fa=1.0):
    pi = effective_prior(p_target, c_miss, c_fa)
    if pi <= 0:
        return math.inf
    if pi >= 1:
        return -math.inf
    return -math.log(pi / (1.0 - pi))


# ------------------------------------------------------------------------------------------------ score families
def _labels(rng, P, share=0.3):
    y = (rng.random(P) < share).astype(np.uint8)
    y[0], y[1] = 1, 0                                   # both classes, whatever the draw
    return y


def family(name: str, P: int, K: int, seed: int):
    """-> (S float32 [K, P], y uint8 [P]) of the named family."""
    rng = np.random.default_rng(1000 * seed + 17 * P + K)
    y = _labels(rng, P)
    yf = y.astype(np.float64)
    if name.startswith("gauss"):                        # "gauss0.2" .. "gauss2.5": separation in standard deviations
        sep = float(name[5:])
        S = rng.standard_normal((K, P)) + sep * yf * (0.5 + 0.5 * rng.random((K, 1)))
    elif name == "plda":                                # llr-like: scale 40, offset
        S = 40.0 * (rng.standard_normal((K, P)) + 1.2 * yf) - 25.0
    elif name == "cosine":                              # (cos + 1) / 2 clipped to [0, 1]
        S = np.clip(0.45 + 0.17 * rng.standard_normal((K, P)) + 0.2 * yf, 0.0, 1.0)
    elif name == "ties":                                # seven distinct values
        S = np.clip(np.round(3.0 + 1.2 * rng.standard_normal((K, P)) + 1.0 * yf), 0, 6) / 6.0
        S[:, :min(7, P)] = (np.arange(7) / 6.0)[None, :min(7, P)]       # every value present: no constant system
    elif name == "one_target":                          # one target among P, strictly inside the non-targets' range
        y = np.zeros(P, dtype=np.uint8)
        S = rng.standard_normal((K, P))
        at = P // 3
        y[at] = 1
        for k in range(K):
            S[k, at] = np.sort(np.delete(S[k], at))[int(0.9 * (P - 1))] + 1e-3
    elif name == "collinear":                           # system 2 = system 1 + 2 % noise; further systems independent
        S = rng.standard_normal((K, P)) + 1.0 * yf
        if K > 1:
            S[1] = S[0] + 0.02 * rng.standard_normal(P)
    else:
        raise KeyError(name)
    return S.astype(np.float32), y


def padded(S: np.ndarray, pad: int = PAD) -> np.ndarray:
    """[K, P] -> the same values as a view of a [K, P + pad] buffer whose pad holds NaN (the pad must not be read)."""
    buf = np.full((S.shape[0], S.shape[1] + pad), np.nan, dtype=S.dtype)
    buf[:, :S.shape[1]] = S
    return buf


def start_point(K: int, seed: int) -> np.ndarray:
    """A moderate w for the forced single round of the statistics test."""
    rng = np.random.default_rng(77 + seed)
    return np.concatenate([[0.3], 0.7 * rng.standard_normal(K)])


@functools.lru_cache(maxsize=None)
def stat_cases(tile: int):
    """(name, P, K, p_target, pad) of the statistics / apply cases: every size x every K, the families and priors cycled."""
    fams = ("gauss0.2", "plda", "cosine", "ties", "gauss2.5", "collinear", "gauss1.0")
    out, n = [], 0
    for P in sizes(tile):
        for K in SYSTEMS:
            out.append((fams[n % len(fams)], P, K, PRIORS[n % 3], PAD if n % 2 else 0))
            n += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fitted_cases(tile: int):
    """(name, P, K, p_target, pad) of the cases that are fitted: P >= 63, every family, every K, the three priors; each is
    asserted non-separable here."""
    T = tile
    out = [("gauss0.2", 63, 1, 0.05, 0), ("gauss1.0", 64, 2, 0.5, PAD), ("gauss2.5", T + 1, 1, 0.01, PAD),
           ("gauss1.5", 65, 3, 0.05, 0), ("plda", T - 1, 1, 0.05, PAD), ("plda", 3 * T + 5, 3, 0.01, 0),
           ("cosine", T, 1, 0.05, 0), ("cosine", 3 * T + 5, 8, 0.5, PAD), ("ties", T + 1, 2, 0.05, 0),
           ("ties", 513, 1, 0.5, PAD), ("one_target", 5000, 1, 0.05, 0), ("one_target", 5000, 2, 0.01, PAD),
           ("collinear", T, 2, 0.05, 0), ("collinear", 3 * T + 5, 3, 0.5, PAD), ("gauss1.0", T - 1, 8, 0.05, 0)]
    for name, P, K, _, _ in out:
        S, y = family(name, P, K, 1)
        m, sd = moments(S)
        assert not separable(features(S, m, 1.0 / sd), y), (name, P, K)
    return tuple(out)


def separable(X: np.ndarray, y) -> bool:
    """Complete or quasi-complete separation of the rows of X [P, K + 1] (column 0 ones, full column rank) by labels y: a
    w != 0 with t_i w.x_i >= 0 for all i (t = +-1).  LP: maximise sum_i t_i w.x_i under those constraints and |w_k| <= 1;
    the optimum is 0 exactly when only w with t_i w.x_i = 0 for every i -- w = 0 at full rank -- is feasible."""
    from scipy.optimize import linprog
    A = X * np.where(np.asarray(y) != 0, 1.0, -1.0)[:, None]
    assert np.linalg.matrix_rank(X) == X.shape[1]
    res = linprog(-A.sum(axis=0), A_ub=-A, b_ub=np.zeros(len(A)), bounds=[(-1, 1)] * X.shape[1], method="highs")
    assert res.status == 0, res.message
    return -res.fun > 1e-9 * len(A)


# ------------------------------------------------------------------------------------------------ the oracle
def moments(S):
    """(m [K], sd [K]) float64 of scores [K, P]: mean and unbiased std, two passes."""
    S = np.asarray(S, dtype=np.float64)
    P = S.shape[1]
    m = np.array([math.fsum(row) / P for row in S])
    sd = np.array([math.sqrt(math.fsum((row - mk) ** 2) / (P - 1)) for row, mk in zip(S, m)])
    return m, sd


def features(S, m, r):
    S = np.asarray(S, dtype=np.float64)
    return np.concatenate([np.ones((S.shape[1], 1)), ((S - m[:, None]) * r[:, None]).T], axis=1)


def _parts(z):
    e = np.exp(-np.abs(z))
    p_big, p_small = 1.0 / (1.0 + e), e / (1.0 + e)
    p = np.where(z >= 0, p_big, p_small)
    q = np.where(z >= 0, p_small, p_big)
    return p, q, np.log1p(e)


def stats(X, y, w, pi, ridge=0.0, with_abs=False):
    """J, g, H of step 2 at w -> (J, g [N], H [N, N]) and, with ``with_abs``, the sums of |term| of each: (J, g, H, Ja, ga, Ha)."""
    y = np.asarray(y) != 0
    w = np.asarray(w, dtype=np.float64)
    tau = math.log(pi / (1.0 - pi))
    c = np.where(y, pi / y.sum(), (1.0 - pi) / (~y).sum())
    z = X @ w + tau
    p, q, lp = _parts(z)
    jt = c * (np.maximum(np.where(y, -z, z), 0.0) + lp)
    gt = (c * np.where(y, -q, p))[:, None] * X
    ht = (c * p * q)[:, None, None] * X[:, :, None] * X[:, None, :]
    N = len(w)
    pen = np.concatenate([[0.0], np.full(N - 1, float(ridge))])
    J = math.fsum(jt) + 0.5 * ridge * float(np.sum(w[1:] ** 2))
    g = np.array([math.fsum(gt[:, a]) for a in range(N)]) + pen * w
    H = np.array([[math.fsum(ht[:, a, b]) for b in range(N)] for a in range(N)]) + np.diag(pen)
    if not with_abs:
        return J, g, H
    return J, g, H, float(np.abs(jt).sum()), np.abs(gt).sum(axis=0), np.abs(ht).sum(axis=0)


def stats_fast(X, y, w, pi, ridge=0.0):
    """The same J, g, H by matrix products (the solver's inner loop; ``stats`` is the element-by-element form)."""
    y = np.asarray(y) != 0
    tau = math.log(pi / (1.0 - pi))
    c = np.where(y, pi / y.sum(), (1.0 - pi) / (~y).sum())
    z = X @ w + tau
    p, q, lp = _parts(z)
    N = len(w)
    pen = np.concatenate([[0.0], np.full(N - 1, float(ridge))])
    J = float(np.sum(c * (np.maximum(np.where(y, -z, z), 0.0) + lp))) + 0.5 * ridge * float(np.sum(w[1:] ** 2))
    return J, X.T @ (c * np.where(y, -q, p)) + pen * w, (X * (c * p * q)[:, None]).T @ X + np.diag(pen)


def decrement(X, y, w, pi, ridge=0.0):
    _, g, H = stats_fast(X, y, np.asarray(w, dtype=np.float64), pi, ridge)
    return float(g @ np.linalg.solve(H, g)) / 2


def newton(X, y, pi, ridge=0.0, max_rounds=200, stop=1e-13):
    """A plain Newton iteration from w = 0, each step halved until J does not rise -> (w, J, statistics evaluations)."""
    w = np.zeros(X.shape[1])
    J, g, H = stats_fast(X, y, w, pi, ridge)
    evals = 1
    while evals < max_rounds:
        d = np.linalg.solve(H, g)
        if float(g @ d) / 2 < stop:
            break
        t = 1.0
        while True:
            Jn, gn, Hn = stats_fast(X, y, w - t * d, pi, ridge)
            evals += 1
            if Jn <= J or t < 2.0 ** -30:
                break
            t *= 0.5
        w, J, g, H = w - t * d, Jn, gn, Hn
    return w, J, evals


def affine(w, m, r):
    a = np.asarray(w[1:]) * r
    return np.concatenate([[w[0] - float(np.sum(a * m))], a])


def apply_ref(S, a):
    """llr of step 5: (the f32 the kernel must write, the float64 value, the mask of values within 2^-52 relative of an f32
    rounding boundary).  The float64 value takes the kernel's order: a_0, then + a_k * s_k with k ascending."""
    S = np.asarray(S, dtype=np.float32)
    v = np.full(S.shape[1], float(a[0]))
    for k in range(S.shape[0]):
        v = v + float(a[k + 1]) * S[k].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = v.astype(np.float32)
        other = np.where(f.astype(np.float64) <= v, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf)))
        mid = (f.astype(np.float64) + other.astype(np.float64)) / 2
        boundary = np.isfinite(v) & (np.abs(v - mid) <= 2.0 ** -52 * np.abs(v))
    return f, v, boundary


def llr_metrics_ref(llr, y, c_miss=1.0, c_fa=1.0, p_target=0.05, f32=True):
    """Step 6 in float64 -> dict of the eight outputs; ``f32``: the llrs are the kernel's f32 values (the host path of the
    evaluators keeps float64 llrs: f32=False)."""
    z = np.asarray(llr, dtype=np.float32).astype(np.float64) if f32 else np.asarray(llr, dtype=np.float64)
    y = np.asarray(y) != 0
    theta = theta_of(p_target, c_miss, c_fa)
    with np.errstate(all="ignore"):
        sp = np.maximum(np.where(y, -z, z), 0.0) + np.log1p(np.exp(-np.abs(z)))
    n_tar, n_non = int(y.sum()), int((~y).sum())

    def total(v):
        return math.fsum(v) if np.isfinite(v).all() else float(np.sum(v))
    ct, cn = total(sp[y]) / n_tar / math.log(2.0), total(sp[~y]) / n_non / math.log(2.0)
    p_miss, p_fa = int(np.sum(y & (z < theta))) / n_tar, int(np.sum(~y & (z >= theta))) / n_non
    c_det = c_miss * p_miss * p_target + c_fa * p_fa * (1 - p_target)
    return {"cllr": 0.5 * (ct + cn), "cllr_tar": ct, "cllr_non": cn,
            "act_dcf": c_det / min(c_miss * p_target, c_fa * (1 - p_target)), "act_p_miss": p_miss, "act_p_fa": p_fa,
            "n_pos": float(n_tar), "n_nan": float(np.isnan(z).sum())}


# ------------------------------------------------------------------------------------------------ llr metric cases
@functools.lru_cache(maxsize=None)
def llr_cases(tile: int):
    """name -> (llr f32 [P], y uint8 [P], p_target): tile edges, llrs equal to theta (p_target 0.5: theta = 0, both zeros),
    the f32 neighbours of an irrational theta, +-inf on the harmless and on the costly side."""
    out = {}
    for n, P in enumerate(sizes(tile)):
        rng = np.random.default_rng(300 + P)
        y = _labels(rng, P)
        z = (3.0 * rng.standard_normal(P) + 4.0 * y - 2.0).astype(np.float32)
        out[f"size{P}"] = (z, y, PRIORS[n % 3])
    rng = np.random.default_rng(9)
    P = tile + 9
    y = _labels(rng, P)
    z = (2.0 * rng.standard_normal(P) + 2.0 * y).astype(np.float32)
    z0 = z.copy()
    z0[2:10] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0]
    y0 = y.copy()
    y0[2:10] = [1, 1, 0, 0, 1, 0, 1, 0]
    out["equal_theta_zero"] = (z0, y0, 0.5)
    th = np.float32(theta_of(0.05))
    lo, hi = (th, np.nextafter(th, np.float32(np.inf))) if float(th) < theta_of(0.05) else (np.nextafter(th, np.float32(-np.inf)), th)
    assert float(lo) < theta_of(0.05) < float(hi)
    zn = z.copy()
    zn[2:10] = [lo, hi, lo, hi, lo, hi, hi, lo]
    out["theta_neighbours"] = (zn, y0, 0.05)
    zi = z.copy()
    zi[2:6] = [np.inf, np.inf, -np.inf, -np.inf]
    yi = y.copy()
    yi[2:6] = [1, 1, 0, 0]
    out["inf_harmless"] = (zi, yi, 0.05)
    yb = yi.copy()
    yb[2:6] = [0, 1, 0, 1]
    out["inf_costly"] = (zi, yb, 0.01)
    return out


# ------------------------------------------------------------------------------------------------ sets that must fail
def separable_set(P=400, seed=3):
    """Targets strictly above every non-target (gap 0.05 sd): no finite optimum."""
    rng = np.random.default_rng(seed)
    y = _labels(rng, P)
    s = rng.standard_normal(P)
    s = np.where(y != 0, np.abs(s) + 0.05, -np.abs(s))
    return s[None, :].astype(np.float32), y


def constant_system(P=300, seed=4):
    S, y = family("gauss1.0", P, 2, seed)
    S[1] = 0.25
    return S, y


def one_class(P=100, seed=5):
    S, _ = family("gauss1.0", P, 1, seed)
    return S, np.ones(P, dtype=np.uint8)
