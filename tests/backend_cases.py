"""The float64 oracle of the LDA / PLDA scoring back-ends (the "scoring back-ends" block of include/w2v2_hip.h), the case
generators and the bounds of tests/test_backend_cpu.py and tests/test_backend_gpu.py.

The oracle is plain numpy written from the definition, with a Python loop over the classes wherever the product code
groups or batches: it shares no code with w2v2_speaker_amd.evaluation.speaker.backend.  With ``work=np.float32`` every
O(N) and O(P) step -- the sums of the statistics, the projections, the latent transform, the score -- runs in f32 numpy
while the solves stay in float64: a plain f32 implementation, whose distance from the all-float64 oracle is the yardstick
of the device path (the eigen-solves amplify the statistics' rounding by the problem's conditioning, so no fixed bound is
right)."""
from __future__ import annotations

import numpy as np

EIG_FLOOR = 1e-10
DEVICE_MARGIN = 4.0         # the device may be this many times as far from float64 as the f32 numpy pipeline is
EER_RATIO = 0.6             # PLDA EER from the device <= EER_RATIO x plain-cosine EER of the raw test bank


# ------------------------------------------------------------------------------------------ the definition, step by step
def ids_of(labels):
    speakers = sorted(set(labels))
    index = {s: i for i, s in enumerate(speakers)}
    return np.array([index[l] for l in labels], dtype=np.int64), len(speakers)


def class_statistics(X, ids, C, work=np.float64):
    """counts, class means, global mean, S_w, S_b -- summed in ``work``, returned as float64."""
    X = X.astype(work)
    counts = np.bincount(ids, minlength=C)
    means = np.stack([X[ids == c].sum(axis=0, dtype=work) / work(counts[c]) for c in range(C)])
    mu0 = X.sum(axis=0, dtype=work) / work(len(X))
    Sw = np.zeros((X.shape[1], X.shape[1]), dtype=work)
    for c in range(C):
        A = X[ids == c] - means[c]
        Sw += A.T @ A
    M = (means - mu0) * np.sqrt(counts.astype(work))[:, None]
    Sb = M.T @ M
    f = np.float64
    return counts.astype(f), means.astype(f), mu0.astype(f), (Sw.astype(f) + Sw.astype(f).T) / 2, (Sb.astype(f) + Sb.astype(f).T) / 2


def _top(S, R):
    lam, V = np.linalg.eigh((S + S.T) / 2)
    lam, V = lam[::-1][:R], V[:, ::-1][:, :R]
    if lam[-1] <= EIG_FLOOR * lam[0]:
        raise ValueError("singular covariance")
    return lam, V


def projection(counts, Sw, Sb, R, kind):
    N, C = int(counts.sum()), len(counts)
    if kind == "pca":
        lam, V = _top((Sw + Sb) / (N - 1), R)
        return (V / np.sqrt(lam)).T
    lam, V = _top(Sw / (N - C), Sw.shape[0])
    T = (V / np.sqrt(lam)).T
    _, U = _top(T @ (Sb / (C - 1)) @ T.T, R)
    return U.T @ T


def plda_em(counts, means, mu, Sw, iterations, trace=None):
    """The EM of step 4, one class at a time, with explicit inverses.  ``trace``: a list that receives (B, W) before the
    first step and after every step."""
    C, N = len(counts), counts.sum()
    d = means - mu
    W = Sw / N
    B = d.T @ d / C
    if trace is not None:
        trace.append((B.copy(), W.copy()))
    for _ in range(iterations):
        Bi, Wi = np.linalg.inv(B), np.linalg.inv(W)
        Bn = np.zeros_like(B)
        Wn = Sw.copy()
        for c in range(C):
            phi = np.linalg.inv(Bi + counts[c] * Wi)
            y = phi @ (counts[c] * Wi @ d[c])
            Bn += phi + np.outer(y, y)
            r = d[c] - y
            Wn += counts[c] * (np.outer(r, r) + phi)
        B, W = (Bn + Bn.T) / (2 * C), (Wn + Wn.T) / (2 * N)
        if trace is not None:
            trace.append((B.copy(), W.copy()))
    return B, W


def diagonalise(B, W, Q=None):
    lam, V = _top(W, W.shape[0])
    T = (V / np.sqrt(lam)).T
    psi, U = np.linalg.eigh(T @ B @ T.T)
    psi, U = psi[::-1], U[:, ::-1]
    Q = len(psi) if Q is None else Q
    return (U.T @ T)[:Q], np.maximum(psi[:Q], 0.0)


def coefficients(psi):
    p = psi / (2 * psi + 1)
    q = psi ** 2 / (2 * (psi + 1) * (2 * psi + 1))
    k = float(np.sum(np.log(psi + 1) - 0.5 * np.log(2 * psi + 1)))
    return p, q, k


def llr_closed_form(ue, ut, p, q, k):
    """float64 llr of rows ue / ut [P, Q] and the sum of the magnitudes of its terms (for the kernel's bound)."""
    ue, ut = ue.astype(np.float64), ut.astype(np.float64)
    cross, sq = p * ue * ut, q * (ue * ue + ut * ut)
    return k + cross.sum(axis=1) - sq.sum(axis=1), abs(k) + np.abs(cross).sum(axis=1) + np.abs(sq).sum(axis=1)


def _log_gauss(x, cov):
    sign, logdet = np.linalg.slogdet(cov)
    assert sign > 0
    return -0.5 * (len(x) * np.log(2 * np.pi) + logdet + x @ np.linalg.solve(cov, x))


def llr_direct(z1, z2, mu, B, W):
    """log N([z1; z2]; same speaker) - log N(z1) - log N(z2) with the 2R-dimensional joint covariance written out."""
    T = B + W
    joint = np.block([[T, B], [B, T]])
    return _log_gauss(np.concatenate([z1 - mu, z2 - mu]), joint) - _log_gauss(z1 - mu, T) - _log_gauss(z2 - mu, T)


def log_likelihood(Z, ids, C, mu, B, W):
    """The exact log-likelihood of the rows Z under the two-covariance model: per class of n rows one n R-dimensional
    Gaussian with covariance I_n (x) W + 1 1^T (x) B."""
    total = 0.0
    for c in range(C):
        Zc = Z[ids == c] - mu
        n = len(Zc)
        cov = np.kron(np.eye(n), W) + np.kron(np.ones((n, n)), B)
        total += _log_gauss(Zc.reshape(-1), cov)
    return total


def latent(X, P, mu0, mean, std, centre=True, length_norm=True, work=np.float64):
    """Steps 2 and 3 on rows X: y = P (x - mu0) as one product with the bias -P mu0, then the transform."""
    b = -(P @ mu0)
    y = X.astype(work) @ P.astype(work).T + b.astype(work)
    if centre:
        y = (y - mean.astype(work)) / (std.astype(work) + work(1e-12))
    if length_norm:
        y = y / np.maximum(np.sqrt((y * y).sum(axis=1, dtype=work, keepdims=True)), work(1e-12))
    return y


def fit_and_score(train, labels, test, pairs, *, kind, projection_kind, R, Q=None, iterations=0, centre=True,
                  length_norm=True, work=np.float64):
    """The whole chain on a training bank and a test bank -> raw trial scores float64 [P]: the cosine of the latent rows
    (kind "lda": before (s + 1) / 2) or the llr (kind "plda")."""
    ids, C = ids_of(labels)
    counts, means, mu0, Sw, Sb = class_statistics(train, ids, C, work)
    P = projection(counts, Sw, Sb, R, projection_kind)
    Y = latent(train, P, mu0, None, None, False, False, work)
    mean = (Y.sum(axis=0, dtype=work) / work(len(Y))).astype(work)
    std = np.sqrt(((Y - mean) ** 2).sum(axis=0, dtype=work) / work(len(Y) - 1))
    e, t = pairs[:, 0], pairs[:, 1]
    if kind == "lda":
        z = latent(test, P, mu0, mean, std, centre, length_norm, work)
        a, b = z[e], z[t]
        den = np.maximum(np.sqrt((a * a).sum(axis=1)), 1e-8) * np.maximum(np.sqrt((b * b).sum(axis=1)), 1e-8)
        return ((a * b).sum(axis=1) / den).astype(np.float64)
    Z = latent(train, P, mu0, mean, std, True, True, work)
    zc, zm, mu, zSw, _ = class_statistics(Z, ids, C, work)
    B, W = plda_em(zc, zm, mu, zSw, iterations)
    A, psi = diagonalise(B, W, Q)
    p, q, k = coefficients(psi)
    z = latent(test, P, mu0, mean, std, True, True, work)
    u = z @ A.astype(work).T - (A @ mu).astype(work)
    if work is np.float64:
        return llr_closed_form(u[e], u[t], p, q, k)[0]
    ue, ut, p32, q32 = u[e], u[t], p.astype(work), q.astype(work)
    return (work(k) + (p32 * ue * ut).sum(axis=1, dtype=work) - (q32 * (ue * ue + ut * ut)).sum(axis=1, dtype=work)).astype(np.float64)


# ------------------------------------------------------------------------------------------ the synthetic set
E2E = dict(D=32, train_speakers=60, train_per=8, test_speakers=40, test_per=4, R=16, Q=16, iterations=10)


def two_covariance_set(seed=0, D=32, train_speakers=60, train_per=8, test_speakers=40, test_per=4, **_):
    """x = rot (y_c + e) + 0.5 with y_c ~ N(0, diag(b)), e ~ N(0, diag(w)): between-speaker variances 1.0 on 8 axes and
    0.05 on 24, within-speaker variances 0.3 / 2.0 / 0.1 on 8 / 8 / 16 axes, one random rotation.  -> train f32 [480, D],
    train labels, test f32 [160, D], test labels, pairs int32 [12720, 2] (all pairs), ground truth."""
    rng = np.random.default_rng(seed)
    b = np.array([1.0] * 8 + [0.05] * (D - 8))
    w = np.array([0.3] * 8 + [2.0] * 8 + [0.1] * (D - 16))
    rot, _ = np.linalg.qr(rng.standard_normal((D, D)))

    def draw(speakers, per, first):
        y = rng.standard_normal((speakers, D)) * np.sqrt(b)
        x = np.repeat(y, per, axis=0) + rng.standard_normal((speakers * per, D)) * np.sqrt(w)
        return (x @ rot.T + 0.5).astype(np.float32), [first + i // per for i in range(speakers * per)]

    train, train_labels = draw(train_speakers, train_per, 0)
    test, test_labels = draw(test_speakers, test_per, 10_000)
    n = len(test)
    pairs = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int32)
    gt = [int(test_labels[i] == test_labels[j]) for i, j in pairs]
    return train, train_labels, test, test_labels, pairs, gt


def cosine_scores(bank, pairs):
    bank = bank.astype(np.float64)
    a, b = bank[pairs[:, 0]], bank[pairs[:, 1]]
    return (a * b).sum(axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


# ------------------------------------------------------------------------------------------ kernel cases
def strided(rng, rows, D, gap=4, fill=np.nan):
    """A [rows, D] f32 view into a [rows, D + gap] buffer whose gap columns hold ``fill``."""
    buf = np.full((rows, D + gap), fill, dtype=np.float32)
    buf[:, :D] = rng.standard_normal((rows, D)).astype(np.float32)
    return buf


def rows_center_reference(x, means, seg_id, weight):
    """The kernel's two operations in numpy f32 (bit for bit); a seg_id outside [0, S) gives a NaN row."""
    S = len(means)
    seg = np.zeros(len(x), dtype=np.int64) if seg_id is None else seg_id.astype(np.int64)
    ok = (seg >= 0) & (seg < S)
    c = x - means[np.where(ok, seg, 0)]
    out = c if weight is None else (weight[:, None] * c).astype(np.float32)
    out = out.astype(np.float32)
    out[~ok] = np.nan
    return out


def scatter_reference(a, rows_per_block):
    """(float64 A^T A, the per-element bound (rows_per_block + 4) 2^-24 sum_r |a_ri| |a_rj|) of f32 centred rows a: the
    fma chain of one block product; the fold over blocks is in double."""
    a64 = a.astype(np.float64)
    return a64.T @ a64, (rows_per_block + 4) * 2.0 ** -24 * (np.abs(a64).T @ np.abs(a64))


def scatter_case(rng, N, D, rows_per_block):
    """A bank of N rows with a one-row class, a class that fills a whole block (when N allows) and classes that straddle
    block cuts -> (bank f32 [N, D], seg_id int32 [N], C)."""
    ids, c, r = [], 0, 0
    sizes = [1, 3, rows_per_block + rows_per_block // 2, 5, 2 * rows_per_block, 7]
    while r < N:
        n = min(sizes[c % len(sizes)], N - r)
        ids += [c] * n
        r += n
        c += 1
    ids = np.array(ids, dtype=np.int32)
    if N > 2 * rows_per_block:                              # one class on exactly the rows of the second block
        ids[rows_per_block:2 * rows_per_block] = c
        c += 1
    ids = np.unique(ids, return_inverse=True)[1].astype(np.int32)
    bank = (rng.standard_normal((N, D)) + rng.standard_normal((int(ids.max()) + 1, D))[ids] * 2 + 3).astype(np.float32)
    return bank, ids, int(ids.max()) + 1
