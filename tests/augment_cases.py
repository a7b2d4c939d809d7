"""Float64 oracles of the waveform augmentation, written from the definitions in include/w2v2_hip.h ("waveform
augmentation") and from nothing else, the numpy restatement of the counter hash of csrc/common.h, and the case lists of
tests/test_augment_cpu.py, tests/test_augment_gpu.py and tools/augment_parity.py.

Tolerances are derived, not tuned (u = 2^-24, the unit roundoff of f32):
  FIR, resampler   an output is one chain of K fmas over f32 operands (K = the taps of that output that meet a sample of
                   the row; the others add an exact zero), for the resampler followed by one multiply: at most K + 1
                   roundings, |y - y64| <= gamma_(K+1) sum_j |h_j x_j| <= (K + 2) u sum_j |h_j x_j| while (K + 2)^2 u < 2,
                   i.e. up to K = 5,790.  The oracle forms the sum of magnitudes alongside the sum.
  mixes            fl(1 - c), the product with u and the fma are one rounding each: 3 u (|c x| + |(1 - c) u|).
  dropout, copy    bit-exact.   the uniform stream   bit-exact against the restated hash.
"""
import numpy as np

U32 = np.uint32
EPS = 2.0 ** -24
FIR_TILE = 2048                 # ops.AUG_FIR_TILE
RESAMPLE_TILE = 256             # ops.AUG_RESAMPLE_TILE
MAX_TAPS = 2561                 # ops.AUG_MAX_TAPS


# ------------------------------------------------------------------------------------------------ the hash, in uint32
def rng_key(seed: int) -> int:
    """rng_key of csrc/common.h on a 64-bit seed."""
    seed &= 2 ** 64 - 1
    with np.errstate(over="ignore"):
        k = U32(seed & 0xFFFFFFFF) * U32(0x9E3779B1) ^ U32(seed >> 32) * U32(0x85EBCA77) ^ U32(0x27D4EB2F)
        k ^= k >> U32(15); k *= U32(0x2C1B3C6D)
        k ^= k >> U32(12); k *= U32(0x297A2D39)
        k ^= k >> U32(15)
    return int(k)


def rng_pair(key: int, idx: np.ndarray) -> np.ndarray:
    """rng_pair of csrc/common.h for indices below 2^32 (the high word's term is zero)."""
    with np.errstate(over="ignore"):
        x = idx.astype(U32) ^ U32(key)
        x ^= x >> U32(16); x *= U32(0x85EBCA6B)
        x ^= x >> U32(13); x *= U32(0xC2B2AE35)
        x ^= x >> U32(16)
    return x


def uniform_stream(seed: int, row: int, n: int) -> np.ndarray:
    """u[i] of w2v2_aug_mix_uniform for one row, exactly: f32 values k 2^-24, k < 2^24."""
    key = rng_key((int(row) << 32) | rng_key(seed))
    return (rng_pair(key, np.arange(n, dtype=np.int64)) >> U32(8)).astype(np.float32) * np.float32(EPS)


# ------------------------------------------------------------------------------------------------ oracles (float64)
def _live(x, n):
    x = np.asarray(x, np.float64).copy()
    x[n:] = 0.0                                         # zero by index, whatever the buffer holds
    return x


def dropout_ref(x, n, spans):
    """x: one row [N] f32 -> the row after the spans, bit for bit."""
    y = np.asarray(x, np.float32).copy()
    y[n:] = 0.0
    for start, length in spans:
        if length > 0:
            a, b = max(start, 0), min(start + length, n)
            if b > a:
                y[a:b] = 0.0
    return y


def mix_ref(x, n, c, u):
    """-> (y64, bound); c is the f32 coefficient, u the noise [>= n] (f32 values)."""
    N = len(x)
    c = float(np.float32(c))
    xs, us = _live(x, n), np.zeros(N)
    us[:n] = np.asarray(u, np.float64)[:n]
    y = c * xs + (1.0 - c) * us
    bound = 3 * EPS * (np.abs(c * xs) + np.abs((1.0 - c) * us))
    y[n:], bound[n:] = 0.0, 0.0
    return y, bound


def bank_noise(bank_row, L, n):
    return np.asarray(bank_row)[np.arange(n) % L]


def fir_ref(x, n, h, N_out):
    """y[m] = sum_j h[j] x[m + (K - 1) / 2 - j], x zero outside [0, n) -> (y64 [N_out], bound [N_out])."""
    h = np.asarray(h, np.float64)
    K = h.size
    assert K % 2 == 1
    P = (K - 1) // 2
    xs = _live(x, n)[:n]
    y, bound = np.zeros(N_out), np.zeros(N_out)
    live = min(n, N_out)
    if live == 0:
        return y, bound
    full = np.convolve(xs, h)                           # full[m + P] = y[m]
    mag = np.convolve(np.abs(xs), np.abs(h))
    y[:live], s = full[P:P + live], mag[P:P + live]
    m = np.arange(live)
    j_lo, j_hi = np.maximum(0, m + P - (n - 1)), np.minimum(K - 1, m + P)      # taps that meet a sample of the row
    bound[:live] = ((j_hi - j_lo + 1) + 2) * EPS * s
    return y, bound


def resample_ref(x, n, U, D, h, N_out):
    """y[m] = U sum_j x[j] h[m D - j U + half] over the taps that exist -> (y64 [N_out], bound [N_out], out_len)."""
    out_len = min(-(-n * U // D), N_out)
    y, bound = np.zeros(N_out), np.zeros(N_out)
    xs = _live(x, n)
    if U == D:
        y[:out_len] = xs[:out_len]
        return y, bound, out_len
    h = np.asarray(h, np.float64)
    half = (h.size - 1) // 2
    for m in range(out_len):
        c = m * D + half
        j_lo, j_hi = max(0, -(-(c - 2 * half) // U)), min(c // U, n - 1)
        if j_hi < j_lo:
            continue
        j = np.arange(j_lo, j_hi + 1)
        t = xs[j] * h[c - j * U]
        y[m] = U * t.sum()
        bound[m] = (j.size + 2) * EPS * U * np.abs(t).sum()
    return y, bound, out_len


# ------------------------------------------------------------------------------------------------ inputs and case lists
def wave(rows, N, seed):
    """Speech-sized f32 noise with a slow component, so neighbouring samples correlate as audio does."""
    r = np.random.RandomState(seed)
    t = np.arange(N)[None, :]
    return (0.3 * r.standard_normal((rows, N)) + 0.5 * np.sin(0.01 * t * (1 + np.arange(rows)[:, None]))).astype(np.float32)


def fir_taps(K, seed):
    """K f32 taps of a plausible filter: a decaying random shape around a centre tap near 1."""
    r = np.random.RandomState(1000 + seed + K)
    P = (K - 1) // 2
    h = r.standard_normal(K) * np.exp(-np.abs(np.arange(K) - P) / max(K / 8.0, 1.0)) * 0.1
    h[P] += 1.0
    return h.astype(np.float32)


DROPOUT_N = 257
# (name, spans of the one listed row, len or None): every edge the issue names
DROPOUT_CASES = [
    ("no-spans", [], None),
    ("zero-length", [(40, 0)], None),
    ("at-zero", [(0, 9)], None),
    ("ends-at-len", [(250, 7)], None),
    ("past-len", [(250, 40)], None),
    ("overlapping", [(30, 20), (45, 20), (45, 3)], None),
    ("straddles-4", [(2, 4), (101, 6), (127, 2)], None),
    ("lens<N", [(5, 3), (190, 30)], 200),
    ("lens<N-past", [(199, 5), (230, 10)], 200),
    ("negative-start", [(-3, 8)], None),
]

MIX_SNRS = [100, 15]                                    # c rounds to 1.0f at 100 dB
MIX_BANK_LENS = [1, 100, 257, 400]                      # length 1, shorter than, equal to and longer than the row (N = 257)

FIR_TAPS_IN_ONE_LAUNCH = [1, 3, 513, MAX_TAPS]
FIR_N = [1, 100, FIR_TILE - 1, FIR_TILE, FIR_TILE + 1]  # 100 is shorter than the half-width of 513 and 2,561 taps

RESAMPLE_RATIOS = [(1, 1), (20, 19), (20, 21), (2, 1), (1, 2), (3, 7)]


def resample_lens(D):
    """len in {1, D - 1, tile - 1, tile + 1} (D - 1 only where it is a length)."""
    return sorted({1, max(D - 1, 1), RESAMPLE_TILE - 1, RESAMPLE_TILE + 1})
