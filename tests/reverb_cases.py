"""Oracles and cases of the reverb augmentation (w2v2_aug_reverb), written from the definition in include/w2v2_hip.h
("waveform augmentation", Reverb) and from nothing else.

Two oracles run the same code in two number formats: float64, and float32 with sox's own order of operations -- the
sequential loop, one rounding per operation, no fused multiply-add.  Both walk a filter in blocks of its delay (the
samples of a block read what the block before wrote, so a block's delay-line outputs are one array); only the comb's
one-pole low-pass is a loop over samples.

Tolerance, per row (the device evaluates the low-pass as a scan, so it is defined to a tolerance, not bit for bit):
    max |y_dev - y_f64|  <=  max(4 max |y_seq32 - y_f64|,  2^-22 max |y_f64|)
The yardstick is sox's own f32 arithmetic, never the kernel.  The factor 4: a CPU simulation of a block-scan schedule
(Kogge-Stone, ratio powers by repeated squaring in f32) stayed within 2.1 times the sequential loop's error on the wet
signal, worst at reverberance 100, damping 0, room scale 0.  The floor is the project's f32 floor.
"""
import numpy as np

MAX_DELAY = 1024                # ops.AUG_REVERB_MAX_DELAY
PARAMS = 28                     # ops.AUG_REVERB_PARAMS
CHUNK = 512                     # ops.AUG_REVERB_CHUNK
WET_GAIN = 0.015
FACTOR, FLOOR = 4.0, 2.0 ** -22

DELAY_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, MAX_DELAY]
FEEDBACKS = [0.3, 0.8817, 0.98]
DAMPS = [0.2, 0.5]
DRY_GAINS = [0.0, 1.0]
COEFS = [(f, d, g) for f in FEEDBACKS for d in DAMPS for g in DRY_GAINS]           # 12 combinations
# 0, 1, delay - 1, delay, delay + 1 of every edge, chunk - 1, chunk, chunk + 1, 2 chunk + 3
LENGTHS = sorted({0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3} | {d + e for d in DELAY_EDGES for e in (-1, 0, 1)})
N_MAX = 2 * CHUNK + 3
ROOMS = [0, 37, 100]


def table_row(combs, allpasses, feedback, damp, wet_gain=WET_GAIN, dry_gain=1.0):
    """int32 [PARAMS]: comb delays [2][8], all-pass delays [2][4], then the f32 coefficients by their bits."""
    c, a = np.asarray(combs, np.int32).reshape(16), np.asarray(allpasses, np.int32).reshape(8)
    return np.concatenate([c, a, np.asarray([feedback, damp, wet_gain, dry_gain], np.float32).view(np.int32)])


def edge_row(k, feedback, damp, dry_gain):
    """A hand-built table: the delay edges dealt round the 16 combs starting at edge k, and round the 8 all-passes
    starting at edge k + 4: every row holds every edge."""
    E = len(DELAY_EDGES)
    return table_row([DELAY_EDGES[(k + i) % E] for i in range(16)], [DELAY_EDGES[(k + 4 + 2 * j) % E] for j in range(8)],
                     feedback, damp, WET_GAIN, dry_gain)


def wave(rows, N, seed):
    """Gaussian rows of amplitude 0.1, f32."""
    return (0.1 * np.random.RandomState(seed).standard_normal((rows, N))).astype(np.float32)


def _comb(x, D, feedback, damp, dt):
    N = x.size
    out, line, store = np.zeros(N, dt), np.zeros(D, dt), dt(0)
    st = np.zeros(D, dt)
    for n0 in range(0, N, D):
        m = min(D, N - n0)
        o = line[:m].copy()
        out[n0:n0 + m] = o
        for k in range(m):                              # store = o + (store - o) damp, one rounding per operation
            store = o[k] + (store - o[k]) * damp
            st[k] = store
        line[:m] = x[n0:n0 + m] + st[:m] * feedback
    return out


def _allpass(x, D, dt):
    N = x.size
    out, line = np.zeros(N, dt), np.zeros(D, dt)
    for n0 in range(0, N, D):
        m = min(D, N - n0)
        o = line[:m].copy()
        line[:m] = x[n0:n0 + m] + dt(0.5) * o
        out[n0:n0 + m] = o - x[n0:n0 + m]
    return out


def reverb_ref(x, n, row, N_out, dt=np.float64):
    """One row of the definition in the number format dt: x [N_in] f32, n its length, row the int32 table row ->
    y [N_out] (dt), zeros behind min(n, N_out).  A sample depends on no later one, so a cropped row is a prefix."""
    row = np.asarray(row, np.int32)
    combs, aps = row[:16].reshape(2, 8), row[16:24].reshape(2, 4)
    feedback, damp, wet_gain, dry_gain = (dt(v) for v in row[24:28].view(np.float32))
    live = min(int(n), int(N_out))
    y = np.zeros(N_out, dt)
    if live == 0:
        return y
    xs = np.asarray(x[:live], np.float32).astype(dt)    # zero by index behind n: nothing behind it is read
    wet = []
    for w in range(2):
        acc = np.zeros(live, dt)
        for i in range(7, -1, -1):
            acc = acc + _comb(xs, int(combs[w, i]), feedback, damp, dt)
        for j in range(3, -1, -1):
            acc = _allpass(acc, int(aps[w, j]), dt)
        wet.append(acc * wet_gain)
    y[:live] = dt(0.5) * ((dry_gain * xs + wet[0]) + (dry_gain * xs + wet[1]))
    return y


def reverb_refs(x, n, row, N_out):
    """-> (y_f64, bound, seq_err): the float64 oracle, the row's tolerance, and the f32 sequential loop's own error that
    the tolerance is taken from."""
    y64, y32 = reverb_ref(x, n, row, N_out, np.float64), reverb_ref(x, n, row, N_out, np.float32)
    seq_err = float(np.abs(y32.astype(np.float64) - y64).max())
    return y64, max(FACTOR * seq_err, FLOOR * float(np.abs(y64).max())), seq_err
