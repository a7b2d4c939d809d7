"""Cases of the device trial metrics (csrc/metrics.hip) with their references.  No GPU and no ``ops`` import here:
test_metrics_cpu.py holds the reference rule to the host metrics (eval_metrics.py), test_metrics_gpu.py holds the kernels
to the rule and to the host metrics.

``sort_ref``: np.argsort(kind="stable").  ``metrics_ref``: the rule of w2v2_trial_metrics in numpy int64 / float64 -- the
ROC of sklearn's roc_curve (group ends in descending score order behind the origin; kept: origin, first and last point,
and between them where the second difference of fp or tp is non-zero), the crossing test in exact integers, the closed
forms of the segment it falls in, and calculate_mdc's sweep over every position of the stable order.

Bounds (all stated against the HOST functions, whose own values are defined no better):
  eer            5e-12: brentq stops within scipy's default xtol = 2e-12 of the root.
  eer_threshold  interior crossing with a finite thr_lo: 4e-12 * |thr_hi - thr_lo| / (x1 - x0) + 1e-12 -- the same xtol
                 (twice, for the root on either side) carried through the slope of the threshold along the segment.
                 Vertical crossing: the host's value depends on which side of the jump brentq stops; only "one end of
                 the kept run, or not finite" holds, an end being met to vertical_atol (below).
  mdc            16 * 2^-53 relative: six rounded f64 operations with margin.
  mdc_threshold  the sorted score at a position whose host c_det is within that distance of the host minimum."""
import functools

import numpy as np

from w2v2_speaker_amd.eval_metrics import calculate_eer, calculate_mdc, roc_curve

EER_BOUND = 5e-12
MDC_REL = 16 * 2.0 ** -53


def vertical_atol(m) -> float:
    """How closely a host threshold "at an end" of a vertical run meets that end: it is interpolated along the NEIGHBOURING
    segment from an abscissa within xtol of the jump (4e-12: either side).  Scores lie in [-1, 1], so a threshold moves by
    at most 2 over a segment, and a segment is at least 1 / n_neg wide.  At the largest case here (n_neg < 4000) this is
    3.2e-8, far below the 1e-5 between two distinct scores of the generator's finest level."""
    return 4e-12 * 2 * m["n_neg"] + 1e-12


def sort_ref(keys):
    return np.argsort(np.asarray(keys, dtype=np.float32), kind="stable")


def thr_bound(m) -> float:
    """Bound on an interior eer_threshold of the case whose metrics_ref is ``m``."""
    return 4e-12 * abs(m["thr_hi"] - m["thr_lo"]) / (m["x1"] - m["x0"]) + 1e-12


def metrics_ref(gt, scores_f32, c_miss=1, c_fa=1, p_target=0.05):
    """The rule of w2v2_trial_metrics on scores WITHOUT NaN and labels of both classes -> dict of the eight outputs plus
    what the tests classify by: ``kind`` ("vertical", "exact", "interior"), lo / hi (ROC point numbers), x0 / x1, thr_lo /
    thr_hi, ``c_det`` (per position of the stable order) and ``sorted_scores``."""
    s32 = np.asarray(scores_f32, dtype=np.float32)
    assert s32.ndim == 1 and not np.isnan(s32).any()
    order = np.argsort(s32, kind="stable")
    ss = s32[order].astype(np.float64)
    g = np.asarray(gt, dtype=np.int64)[order]
    P = len(ss)
    cpos = np.cumsum(g)
    cneg = np.arange(1, P + 1, dtype=np.int64) - cpos
    n_pos, n_neg = int(cpos[-1]), int(cneg[-1])
    assert n_pos > 0 and n_neg > 0
    ends = np.flatnonzero(np.r_[ss[1:] != ss[:-1], True])
    K = len(ends)
    # ROC point j = 1 .. K is group K - j: everything behind the end of the group in front of it
    tp = np.r_[0, (n_pos - np.r_[0, cpos[ends][:-1]])[::-1]].astype(np.int64)
    fp = np.r_[0, (n_neg - np.r_[0, cneg[ends][:-1]])[::-1]].astype(np.int64)
    thr = np.r_[np.inf, ss[ends][::-1]]
    keep = np.ones(K + 1, dtype=bool)
    if K >= 3:
        keep[2:K] = (np.diff(fp, 2)[1:] != 0) | (np.diff(tp, 2)[1:] != 0)
    passes = fp * n_pos + tp * n_neg >= n_neg * n_pos
    kept = np.flatnonzero(keep)
    hi = int(kept[passes[kept]][0])
    lo = int(kept[~passes[kept]][-1])
    N, Pn = float(n_neg), float(n_pos)
    x0, x1, y0, y1 = fp[lo] / N, fp[hi] / N, tp[lo] / Pn, tp[hi] / Pn
    if fp[lo] == fp[hi]:
        kind, eer, eer_thr = "vertical", fp[hi] / N, thr[hi]
    else:
        kind = "exact" if fp[hi] * n_pos + tp[hi] * n_neg == n_neg * n_pos else "interior"
        m = (y1 - y0) / (x1 - x0)
        eer = (1.0 - y0 + m * x0) / (1.0 + m)
        eer_thr = thr[lo] + (eer - x0) * (thr[hi] - thr[lo]) / (x1 - x0) if lo > 0 else np.inf
    if lo == 0:
        eer_thr = np.inf
    fnr = cpos / Pn
    fpr = 1.0 - cneg / N
    c_det = c_miss * fnr * p_target + c_fa * fpr * (1 - p_target)
    i = int(np.argmin(c_det))
    c_def = min(c_miss * p_target, c_fa * (1 - p_target))
    return {"eer": float(eer), "eer_threshold": float(eer_thr), "mdc": float(c_det[i] / c_def), "mdc_threshold": float(ss[i]),
            "n_pos": n_pos, "n_neg": n_neg, "n_nan": 0, "n_thresholds": int(keep.sum()),
            "kind": kind, "lo": lo, "hi": hi, "x0": float(x0), "x1": float(x1), "thr_lo": float(thr[lo]),
            "thr_hi": float(thr[hi]), "c_det": c_det, "sorted_scores": ss, "mdc_index": i}


def host_c_det(gt, scores, c_miss=1, c_fa=1, p_target=0.05):
    """calculate_mdc's own cost per position of its stable order (eval_metrics.py), and the sorted scores."""
    g = np.asarray(gt, dtype=np.float64)
    sc = np.asarray(scores, dtype=np.float64)
    order = np.argsort(sc, kind="stable")
    g, thr = g[order], sc[order]
    fnrs = np.cumsum(g) / g.sum()
    fprs = 1.0 - np.cumsum(1.0 - g) / (len(g) - g.sum())
    return c_miss * fnrs * p_target + c_fa * fprs * (1 - p_target), thr


def host_metrics(gt, scores_f32, c_miss=1, c_fa=1, p_target=0.05):
    """The host functions on the lists ``evaluate_bank`` hands them (Python floats of the f32 scores)."""
    gt = [int(v) for v in gt]
    scores = np.asarray(scores_f32, dtype=np.float32).astype(np.float64).tolist()
    with np.errstate(all="ignore"):
        eer, eer_thr = calculate_eer(gt, scores)
    mdc, mdc_thr = calculate_mdc(gt, scores, c_miss, c_fa, p_target)
    return {"eer": float(eer), "eer_threshold": float(eer_thr), "mdc": float(mdc), "mdc_threshold": float(mdc_thr),
            "n_thresholds": len(roc_curve(gt, scores)[2])}


def vertical_threshold_ok(host_thr: float, m) -> bool:
    return (not np.isfinite(host_thr)) or min(abs(host_thr - m["thr_lo"]), abs(host_thr - m["thr_hi"])) <= vertical_atol(m)


def check_against_host(got, m, h, what=""):
    """The assertions both test files make: ``got`` (eer, eer_threshold, mdc, mdc_threshold as floats) against the rule's
    values ``m`` and the host's ``h`` of the same case.  -> the figures, for the parity lines."""
    e_ref, e_host = abs(got["eer"] - m["eer"]), abs(got["eer"] - h["eer"])
    assert e_ref <= EER_BOUND and e_host <= EER_BOUND, (what, got["eer"], m["eer"], h["eer"])
    t_err = t_bound = 0.0
    if m["kind"] == "vertical":
        assert got["eer_threshold"] == m["eer_threshold"], (what, got["eer_threshold"], m["eer_threshold"])
        assert vertical_threshold_ok(h["eer_threshold"], m), (what, h["eer_threshold"], m["thr_lo"], m["thr_hi"])
    elif np.isfinite(m["thr_lo"]):
        t_bound = thr_bound(m)
        t_err = abs(got["eer_threshold"] - m["eer_threshold"])
        if m["kind"] == "interior":     # (an exact crossing: the host may stop behind it, on the NEXT segment's slope)
            t_err = max(t_err, abs(got["eer_threshold"] - h["eer_threshold"]))
        assert t_err <= t_bound, (what, got["eer_threshold"], m["eer_threshold"], h["eer_threshold"], t_bound)
    else:                               # the crossing lies in the segment from the origin
        assert got["eer_threshold"] == np.inf and not np.isfinite(h["eer_threshold"]), (what, got, h)
    d_ref = abs(got["mdc"] - m["mdc"]) / abs(m["mdc"]) if m["mdc"] else abs(got["mdc"])
    d_host = abs(got["mdc"] - h["mdc"]) / abs(h["mdc"]) if h["mdc"] else abs(got["mdc"])
    assert d_ref <= MDC_REL and d_host <= MDC_REL, (what, got["mdc"], m["mdc"], h["mdc"])
    return {"eer_ref": e_ref, "eer_host": e_host, "thr": t_err, "thr_bound": t_bound, "mdc_ref": d_ref, "mdc_host": d_host}


def check_mdc_threshold(got_thr, gt, scores_f32, c_miss=1, c_fa=1, p_target=0.05):
    """``got_thr`` is the sorted score at a position whose HOST c_det is within MDC_REL (relative) of the host minimum."""
    c_det, thr = host_c_det(gt, np.asarray(scores_f32, dtype=np.float32).astype(np.float64), c_miss, c_fa, p_target)
    best = c_det.min()
    near = np.abs(c_det - best) <= MDC_REL * abs(best) if best else c_det == best
    assert (thr[near] == got_thr).any(), (got_thr, thr[near][:8])


# ------------------------------------------------------------------------------------------------ the seeded generator
SEED, NUM_CASES = 20241, 400
LEVELS = (3, 8, 50, 100000)


def draw_case(rng):
    n = int(rng.integers(4, 300))
    while True:
        gt = rng.integers(0, 2, n)
        if 0 < gt.sum() < n:
            break
    levels = LEVELS[int(rng.integers(0, len(LEVELS)))]
    s = np.clip(0.3 * gt + rng.normal(0.4, 0.25, n), 0, 1)
    return gt.astype(np.int64), (np.round(s * (levels - 1)) / (levels - 1)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """The committed list: NUM_CASES draws of the seeded generator, a vertical draw kept only where the host's threshold
    is an end of the kept run or not finite (elsewhere the host value is ill-defined and nothing can be said of it).
    -> tuple of (gt, scores f32, metrics_ref, host_metrics)."""
    rng = np.random.default_rng(SEED)
    out = []
    while len(out) < NUM_CASES:
        gt, s = draw_case(rng)
        m, h = metrics_ref(gt, s), host_metrics(gt, s)
        if m["kind"] == "vertical" and not vertical_threshold_ok(h["eer_threshold"], m):
            continue
        out.append((gt, s, m, h))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the edges
TIE_GT = (np.array([1, 0, 1, 0, 0, 1, 0, 0]), np.array([1, 1, 1, 0, 0, 0, 0, 0]))      # ... tied positives in front
TIE_SCORES = np.array([.9, .5, .5, .5, .5, .5, .2, .1], dtype=np.float32)
TIE_P_TARGET = 0.5
TIE_HOST = ((1 / 3, 0.5), (0.6, 0.2))                  # calculate_mdc's (mdc, threshold) of the two orders


def _noisy(n, seed, levels=100000, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, 2, n)
    gt[:2] = (0, 1)
    s = np.clip(0.3 * gt + rng.normal(0.4, 0.25, n), 0, 1)
    s = np.round(s * (levels - 1)) / (levels - 1)
    return gt.astype(np.int64), (lo + (hi - lo) * s).astype(np.float32)


def collinear_run(tile: int):
    """Three positives above and three below ``tile + 501`` DISTINCT negative scores: the ROC runs flat at tp = 1/2 from
    fp = 0 to fp = 1, more than a tile of dropped points with the crossing in their middle."""
    n = tile + 501
    neg = (0.1 + 0.8 * np.arange(n) / n).astype(np.float32)
    assert len(np.unique(neg)) == n
    perm = np.random.default_rng(3).permutation(n + 6)
    s = np.r_[neg, np.float32([0.97, 0.98, 0.99, 0.01, 0.02, 0.03])].astype(np.float32)
    gt = np.r_[np.zeros(n, dtype=np.int64), np.ones(6, dtype=np.int64)]
    return gt[perm], s[perm]


def edge_cases(tile: int):
    """name -> (gt, scores f32, p_target)."""
    e = {
        "two": (np.array([0, 1]), np.float32([0.2, 0.7]), 0.05),                # P = 2, the positive above
        "two_inverted": (np.array([1, 0]), np.float32([0.2, 0.7]), 0.05),       # ... and below
        "all_equal": (np.array([1, 0, 0, 1, 0]), np.full(5, 0.5, dtype=np.float32), 0.05),
        # every positive at ONE score above every negative: hi is the first point, the crossing lies in the segment
        # from the origin
        "separated_first_segment": (np.array([0, 1, 0, 1, 1, 0, 0]), np.float32([.1, .9, .3, .9, .9, .2, .4]), 0.05),
        "separated_distinct": (np.array([0, 1, 0, 1, 1, 0, 0]), np.float32([.1, .9, .3, .8, .7, .2, .4]), 0.05),
        "inverted": (np.array([1, 0, 1, 0, 0, 1, 1]), np.float32([.1, .9, .3, .8, .7, .2, .4]), 0.05),
        "collinear_run": collinear_run(tile) + (0.05,),
        "raw_cosines": _noisy(777, 11, lo=-1.0, hi=1.0) + (0.05,),
        "signed_zeros": (np.array([1, 0, 0, 1, 1, 0]), np.float32([-0.0, 0.0, -0.5, 0.0, 0.5, -0.0]), 0.05),
        "tie_order_0": (TIE_GT[0], TIE_SCORES, TIE_P_TARGET),
        "tie_order_1": (TIE_GT[1], TIE_SCORES, TIE_P_TARGET),
    }
    for name, n in (("tile_m1", tile - 1), ("tile", tile), ("tile_p1", tile + 1), ("three_tiles_p5", 3 * tile + 5)):
        e[name] = _noisy(n, 100 + n, levels=50 if name == "tile" else 100000) + (0.05,)
    return e


# ------------------------------------------------------------------------------------------------ sort cases
def sort_sizes(tile: int):
    return (1, 2, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 5, 70001)


SORT_KINDS = ("equal", "two_values", "unit", "full_range", "ascending", "descending", "top_byte", "bottom_byte")


def sort_keys(kind: str, P: int) -> np.ndarray:
    rng = np.random.default_rng(7000 + 13 * P + SORT_KINDS.index(kind))
    if kind == "equal":
        return np.full(P, 0.25, dtype=np.float32)
    if kind == "two_values":
        return rng.choice(np.float32([0.25, 0.75]), P)
    if kind == "unit":
        return rng.random(P, dtype=np.float32)
    if kind == "full_range":        # random bit patterns (denormals, NaNs of both signs among them) and the special values
        u = rng.integers(0, 2 ** 32, P, dtype=np.uint64).astype(np.uint32)
        for start, step, bits in ((0, 7, 0x00000000), (3, 7, 0x80000000), (5, 31, 0x7f800000), (6, 31, 0xff800000),
                                  (2, 13, 0x7fc00001), (4, 17, 0xffc00000), (1, 11, 0x00000001), (8, 19, 0x80000002),
                                  (9, 23, 0x7fffffff), (10, 29, 0xff800001)):
            u[start::step] = bits
        return u.view(np.float32)
    if kind in ("ascending", "descending"):
        a = np.sort(rng.standard_normal(P).astype(np.float32))
        return a if kind == "ascending" else a[::-1].copy()
    if kind == "top_byte":          # 0x80000000 (-0.0) ties with 0x00000000; top bytes 0x7f / 0xff stay finite
        return (rng.integers(0, 256, P, dtype=np.uint64).astype(np.uint32) << np.uint32(24)).view(np.float32)
    if kind == "bottom_byte":
        return (np.uint32(0x3f000000) | rng.integers(0, 256, P, dtype=np.uint64).astype(np.uint32)).view(np.float32)
    raise KeyError(kind)
