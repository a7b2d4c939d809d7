"""Device score normalisation on the GPU: the kernels of csrc/score_norm.hip and ops.cohort_stats on the cases of
tests/score_norm_cases.py within the bounds stated there, bitwise reproducibility, the NaN answers, and
evaluate_bank / evaluate_trials with ``score_norm`` against the host evaluator and float64."""
import numpy as np
import pytest
import torch

import metrics_cases as MC
import score_norm_cases as NC
import scoring_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ topk_stats
def _lds_keys():
    from w2v2_speaker_amd import ops
    return ops.TOPK_LDS_KEYS


def _run_topk(S, K, gap=4):
    """S [R, M] numpy -> (mu, sd) of the kernel over a buffer with ldS = M rounded up to 4 plus a NaN-filled gap, and
    sentinel cells behind the outputs."""
    from w2v2_speaker_amd import ops
    R, M = S.shape
    buf = dev(NC.padded(S, (-M) % 4 + gap))
    mu = torch.full((R + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    sd = torch.full((R + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.topk_stats(buf, K, M, mu, sd)
    mu, sd = mu.cpu().numpy(), sd.cpu().numpy()
    assert (mu[R:] == SENTINEL).all() and (sd[R:] == SENTINEL).all(), "written past the outputs"
    return mu[:R], sd[:R]


# both routes: a row that fits the LDS stage, the longest that does, and the first that is re-read from global memory
@pytest.mark.parametrize("M", NC.TOPK_M + (8191, 8192, 8193))
def test_topk_stats_exact_selection_on_hand_made_rows(M):
    assert _lds_keys() == 8192, "the route switch moved: put both of its sides into the list above"
    worst = (0.0, 0.0)
    for R in (1, 2, 5, 7):                                   # one workgroup per row: 2 is one more than a launch groups
        S = NC.topk_rows(M, R)
        for K in NC.topk_ks(M):
            ref_mu, ref_sd = NC.topk_stats_ref(S, K)
            mu, sd = _run_topk(S, K)
            em, es = NC.topk_within(mu, sd, ref_mu, ref_sd)
            worst = (max(worst[0], em), max(worst[1], es))
            assert em <= NC.FLOOR and es <= NC.FLOOR, (M, R, K, em, es)
            for r in range(R):
                if NC.SPECIAL_ROWS[r % len(NC.SPECIAL_ROWS)] == "all_equal":
                    assert mu[r] == S[r, 0] and sd[r] == 0.0, (M, R, K, mu[r], sd[r])
            mu2, sd2 = _run_topk(S, K)                       # a second run: the same bits
            assert np.array_equal(mu, mu2) and np.array_equal(sd, sd2)
    print(f"score-norm-parity: topk_stats M={M} K in {NC.topk_ks(M)} R in (1, 2, 5, 7): mu {worst[0]:.2e} sd {worst[1]:.2e} "
          f"relative to max(|mu|, sd), bound {NC.FLOOR:.2e}")


@pytest.mark.parametrize("M", (5, 257, 8193))
def test_topk_stats_a_nan_poisons_its_own_row_only(M):
    S = NC.topk_rows(M, 5, seed=1)
    K = min(3, M)
    clean = _run_topk(S, K)
    S[2, M - 1 if M % 2 else M // 2] = np.nan
    mu, sd = _run_topk(S, K)
    assert np.isnan(mu[2]) and np.isnan(sd[2])
    keep = [0, 1, 3, 4]
    assert np.array_equal(mu[keep], clean[0][keep]) and np.array_equal(sd[keep], clean[1][keep])


def test_topk_stats_tie_group_at_the_boundary_and_signed_zeros():
    # five copies of the K-th value, two of them inside the top K; -0.0 and +0.0 are one value
    S = np.array([[0.9, 0.5, 0.5, 0.8, 0.5, 0.5, 0.1, 0.5, -0.3, 0.0],
                  [-0.0, 0.0, -0.0, -1.0, 0.0, -2.0, -0.0, 0.0, -3.0, -4.0]], dtype=np.float32)
    mu, sd = _run_topk(S, 4)
    top = np.array([0.9, 0.8, 0.5, 0.5], dtype=np.float32).astype(np.float64)
    assert mu[0] == np.float32(top.mean()) and sd[0] == np.float32(top.std(ddof=1))
    assert mu[1] == 0.0 and sd[1] == 0.0
    mu, sd = _run_topk(S, 8)                                 # row 1: six zeros of either sign, then -1 and -2
    top = np.array([0, 0, 0, 0, 0, 0, -1, -2], dtype=np.float64)
    assert mu[1] == np.float32(top.mean()) and sd[1] == np.float32(top.std(ddof=1))


# ------------------------------------------------------------------------------------------------ rows_transform
def _transform_case(D, centre, length_norm):
    rng = np.random.default_rng(5000 + D)
    x = (rng.standard_normal((9, D)) * 1.5 + 0.4).astype(np.float32)
    x[3] = 0                                                 # the zero row: both clamps
    mean = std = None
    if centre:
        m, s = SC.stats_ref(x[[0, 1, 2, 4, 5]])
        mean, std = m.astype(np.float32), s.astype(np.float32)
    u = SC.transform_ref(x, mean, std, length_norm)
    inv = 1.0 / np.maximum(np.linalg.norm(u, axis=1), 1e-8)
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import center_batch, length_norm_batch
    h = torch.from_numpy(x)
    if centre:
        h = center_batch(h, torch.from_numpy(mean), torch.from_numpy(std))
    if length_norm:
        h = length_norm_batch(h)
    h_inv = (1.0 / torch.linalg.vector_norm(h, dim=1).clamp_min(1e-8)).numpy()
    scale = np.maximum(1.0, np.abs(u))
    return {"x": x, "mean": mean, "std": std, "u": u, "inv": inv, "scale": scale,
            "bound_u": NC.bound((np.abs(h.numpy() - u) / scale).max()), "bound_inv": NC.bound(np.abs(h_inv / inv - 1.0).max())}


@pytest.mark.parametrize("centre,length_norm", NC.CENTRE_MODES)
@pytest.mark.parametrize("D", (4, 252, 256, 260))
def test_rows_transform_against_float64(D, centre, length_norm):
    from w2v2_speaker_amd import ops
    c = _transform_case(D, centre, length_norm)
    rows = c["x"].shape[0]
    mean, std = (None, None) if c["mean"] is None else (dev(c["mean"]), dev(c["std"]))
    x_ld = dev(NC.padded(c["x"], 4))[:, :D]                  # ld = D + 4, NaN in the gap
    out = torch.full((rows, D + 4), SENTINEL, dtype=torch.float32, device=DEV)
    inv = torch.full((rows + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    u, inv_r = ops.rows_transform(x_ld, mean, std, length_norm, out=out[:, :D], inv_norm=inv)
    got_u, got_inv = u.cpu().numpy().astype(np.float64), inv.cpu().numpy()
    assert (out[:, D:] == SENTINEL).all() and (got_inv[rows:] == SENTINEL).all(), "written past the outputs"
    got_inv = got_inv[:rows].astype(np.float64)
    e_u, e_inv = (np.abs(got_u - c["u"]) / c["scale"]).max(), np.abs(got_inv / c["inv"] - 1.0).max()
    print(f"score-norm-parity: rows_transform D={D} centre={int(centre)} lnorm={int(length_norm)}: u {e_u:.2e} bound "
          f"{c['bound_u']:.2e}; inv_norm rel {e_inv:.2e} bound {c['bound_inv']:.2e}")
    assert e_u <= c["bound_u"] and e_inv <= c["bound_inv"]
    if not centre:
        assert got_inv[3] == float(np.float32(1e8)) and (got_u[3] == 0).all()        # the zero row through the clamps
    # without an `out`: the same bits from contiguous rows; and nothing is copied when there is nothing to transform
    u2, inv2 = ops.rows_transform(dev(c["x"]), mean, std, length_norm)
    assert torch.equal(inv2, inv[:rows])
    if centre or length_norm:
        assert torch.equal(u2, u)
    else:
        assert u2 is None and torch.equal(u, dev(c["x"]))


# ------------------------------------------------------------------------------------------------ segment_mean
@pytest.mark.parametrize("D", (4, 260))
def test_segment_mean_against_float64(D):
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import speaker_mean_cohort
    rng = np.random.default_rng(6000 + D)
    labels = np.array([7] * 129 + [3] * 2 + [5] * 1)         # segments of 129, 2 and 1 rows ...
    labels = labels[rng.permutation(len(labels))]            # ... scattered over the bank: a genuine permutation
    N = len(labels)
    bank = (rng.standard_normal((N, D)) + 0.5).astype(np.float32)
    ref = NC.segment_mean_ref(bank, labels).astype(np.float32)
    got = speaker_mean_cohort(dev(NC.padded(bank, 4))[:, :D], labels.tolist()).cpu().numpy()
    assert got.shape == (3, D)
    ulp = np.abs(got - ref) / np.spacing(np.abs(ref))
    print(f"score-norm-parity: segment_mean D={D} segments (2, 1, 129): {ulp.max():.1f} ulp of the float64 mean to f32")
    assert ulp.max() <= 1.0
    order = np.argsort(labels, kind="stable").astype(np.int32)
    assert not np.array_equal(order, np.arange(N))
    offsets = np.array([0, 2, 3, N], dtype=np.int32)
    again = ops.segment_mean(dev(bank), dev(order), dev(offsets)).cpu().numpy()
    assert np.array_equal(again, got)                        # gap or none, twice: the same bits
    # a row number outside the bank is not dereferenced: that mean is NaN, the others are untouched
    order[1] = N
    bad = ops.segment_mean(dev(bank), dev(order), dev(offsets)).cpu().numpy()
    assert np.isnan(bad[0]).all() and np.array_equal(bad[1:], got[1:])


# ------------------------------------------------------------------------------------------------ cohort_stats end to end
# Cases whose mu / sd take the a-priori bound of an f32 dot product of unit vectors (D 2^-24) instead of 2 x the host
# path's error: the MFMA product adds in another order than torch's CPU matmul, and with the host error at 1e-8 .. 1e-7
# the 2 x rule would ask the device to be closer to float64 than one rounding of the product allows.  The measured figures
# are in profiles/score_norm_parity.txt.
APRIORI_CASES = frozenset()


def _stats_bounds(c, key):
    if key in APRIORI_CASES:
        return max(c["bound_mu"], c["apriori"]), max(c["bound_sd"], c["apriori"]), "a priori"
    return c["bound_mu"], c["bound_sd"], "2 x host"


def _run_cohort(c, rows_per_block=None, workspace=None):
    from w2v2_speaker_amd import ops
    mean, std = (None, None) if c["mean"] is None else (dev(c["mean"]), dev(c["std"]))
    mu, sd = ops.cohort_stats(dev(c["bank"]), dev(c["cohort"]), c["K"], mean, std, c["length_norm"],
                              rows_per_block=rows_per_block, workspace=workspace)
    return mu.cpu().numpy(), sd.cpu().numpy()


@pytest.mark.parametrize("shape", NC.COHORT_SHAPES)
def test_cohort_stats_end_to_end_and_across_block_edges(shape):
    c = NC.cohort_case(*shape)
    N = shape[0]
    b_mu, b_sd, rule = _stats_bounds(c, (shape, False, False))
    base = None
    for rpb in (3, N, None):
        mu, sd = _run_cohort(c, rpb)
        e_mu, e_sd = np.abs(mu - c["mu"]).max(), np.abs(sd - c["sd"]).max()
        print(f"score-norm-parity: cohort_stats N,M,D,K={shape} rows_per_block={rpb}: mu {e_mu:.2e} bound {b_mu:.2e}; sd "
              f"{e_sd:.2e} bound {b_sd:.2e} ({rule}; host path mu {np.abs(c['host_mu'] - c['mu']).max():.2e} sd "
              f"{np.abs(c['host_sd'] - c['sd']).max():.2e}; a priori {c['apriori']:.2e})")
        assert not np.isnan(mu).any() and not np.isnan(sd).any()
        assert e_mu <= b_mu and e_sd <= b_sd
        if base is None:
            base = (mu, sd)
        # a block edge corrupts nothing: every blocking gives every row the same statistics up to the product's rounding
        # (the GEMM router may pick another kernel, and with it another order of the adds, for another block height)
        assert np.abs(mu - base[0]).max() <= 2 * c["apriori"] and np.abs(sd - base[1]).max() <= 2 * c["apriori"]
    # a caller-owned workspace of exactly rows_per_block * ldS, NaN-filled: the bits of the first run, which had the same blocks
    ldS = (shape[1] + 3) // 4 * 4
    ws = torch.full((3 * ldS,), float("nan"), dtype=torch.float32, device=DEV)
    mu, sd = _run_cohort(c, 3, ws)
    assert np.array_equal(mu, base[0]) and np.array_equal(sd, base[1])


@pytest.mark.parametrize("centre,length_norm", NC.CENTRE_MODES)
def test_cohort_stats_every_centring_mode(centre, length_norm):
    c = NC.cohort_case(*NC.MIDDLE, centre, length_norm)
    b_mu, b_sd, rule = _stats_bounds(c, (NC.MIDDLE, centre, length_norm))
    mu, sd = _run_cohort(c)
    e_mu, e_sd = np.abs(mu - c["mu"]).max(), np.abs(sd - c["sd"]).max()
    print(f"score-norm-parity: cohort_stats N,M,D,K={NC.MIDDLE} centre={int(centre)} lnorm={int(length_norm)}: mu {e_mu:.2e} "
          f"bound {b_mu:.2e}; sd {e_sd:.2e} bound {b_sd:.2e} ({rule}; host path mu {np.abs(c['host_mu'] - c['mu']).max():.2e} "
          f"sd {np.abs(c['host_sd'] - c['sd']).max():.2e}; a priori {c['apriori']:.2e})")
    assert e_mu <= b_mu and e_sd <= b_sd


# ------------------------------------------------------------------------------------------------ score_pairs_norm
@pytest.mark.parametrize("mode", NC.MODES)
def test_score_pairs_norm_modes_counts_and_bad_indices(mode):
    from w2v2_speaker_amd import ops
    mu = np.array([0.10, 0.25, -0.05, 0.40, 0.20], dtype=np.float32)
    sd = np.array([0.05, 0.0, 0.11, 0.02, 0.30], dtype=np.float32)          # row 1: sd = 0, the formula divides by 1e-12
    all_pairs = np.array([(0, 2), (1, 3), (4, 1), (3, 3), (2, 0)], dtype=np.int32)
    all_cos = np.array([0.31, -0.2, 0.25, 1.0, 0.07], dtype=np.float32)
    for P in (1, 4, 5):
        pairs, cos = all_pairs[:P], all_cos[:P]
        ref = NC.norm_scores_ref(cos, pairs, mu, sd, mode)
        out = torch.full((P + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        ops.score_pairs_norm(dev(cos), dev(pairs), dev(mu), dev(sd), mode, out)
        got = out.cpu().numpy()
        assert (got[P:] == SENTINEL).all(), "written past the outputs"
        rel = np.abs(got[:P].astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-30)
        print(f"score-norm-parity: score_pairs_norm mode={mode} P={P}: rel {rel.max():.2e} bound {2.0 ** -23:.2e}")
        assert np.isfinite(got[:P]).all() and (rel <= 2.0 ** -23).all()       # double arithmetic, one rounding to f32
    for bad in ((5, 0), (0, -1), (2 ** 31 - 1, 1)):
        pairs = all_pairs.copy()
        pairs[2] = bad
        got = ops.score_pairs_norm(dev(all_cos), dev(pairs), dev(mu), dev(sd), mode).cpu().numpy()
        ref = NC.norm_scores_ref(all_cos, all_pairs, mu, sd, mode)
        keep = [0, 1, 3, 4]
        assert np.isnan(got[2]) and np.allclose(got[keep], ref[keep], rtol=2.0 ** -23, atol=0)


# ------------------------------------------------------------------------------------------------ score_trials_device
@pytest.mark.parametrize("mode", NC.MODES)
def test_score_trials_device_with_score_norm_within_the_bound(mode):
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import ScoreNorm, TrialIndex, score_trials_device
    t = NC.trials_case(mode)
    c = t["case"]
    idx = TrialIndex.from_rows(t["pairs"], [0] * len(t["pairs"]), len(c["bank"]))
    rec = score_trials_device(dev(c["bank"]), idx, score_norm=ScoreNorm(dev(c["cohort"]), c["K"], mode))
    err, err_h = np.abs(rec.scores - t["score"]), np.abs(t["host_score"] - t["score"])
    print(f"score-norm-parity: score_trials_device(score_norm=) N,M,D,K={NC.MIDDLE} mode={mode}: max err {err.max():.2e}, "
          f"max err / bound {(err / t['bound']).max():.2f}; host path {err_h.max():.2e}; floor_z in "
          f"[{NC.floor_z(t['cos'], t['pairs'], c['mu'], c['sd'], mode).min():.2e}, "
          f"{NC.floor_z(t['cos'], t['pairs'], c['mu'], c['sd'], mode).max():.2e}]")
    assert (err <= t["bound"]).all()
    assert rec.host_copy_floats == len(t["pairs"]) and rec.bank_floats == c["bank"].size


def test_score_norm_none_leaves_the_device_scores_bitwise_as_they_were():
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import TrialIndex, score_trials_device
    c = SC.g12_case("")
    idx = TrialIndex.from_rows(c["pairs"], c["gt"], 32)
    bank = dev(c["bank"])
    a = score_trials_device(bank, idx)
    b = score_trials_device(bank, idx, score_norm=None)
    _, parent = ops.score_pairs(bank, dev(c["pairs"]))        # what the parent commit's score_trials_device copies back
    assert np.array_equal(a.scores, b.scores) and np.array_equal(a.scores, parent.cpu().numpy().astype(np.float64))
    k = score_trials_device(bank, idx, keep_on_device=True, score_norm=None)
    assert k.scores is None and torch.equal(k.device_scores, parent)


# ------------------------------------------------------------------------------------------------ the evaluator
def _g12_eval(c):
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    keys = [f"u{i:02d}" for i in range(32)]
    return keys, [EvaluationPair(bool(g), keys[i], keys[j]) for g, (i, j) in zip(c["gt"], c["pairs"])]


@pytest.mark.parametrize("mode", NC.MODES)
def test_evaluate_bank_with_score_norm_against_the_host_evaluator_on_g12(mode):
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EmbeddingSample
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import ScoreNorm, host_metrics, speaker_mean_cohort
    c = NC.g12_norm_case(mode)
    keys, pairs = _g12_eval(c)
    bank = dev(c["bank"])
    cohort = speaker_mean_cohort(bank, c["speaker"].tolist())
    ulp = np.abs(cohort.cpu().numpy() - c["cohort"]) / np.spacing(np.abs(c["cohort"]))
    assert cohort.shape == c["cohort"].shape and ulp.max() <= 1.0
    sn = ScoreNorm(cohort, c["K"], mode)
    ev = CosineDistanceEvaluator()
    res = ev.evaluate_bank_metrics(pairs, keys, bank, score_norm=sn)        # metrics="host"
    scores = ev.last_bank_scoring.scores
    err, err_h = np.abs(scores - c["score"]), np.abs(scores - c["host_score"])
    from w2v2_speaker_amd import ops
    mu, sd = (v.cpu().numpy() for v in ops.cohort_stats(bank, cohort, c["K"]))
    e_mu, e_sd = np.abs(mu - c["mu"]).max(), np.abs(sd - c["sd"]).max()
    print(f"score-norm-parity: g12 evaluate_bank_metrics(score_norm=) mode={mode} K={c['K']} M={len(c['cohort'])} D=1536: mu {e_mu:.2e} "
          f"(2 x host {c['bound_mu']:.2e}) sd {e_sd:.2e} (2 x host {c['bound_sd']:.2e}), a priori {c['apriori']:.2e}; scores vs "
          f"float64 {err.max():.2e} = {(err / c['bound']).max():.2f} of the 2 x rule's bound, {(err / c['bound_apriori']).max():.4f} "
          f"of the a-priori one; vs the host evaluator {err_h.max():.2e}; host path {np.abs(c['host_score'] - c['score']).max():.2e}; "
          f"cohort {ulp.max():.1f} ulp")
    # THE A-PRIORI CASE of this file.  Every cohort cosine of g12 lies in [0.9966, 0.9993]: the 1536 products of a row
    # pair are all positive, the f32 MFMA accumulator grows monotonically, and its rounding (another order of adds than
    # the blocked sums of torch's CPU matmul, not a worse one by construction) leaves mu / sd a few 2^-24 further from
    # float64 than the host path lands on a given machine: measured on the MI355X mu 5.0e-07 and sd 6.5e-07 against 2 x
    # host bounds of 4.0e-07 and 3.1e-07 (they change with the host's CPU); with sd near 5e-4 that is 1.30 - 1.47 x the 2 x
    # rule's score bound (3.1e-3, 3.6e-3 and 2.0e-3 for z, t and s).  The statistics therefore take the a-priori bound of an f32 dot product of unit vectors, D 2^-24, and
    # the scores its propagation (score_norm_cases.floor_z(f_stats=)); profiles/score_norm_parity.txt has the figures.
    assert e_mu <= c["apriori"] and e_sd <= c["apriori"]
    assert (err <= c["bound_apriori"]).all() and (err_h <= 2 * c["bound_apriori"]).all()
    assert ev.last_bank_scoring.host_copy_floats == 496
    assert res == host_metrics(c["gt"], scores.tolist())
    # the host evaluator with the same cohort: the same kind of answer from plain torch
    samples = [EmbeddingSample(k, torch.from_numpy(r)) for k, r in zip(keys, c["bank"])]
    host = ev.evaluate(pairs, samples, score_norm=ScoreNorm(cohort.cpu(), c["K"], mode))
    assert set(host) == set(res) and 0.0 <= host["eer"] <= 1.0
    # metrics="device": the scores stay, the four metrics are the host metrics of those device scores
    got = ev.evaluate_bank_metrics(pairs, keys, bank, metrics="device", score_norm=sn)
    rec = ev.last_bank_scoring
    assert rec.scores is None and rec.host_copy_floats == 0 and ev.last_bank_metrics.path == "device"
    dscores = rec.device_scores.cpu().numpy()
    assert np.array_equal(dscores.astype(np.float64), scores)
    m = MC.metrics_ref(c["gt"], dscores)
    MC.check_against_host(got, m, {**res, "n_thresholds": m["n_thresholds"]}, what=f"g12 score_norm {mode}")
    MC.check_mdc_threshold(got["mdc_threshold"], c["gt"], dscores)


@pytest.mark.parametrize("name", ["wav2vec2", "ecapa"])
def test_evaluate_trials_with_score_norm_on_the_device_and_on_the_host(name):
    from test_scoring_gpu import _module_case
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import ScoreNorm, TrialIndex, score_trials_device
    mod, inputs, kw = _module_case(name)
    keys = sorted(inputs)
    idx = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    gt = [int((i + j) % 3 == 0 or j == i + 1) for i, j in idx]
    pairs = [EvaluationPair(bool(t), keys[i], keys[j]) for t, (i, j) in zip(gt, idx)]
    bank = torch.cat(mod.compute_speaker_embeddings([inputs[k] for k in keys], **kw)).detach().float()
    D = bank.shape[1]
    rng = np.random.default_rng(11)
    host_bank = bank.cpu().numpy()
    cohort = (host_bank[rng.integers(0, 6, 9)] + host_bank.std() * rng.standard_normal((9, D))).astype(np.float32)
    K, mode = 4, "s"
    sn = ScoreNorm(torch.from_numpy(cohort), K, mode)
    mu, sd = NC.cohort_stats_ref(host_bank, cohort, K)
    cos, _ = SC.score_pairs_ref(host_bank, idx)
    ref = NC.norm_scores_ref(cos, idx, mu, sd, mode)
    host_scores = NC.host_norm_scores(host_bank, cohort, idx, K, mode)
    b = np.maximum(2.0 * np.abs(host_scores - ref).max(), NC.floor_z(cos, idx, mu, sd, mode))
    got = mod.evaluate_trials(pairs, inputs, scoring="device", score_norm=sn, **kw)
    rec = mod.evaluator.last_bank_scoring
    err = np.abs(rec.scores - ref)
    print(f"score-norm-parity: {name} evaluate_trials(scoring='device', score_norm=) D={D}: max err {err.max():.2e}, max err / "
          f"bound {(err / b).max():.2f}; host path {np.abs(host_scores - ref).max():.2e}")
    assert (err <= b).all() and rec.host_copy_floats == 15
    host = mod.evaluate_trials(pairs, inputs, scoring="host", score_norm=sn, **kw)
    assert set(host) == set(got) and 0.0 <= got["eer"] <= 1.0 and 0.0 <= host["eer"] <= 1.0
    dm = mod.evaluate_trials(pairs, inputs, scoring="device", metrics="device", score_norm=sn, **kw)
    assert abs(dm["eer"] - got["eer"]) <= MC.EER_BOUND
    # score_norm=None: bitwise what score_trials_device gives without the argument
    plain = mod.evaluate_trials(pairs, inputs, scoring="device", score_norm=None, **kw)
    scores = mod.evaluator.last_bank_scoring.scores
    parent = score_trials_device(bank, TrialIndex(pairs, keys))
    assert np.array_equal(scores, parent.scores) and plain == mod.evaluate_trials(pairs, inputs, scoring="device", **kw)
