"""Score calibration on the GPU (csrc/calibration.hip): the statistics of one forced round, the whole fit, the status
codes, the apply map and the llr metrics against the float64 oracle of tests/calibration_cases.py within the bounds stated
there, then the public interface -- ``evaluate_bank_metrics(calibration=)`` of the three evaluators, a fused three-member
ensemble, ``evaluate_trials`` of a module, and the unchanged defaults.  Every output sits in front of sentinel cells; every
kernel runs twice and the second run is compared for equal bits only.  Every ``calibration-parity:`` line goes to
profiles/calibration_parity.txt.

Measured on an MI355X (profiles/calibration_parity.txt): statistics at most 2.1e-16 (J), 3.1e-16 (g), 6.6e-16 (H) of
sum |term| against the bound 1e-12; the oracle's decrement at the device's weights at most 7.3e-14 against 1e-10 after 4 - 9
rounds; apply bit-equal on 49,948 llrs, none at a rounding boundary; cllr within 2.7e-16 relative against 1e-12."""
import numpy as np
import pytest
import torch

import backend_cases as bc
import calibration_cases as CC
import metrics_cases as MC
import scoring_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
T = 2048
KEYS = ("eer", "eer_threshold", "mdc", "mdc_threshold")
LLR_KEYS = ("cllr", "act_dcf", "act_p_miss", "act_p_fa")
SENTINEL = -777.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_scores(S, pad):
    """[K, P] f32 on the device; with ``pad`` as a view of a [K, P + pad] buffer whose pad holds NaN."""
    return dev(CC.padded(S, pad))[:, :S.shape[1]] if pad else dev(S)


def run_fit(S, y, pad=0, **kw):
    """ops.calib_fit twice into a guarded record with a guarded workspace -> (fields, the record's doubles)."""
    from w2v2_speaker_amd import ops
    R = ops.CALIB_RECORD_DOUBLES
    scores, labels = dev_scores(S, pad), dev(y)
    need = ops.calib_workspace(S.shape[1], "cpu").numel()
    recs = []
    for _ in range(2):
        rec = torch.full((R + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
        ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        ops.calib_fit(scores, labels, record=rec, workspace=ws, **kw)
        host = rec.cpu().numpy()
        assert (host[R:] == SENTINEL).all() and (ws[need:].cpu().numpy() == 0xAB).all(), "written past the outputs"
        recs.append(host[:R])
    assert np.array_equal(recs[0].view(np.uint64), recs[1].view(np.uint64)), "a second run gave other bits"
    return ops.calib_record_fields(recs[0].tolist()), recs[0]


def oracle_problem(S, y, p_target):
    m, sd = CC.moments(S)
    return m, sd, CC.features(S, m, 1.0 / sd), CC.effective_prior(p_target)


# ------------------------------------------------------------------------------------------------ 1. statistics
def test_statistics_of_one_forced_round_at_every_case():
    from w2v2_speaker_amd import ops
    assert ops.CALIB_TILE == T
    worst = {"J": 0.0, "g": 0.0, "H": 0.0}
    for n, (name, P, K, p_target, pad) in enumerate(CC.stat_cases(T)):
        S, y = CC.family(name, P, K, 1)
        w = CC.start_point(K, P + K)
        f, _ = run_fit(S, y, pad, p_target=p_target, max_iter=1, w_start=w.tolist())
        m, sd, X, pi = oracle_problem(S, y, p_target)
        J, g, H, Ja, ga, Ha = CC.stats(X, y, w, pi, with_abs=True)
        assert f["rounds"] == 1 and f["K"] == K and f["w"] == w.tolist(), (name, P, K)
        assert (f["n_tar"], f["n_non"], f["n_nan"]) == (int(y.sum()), int(P - y.sum()), 0)
        rel = {"J": abs(f["J"] - J) / Ja, "g": float(np.max(np.abs(np.array(f["g"]) - g) / ga)),
               "H": float(np.max(np.abs(np.array(f["H"]) - H) / Ha))}
        for k in worst:
            worst[k] = max(worst[k], rel[k])
        print(f"calibration-parity: statistics {name} P={P} K={K} p_target={p_target} ld=P+{pad}: |error| / sum|term| J "
              f"{rel['J']:.2e} g {rel['g']:.2e} H {rel['H']:.2e} (bound {CC.STAT_REL:.0e})")
        assert rel["J"] <= CC.STAT_REL and rel["g"] <= CC.STAT_REL and rel["H"] <= CC.STAT_REL, (name, P, K, rel)
        assert np.array_equal(np.array(f["H"]), np.array(f["H"]).T)
    print(f"calibration-parity: statistics over {len(CC.stat_cases(T))} cases: worst |error| / sum|term| J {worst['J']:.2e} "
          f"g {worst['g']:.2e} H {worst['H']:.2e} (bound {CC.STAT_REL:.0e})")


# ------------------------------------------------------------------------------------------------ 2. the fit
@pytest.mark.parametrize("case", CC.fitted_cases(T), ids=lambda c: f"{c[0]}-P{c[1]}-K{c[2]}-p{c[3]}")
def test_fit_is_optimal_by_the_oracles_decrement(case):
    name, P, K, p_target, pad = case
    S, y = CC.family(name, P, K, 1)
    f, rec = run_fit(S, y, pad, p_target=p_target)
    m, sd, X, pi = oracle_problem(S, y, p_target)
    assert f["status"] == 1 and 1 <= f["rounds"] <= 32, (f["status"], f["rounds"])
    w = np.array(f["w"])
    dec = CC.decrement(X, y, w, pi)
    e_m = float(np.abs(np.array(f["mean"]) - m).max() / np.abs(S).mean())
    e_sd = float(np.abs(np.array(f["sd"]) / sd - 1).max())
    e_r = float(np.abs(np.array(f["r"]) * np.array(f["sd"]) - 1).max())
    a = CC.affine(w, np.array(f["mean"]), np.array(f["r"]))
    scale = abs(w[0]) + np.abs(a[1:] * np.array(f["mean"])).sum()
    e_a0, e_ak = abs(f["a"][0] - a[0]) / scale, float(np.abs(np.array(f["a"][1:]) / a[1:] - 1).max())
    print(f"calibration-parity: fit {name} P={P} K={K} p_target={p_target} ld=P+{pad}: {f['rounds']} rounds, own decrement "
          f"{f['decrement']:.2e}, oracle's decrement at the device's w {dec:.2e} (bound {CC.FIT_DECREMENT:.0e}); mean "
          f"{e_m:.1e} sd {e_sd:.1e} r {e_r:.1e} a0 {e_a0:.1e} a_k {e_ak:.1e}")
    assert dec <= CC.FIT_DECREMENT
    assert e_m <= 1e-12 and e_sd <= 1e-12 and e_r <= 4 * 2.0 ** -53 and e_a0 <= 1e-11 and e_ak <= 4 * 2.0 ** -53
    assert (f["n_tar"], f["n_non"], f["n_nan"]) == (int(y.sum()), int(P - y.sum()), 0)
    # the rounds behind the convergence changed nothing: a fit of exactly `rounds` rounds leaves the same bits
    _, short = run_fit(S, y, pad, p_target=p_target, max_iter=f["rounds"])
    assert np.array_equal(short.view(np.uint64), rec.view(np.uint64))
    if f["rounds"] > 1:
        g, _ = run_fit(S, y, pad, p_target=p_target, max_iter=f["rounds"] - 1)
        assert g["status"] == 0 and g["rounds"] == f["rounds"] - 1


def test_fit_with_a_ridge_against_the_oracle():
    S, y = CC.family("collinear", T + 1, 2, 1)
    f, _ = run_fit(S, y, 0, ridge=0.05)
    m, sd, X, pi = oracle_problem(S, y, 0.05)
    assert f["status"] == 1 and CC.decrement(X, y, np.array(f["w"]), pi, ridge=0.05) <= CC.FIT_DECREMENT
    w0, J0, _ = CC.newton(X, y, pi, ridge=0.05)
    assert abs(f["J"] - J0) <= 2e-12


# ------------------------------------------------------------------------------------------------ 3. status codes
def test_status_codes_and_their_calibration_errors():
    from w2v2_speaker_amd.evaluation.speaker import CalibrationError, ScoreCalibration
    S, y = CC.separable_set()
    f, _ = run_fit(S, y)
    assert f["status"] == 0 and f["rounds"] == 32 and f["J"] < 1e-9
    with pytest.raises(CalibrationError, match="ridge") as e:
        ScoreCalibration().fit_scores(dev(S), dev(y))
    assert e.value.status == 0
    assert ScoreCalibration(ridge=1e-3).fit_scores(dev(S), dev(y)).status == 1
    S, y = CC.constant_system()
    f, _ = run_fit(S, y)
    assert f["status"] == 2 and f["rounds"] == 0 and f["sd"][1] == 0.0
    with pytest.raises(CalibrationError, match="constant"):
        ScoreCalibration().fit_scores(dev(S), dev(y))
    S, y = CC.family("gauss1.0", T + 3, 2, 2)
    S[1, T + 1] = np.nan
    S[0, 5] = np.nan
    f, _ = run_fit(S, y)
    assert f["status"] == 2 and f["n_nan"] == 2 and f["rounds"] == 0
    with pytest.raises(CalibrationError, match="NaN"):
        ScoreCalibration().fit_scores(dev(S), dev(y))
    S, y = CC.one_class()
    for label in (0, 1):
        f, _ = run_fit(S, np.full_like(y, label))
        assert f["status"] == 2 and f["rounds"] == 0 and (f["n_tar"], f["n_non"]) == ((100, 0) if label else (0, 100))
    with pytest.raises(CalibrationError, match="one class"):
        ScoreCalibration().fit_scores(dev(S), dev(y))


# ------------------------------------------------------------------------------------------------ 4. apply
def test_apply_equals_the_rounded_float64_map():
    from w2v2_speaker_amd import ops
    boundary = total = 0
    for name, P, K, p_target, pad in CC.stat_cases(T):
        S, y = CC.family(name, P, K, 1)
        m, sd = CC.moments(S)
        a = CC.affine(CC.start_point(K, P + K), m, 1.0 / sd)
        want, v, edge = CC.apply_ref(S, a)
        outs = []
        for _ in range(2):
            out = torch.full((P + GUARD,), -12345.0, dtype=torch.float32, device=DEV)
            ops.calib_apply(dev_scores(S, pad), dev(a), out)
            host = out.cpu().numpy()
            assert (host[P:] == -12345.0).all(), "written past the outputs"
            outs.append(host[:P])
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
        got = outs[0]
        assert np.array_equal(got[~edge].view(np.uint32), want[~edge].view(np.uint32)), (name, P, K)
        assert (np.abs(got[edge].astype(np.float64) - v[edge]) <= np.spacing(np.abs(want[edge])).astype(np.float64)).all()
        boundary += int(edge.sum())
        total += P
    print(f"calibration-parity: apply over {len(CC.stat_cases(T))} cases, {total} llrs: bit-equal to f32(a_0 + sum a_k s_k) "
          f"in float64; {boundary} values at an f32 rounding boundary")
    assert boundary == 0


def test_apply_reads_the_record_and_a_nan_score_gives_a_nan_llr():
    from w2v2_speaker_amd import ops
    S, y = CC.family("plda", T + 5, 3, 1)
    rec = ops.calib_fit(dev(S), dev(y))
    f = ops.calib_record_fields(rec)
    assert f["status"] == 1
    want, _, edge = CC.apply_ref(S, f["a"])
    got = ops.calib_apply(dev(S), rec).cpu().numpy()
    assert not edge.any() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    S2 = S.copy()
    S2[1, 7] = np.nan
    got = ops.calib_apply(dev_scores(S2, CC.PAD), rec).cpu().numpy()
    assert np.isnan(got[7]) and np.array_equal(np.delete(got, 7).view(np.uint32), np.delete(want, 7).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. llr metrics
@pytest.mark.parametrize("name", sorted(CC.llr_cases(T)))
def test_llr_metrics_against_numpy(name):
    from w2v2_speaker_amd import ops
    z, y, p_target = CC.llr_cases(T)[name]
    outs = []
    for _ in range(2):
        out = torch.full((8 + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
        ops.llr_metrics(dev(z), dev(y), p_target=p_target, out=out)
        host = out.cpu().numpy()
        assert (host[8:] == SENTINEL).all(), "written past the outputs"
        outs.append(host[:8])
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)), "a second run gave other bits"
    got, want = dict(zip(ops.LLR_METRICS_FIELDS, outs[0].tolist())), CC.llr_metrics_ref(z, y, p_target=p_target)
    for k in ("n_pos", "n_nan", "act_p_miss", "act_p_fa", "act_dcf"):
        assert got[k] == want[k], (k, got[k], want[k])
    rel = 0.0
    for k in ("cllr", "cllr_tar", "cllr_non"):
        if np.isfinite(want[k]):
            rel = max(rel, abs(got[k] - want[k]) / abs(want[k]))
            assert abs(got[k] - want[k]) <= CC.CLLR_REL * abs(want[k]), (k, got[k], want[k])
        else:
            assert got[k] == want[k], (k, got[k], want[k])
    print(f"calibration-parity: llr_metrics {name} (P = {len(z)}, p_target {p_target}): counts, act_p_miss {got['act_p_miss']:.6f}, "
          f"act_p_fa {got['act_p_fa']:.6f}, act_dcf {got['act_dcf']:.6f} exact; cllr {got['cllr']:.12f} rel {rel:.2e} "
          f"(bound {CC.CLLR_REL:.0e})")


def test_llr_metrics_count_nan_llrs():
    from w2v2_speaker_amd import ops
    z, y, p_target = CC.llr_cases(T)[f"size{T + 1}"]
    z = z.copy()
    z[[3, T]] = np.nan
    got = dict(zip(ops.LLR_METRICS_FIELDS, ops.llr_metrics(dev(z), dev(y), p_target=p_target).cpu().tolist()))
    assert got["n_nan"] == 2 and np.isnan(got["cllr"]) and got["n_pos"] == int(y.sum())


# ------------------------------------------------------------------------------------------------ 6. the public interface
def check_metrics(got, gt, llr, host, what):
    """EER / minDCF of device llrs against the rule of metrics_cases.py and against the host path, within the bounds stated
    there (the EER and minDCF bounds; an EER threshold against the rule, within the rule's own bound -- the host's
    tolerance for a vertical crossing is written for scores in [-1, 1], which llrs are not)."""
    m = MC.metrics_ref(gt, llr)
    e_ref, e_host = abs(got["eer"] - m["eer"]), abs(got["eer"] - host["eer"])
    assert e_ref <= MC.EER_BOUND and e_host <= MC.EER_BOUND, (what, got["eer"], m["eer"], host["eer"])
    d_ref, d_host = abs(got["mdc"] - m["mdc"]) / m["mdc"], abs(got["mdc"] - host["mdc"]) / host["mdc"]
    assert d_ref <= MC.MDC_REL and d_host <= MC.MDC_REL, (what, got["mdc"], m["mdc"], host["mdc"])
    MC.check_mdc_threshold(got["mdc_threshold"], gt, llr)
    if m["kind"] == "vertical":
        assert got["eer_threshold"] == m["eer_threshold"], what
    elif np.isfinite(m["thr_lo"]):
        assert abs(got["eer_threshold"] - m["eer_threshold"]) <= MC.thr_bound(m), what
    else:
        assert got["eer_threshold"] == np.inf, what
    return {"eer_host": e_host, "mdc_host": d_host}


def check_applied(llr, rows, a):
    """Device llrs against the oracle's map of the scores ``rows`` [K, P] f32: the rule of the apply test."""
    want, v, edge = CC.apply_ref(rows, a)
    assert np.array_equal(llr[~edge].view(np.uint32), want[~edge].view(np.uint32))
    assert (np.abs(llr[edge].astype(np.float64) - v[edge]) <= np.spacing(np.abs(want[edge])).astype(np.float64)).all()


def _check_device_against_host(ev, pairs, keys, bank, gt, cal, what):
    """evaluate_bank_metrics(metrics="device", calibration=cal) against the host path of the same call."""
    plain = ev.evaluate_bank_metrics(pairs, keys, bank, metrics="host" if isinstance(bank, list) else "device")
    assert set(plain) == set(KEYS)
    got = ev.evaluate_bank_metrics(pairs, keys, bank, metrics="device", calibration=cal)
    rec, met = ev.last_bank_scoring, ev.last_bank_metrics
    assert rec.scores is None and rec.host_copy_floats == 0 and met.path == "device"
    assert met.host_copy_floats == 0 and met.host_copy_doubles == 8           # eight doubles crossed, no floats
    llr = rec.device_scores.cpu().numpy()
    host = ev.evaluate_bank_metrics(pairs, keys, bank, metrics="host", calibration=cal)
    assert ev.last_bank_scoring.host_copy_floats == len(gt)
    assert np.array_equal(ev.last_bank_scoring.scores, llr.astype(np.float64))  # the same llrs on either path
    assert set(got) == set(host) == set(KEYS) | set(LLR_KEYS)
    f = check_metrics(got, gt, llr, host, what)
    want = CC.llr_metrics_ref(llr, gt, cal.c_miss, cal.c_fa, cal.p_target)
    for k in ("act_dcf", "act_p_miss", "act_p_fa"):
        assert got[k] == want[k] == host[k], (what, k)
    assert abs(got["cllr"] - want["cllr"]) <= CC.CLLR_REL * want["cllr"] and abs(host["cllr"] - want["cllr"]) <= CC.CLLR_REL * want["cllr"]
    assert cal.weights[1:].min() > 0 or len(cal.weights) > 2
    if len(cal.weights) == 2:                               # a positive slope keeps the order: the EER does not move
        assert abs(got["eer"] - plain["eer"]) <= MC.EER_BOUND, (what, got["eer"], plain["eer"])
    print(f"calibration-parity: {what} evaluate_bank_metrics(metrics='device', calibration=): a = "
          f"{np.array2string(cal.weights, precision=4)}, eer {got['eer']:.6f} (uncalibrated {plain['eer']:.6f}) vs host "
          f"{f['eer_host']:.2e}, mdc rel vs host {f['mdc_host']:.2e}, cllr {got['cllr']:.6f} act_dcf {got['act_dcf']:.6f}")
    return got


@pytest.mark.parametrize("tag", ["_c", "_cl"])
def test_cosine_evaluate_bank_metrics_with_a_calibration_on_g12(tag):
    from test_scoring_gpu import _g12_eval
    from w2v2_speaker_amd.evaluation.speaker import CosineDistanceEvaluator, ScoreCalibration
    g, c = SC.g12(), SC.g12_case(tag)
    keys, pairs = _g12_eval()
    centre, ln = SC.G12_BRANCHES[tag]
    ev = CosineDistanceEvaluator(centre, ln, 32)
    ev.mean, ev.std = torch.from_numpy(g["fit_mean"]), torch.from_numpy(g["fit_std"])
    bank = dev(c["bank"])
    cal = ScoreCalibration().fit_bank(ev, pairs, keys, bank)
    assert cal.status == 1 and cal.record is not None and cal.record.is_cuda
    # the fit saw the evaluator's own metric scores: the oracle's decrement at its weights, on those scores
    ev.evaluate_bank_metrics(pairs, keys, bank, metrics="device")
    scores = ev.last_bank_scoring.device_scores.cpu().numpy()
    m, sd, X, pi = oracle_problem(scores[None, :], np.asarray(c["gt"]), 0.05)
    assert CC.decrement(X, np.asarray(c["gt"]), np.array(cal.fields["w"]), pi) <= CC.FIT_DECREMENT
    _check_device_against_host(ev, pairs, keys, bank, np.asarray(c["gt"]), cal, f"cosine g12{tag}")


@pytest.fixture(scope="module")
def e2e():
    from w2v2_speaker_amd.evaluation.speaker import EvaluationPair
    train, labels, test, _, pairs, gt = bc.two_covariance_set(0, **bc.E2E)
    keys = [f"u{r}" for r in range(len(test))]
    trial = [EvaluationPair(bool(g), keys[i], keys[j]) for (i, j), g in zip(pairs.tolist(), gt)]
    return dict(train=train, labels=labels, test=test, pairs=pairs, gt=np.asarray(gt, dtype=np.uint8), keys=keys, trial=trial)


@pytest.mark.parametrize("kind", ("lda", "plda"))
def test_latent_evaluators_evaluate_bank_metrics_with_a_calibration(e2e, kind):
    from w2v2_speaker_amd.evaluation.speaker import LDAEvaluator, PLDAEvaluator, ScoreCalibration
    ev = LDAEvaluator(True, True, 0, 16, False, projection="lda") if kind == "lda" else PLDAEvaluator(16, 16, 10, 0)
    ev.fit_parameters_bank(dev(e2e["train"]), e2e["labels"])
    bank = dev(e2e["test"])
    cal = ScoreCalibration(p_target=0.01 if kind == "plda" else 0.05).fit_bank(ev, e2e["trial"], e2e["keys"], bank)
    got = _check_device_against_host(ev, e2e["trial"], e2e["keys"], bank, e2e["gt"], cal, kind)
    if kind == "plda":                                      # the raw PLDA llr, judged as an llr
        raw = ev.evaluate_bank_metrics(e2e["trial"], e2e["keys"], bank, metrics="device", llr_metrics=True)
        want = CC.llr_metrics_ref(ev.last_bank_scoring.device_scores.cpu().numpy(), e2e["gt"])
        assert set(raw) == set(KEYS) | set(LLR_KEYS) and ev.last_bank_metrics.host_copy_doubles == 8
        assert all(raw[k] == want[k] for k in ("act_dcf", "act_p_miss", "act_p_fa"))
        assert abs(raw["cllr"] - want["cllr"]) <= CC.CLLR_REL * want["cllr"]
        print(f"calibration-parity: plda raw llr (llr_metrics=True, p_target 0.05): cllr {raw['cllr']:.4f} act_dcf "
              f"{raw['act_dcf']:.4f}; calibrated at p_target 0.01: cllr {got['cllr']:.4f} act_dcf {got['act_dcf']:.4f}")


def _members(test):
    rng = np.random.default_rng(11)
    return [test, (test + 0.8 * rng.standard_normal(test.shape)).astype(np.float32),
            (test[:, ::-1] * 0.5 + 0.6 * rng.standard_normal(test.shape)).astype(np.float32)]


def test_three_member_ensemble_is_fused_on_the_device(e2e):
    from w2v2_speaker_amd.evaluation.speaker import CosineDistanceEvaluator, ScoreCalibration
    ev = CosineDistanceEvaluator()
    banks = [dev(m) for m in _members(e2e["test"])]
    P = len(e2e["gt"])
    with pytest.raises(NotImplementedError):                # without a calibration: today's host combination only
        ev.evaluate_bank_metrics(e2e["trial"], e2e["keys"], banks, metrics="device")
    mean = ev.evaluate_bank_metrics(e2e["trial"], e2e["keys"], banks)
    assert ev.last_bank_scoring.host_copy_floats == 3 * P and set(mean) == set(KEYS)
    cal = ScoreCalibration().fit_bank(ev, e2e["trial"], e2e["keys"], banks)
    assert cal.num_systems == 3 and cal.status == 1
    got = _check_device_against_host(ev, e2e["trial"], e2e["keys"], banks, e2e["gt"], cal, "three-member ensemble")
    # the fused llr is the oracle's map of the three members' own scores
    rows = np.stack([ev._metric_scores_device(b, _index(e2e)).cpu().numpy() for b in banks])
    ev.evaluate_bank_metrics(e2e["trial"], e2e["keys"], banks, metrics="device", calibration=cal)
    check_applied(ev.last_bank_scoring.device_scores.cpu().numpy(), rows, cal.weights)
    m, sd, X, pi = oracle_problem(rows, e2e["gt"], 0.05)
    assert CC.decrement(X, e2e["gt"], np.array(cal.fields["w"]), pi) <= CC.FIT_DECREMENT
    print(f"calibration-parity: fusion of 3 members over {P} trials: eer {got['eer']:.4f} against the members' mean "
          f"{mean['eer']:.4f}; 8 doubles cross, 0 floats (the host combination copies {3 * P})")
    with pytest.raises(ValueError, match="fitted on 3 system"):
        ev.evaluate_bank_metrics(e2e["trial"], e2e["keys"], banks[0], metrics="device", calibration=cal)


def _index(e2e):
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import TrialIndex
    return TrialIndex(e2e["trial"], e2e["keys"])


def test_evaluate_trials_with_a_calibration_on_a_module():
    from test_scoring_gpu import _module_case
    from w2v2_speaker_amd.evaluation.speaker import EvaluationPair, ScoreCalibration
    mod, inputs, kw = _module_case("wav2vec2")
    keys = sorted(inputs)
    idx = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    gt = [int((i + j) % 3 == 0 or j == i + 1) for i, j in idx]
    pairs = [EvaluationPair(bool(t), keys[i], keys[j]) for t, (i, j) in zip(gt, idx)]
    plain = mod.evaluate_trials(pairs, inputs, scoring="device", metrics="device", **kw)
    raw = mod.evaluator.last_bank_scoring.device_scores
    cal = ScoreCalibration(ridge=1e-2).fit_scores(raw, dev(np.asarray(gt, dtype=np.uint8)))     # 15 trials: keep it finite
    got = mod.evaluate_trials(pairs, inputs, scoring="device", metrics="device", calibration=cal, **kw)
    rec = mod.evaluator.last_bank_scoring
    assert rec.host_copy_floats == 0 and mod.evaluator.last_bank_metrics.host_copy_doubles == 8
    llr = rec.device_scores.cpu().numpy()
    check_applied(llr, raw.cpu().numpy()[None, :], cal.weights)
    host = mod.evaluate_trials(pairs, inputs, scoring="device", metrics="host", calibration=cal, **kw)
    check_metrics(got, gt, llr, host, "module")
    ref = CC.llr_metrics_ref(llr, gt)
    assert all(got[k] == ref[k] == host[k] for k in ("act_dcf", "act_p_miss", "act_p_fa"))
    assert abs(got["cllr"] - ref["cllr"]) <= CC.CLLR_REL * ref["cllr"]
    assert set(plain) == set(KEYS) and set(got) == set(KEYS) | set(LLR_KEYS)
    # the host scoring path: float64 numpy of the same definition
    cpu = mod.evaluate_trials(pairs, inputs, calibration=cal, **kw)
    assert set(cpu) == set(got) and abs(cpu["eer"] - got["eer"]) <= 1e-2 + 1.0 / 15


def test_the_defaults_launch_and_copy_what_they_did(e2e):
    """calibration=None, llr_metrics=False: no calibration entry is called, the records and the dicts are today's."""
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.evaluation.speaker import CosineDistanceEvaluator, PLDAEvaluator
    calls = []
    names = ("calib_fit", "calib_apply", "llr_metrics", "trial_metrics", "score_pairs", "plda_score_pairs")
    real = {n: getattr(ops, n) for n in names}
    for n in names:
        setattr(ops, n, (lambda n: lambda *a, **k: calls.append(n) or real[n](*a, **k))(n))
    try:
        ev = CosineDistanceEvaluator()
        bank = dev(e2e["test"])
        P = len(e2e["gt"])
        d = ev.evaluate_bank_metrics(e2e["trial"], e2e["keys"], bank, metrics="device")
        assert calls == ["score_pairs", "trial_metrics"] and set(d) == set(KEYS)
        assert ev.last_bank_scoring.host_copy_floats == 0 and ev.last_bank_metrics.host_copy_doubles == 8
        del calls[:]
        h = ev.evaluate_bank(e2e["trial"], e2e["keys"], bank)
        assert calls == ["score_pairs"] and ev.last_bank_scoring.host_copy_floats == P and set(h) == set(KEYS)
        del calls[:]
        ev.evaluate_bank(e2e["trial"], e2e["keys"], [bank, bank])
        assert calls == ["score_pairs"] * 2 and ev.last_bank_scoring.host_copy_floats == 2 * P
        pl = PLDAEvaluator(16, 16, 2, 0)
        pl.fit_parameters_bank(dev(e2e["train"]), e2e["labels"])
        del calls[:]
        d = pl.evaluate_bank_metrics(e2e["trial"], e2e["keys"], bank, metrics="device")
        assert calls == ["plda_score_pairs", "trial_metrics"] and set(d) == set(KEYS)
    finally:
        for n in names:
            setattr(ops, n, real[n])
