"""CPU tests of the score calibration: the oracle of tests/calibration_cases.py against scipy's minimiser, the float64 numpy
path of ScoreCalibration against the oracle, the argument errors (raised before any launch), CalibrationError for the sets
that have no fit, and ``evaluate(..., calibration=)`` of the three evaluators against the oracle applied to their own
uncalibrated scores.  The kernels themselves: test_calibration_gpu.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import backend_cases as bc
import calibration_cases as CC
from conftest import ROOT

T = 2048
KEYS = ("eer", "eer_threshold", "mdc", "mdc_threshold")
LLR_KEYS = ("cllr", "act_dcf", "act_p_miss", "act_p_fa")


def _problem(name, P, K, p_target):
    S, y = CC.family(name, P, K, 1)
    m, sd = CC.moments(S)
    return S, y, m, sd, CC.features(S, m, 1.0 / sd), CC.effective_prior(p_target)


def test_cases_module_states_its_tile_and_fitted_cases_are_not_separable():
    from w2v2_speaker_amd import ops
    assert ops.CALIB_TILE == T and ops.lib().w2v2_calib_tile() == T
    assert len(CC.fitted_cases(T)) >= 12                    # (the non-separability assertions run in fitted_cases)
    S, y = CC.separable_set()
    m, sd = CC.moments(S)
    assert CC.separable(CC.features(S, m, 1.0 / sd), y)
    assert {K for _, _, K, _, _ in CC.fitted_cases(T)} == set(CC.SYSTEMS)
    assert {p for _, _, _, p, _ in CC.fitted_cases(T)} == set(CC.PRIORS)
    assert {P for _, P, _, _, _ in CC.stat_cases(T)} == set(CC.sizes(T))


@pytest.mark.parametrize("case", CC.fitted_cases(T), ids=lambda c: f"{c[0]}-P{c[1]}-K{c[2]}-p{c[3]}")
def test_oracle_newton_against_scipy_minimize(case):
    """By objective value and by the decrement at the returned point, not by weights."""
    from scipy.optimize import minimize
    name, P, K, p_target, _ = case
    S, y, m, sd, X, pi = _problem(name, P, K, p_target)
    w, J, evals = CC.newton(X, y, pi)
    assert evals <= 32 and CC.decrement(X, y, w, pi) < 1e-12
    res = minimize(lambda v: CC.stats_fast(X, y, v, pi)[0], np.zeros(K + 1), jac=lambda v: CC.stats_fast(X, y, v, pi)[1],
                   method="BFGS", options={"gtol": 1e-10, "maxiter": 2000})
    # Newton stopped at a decrement below 1e-12, which is its distance from the minimum in J; scipy's point is optimal to
    # its own gradient tolerance: neither objective is more than that (plus the rounding of a sum of P terms) below the other
    assert J <= res.fun + 2e-12
    assert res.fun - J <= 1e-10 and CC.decrement(X, y, res.x, pi) <= 1e-8
    # the element-by-element statistics and the matrix-product form are one function
    Je, ge, He = CC.stats(X, y, w, pi)
    Jf, gf, Hf = CC.stats_fast(X, y, w, pi)
    assert abs(Je - Jf) <= 1e-13 and np.abs(He - Hf).max() <= 1e-13 and np.abs(ge - gf).max() <= 1e-13


@pytest.mark.parametrize("case", CC.fitted_cases(T), ids=lambda c: f"{c[0]}-P{c[1]}-K{c[2]}-p{c[3]}")
def test_numpy_path_of_score_calibration_against_the_oracle(case):
    from w2v2_speaker_amd.evaluation.speaker.calibration import ScoreCalibration
    name, P, K, p_target, _ = case
    S, y, m, sd, X, pi = _problem(name, P, K, p_target)
    cal = ScoreCalibration(p_target=p_target).fit_scores(S, y)
    f = cal.fields
    assert cal.status == 1 and 1 <= f["rounds"] <= 32 and cal.num_systems == K
    assert CC.decrement(X, y, np.array(f["w"]), pi) <= CC.FIT_DECREMENT
    assert np.abs(np.array(f["mean"]) - m).max() <= 1e-12 * np.abs(S).mean() + 1e-300
    assert np.abs(np.array(f["sd"]) / sd - 1).max() <= 1e-12
    a = CC.affine(np.array(f["w"]), np.array(f["mean"]), np.array(f["r"]))
    scale = abs(f["w"][0]) + np.abs(a[1:] * np.array(f["mean"])).sum()
    assert abs(cal.weights[0] - a[0]) <= 1e-11 * scale and np.abs(cal.weights[1:] / a[1:] - 1).max() <= 1e-12
    # apply: float64 on the host, the oracle's order of operations
    _, v, _ = CC.apply_ref(S, cal.weights)
    assert np.array_equal(cal.apply(S), v) and np.array_equal(cal.apply(torch.from_numpy(S)), v)
    if K == 1:
        assert np.array_equal(cal.apply(S[0]), v)
    # a torch CPU tensor takes the same path
    again = ScoreCalibration(p_target=p_target).fit_scores(torch.from_numpy(S), torch.from_numpy(y))
    assert np.array_equal(again.weights, cal.weights)


def test_llr_metrics_numpy_against_the_oracle():
    from w2v2_speaker_amd.evaluation.speaker.calibration import llr_metrics_numpy
    for name, (z, y, p_target) in CC.llr_cases(T).items():
        got, want = llr_metrics_numpy(z, y, p_target=p_target), CC.llr_metrics_ref(z, y, p_target=p_target)
        for k in ("act_dcf", "act_p_miss", "act_p_fa", "n_pos", "n_nan"):
            assert got[k] == want[k], (name, k)
        for k in ("cllr", "cllr_tar", "cllr_non"):
            assert got[k] == want[k] or abs(got[k] - want[k]) <= CC.CLLR_REL * abs(want[k]), (name, k)
    z, y, _ = CC.llr_cases(T)["inf_costly"]
    assert llr_metrics_numpy(z, y)["cllr"] == np.inf
    assert llr_metrics_numpy(np.zeros(4), [1, 0, 1, 0], p_target=0.5)["cllr"] == pytest.approx(1.0, abs=1e-15)


def test_calibration_error_for_sets_without_a_fit():
    from w2v2_speaker_amd.evaluation.speaker import CalibrationError, ScoreCalibration
    S, y = CC.separable_set()
    with pytest.raises(CalibrationError, match="ridge") as e:
        ScoreCalibration().fit_scores(S, y)
    assert e.value.status == 0 and e.value.fields["rounds"] == 32 and isinstance(e.value, ValueError)
    ok = ScoreCalibration(ridge=1e-3).fit_scores(S, y)       # the penalty gives a separable set a finite optimum
    assert ok.status == 1 and np.all(np.isfinite(ok.weights)) and ok.weights[1] > 0
    S, y = CC.constant_system()
    with pytest.raises(CalibrationError, match=r"system\(s\) \[1\] have a constant") as e:
        ScoreCalibration().fit_scores(S, y)
    assert e.value.status == 2
    S, y = CC.one_class()
    with pytest.raises(CalibrationError, match="one class is absent") as e:
        ScoreCalibration().fit_scores(S, y)
    assert e.value.status == 2
    S, y = CC.family("gauss1.0", 100, 1, 2)
    S[0, 5] = np.nan
    with pytest.raises(CalibrationError, match="1 trial.s. with a NaN score"):
        ScoreCalibration().fit_scores(S, y)
    with pytest.raises(ValueError, match="has not been called"):
        ScoreCalibration().weights


def test_argument_errors_need_no_device():
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.evaluation.speaker import ScoreCalibration
    s, l = torch.zeros(2, 8), torch.zeros(8, dtype=torch.uint8)
    for kw, msg in ((dict(c_miss=0.5), "c_miss=0.5 should be >= 1"), (dict(c_fa=0), "c_fa=0 should be >= 1"),
                    (dict(p_target=1.5), "p_target=1.5 should be between 0 and 1"),
                    (dict(p_target=0), "strictly between 0 and 1"), (dict(p_target=1), "strictly between 0 and 1")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            ops.calib_fit(s, l, **kw)
        with pytest.raises(ValueError, match=re.escape(msg)):
            ScoreCalibration(**kw)
        if "strictly" not in msg:
            with pytest.raises(ValueError, match=re.escape(msg)):
                ops.llr_metrics(s[0], l, **kw)
    for bad_s, bad_l in ((s.double(), l), (s, l.int()), (s[:, :0], l[:0]), (s, l[:3]), (torch.zeros(9, 8), l),
                         (torch.zeros(2, 16)[:, ::2], l), (torch.zeros(2, 2, 2), l)):
        with pytest.raises(ValueError, match="calib_fit"):
            ops.calib_fit(bad_s, bad_l)
    for kw in (dict(ridge=-1.0), dict(ridge=float("inf")), dict(ridge=float("nan")), dict(max_iter=0), dict(max_iter=2.5),
               dict(w_start=[0.0, 1.0]), dict(w_start=[0.0, 1.0, float("nan")]), dict(record=torch.zeros(168)),
               dict(record=torch.zeros(100, dtype=torch.float64))):
        with pytest.raises(ValueError, match="calib_fit"):
            ops.calib_fit(s, l, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.calib_fit(s, l)
    rec = torch.zeros(ops.CALIB_RECORD_DOUBLES, dtype=torch.float64)
    for bad in (dict(scores=s.double(), record=rec), dict(scores=s, record=rec.float()), dict(scores=s, record=rec[:5]),
                dict(scores=s, record=rec, out=torch.zeros(4)), dict(scores=torch.zeros(9, 8), record=rec)):
        with pytest.raises(ValueError, match="calib_apply"):
            ops.calib_apply(**bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.calib_apply(s, rec)
    for bad_s, bad_l in ((s[0].double(), l), (s[0], l.int()), (s[0][:0], l[:0]), (s[0], l[:3]), (s, l)):
        with pytest.raises(ValueError, match="llr_metrics"):
            ops.llr_metrics(bad_s, bad_l)
    with pytest.raises(ValueError, match="out is"):
        ops.llr_metrics(s[0], l, out=torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.llr_metrics(s[0], l)
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="outside"):
            ops.calib_workspace(bad, "cpu")
    for kw in (dict(max_iter=0), dict(ridge=-1)):
        with pytest.raises(ValueError):
            ScoreCalibration(**kw)
    with pytest.raises(ValueError, match="systems"):
        ScoreCalibration().fit_scores(np.zeros((9, 8)), np.zeros(8))
    with pytest.raises(ValueError, match="one label per trial"):
        ScoreCalibration().fit_scores(np.zeros((2, 8)), np.zeros(7))


def _c_decl(hdr, name):
    m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    kinds = []
    for p in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(","):
        p = " ".join(p.replace("const", "").split())
        if p == "void":
            continue
        kinds.append("p" if "*" in p else {"int64_t": "i64", "int": "i32", "float": "f32", "double": "f64"}[p.split(" ")[0]])
    return {"int": "i32", "int64_t": "i64"}[m.group(1)], kinds


def test_new_symbols_declared_exported_and_wrapped_with_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32", C.c_double: "f64"}
    for name in ("w2v2_calib_tile", "w2v2_calib_record_doubles", "w2v2_calib_workspace_bytes", "w2v2_calib_fit",
                 "w2v2_calib_apply", "w2v2_llr_metrics"):
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        res, args = _lib._SIGS[name]
        assert (kind[res], [kind[a] for a in args]) == _c_decl(hdr, name), name
    assert "calibration.hip" in _build.SOURCES and "-ffp-contract=off" in _build.EXTRA_FLAGS["calibration.hip"]
    assert "#define W2V2_CALIB_MAX_SYSTEMS 8" in hdr and ops.CALIB_MAX_SYSTEMS == 8
    lib = _lib.load()
    assert lib.w2v2_calib_record_doubles() == ops.CALIB_RECORD_DOUBLES
    at, n = ops.CALIB_RECORD["H"]
    assert at + n <= ops.CALIB_RECORD_DOUBLES and ops.CALIB_RECORD["a"][0] == 16 + 3 * 9 + 3 * 8
    wb = lib.w2v2_calib_workspace_bytes
    assert wb(1) == wb(T) > 0 and wb(T + 1) == 2 * wb(T) and wb(T) % 16 == 0
    assert wb(T) >= 8 * (1 + 9 + 45)                        # one row holds J, g and the upper triangle of H at K = 8
    for bad in (0, -1, 2 ** 31):
        assert wb(bad) == -1
    assert ops.calib_workspace(5000, "cpu").numel() == wb(5000) and ops.llr_metrics_workspace is ops.calib_workspace
    assert list(inspect.signature(ops.calib_fit).parameters) == ["scores", "labels", "c_miss", "c_fa", "p_target", "ridge",
                                                                 "max_iter", "w_start", "record", "workspace"]
    assert list(inspect.signature(ops.llr_metrics).parameters) == ["llr", "labels", "c_miss", "c_fa", "p_target", "out",
                                                                   "workspace"]
    assert ops.LLR_METRICS_FIELDS == ("cllr", "cllr_tar", "cllr_non", "act_dcf", "act_p_miss", "act_p_fa", "n_pos", "n_nan")
    f = ops.calib_record_fields([float(i) for i in range(2)] + [3.0] + [float(i) for i in range(3, 168)])
    assert f["K"] == 3 and len(f["w"]) == 4 and len(f["mean"]) == 3 and len(f["H"]) == 4 and f["H"][1][0] == float(at + 9)


# ------------------------------------------------------------------------------------------------ the evaluators' host path
def apply64(rows, a):
    """a_0 + sum_k a_k s_k over float64 rows [K, P], k ascending (the oracle's order, on host scores)."""
    v = np.full(rows.shape[1], float(a[0]))
    for k in range(rows.shape[0]):
        v = v + float(a[k + 1]) * rows[k]
    return v


def _expected(scores64, gt, cal):
    """The dict ``evaluate(..., calibration=cal)`` must return for the evaluator's own uncalibrated ``scores64``: the host
    metrics of the oracle's llrs under cal's map, and the oracle's llr metrics of them."""
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import host_metrics
    llr = apply64(np.asarray(scores64, dtype=np.float64)[None, :], cal.weights)
    want = host_metrics(list(gt), llr.tolist())
    m = CC.llr_metrics_ref(llr, gt, cal.c_miss, cal.c_fa, cal.p_target, f32=False)
    want.update({k: m[k] for k in LLR_KEYS})
    return want, llr


def _check_evaluator(ev, pairs, samples, gt, scores64, p_target):
    from w2v2_speaker_amd.evaluation.speaker import ScoreCalibration
    plain = ev.evaluate(pairs, samples)
    assert set(plain) == set(KEYS)                          # the defaults: today's dict
    cal = ScoreCalibration(p_target=p_target).fit_scores(scores64, gt)
    m, sd = CC.moments(scores64[None, :])
    X = CC.features(scores64[None, :], m, 1.0 / sd)
    assert CC.decrement(X, gt, np.array(cal.fields["w"]), CC.effective_prior(p_target)) <= CC.FIT_DECREMENT
    got = ev.evaluate(pairs, samples, calibration=cal)
    want, llr = _expected(scores64, gt, cal)
    assert set(got) == set(KEYS) | set(LLR_KEYS)
    for k in KEYS + LLR_KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert cal.weights[1] > 0 and abs(got["eer"] - plain["eer"]) <= 5e-12      # a positive slope keeps the order
    raw = ev.evaluate(pairs, samples, llr_metrics=True)     # the raw scores as llrs, at the default operating point
    rm = CC.llr_metrics_ref(scores64, gt, f32=False)
    assert {k: raw[k] for k in KEYS} == plain and all(raw[k] == rm[k] for k in LLR_KEYS)
    return got, raw


@pytest.fixture(scope="module")
def e2e():
    from w2v2_speaker_amd.evaluation.speaker import EmbeddingSample, EvaluationPair
    train, labels, test, _, pairs, gt = bc.two_covariance_set(0, **bc.E2E)
    keys = [f"u{r}" for r in range(len(test))]
    trial = [EvaluationPair(bool(g), keys[i], keys[j]) for (i, j), g in zip(pairs.tolist(), gt)]
    samples = [EmbeddingSample(k, torch.from_numpy(test[r])) for r, k in enumerate(keys)]
    return dict(train=train, labels=labels, test=test, pairs=pairs, gt=np.asarray(gt, dtype=np.uint8), trial=trial, samples=samples)


def test_cosine_evaluate_with_a_calibration(e2e):
    from w2v2_speaker_amd.evaluation.speaker import CosineDistanceEvaluator
    ev = CosineDistanceEvaluator()
    t = torch.from_numpy(e2e["test"])
    i, j = e2e["pairs"][:, 0], e2e["pairs"][:, 1]
    cos = np.array(torch.nn.functional.cosine_similarity(t[i], t[j], dim=1, eps=1e-8).numpy().tolist())
    scores = np.clip((cos + 1) / 2, 0, 1)
    _check_evaluator(ev, e2e["trial"], e2e["samples"], e2e["gt"], scores, 0.05)


@pytest.mark.parametrize("kind", ("lda", "plda"))
def test_latent_evaluators_evaluate_with_a_calibration(e2e, kind):
    from w2v2_speaker_amd.evaluation.speaker import LDAEvaluator, PLDAEvaluator
    ev = LDAEvaluator(True, True, 0, 16, False, projection="lda") if kind == "lda" else PLDAEvaluator(16, 16, 5, 0)
    ev.fit_parameters([torch.from_numpy(e2e["train"])], [torch.tensor(e2e["labels"])])
    pairs = torch.from_numpy(e2e["pairs"].astype(np.int64))
    with torch.no_grad():
        s = ev._host_scores(ev._host_latent(torch.from_numpy(e2e["test"])), pairs[:, 0], pairs[:, 1], None)
    scores = s.numpy().astype(np.float64)
    if kind == "lda":
        scores = np.clip((scores + 1) / 2, 0, 1)
    got, raw = _check_evaluator(ev, e2e["trial"], e2e["samples"], e2e["gt"], scores, 0.05 if kind == "plda" else 0.5)
    if kind == "plda":                                      # the PLDA llr is what llr_metrics=True is for
        print(f"calibration-parity: plda host path raw cllr {raw['cllr']:.4f} act_dcf {raw['act_dcf']:.4f} -> calibrated "
              f"cllr {got['cllr']:.4f} act_dcf {got['act_dcf']:.4f}")


def test_cosine_host_ensemble_fused_with_a_three_system_calibration(e2e):
    from w2v2_speaker_amd.evaluation.speaker import CosineDistanceEvaluator, EmbeddingSample, ScoreCalibration
    ev = CosineDistanceEvaluator()
    test = e2e["test"]
    rng = np.random.default_rng(11)
    members = [test, (test + 0.8 * rng.standard_normal(test.shape)).astype(np.float32), test[:, ::-1].copy() * 0.5 +
               (0.6 * rng.standard_normal(test.shape)).astype(np.float32)]
    i, j = e2e["pairs"][:, 0], e2e["pairs"][:, 1]
    rows = []
    for mem in members:
        t = torch.from_numpy(np.ascontiguousarray(mem))
        cos = np.array(torch.nn.functional.cosine_similarity(t[i], t[j], dim=1, eps=1e-8).numpy().tolist())
        rows.append(np.clip((cos + 1) / 2, 0, 1))
    rows = np.array(rows)
    cal = ScoreCalibration().fit_scores(rows, e2e["gt"])
    samples = [EmbeddingSample(s.sample_id, [torch.from_numpy(np.ascontiguousarray(mem[r])) for mem in members])
               for r, s in enumerate(e2e["samples"])]
    got = ev.evaluate(e2e["trial"], samples, calibration=cal)
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import host_metrics
    llr = apply64(rows, cal.weights)
    want = host_metrics(e2e["gt"].tolist(), llr.tolist())
    want.update({k: v for k, v in CC.llr_metrics_ref(llr, e2e["gt"], f32=False).items() if k in LLR_KEYS})
    assert got == want
    with pytest.raises(ValueError, match="fitted on 3 systems"):
        ev.evaluate(e2e["trial"], e2e["samples"], calibration=cal)
    plain = ev.evaluate(e2e["trial"], samples)              # the reference's mean of the members, unchanged
    assert set(plain) == set(KEYS)
