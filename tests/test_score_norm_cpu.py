"""CPU tests of the score normalisation: the host evaluator's ``score_norm`` path (plain torch f32) against the float64
references of tests/score_norm_cases.py within the bounds stated there, ``score_norm=None`` unchanged on the reference
evaluator's golden, mode / K validation, the C ABI of the new entries, the argument errors of ``ops`` that need no device,
and the forms ``ScoreNorm`` refuses.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import score_norm_cases as NC
import scoring_cases as SC
from test_metrics_cpu import _c_decl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float64_reference_counts_ties_as_a_multiset_and_poisons_nan_rows_only():
    S = np.array([[0.5, 0.5, 0.5, 0.1, -0.0], [0.0, -0.0, -1.0, np.nan, 2.0], [3.0, 1.0, 2.0, 0.0, -1.0]])
    mu, sd = NC.topk_stats_ref(S, 2)
    assert mu[0] == 0.5 and sd[0] == 0.0 and np.isnan(mu[1]) and np.isnan(sd[1])
    assert mu[2] == 2.5 and sd[2] == pytest.approx(np.sqrt(0.5))
    mu, sd = NC.topk_stats_ref(S[[0, 2]], 5)                 # K = M: the non-adaptive norm
    assert mu[0] == pytest.approx(S[0].mean()) and sd[1] == pytest.approx(S[2].std(ddof=1))


@pytest.mark.parametrize("centre,length_norm", NC.CENTRE_MODES)
@pytest.mark.parametrize("shape", NC.COHORT_SHAPES)
def test_host_cohort_statistics_against_float64(shape, centre, length_norm):
    c = NC.cohort_case(*shape, centre, length_norm)
    e_mu, e_sd = np.abs(c["host_mu"] - c["mu"]).max(), np.abs(c["host_sd"] - c["sd"]).max()
    print(f"score-norm-parity (cpu): host cohort_stats N,M,D,K={shape} centre={int(centre)} lnorm={int(length_norm)}: mu "
          f"{e_mu:.2e} sd {e_sd:.2e}; sd in [{c['sd'].min():.3f}, {c['sd'].max():.3f}]; a priori {c['apriori']:.2e}")
    assert e_mu <= c["bound_mu"] and e_sd <= c["bound_sd"]
    # a sanity bound that does not come from the host path itself: an f32 dot product of unit vectors is off by at most
    # D 2^-24, the two divisions by the norms and the stored result by a few 2^-24 more; mu averages such errors, and the
    # std of K values each off by d moves by at most 2 d sqrt(K / (K - 1)) <= 2.9 d
    d = (shape[2] + 8) * 2.0 ** -24
    assert e_mu <= d and e_sd <= 2.9 * d
    assert c["sd"].min() > 1e-3                                     # the data has spread: the scores are well-conditioned


@pytest.mark.parametrize("mode", NC.MODES)
def test_host_evaluator_score_norm_against_float64(mode):
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EmbeddingSample, EvaluationPair
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import ScoreNorm
    c = NC.g12_norm_case(mode)
    err = np.abs(c["host_score"] - c["score"])
    print(f"score-norm-parity (cpu): host evaluate(score_norm=) g12 mode={mode}: max err {err.max():.2e}, max err / bound "
          f"{(err / c['bound']).max():.2f}; scores in [{c['score'].min():.2f}, {c['score'].max():.2f}]")
    assert (err <= c["bound"]).all()
    assert c["score"].min() < 0 or c["score"].max() > 1            # unbounded: not a [0, 1] score
    # through the public entry: the same scores reach the metrics, unclipped
    keys = [f"u{i:02d}" for i in range(len(c["bank"]))]
    samples = [EmbeddingSample(k, torch.from_numpy(r)) for k, r in zip(keys, c["bank"])]
    pairs = [EvaluationPair(bool(g), keys[i], keys[j]) for g, (i, j) in zip(c["gt"], c["pairs"])]
    ev = CosineDistanceEvaluator()
    sn = ScoreNorm(torch.from_numpy(c["cohort"]), c["K"], mode)
    res = ev.evaluate(pairs, samples, score_norm=sn)
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import host_metrics
    assert res == host_metrics(c["gt"], c["host_score"].tolist())
    assert 0.0 <= res["eer"] <= 1.0


def test_score_norm_none_is_the_reference_evaluation_on_g12():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EmbeddingSample, EvaluationPair
    g = SC.g12()
    keys = [f"u{i:02d}" for i in range(32)]
    samples = [EmbeddingSample(k, torch.from_numpy(r)) for k, r in zip(keys, g["embedding"])]
    pairs = [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in g["trials"]]
    ev = CosineDistanceEvaluator()
    a, b = ev.evaluate(pairs, samples), ev.evaluate(pairs, samples, score_norm=None)
    assert a == b
    assert a["eer"] == pytest.approx(float(g["eer"]), abs=1e-12) and a["mdc"] == pytest.approx(float(g["mdc"]), abs=1e-12)
    for fn in (ev.evaluate, ev.evaluate_bank_metrics):
        assert inspect.signature(fn).parameters["score_norm"].default is None


def test_mode_and_top_k_validation():
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import cohort_stats_host, normalise_scores
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import ScoreNorm
    cohort = torch.zeros(5, 4)
    for bad in ("x", "S", None, 0):
        with pytest.raises(ValueError, match="mode"):
            ScoreNorm(cohort, 2, bad)
        with pytest.raises(ValueError, match="mode"):
            normalise_scores(torch.zeros(1), 0, 1, 0, 1, bad)
        with pytest.raises(ValueError, match="mode"):
            ops.score_pairs_norm(torch.zeros(1), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(2), torch.ones(2), bad)
    for bad in (1, 6, 0, -2, 2.0, True):
        with pytest.raises(ValueError, match="top_k"):
            ScoreNorm(cohort, bad)
        with pytest.raises(ValueError, match="top_k"):
            cohort_stats_host(torch.zeros(3, 4), cohort, bad)
        with pytest.raises(ValueError, match="K = "):
            ops.cohort_stats(torch.zeros(3, 4), cohort, bad)
        with pytest.raises(ValueError, match="K = "):
            ops.topk_stats(torch.zeros(3, 8), bad, 5)
    with pytest.raises(ValueError, match="cohort"):
        ScoreNorm(torch.zeros(4), 2)
    assert (ScoreNorm(cohort, 5).mode, ScoreNorm(cohort, 2, "z").top_k) == ("s", 2)


def test_new_symbols_declared_exported_and_wrapped_with_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32", C.c_double: "f64"}
    for name in ("w2v2_rows_transform", "w2v2_topk_stats", "w2v2_topk_stats_lds_keys", "w2v2_score_pairs_norm",
                 "w2v2_segment_mean"):
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        res, args = _lib._SIGS[name]
        assert (kind[res], [kind[a] for a in args]) == _c_decl(hdr, name), name
    assert _c_decl(hdr, "w2v2_topk_stats") == ("i32", ["p", "i64", "i32", "i32", "i32", "p", "p", "p"])
    assert "score_norm.hip" in _build.SOURCES
    lib = _lib.load()
    assert lib.w2v2_topk_stats_lds_keys() == ops.TOPK_LDS_KEYS and ops.TOPK_LDS_KEYS % 4 == 0
    assert list(inspect.signature(ops.cohort_stats).parameters) == ["bank", "cohort", "K", "mean", "std", "length_norm",
                                                                    "rows_per_block", "workspace"]
    for name in ("rows_transform", "topk_stats", "score_pairs_norm", "segment_mean"):
        assert callable(getattr(ops, name))
    # the default block keeps the [rows_per_block, ldS] f32 buffer at or below 256 MiB, and is never empty
    for N, M in ((145160, 5994), (7, 5), (10, 2 ** 24 - 1)):
        rpb = ops.cohort_rows_per_block(N, M)
        assert 1 <= rpb <= N and (rpb * ((M + 3) // 4 * 4) * 4 <= 256 << 20 or rpb == 1)
    assert ops.cohort_rows_per_block(145160, 5994) == (256 << 20) // (4 * 5996)


def test_ops_argument_checks_need_no_device():
    from w2v2_speaker_amd import ops
    bank, cohort = torch.zeros(6, 8), torch.zeros(5, 8)
    with pytest.raises(ValueError, match="D = 4, the bank D = 8"):
        ops.cohort_stats(bank, torch.zeros(5, 4), 2)
    with pytest.raises(ValueError, match="2-D float32"):
        ops.cohort_stats(bank.double(), cohort, 2)
    with pytest.raises(ValueError, match="2-D float32"):
        ops.cohort_stats(bank, cohort.double(), 2)
    with pytest.raises(ValueError, match="row stride"):
        ops.cohort_stats(torch.zeros(6, 16)[:, ::2], cohort, 2)
    with pytest.raises(ValueError, match="together"):
        ops.cohort_stats(bank, cohort, 2, mean=torch.zeros(8))
    with pytest.raises(ValueError, match="mean / std"):
        ops.cohort_stats(bank, cohort, 2, mean=torch.zeros(4), std=torch.ones(4))
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="rows_per_block"):
            ops.cohort_stats(bank, cohort, 2, rows_per_block=bad)
    with pytest.raises(ValueError, match=r"workspace holds rows_per_block \* ldS = 3 \* 8"):
        ops.cohort_stats(bank, cohort, 2, rows_per_block=3, workspace=torch.zeros(23))
    with pytest.raises(ValueError, match="workspace"):
        ops.cohort_stats(bank, cohort, 2, rows_per_block=3, workspace=torch.zeros(24, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cohort_stats(bank, cohort, 2)
    with pytest.raises(ValueError, match="M = 9"):
        ops.topk_stats(torch.zeros(2, 8), 2, 9)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.topk_stats(torch.zeros(2, 6), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_stats(torch.zeros(2, 8), 2, 5)
    with pytest.raises(ValueError, match="out is"):
        ops.rows_transform(bank, out=torch.zeros(6, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_transform(bank)
    pairs, v = torch.zeros(3, 2, dtype=torch.int32), torch.zeros(4)
    with pytest.raises(ValueError, match="pairs"):
        ops.score_pairs_norm(torch.zeros(3), pairs.long(), v, v)
    with pytest.raises(ValueError, match="cos is"):
        ops.score_pairs_norm(torch.zeros(2), pairs, v, v)
    with pytest.raises(ValueError, match="mu / sd"):
        ops.score_pairs_norm(torch.zeros(3), pairs, v, torch.zeros(5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_pairs_norm(torch.zeros(3), pairs, v, v)
    order, off = torch.arange(6, dtype=torch.int32), torch.tensor([0, 2, 6], dtype=torch.int32)
    with pytest.raises(ValueError, match="order"):
        ops.segment_mean(bank, order[:5], off)
    with pytest.raises(ValueError, match="offsets"):
        ops.segment_mean(bank, order, off.long())
    with pytest.raises(ValueError, match="out is"):
        ops.segment_mean(bank, order, off, out=torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segment_mean(bank, order, off)


def test_score_norm_refuses_an_ensemble_and_a_frame_bank():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EmbeddingSample, EvaluationPair
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import ScoreNorm, TrialIndex, score_trials_device
    from w2v2_speaker_amd.lightning_modules.speaker._optim_surface import EmbeddingEvaluation
    pairs, keys, bank = [EvaluationPair(True, "a", "b")], ["a", "b"], torch.zeros(2, 4)
    sn = ScoreNorm(torch.zeros(3, 4), 2)
    idx = TrialIndex(pairs, keys)
    with pytest.raises(NotImplementedError, match="score_norm takes one bank"):
        score_trials_device([bank, bank], idx, score_norm=sn)
    with pytest.raises(NotImplementedError, match="score_norm takes pooled embeddings"):
        score_trials_device(torch.zeros(5, 4), idx, frame_offsets=[0, 2, 5], score_norm=sn)
    ev = CosineDistanceEvaluator()
    with pytest.raises(NotImplementedError, match="score_norm takes one bank"):
        ev.evaluate_bank_metrics(pairs, keys, [bank, bank], score_norm=sn)
    with pytest.raises(NotImplementedError, match="score_norm takes pooled embeddings"):
        ev.evaluate_bank_metrics(pairs, keys, torch.zeros(5, 4), frame_offsets=[0, 2, 5], score_norm=sn)
    with pytest.raises(NotImplementedError, match="ensemble"):
        ev.evaluate(pairs, [EmbeddingSample(k, [torch.zeros(4), torch.zeros(4)]) for k in keys], score_norm=sn)
    with pytest.raises(NotImplementedError, match="pooled"):
        ev.evaluate(pairs, [EmbeddingSample(k, torch.zeros(3, 4)) for k in keys], score_norm=sn)
    assert inspect.signature(EmbeddingEvaluation.evaluate_trials).parameters["score_norm"].default is None
    assert inspect.signature(score_trials_device).parameters["score_norm"].default is None


def test_speaker_mean_cohort_groups_the_rows_on_the_host(monkeypatch):
    """The order / offsets tables speaker_mean_cohort hands the kernel: a stable grouping, speakers in sorted order."""
    from w2v2_speaker_amd.evaluation.speaker import device_scoring as DS
    seen = {}
    monkeypatch.setattr(DS.ops, "segment_mean", lambda bank, order, offsets: seen.update(order=order, offsets=offsets) or bank)
    labels = ["b", "a", "c", "a", "b", "a"]
    DS.speaker_mean_cohort(torch.zeros(6, 4), labels)
    assert seen["order"].tolist() == [1, 3, 5, 0, 4, 2] and seen["offsets"].tolist() == [0, 3, 5, 6]
    assert seen["order"].dtype == torch.int32 and seen["offsets"].dtype == torch.int32
    with pytest.raises(ValueError, match="one label per bank row"):
        DS.speaker_mean_cohort(torch.zeros(6, 4), labels[:5])
    x = np.arange(24, dtype=np.float32).reshape(6, 4)
    assert np.array_equal(NC.segment_mean_ref(x, labels), np.stack([x[[1, 3, 5]].mean(0), x[[0, 4]].mean(0), x[[2]].mean(0)]))
