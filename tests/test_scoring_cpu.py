"""Host side of the device trial scoring (no GPU needed): the three C-ABI symbols, the float64 references of
tests/scoring_cases.py against what the REFERENCE evaluator produced (tests/golden/g12_eer.npz), the identity the
frame-set kernel rests on, the frame draws, and the argument checks of the wrappers."""
import ctypes as C
import inspect
import os
import random
import warnings

import numpy as np
import pytest
import torch

import scoring_cases as SC
from test_fbank_cpu import _c_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("w2v2_embed_stats", "w2v2_score_pairs", "w2v2_score_frame_sets")


def test_symbols_declared_listed_with_the_headers_parameter_kinds_and_exported():
    from w2v2_speaker_amd import _build, _lib, ops
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32"}
    assert "score.hip" in _build.SOURCES
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib._SIGS and name in _lib.EXPORTS
        res, args = _lib._SIGS[name]
        assert res is C.c_int32 and [kind[a] for a in args] == _c_params(hdr, name), name
        assert hasattr(lib, name)
    for fn in ("embed_stats", "score_pairs", "score_frame_sets"):
        assert callable(getattr(ops, fn))


def test_float64_references_reproduce_the_reference_evaluators_scores():
    """scores, scores_c, scores_cl, scores_l of g12 are the reference's f32 results: each lies within the host-f32 bound of
    the float64 restatement (the bound is 2 x the error of this machine's host path, itself such an f32 result)."""
    g = SC.g12()
    for tag in SC.G12_BRANCHES:
        c = SC.g12_case(tag)
        err = float(np.abs(c["score"] - g[f"scores{tag}"]).max())
        print(f"scoring-parity: g12 scores{tag} float64 reference vs golden {err:.2e} bound {c['bound_score']:.2e}")
        assert err <= c["bound_score"], tag


def test_float64_statistics_reproduce_the_reference_evaluators_fit():
    g = SC.g12()
    mean, std = SC.stats_ref(g["embedding"])
    hm, hs = SC.host_stats(g["embedding"])
    bm, bs = (SC.bound(e) for e in SC.stats_err(hm, hs, mean, std))
    em, es = SC.stats_err(g["fit_mean"], g["fit_std"], mean, std)
    print(f"scoring-parity: g12 fit_mean {em:.2e} bound {bm:.2e}; fit_std {es:.2e} bound {bs:.2e}")
    assert em <= bm and es <= bs


def _g12_frame_trials():
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import TrialIndex
    frames, offsets, trials = SC.g12_frames()
    return frames, offsets, trials, TrialIndex.from_rows(trials[:, 1:], trials[:, 0], 6)


def test_float64_frame_set_reference_reproduces_the_reference_evaluator_under_its_seed():
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import draw_frame_sets
    g = SC.g12()
    frames, offsets, _, index = _g12_frame_trials()
    random.seed(int(g["nonpooled_seed"]))
    sel, counts = draw_frame_sets(np.diff(offsets), index)
    assert sel.shape == (15, 2, 50) and counts.max() == 50 and counts.min() == 10
    cos, _ = SC.frame_sets_ref(frames, sel, counts)
    hcos, _ = SC.host_frame_sets(frames, sel, counts)
    b = SC.bound(np.abs(hcos - cos).max())
    err = float(np.abs(cos - g["nonpooled_scores"]).max())
    print(f"scoring-parity: g12 nonpooled float64 reference vs golden {err:.2e} bound {b:.2e}")
    assert err <= b


def test_separated_form_equals_the_evaluators_pairwise_mean_in_float64():
    """The tripwire for torch's clamp: with an all-zero row and a row of norm 1e-10 the identity holds only while
    cosine_similarity clamps each norm on its own."""
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import compute_non_pooled_cosine_scores
    frames, sel, counts = SC.clamp_case()
    x = torch.from_numpy(frames).double()
    pairwise = compute_non_pooled_cosine_scores(x[:7], x[7:12])      # (its draw is a permutation here: 7 and 5 < 50)
    separated = SC.frame_sets_separated_ref(frames, sel, counts)[0]
    assert abs(pairwise - separated) < 1e-12
    assert abs(SC.frame_sets_ref(frames, sel, counts)[0][0] - separated) < 1e-12
    for D in SC.FRAME_DIMS:
        c = SC.frames_case(D)
        assert np.abs(SC.frame_sets_separated_ref(c["frames"], c["sel"], c["counts"]) - c["cos"]).max() < 1e-12


def test_draw_frame_sets_consumes_random_exactly_as_the_host_evaluator():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EmbeddingSample
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import draw_frame_sets
    g = SC.g12()
    _, offsets, trials, index = _g12_frame_trials()
    smp = [EmbeddingSample(f"np{i}", torch.from_numpy(g[f"nonpooled_emb{i}"])) for i in range(6)]
    random.seed(99)
    CosineDistanceEvaluator()._compute_prediction_scores([(smp[i], smp[j]) for _, i, j in trials])
    after_host = random.getstate()
    random.seed(99)
    sel, counts = draw_frame_sets(np.diff(offsets), index)
    assert random.getstate() == after_host
    random.seed(99)                              # the same indices: left side first, then the right side
    for t, (_, i, j) in enumerate(trials):
        for side, u in ((0, i), (1, j)):
            p = int(offsets[u + 1] - offsets[u])
            want = random.sample(range(p), min(50, p))
            assert counts[t, side] == len(want)
            assert (sel[t, side, :len(want)] - offsets[u]).tolist() == want


def test_wrappers_reject_bad_arguments():
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import TrialIndex
    bank, pairs = torch.zeros(4, 8), torch.zeros(3, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_pairs(bank, pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.embed_stats(bank)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_frame_sets(bank, torch.zeros(1, 2, 5, dtype=torch.int32), torch.ones(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.score_pairs(torch.zeros(4, 6), pairs)
    with pytest.raises(ValueError, match="row stride"):
        ops.score_pairs(torch.zeros(4, 10)[:, :8], pairs)                    # ld = 10: not a multiple of 4
    with pytest.raises(ValueError, match="row stride"):
        ops.embed_stats(torch.zeros(8, 4).t())                               # features not contiguous
    with pytest.raises(ValueError, match="together"):
        ops.score_pairs(bank, pairs, mean=torch.zeros(8))
    with pytest.raises(ValueError, match="N >= 2"):
        ops.embed_stats(torch.zeros(1, 8))
    with pytest.raises(ValueError, match="int32"):
        ops.score_pairs(bank, pairs.long())
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        TrialIndex.from_rows([(0, 1), (2, 4)], [1, 0], 4)
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        TrialIndex.from_rows([(-1, 1)], [1], 4)


def test_evaluate_bank_answers_a_missing_key_and_unfitted_centring_like_evaluate():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EvaluationPair
    assert list(inspect.signature(CosineDistanceEvaluator.evaluate_bank).parameters) == ["self", "pairs", "keys", "bank",
                                                                                        "frame_offsets"]
    bank = torch.zeros(2, 4)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = CosineDistanceEvaluator().evaluate_bank([EvaluationPair(True, "a", "zz")], ["a", "b"], bank)
    assert res == {"eer": -1, "eer_threshold": -1, "mdc": -1, "mdc_threshold": -1}
    assert any("a or zz not in sample_map" in str(m.message) for m in w)
    with pytest.raises(TypeError, match=r"fit_parameters\(\) has not been called"):
        CosineDistanceEvaluator(True, False, 0).evaluate_bank([EvaluationPair(True, "a", "b")], ["a", "b"], bank)
    with pytest.raises(ValueError, match="duplicate key"):
        CosineDistanceEvaluator().evaluate_bank([EvaluationPair(True, "a", "a")], ["a", "a"], bank)
    with pytest.raises(ValueError, match="more than 2 samples"):
        CosineDistanceEvaluator(True, False, 0).fit_parameters_bank(bank)
    assert CosineDistanceEvaluator().fit_parameters_bank(bank) is None       # no centring: nothing to fit


def test_the_separated_set_keeps_its_classes_apart_by_four_bounds_and_still_overlaps():
    s = SC.separated_set()                       # (asserts both itself)
    assert len(s["gt"]) == 496 and sum(s["gt"]) == 48 and s["bound_score"] >= SC.FLOOR


def test_evaluate_trials_takes_the_scoring_keyword_and_defaults_to_the_host():
    from w2v2_speaker_amd.lightning_modules.speaker._optim_surface import EmbeddingEvaluation
    p = inspect.signature(EmbeddingEvaluation.evaluate_trials).parameters["scoring"]
    assert p.default == "host" and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_evaluate_trials_device_scoring_refuses_a_no_pooling_head():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    from w2v2_speaker_amd.lightning_modules.speaker._optim_surface import EmbeddingEvaluation

    class NoPoolingStub(EmbeddingEvaluation):
        def compute_speaker_embeddings(self, inputs):
            return [torch.zeros(1, 7, 8) for _ in inputs]           # [1, frames, features]

    pairs = [EvaluationPair(True, "a", "b")]
    with pytest.raises(NotImplementedError, match=r"evaluate_bank\(frame_offsets=\)"):
        NoPoolingStub().evaluate_trials(pairs, {"a": None, "b": None}, scoring="device")
    with pytest.raises(ValueError, match="scoring"):
        NoPoolingStub().evaluate_trials(pairs, {"a": None, "b": None}, scoring="gpu")
