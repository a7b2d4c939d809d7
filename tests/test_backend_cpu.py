"""LDA / PLDA scoring back-ends on the host: the closed forms of the definition against direct evaluation, the solvers of
evaluation/speaker/backend.py against their defining properties, the host evaluators against the float64 oracle of
tests/backend_cases.py, and the argument errors.  No GPU."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

import backend_cases as bc
from w2v2_speaker_amd import _lib
from w2v2_speaker_amd.evaluation.speaker import (CosineDistanceEvaluator, EmbeddingSample, EvaluationPair, LDAEvaluator,
                                                 PLDAEvaluator, backend)
from w2v2_speaker_amd.evaluation.speaker.device_scoring import ScoreNorm
from w2v2_speaker_amd.eval_metrics import calculate_eer, calculate_mdc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("w2v2_rows_center", "w2v2_scatter_fold", "w2v2_plda_score_pairs")


def small_set(seed=0, C=40, R=5):
    """40 classes of 3 .. 6 rows in R dimensions, as the latent rows of a PLDA fit."""
    rng = np.random.default_rng(seed)
    labels = [c for c in range(C) for _ in range(3 + c % 4)]
    ids, _ = bc.ids_of(labels)
    Z = rng.standard_normal((C, R))[ids] * np.linspace(1.5, 0.2, R) + rng.standard_normal((len(ids), R)) * np.linspace(0.4, 1.0, R)
    return Z, ids, C


@pytest.fixture(scope="module")
def e2e():
    return bc.two_covariance_set(0, **bc.E2E)


def test_closed_form_llr_equals_direct_gaussian_ratio():
    Z, ids, C = small_set()
    counts, means, mu, Sw, _ = bc.class_statistics(Z, ids, C)
    B, W = bc.plda_em(counts, means, mu, Sw, 3)
    A, psi = bc.diagonalise(B, W)
    p, q, k = bc.coefficients(psi)
    rng = np.random.default_rng(1)
    for _ in range(20):
        z1, z2 = rng.standard_normal(len(mu)) * 2, rng.standard_normal(len(mu)) * 2
        closed, _ = bc.llr_closed_form((A @ (z1 - mu))[None], (A @ (z2 - mu))[None], p, q, k)
        assert abs(closed[0] - bc.llr_direct(z1, z2, mu, B, W)) <= 1e-10
    # the product code's diagonalisation and coefficients give the same number
    At, psit = backend.plda_diagonalise(torch.from_numpy(B), torch.from_numpy(W))
    pt, qt, kt = backend.plda_coefficients(psit)
    closed, _ = bc.llr_closed_form((At.numpy() @ (z1 - mu))[None], (At.numpy() @ (z2 - mu))[None], pt.numpy(), qt.numpy(), kt)
    assert abs(closed[0] - bc.llr_direct(z1, z2, mu, B, W)) <= 1e-10


def test_em_never_lowers_the_exact_log_likelihood():
    Z, ids, C = small_set(2)
    counts, means, mu, Sw, _ = bc.class_statistics(Z, ids, C)
    ll = []
    for it in range(11):                                    # the product EM, stopped after 0 .. 10 steps
        B, W = backend.plda_em(counts, means, mu, Sw, it)
        ll.append(bc.log_likelihood(Z, ids, C, mu, B.numpy(), W.numpy()))
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(ll, ll[1:])), ll
    assert ll[-1] > ll[0]
    trace = []
    bc.plda_em(counts, means, mu, Sw, 10, trace)            # ... and it is the oracle's EM, class by class
    np.testing.assert_allclose(B.numpy(), trace[-1][0], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(W.numpy(), trace[-1][1], rtol=1e-9, atol=1e-12)


def test_diagonalisation():
    Z, ids, C = small_set(3, R=7)
    counts, means, mu, Sw, _ = bc.class_statistics(Z, ids, C)
    B, W = backend.plda_em(counts, means, mu, Sw, 2)
    A, psi = backend.plda_diagonalise(B, W)
    np.testing.assert_allclose((A @ W @ A.T).numpy(), np.eye(7), atol=1e-10)
    np.testing.assert_allclose((A @ B @ A.T).numpy(), np.diag(psi.numpy()), atol=1e-10)
    assert bool((psi[:-1] >= psi[1:]).all())
    A3, psi3 = backend.plda_diagonalise(B, W, 3)
    assert A3.shape == (3, 7) and torch.equal(A3, A[:3]) and torch.equal(psi3, psi[:3])


def test_projections_whiten(e2e):
    train, labels = e2e[0], e2e[1]
    ids, C = backend.label_ids(labels)
    stats = backend.class_statistics_host(train, ids, C)
    N = len(train)
    X = torch.from_numpy(train).double()
    P = backend.pca_projection(stats.Sw + stats.Sb, N, 16)
    Y = (X - stats.mu0) @ P.T
    np.testing.assert_allclose(np.cov(Y.numpy().T), np.eye(16), atol=1e-9)
    L = backend.lda_projection(stats.Sw, stats.Sb, N, C, 16)
    np.testing.assert_allclose((L @ stats.Sw @ L.T / (N - C)).numpy(), np.eye(16), atol=1e-9)
    ocounts, omeans, omu0, oSw, oSb = bc.class_statistics(train, ids, C)
    np.testing.assert_allclose(stats.Sw.numpy(), oSw, rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(stats.Sb.numpy(), oSb, rtol=1e-10, atol=1e-9)


def _samples_and_pairs(e2e):
    test, pairs, gt = e2e[2], e2e[4], e2e[5]
    samples = [EmbeddingSample(f"u{r}", torch.from_numpy(test[r])) for r in range(len(test))]
    trial = [EvaluationPair(bool(g), f"u{i}", f"u{j}") for (i, j), g in zip(pairs.tolist(), gt)]
    return samples, trial


def _host_scores(ev, e2e):
    """The evaluator's own scores: what ``evaluate`` feeds the metrics, before any clip."""
    test, pairs = e2e[2], e2e[4]
    with torch.no_grad():
        lat = ev._host_latent(torch.from_numpy(test))
        return ev._host_scores(lat, torch.from_numpy(pairs[:, 0].astype(np.int64)), torch.from_numpy(pairs[:, 1].astype(np.int64)),
                               None).numpy().astype(np.float64)


@pytest.mark.parametrize("projection", ["pca", "lda"])
def test_lda_host_evaluator_scores_the_oracle(e2e, projection):
    train, labels, test, _, pairs, gt = e2e
    ev = LDAEvaluator(True, True, 100, 16, False, projection=projection)
    chunks = [torch.from_numpy(train[i:i + 96]) for i in range(0, len(train), 96)]
    ev.fit_parameters(chunks, [torch.tensor(labels[i:i + 96]) for i in range(0, len(train), 96)])
    want = bc.fit_and_score(train, labels, test, pairs, kind="lda", projection_kind=projection, R=16)
    got = _host_scores(ev, e2e)
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    samples, trial = _samples_and_pairs(e2e)
    res = ev.evaluate(trial, samples)
    clipped = np.clip((got + 1) / 2, 0, 1).tolist()
    assert res["eer"] == calculate_eer(gt, clipped, pos_label=1)[0]
    assert res["mdc"] == calculate_mdc(gt, clipped)[0]


@pytest.mark.parametrize("projection", ["pca", "lda"])
def test_plda_host_evaluator_scores_the_oracle(e2e, projection):
    train, labels, test, _, pairs, gt = e2e
    ev = PLDAEvaluator(16, 16, 10, 100, projection=projection)
    ev.fit_parameters([torch.from_numpy(train)], [torch.tensor(labels)])
    want = bc.fit_and_score(train, labels, test, pairs, kind="plda", projection_kind=projection, R=16, Q=16, iterations=10)
    got = _host_scores(ev, e2e)
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    samples, trial = _samples_and_pairs(e2e)
    res = ev.evaluate(trial, samples)                       # unbounded: not through (s + 1) / 2, not clipped
    assert res["eer"] == calculate_eer(gt, got.tolist(), pos_label=1)[0]
    assert np.abs(want).max() > 1
    cos_eer = calculate_eer(gt, bc.cosine_scores(test, pairs).tolist(), pos_label=1)[0]
    assert res["eer"] <= bc.EER_RATIO * cos_eer


def test_plda_keeps_fewer_dimensions_than_the_projection(e2e):
    train, labels, test, _, pairs, _ = e2e
    ev = PLDAEvaluator(14, 6, 2, 100)                       # neither a multiple of 4: the pads carry nothing
    ev.fit_parameters([torch.from_numpy(train)], [torch.tensor(labels)])
    want = bc.fit_and_score(train, labels, test, pairs, kind="plda", projection_kind="pca", R=14, Q=6, iterations=2)
    assert np.abs(_host_scores(ev, e2e) - want).max() <= 1e-4 * np.abs(want).max()
    assert ev.psi.shape == (6,)


def test_lda_centre_before_fit_and_latent_flags(e2e):
    train, labels, test, _, pairs, _ = e2e
    ev = LDAEvaluator(False, False, 100, 8, True)
    ev.fit_parameters([torch.from_numpy(train)], [torch.tensor(labels)])
    std, mean = torch.std_mean(torch.from_numpy(train), dim=0)
    z = lambda a: ((torch.from_numpy(a) - mean) / (std + 1e-12)).numpy()
    want = bc.fit_and_score(z(train), labels, z(test), pairs, kind="lda", projection_kind="pca", R=8, centre=False,
                            length_norm=False)
    assert np.abs(_host_scores(ev, e2e) - want).max() <= 1e-4


def test_lda_host_score_norm(e2e):
    train, labels, test, _, pairs, gt = e2e
    ev = LDAEvaluator(True, True, 100, 16, False)
    ev.fit_parameters([torch.from_numpy(train)], [torch.tensor(labels)])
    cohort = torch.from_numpy(np.stack([train[np.array(labels) == s].mean(axis=0) for s in sorted(set(labels))]))
    samples, trial = _samples_and_pairs(e2e)
    res = ev.evaluate(trial, samples, score_norm=ScoreNorm(cohort, 10, "s"))
    lat, coh = ev._host_latent(torch.from_numpy(test)).double().numpy(), ev._host_latent(cohort).double().numpy()
    S = np.sort(lat @ coh.T, axis=1)[:, -10:]
    mu, sd = S.mean(axis=1), S.std(axis=1, ddof=1)
    cos = (lat[pairs[:, 0]] * lat[pairs[:, 1]]).sum(axis=1)
    want = ((cos - mu[pairs[:, 0]]) / sd[pairs[:, 0]] + (cos - mu[pairs[:, 1]]) / sd[pairs[:, 1]]) / 2
    assert abs(res["eer"] - calculate_eer(gt, want.tolist(), pos_label=1)[0]) <= 2e-3


def test_reference_keywords_and_attributes():
    lda = LDAEvaluator(center_before_scoring=True, length_norm_before_scoring=True, max_training_batches_to_fit=30000,
                       num_pca_components=150, center_before_fit_training_batches=True)      # config/evaluator/lda.yaml
    assert lda.max_num_training_samples == 30000 and lda.num_pca_components == 150 and lda.projection == "pca"
    plda = PLDAEvaluator(num_lda_pca_components=50, num_plda_pca_components=50, max_iterations=1,
                         max_training_batches_to_fit=300)                                    # config/evaluator/plda.yaml
    assert plda.max_num_training_samples == 300 and plda.max_iterations == 1
    for ev in (lda, plda):
        for name in ("fit_parameters", "fit_parameters_bank", "reset_parameters", "evaluate", "evaluate_bank",
                     "evaluate_bank_metrics"):
            assert callable(getattr(ev, name))
    assert isinstance(CosineDistanceEvaluator(False, False, 0), CosineDistanceEvaluator)


def test_value_errors(e2e):
    train, labels = torch.from_numpy(e2e[0]), e2e[1]
    samples, trial = _samples_and_pairs(e2e)
    with pytest.raises(ValueError, match="has not been called"):
        PLDAEvaluator(16, 16, 1, 0).evaluate(trial, samples)
    with pytest.raises(ValueError, match="has not been called"):
        LDAEvaluator(True, True, 0, 16, False).evaluate_bank_metrics(trial, [s.sample_id for s in samples], torch.zeros(160, 32))
    with pytest.raises(ValueError, match="at least 2"):
        LDAEvaluator(True, True, 0, 4, False).fit_parameters([train[:8]], [torch.zeros(8, dtype=torch.long)])
    with pytest.raises(ValueError, match="no within-class scatter"):
        PLDAEvaluator(4, 4, 1, 0).fit_parameters([train[:5]], [torch.arange(5)])
    with pytest.raises(ValueError, match="num_plda_pca_components"):
        PLDAEvaluator(8, 9, 1, 0)
    with pytest.raises(ValueError, match="components"):     # R > min(D, N - 1)
        LDAEvaluator(True, True, 0, 33, False).fit_parameters([train], [torch.tensor(labels)])
    with pytest.raises(ValueError, match="components"):     # R > C - 1 for the discriminant projection
        LDAEvaluator(True, True, 0, 4, False, projection="lda").fit_parameters([train[:24]], [torch.tensor(labels[:24])])
    with pytest.raises(ValueError, match="projection"):
        LDAEvaluator(True, True, 0, 4, False, projection="ica")
    flat = train.clone()
    flat[:, 20:] = 0.0                                       # twelve dead dimensions: rank 20
    with pytest.raises(ValueError, match="reduce the number of components"):
        PLDAEvaluator(24, 24, 1, 0).fit_parameters([flat], [torch.tensor(labels)])
    ev = PLDAEvaluator(16, 16, 1, 0)
    ev.fit_parameters([train], [torch.tensor(labels)])
    ev.reset_parameters()
    with pytest.raises(ValueError, match="has not been called"):
        ev.evaluate(trial, samples)
    with pytest.raises(ValueError, match="metrics="):
        ev.evaluate_bank_metrics(trial, [s.sample_id for s in samples], torch.zeros(160, 32), metrics="gpu")


def test_not_implemented(e2e):
    train, labels, test = torch.from_numpy(e2e[0]), e2e[1], e2e[2]
    samples, trial = _samples_and_pairs(e2e)
    keys = [s.sample_id for s in samples]
    ev = PLDAEvaluator(16, 16, 1, 0)
    ev.fit_parameters([train], [torch.tensor(labels)])
    bank = torch.from_numpy(test)
    with pytest.raises(NotImplementedError, match="ensemble"):
        ev.evaluate_bank_metrics(trial, keys, [bank, bank])
    with pytest.raises(NotImplementedError, match="frame"):
        ev.evaluate_bank_metrics(trial, keys, bank, frame_offsets=list(range(161)))
    with pytest.raises(NotImplementedError, match="score normalisation"):
        ev.evaluate_bank_metrics(trial, keys, bank, score_norm=ScoreNorm(train[:8], 4))
    with pytest.raises(NotImplementedError, match="score normalisation"):
        ev.evaluate(trial, samples, score_norm=ScoreNorm(train[:8], 4))
    with pytest.raises(NotImplementedError, match="ensemble"):
        ev.evaluate(trial[:1], [EmbeddingSample("u0", [bank[0], bank[0]]), EmbeddingSample("u1", [bank[1], bank[1]])])
    with pytest.raises(NotImplementedError, match="frame"):
        ev.evaluate(trial[:1], [EmbeddingSample("u0", bank[:3]), EmbeddingSample("u1", bank[3:6])])


def test_new_symbols_in_header_and_ctypes_table():
    header = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    source = open(os.path.join(ROOT, "w2v2_speaker_amd", "csrc", "backend.hip")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r'extern "C" int %s\(' % name, source), name
        assert name in _lib._SIGS and name in _lib.EXPORTS
    from w2v2_speaker_amd import _build
    assert "backend.hip" in _build.SOURCES
    assert "scoring back-ends" in header
