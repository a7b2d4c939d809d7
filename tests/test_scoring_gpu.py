"""Device trial scoring on the GPU: the three kernels of csrc/score.hip on every case of tests/scoring_cases.py within the
bound stated there (2 x the host f32 path's own error against float64, floor 2^-22), bitwise reproducibility, the NaN
answers to indices that must not be dereferenced, CosineDistanceEvaluator.evaluate_bank against the reference evaluator's
goldens and against ``evaluate``, and evaluate_trials(scoring="device") of two modules against the host path."""
import random
import warnings

import numpy as np
import pytest
import torch

import scoring_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENTINEL = 8, 12345.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(P):
    """P output cells of NaN with GUARD sentinel cells behind them: every output must be written, nothing past them."""
    buf = torch.full((P + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    buf[P:] = SENTINEL
    return buf


def landed(buf, P):
    out = buf.cpu().numpy()
    assert (out[P:] == SENTINEL).all(), "written past the outputs"
    return out[:P]


def run_pairs(c, bank, pairs=None):
    from w2v2_speaker_amd import ops
    pairs = c["pairs"] if pairs is None else pairs
    P = len(pairs)
    cos, score = guarded(P), guarded(P)
    mean, std = (None, None) if c.get("mean") is None else (dev(c["mean"]), dev(c["std"]))
    ops.score_pairs(bank, dev(pairs), mean, std, c.get("length_norm", False), cos, score)
    return landed(cos, P), landed(score, P)


@pytest.mark.parametrize("centre,length_norm", SC.PAIR_MODES)
@pytest.mark.parametrize("D", SC.PAIR_DIMS)
def test_score_pairs_cases_within_the_bound_and_bitwise_stable(D, centre, length_norm):
    c = SC.pairs_case(D, centre, length_norm)
    cos, score = run_pairs(c, dev(c["bank"]))
    e_cos, e_score = np.abs(cos - c["cos"]).max(), np.abs(score - c["score"]).max()
    print(f"scoring-parity: score_pairs D={D} centre={int(centre)} lnorm={int(length_norm)}: cos {e_cos:.2e} bound "
          f"{c['bound_cos']:.2e}; score {e_score:.2e} bound {c['bound_score']:.2e}")
    assert not np.isnan(cos).any() and not np.isnan(score).any()
    assert e_cos <= c["bound_cos"] and e_score <= c["bound_score"]
    if not centre:
        assert cos[2] == 0 and score[2] == 0.5          # the zero row scores 0 through the 1e-8 clamp
    cos2, score2 = run_pairs(c, dev(c["bank"]))         # a second run: the same bits
    assert np.array_equal(cos, cos2) and np.array_equal(score, score2)
    cos_ld, score_ld = run_pairs(c, dev(c["ld_bank"])[:, :D])      # ld = D + 4, NaN in the gap
    assert np.array_equal(cos, cos_ld) and np.array_equal(score, score_ld)
    for P in SC.PAIR_COUNTS:                            # around the four-trial workgroup
        cp, sp = run_pairs(c, dev(c["bank"]), c["pairs"][:P])
        assert np.array_equal(cp, cos[:P]) and np.array_equal(sp, score[:P]), P
    for t in range(len(c["pairs"])):                    # a trial scored alone = its entry in the full list
        c1, s1 = run_pairs(c, dev(c["bank"]), c["pairs"][t:t + 1])
        assert c1[0] == cos[t] and s1[0] == score[t], t


def test_score_pairs_on_a_two_row_bank():
    c = SC.two_row_case()
    cos, score = run_pairs(c, dev(c["bank"]))
    assert np.abs(cos - c["cos"]).max() <= c["bound_cos"] and np.abs(score - c["score"]).max() <= c["bound_score"]
    assert cos[0] == cos[1]


def test_score_pairs_index_out_of_range_gives_nan_for_that_trial_alone():
    """The raw entry point: TrialIndex rejects such a list before upload, the kernel must not dereference it."""
    c = SC.pairs_case(260, False, False)
    clean, clean_s = run_pairs(c, dev(c["bank"]))
    pairs = c["pairs"].copy()
    pairs[1] = (8, 0)                                   # N = 8: one past the bank
    pairs[4] = (3, -1)
    pairs[6] = (2 ** 31 - 1, 1)
    cos, score = run_pairs(c, dev(c["bank"]), pairs)
    bad = np.array([1, 4, 6])
    good = np.setdiff1d(np.arange(len(pairs)), bad)
    assert np.isnan(cos[bad]).all() and np.isnan(score[bad]).all()
    assert np.array_equal(cos[good], clean[good]) and np.array_equal(score[good], clean_s[good])


@pytest.mark.parametrize("D", SC.STATS_DIMS)
@pytest.mark.parametrize("N", SC.STATS_ROWS)
def test_embed_stats_cases_within_the_bound_and_exact_on_a_constant_dimension(N, D):
    from w2v2_speaker_amd import ops
    c = SC.stats_case(N, D)

    def run(bank):
        mean, std = guarded(D), guarded(D)
        ops.embed_stats(bank, mean, std)
        return landed(mean, D), landed(std, D)
    mean, std = run(dev(c["bank"]))
    em, es = SC.stats_err(mean, std, c["mean"], c["std"])
    print(f"scoring-parity: embed_stats N={N} D={D}: mean {em:.2e} bound {c['bound_mean']:.2e}; std {es:.2e} bound "
          f"{c['bound_std']:.2e} (relative to the per-dimension std)")
    assert em <= c["bound_mean"] and es <= c["bound_std"]
    assert mean[SC.CONST_DIM] == np.float32(0.37) and std[SC.CONST_DIM] == 0
    mean2, std2 = run(dev(c["bank"]))
    assert np.array_equal(mean, mean2) and np.array_equal(std, std2)
    mean_ld, std_ld = run(dev(c["ld_bank"])[:, :D])
    assert np.array_equal(mean, mean_ld) and np.array_equal(std, std_ld)


def run_frames(c, frames, sel=None, counts=None):
    from w2v2_speaker_amd import ops
    sel = c["sel"] if sel is None else sel
    counts = c["counts"] if counts is None else counts
    P = len(sel)
    cos, score = guarded(P), guarded(P)
    ops.score_frame_sets(frames, dev(sel), dev(counts), cos, score)
    return landed(cos, P), landed(score, P)


@pytest.mark.parametrize("D", SC.FRAME_DIMS)
def test_score_frame_sets_cases_within_the_bound_and_bitwise_stable(D):
    c = SC.frames_case(D)
    cos, score = run_frames(c, dev(c["frames"]))
    e_cos, e_score = np.abs(cos - c["cos"]).max(), np.abs(score - c["score"]).max()
    print(f"scoring-parity: score_frame_sets D={D} counts={SC.FRAME_COUNTS}: cos {e_cos:.2e} bound {c['bound_cos']:.2e}; "
          f"score {e_score:.2e} bound {c['bound_score']:.2e}")
    assert e_cos <= c["bound_cos"] and e_score <= c["bound_score"]
    cos2, score2 = run_frames(c, dev(c["frames"]))
    assert np.array_equal(cos, cos2) and np.array_equal(score, score2)
    cos_ld, score_ld = run_frames(c, dev(c["ld_frames"])[:, :D])
    assert np.array_equal(cos, cos_ld) and np.array_equal(score, score_ld)
    for t in range(len(c["sel"])):
        c1, s1 = run_frames(c, dev(c["frames"]), c["sel"][t:t + 1], c["counts"][t:t + 1])
        assert c1[0] == cos[t] and s1[0] == score[t], t


def test_score_frame_sets_empty_side_or_row_out_of_range_gives_nan_for_that_trial_alone():
    c = SC.frames_case(260)
    clean, clean_s = run_frames(c, dev(c["frames"]))
    sel, counts = np.concatenate([c["sel"]] * 2), np.concatenate([c["counts"]] * 2)
    counts[1] = (3, 0)                                  # an empty side
    sel[2, 1, 17] = SC.FRAME_ROWS                       # one past the bank
    sel[4, 0, 0] = -1
    counts[7] = (51, 50)                                # more than the W slots of a side
    cos, score = run_frames(c, dev(c["frames"]), sel, counts)
    bad = np.array([1, 2, 4, 7])
    good = np.setdiff1d(np.arange(8), bad)
    assert np.isnan(cos[bad]).all() and np.isnan(score[bad]).all()
    assert np.array_equal(cos[good], np.concatenate([clean] * 2)[good])
    assert np.array_equal(score[good], np.concatenate([clean_s] * 2)[good])


# ------------------------------------------------------------------------------------------------ the evaluator
def _g12_eval():
    from w2v2_speaker_amd.data.synthetic import synth_trial_set
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    _, _, keys, trials = synth_trial_set()
    return keys, [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]


@pytest.mark.parametrize("tag", list(SC.G12_BRANCHES))
def test_evaluate_bank_reproduces_the_reference_evaluator_on_g12(tag):
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator
    g, c = SC.g12(), SC.g12_case(tag)
    keys, pairs = _g12_eval()
    centre, ln = SC.G12_BRANCHES[tag]
    ev = CosineDistanceEvaluator(centre, ln, 32)
    bank = dev(c["bank"])
    if centre:                                          # the fit on the device, against the reference's own fit
        ev.fit_parameters_bank(bank)
        mean, std = SC.stats_ref(c["bank"])
        bm, bs = (SC.bound(e) for e in SC.stats_err(*SC.host_stats(c["bank"]), mean, std))
        em, es = SC.stats_err(ev.mean.cpu().numpy(), ev.std.cpu().numpy(), mean, std)
        print(f"scoring-parity: g12 fit on the device: mean {em:.2e} bound {bm:.2e}; std {es:.2e} bound {bs:.2e}")
        assert em <= bm and es <= bs
        ev.mean, ev.std = torch.from_numpy(g["fit_mean"]), torch.from_numpy(g["fit_std"])    # score with the reference's
    res = ev.evaluate_bank(pairs, keys, bank)
    got = ev.last_bank_scoring
    err = float(np.abs(got.scores - c["score"]).max())
    err_g = float(np.abs(got.scores - g[f"scores{tag}"]).max())
    print(f"scoring-parity: g12 evaluate_bank scores{tag}: vs float64 {err:.2e} bound {c['bound_score']:.2e}; vs the "
          f"reference's f32 scores {err_g:.2e}")
    assert err <= c["bound_score"]
    assert got.host_copy_floats == 496 and got.bank_floats == 32 * 1536
    if centre:            # smallest target / non-target gap 4.5e-4 here; 8.9e-8 on the other two branches: scores only
        for k in ("eer", "mdc", "eer_threshold", "mdc_threshold"):
            assert abs(res[k] - float(g[f"{k}{tag}"])) < 1e-6, (tag, k)


def test_evaluate_bank_non_pooled_trials_of_g12():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EvaluationPair
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import TrialIndex, draw_frame_sets
    g = SC.g12()
    frames, offsets, trials = SC.g12_frames()
    keys = [f"np{i}" for i in range(6)]
    pairs = [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]
    random.seed(int(g["nonpooled_seed"]))
    sel, counts = draw_frame_sets(np.diff(offsets), TrialIndex(pairs, keys))
    cos, score = SC.frame_sets_ref(frames, sel, counts)
    b = SC.bound(np.abs(SC.host_frame_sets(frames, sel, counts)[1] - score).max())
    ev = CosineDistanceEvaluator(True, True, 0)         # centring / length norm do not apply to this form
    random.seed(int(g["nonpooled_seed"]))
    res = ev.evaluate_bank(pairs, keys, dev(frames), frame_offsets=offsets)
    err = float(np.abs(ev.last_bank_scoring.scores - score).max())
    err_g = float(np.abs(ev.last_bank_scoring.scores - SC.to_score(g["nonpooled_scores"])).max())
    print(f"scoring-parity: g12 evaluate_bank non-pooled: vs float64 {err:.2e} bound {b:.2e}; vs the reference {err_g:.2e}")
    assert err <= b and err_g <= 2 * b and set(res) == {"eer", "eer_threshold", "mdc", "mdc_threshold"}
    assert ev.last_bank_scoring.host_copy_floats == 15


def test_evaluate_bank_equals_evaluate_on_the_separated_set():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EmbeddingSample
    s = SC.separated_set()
    ev = CosineDistanceEvaluator()
    host = ev.evaluate(s["eval_pairs"], [EmbeddingSample(k, torch.from_numpy(e)) for k, e in zip(s["keys"], s["bank"])])
    got = ev.evaluate_bank(s["eval_pairs"], s["keys"], dev(s["bank"]))
    assert np.abs(ev.last_bank_scoring.scores - s["score"]).max() <= s["bound_score"]
    assert 0.0 < host["eer"] < 0.5
    assert abs(got["eer"] - host["eer"]) < 1e-9 and abs(got["mdc"] - host["mdc"]) < 1e-9


def test_evaluate_bank_ensemble_equals_the_host_ensemble():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EmbeddingSample
    s = SC.separated_set()
    rng = np.random.default_rng(5)
    members = [s["bank"], (s["bank"] + 0.5 * rng.standard_normal(s["bank"].shape)).astype(np.float32),
               (s["bank"] * rng.uniform(0.5, 2, 64)).astype(np.float32)]
    ref = SC.to_score(sum(SC.score_pairs_ref(m, s["pairs"])[0] for m in members) / 3)
    ev = CosineDistanceEvaluator()
    smp = [EmbeddingSample(k, [torch.from_numpy(m[i]) for m in members]) for i, k in enumerate(s["keys"])]
    host = SC.to_score(ev._compute_ensemble_prediction_scores([(smp[i], smp[j]) for i, j in s["pairs"]]))
    b = SC.bound(np.abs(host - ref).max())
    res = ev.evaluate_bank(s["eval_pairs"], s["keys"], [dev(m) for m in members])
    err, err_h = np.abs(ev.last_bank_scoring.scores - ref).max(), np.abs(ev.last_bank_scoring.scores - host).max()
    print(f"scoring-parity: ensemble of 3: vs float64 {err:.2e} bound {b:.2e}; vs the host ensemble {err_h:.2e}")
    assert err <= b and err_h <= b and 0.0 <= res["eer"] <= 1.0
    assert ev.last_bank_scoring.host_copy_floats == 3 * 496


def test_evaluate_bank_missing_key_and_unfitted_centring():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EvaluationPair
    bank = torch.zeros(2, 4, device=DEV)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = CosineDistanceEvaluator().evaluate_bank([EvaluationPair(True, "a", "zz")], ["a", "b"], bank)
    assert res == {"eer": -1, "eer_threshold": -1, "mdc": -1, "mdc_threshold": -1} and len(w) == 1
    with pytest.raises(TypeError, match=r"center_before_scoring=True but fit_parameters\(\) has not been called"):
        CosineDistanceEvaluator(True, False, 0).evaluate_bank([EvaluationPair(True, "a", "b")], ["a", "b"], bank)


# ------------------------------------------------------------------------------------------------ the modules
def _module_case(name):
    """(module, key -> input, batching keywords): six utterances of three lengths."""
    if name == "wav2vec2":
        from test_varlen_gpu import _tiny_module
        mod = _tiny_module()
        make = lambda i, n: torch.randn(n, generator=torch.Generator().manual_seed(i))
        lens, kw = (1200, 4000, 7000), dict(quantum=800, max_batch_samples=4 * 8000, max_batch=4)
    else:
        from test_varlen_ecapa_gpu import _ecapa_module
        mod = _ecapa_module(torch.float32)
        make = lambda i, n: torch.randn(n, mod.cfg.input_mel_coefficients, generator=torch.Generator().manual_seed(i))
        lens, kw = (20, 130, 390), dict(quantum=50, max_batch_frames=4 * 400, max_batch=4)
    return mod, {f"u{i}": make(i, lens[i % 3]) for i in range(6)}, kw


@pytest.mark.parametrize("name", ["wav2vec2", "ecapa"])
def test_evaluate_trials_device_scoring_agrees_with_the_host_path(name):
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    mod, inputs, kw = _module_case(name)
    keys = sorted(inputs)
    idx = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    bank = torch.cat(mod.compute_speaker_embeddings([inputs[k] for k in keys], **kw)).detach().cpu().numpy()
    cos, score = SC.score_pairs_ref(bank, idx)
    host_score = SC.host_pairs(bank, idx)[1]
    b = SC.bound(np.abs(host_score - score).max())
    # a separated list: the target class = the scores above the widest gap of the sorted float64 scores
    order = np.sort(score)
    cut = int(np.argmax(np.diff(order)))
    assert order[cut + 1] - order[cut] > 4 * b, "the six utterances give no separated trial list"
    pairs = [EvaluationPair(bool(s > order[cut]), keys[i], keys[j]) for s, (i, j) in zip(score, idx)]
    # scoring="host" = what the parent commit's evaluate_trials does
    embs = mod.compute_speaker_embeddings([inputs[k] for k in keys], **kw)
    parent = mod._evaluate_embeddings([{"embedding": torch.cat(embs).detach().to("cpu"), "sample_id": keys}], pairs)
    assert mod.evaluate_trials(pairs, inputs, **kw) == parent
    assert mod.evaluate_trials(pairs, inputs, scoring="host", **kw) == parent
    got = mod.evaluate_trials(pairs, inputs, scoring="device", **kw)
    rec = mod.evaluator.last_bank_scoring
    err, err_h = np.abs(rec.scores - score).max(), np.abs(rec.scores - host_score).max()
    print(f"scoring-parity: {name} evaluate_trials(scoring='device'): vs float64 {err:.2e}, vs the host path {err_h:.2e}, "
          f"bound {b:.2e}; D = {bank.shape[1]}")
    assert err <= b and err_h <= b
    assert got["eer"] == parent["eer"] and abs(got["mdc"] - parent["mdc"]) < 1e-9
    # nothing of the bank's size went to the host: the one copy is the P scores
    assert rec.host_copy_floats == len(pairs) == 15 and rec.bank_floats == bank.size > rec.host_copy_floats
    with pytest.raises(ValueError, match="scoring"):
        mod.evaluate_trials(pairs, inputs, scoring="gpu", **kw)
