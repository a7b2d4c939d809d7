"""Device trial metrics on the GPU (csrc/metrics.hip): w2v2_sort_f32_index against np.argsort(kind="stable") around the
tile size on every key set of tests/metrics_cases.py, w2v2_trial_metrics on the committed cases and the edges against the
reference rule and the host metrics within the bounds stated in metrics_cases.py, the NaN and one-class answers of
metrics_device, evaluate_bank_metrics(metrics="device") against the reference evaluator's goldens, and
evaluate_trials(metrics="device") of two modules against metrics="host".  Every comparison is against metrics_ref or the
host functions, never against another run of the code under test (a second run is compared for equal bits only).

Measured with the host metrics of this repository (eval_metrics.py over scipy's interp1d): on a perfectly separated
list whose crossing lies in the segment from the origin (every positive at one score above every negative) calculate_eer
returns thr_hi, a finite value (0.8999999761581421 for the "separated_first_segment" edge): its interpolation at the
repeated abscissa 0 lands on the first score.  The device returns +inf, the origin's threshold.  The host value is
asserted as on every vertical crossing: an end of the kept run, or not finite.  A list of one class: calculate_mdc does
not raise there, so the host's dict is eer 1, eer_threshold 1337 and calculate_mdc's own NaN, and metrics_device returns
that dict."""
import numpy as np
import pytest
import torch

import metrics_cases as MC
import scoring_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
KEYS = ("eer", "eer_threshold", "mdc", "mdc_threshold")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(P, dtype, sentinel):
    """P output cells with GUARD sentinel cells behind them (the pattern of test_scoring_gpu.py): every output must be
    written -- the cells start as a value no output can be -- and nothing past them."""
    return torch.full((P + GUARD,), sentinel, dtype=dtype, device=DEV)


def landed(buf, P, sentinel):
    out = buf.cpu().numpy()
    assert (out[P:].view(np.uint32) == np.array([sentinel], dtype=out.dtype).view(np.uint32)).all(), "written past the outputs"
    return out[:P]


def run_sort(keys):
    from w2v2_speaker_amd import ops
    P = len(keys)
    order, skeys = guarded(P, torch.int32, -7), guarded(P, torch.float32, -12345.0)
    ops.sort_f32_index(dev(keys), order, skeys)
    return landed(order, P, -7), landed(skeys, P, -12345.0)


@pytest.mark.parametrize("kind", MC.SORT_KINDS)
def test_sort_equals_the_stable_argsort_at_every_size(kind):
    from w2v2_speaker_amd import ops
    for P in MC.sort_sizes(ops.SORT_TILE):
        keys = MC.sort_keys(kind, P)
        order, skeys = run_sort(keys)
        ref = MC.sort_ref(keys)
        assert np.array_equal(order, ref), (kind, P, int(np.argmax(order != ref)))
        assert np.array_equal(skeys.view(np.uint32), keys[ref].view(np.uint32)), (kind, P)      # the keys' own bits
        order2, skeys2 = run_sort(keys)
        assert np.array_equal(order, order2) and np.array_equal(skeys.view(np.uint32), skeys2.view(np.uint32)), (kind, P)
    print(f"metrics-parity: sort_f32_index {kind}: order == argsort(stable) and keys bit-equal at P = "
          f"{MC.sort_sizes(ops.SORT_TILE)}")


def test_sort_without_the_sorted_keys_and_with_a_workspace_of_its_own():
    from w2v2_speaker_amd import ops
    keys = MC.sort_keys("full_range", 3 * ops.SORT_TILE + 5)
    ws = ops.sort_f32_index_workspace(len(keys), DEV)
    order, none = ops.sort_f32_index(dev(keys), workspace=ws)
    assert none is None and np.array_equal(order.cpu().numpy(), MC.sort_ref(keys))
    with pytest.raises(ValueError, match="workspace holds"):
        ops.sort_f32_index(dev(keys), workspace=ws[:-16])


def run_metrics(gt, s, p_target=0.05):
    """-> the eight outputs by name (twice run: the same bits), out[8] guarded."""
    from w2v2_speaker_amd import ops
    scores, labels = dev(np.asarray(s, dtype=np.float32)), dev(np.asarray(gt, dtype=np.uint8))
    outs = []
    for _ in range(2):
        out = guarded(8, torch.float64, -777.0)
        ops.trial_metrics(scores, labels, p_target=p_target, out=out)
        host = out.cpu().numpy()
        assert (host[8:] == -777.0).all(), "written past the outputs"
        outs.append(host[:8])
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)), "a second run gave other bits"
    return dict(zip(ops.TRIAL_METRICS_FIELDS, outs[0].tolist()))


def check_case(got, gt, s, m, h, p_target=0.05, what=""):
    f = MC.check_against_host(got, m, h, what=what)
    MC.check_mdc_threshold(got["mdc_threshold"], gt, s, p_target=p_target)
    assert (got["n_pos"], got["n_neg"], got["n_nan"]) == (m["n_pos"], m["n_neg"], 0), what
    assert got["n_thresholds"] == m["n_thresholds"] == h["n_thresholds"], what
    return f


def test_trial_metrics_on_the_committed_cases():
    worst = {"eer_ref": 0.0, "eer_host": 0.0, "mdc_ref": 0.0, "mdc_host": 0.0, "thr / bound": 0.0}
    for n, (gt, s, m, h) in enumerate(MC.cases()):
        f = check_case(run_metrics(gt, s), gt, s, m, h, what=n)
        for k in ("eer_ref", "eer_host", "mdc_ref", "mdc_host"):
            worst[k] = max(worst[k], f[k])
        if f["thr_bound"]:
            worst["thr / bound"] = max(worst["thr / bound"], f["thr"] / f["thr_bound"])
    print(f"metrics-parity: trial_metrics over {MC.NUM_CASES} cases: eer vs rule {worst['eer_ref']:.2e}, vs host "
          f"{worst['eer_host']:.2e} (bound {MC.EER_BOUND:.0e}); interior threshold at most {worst['thr / bound']:.2f} of its "
          f"bound; mdc rel vs rule {worst['mdc_ref']:.2e}, vs host {worst['mdc_host']:.2e} (bound {MC.MDC_REL:.2e})")


@pytest.mark.parametrize("name", sorted(MC.edge_cases(2048)))
def test_trial_metrics_on_the_edges(name):
    from w2v2_speaker_amd import ops
    gt, s, p_target = MC.edge_cases(ops.SORT_TILE)[name]
    m, h = MC.metrics_ref(gt, s, p_target=p_target), MC.host_metrics(gt, s, p_target=p_target)
    got = run_metrics(gt, s, p_target)
    f = check_case(got, gt, s, m, h, p_target, what=name)
    print(f"metrics-parity: trial_metrics {name} (P = {len(s)}, {m['kind']}, {m['n_thresholds']} thresholds): eer "
          f"{got['eer']:.12f} vs rule {f['eer_ref']:.2e} vs host {f['eer_host']:.2e}; threshold {got['eer_threshold']:.9f} "
          f"(host {h['eer_threshold']:.9f}); mdc {got['mdc']:.12f} rel vs host {f['mdc_host']:.2e}")
    if name == "separated_first_segment":
        assert got["eer"] == 0 and got["eer_threshold"] == np.inf
    if name == "separated_distinct":
        assert got["eer"] == 0 and got["eer_threshold"] == m["thr_hi"]
    if name == "inverted":
        assert got["eer"] == 1
    if name.startswith("tie_order"):
        want = MC.TIE_HOST[int(name[-1])]
        assert got["mdc"] == pytest.approx(want[0], abs=1e-15) and got["mdc_threshold"] == float(np.float32(want[1]))
        assert got["mdc_threshold"] == h["mdc_threshold"]


def _index(gt):
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import TrialIndex
    P = len(gt)
    return TrialIndex.from_rows([(i, i) for i in range(P)], gt, P)


def test_nan_scores_are_counted_and_answered_by_the_host_path():
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import host_metrics, metrics_device
    gt, s, _, _ = MC.cases()[0]
    s = s.copy()
    s[1] = np.uint32(0x7fc00000).view(np.float32)
    s[len(s) // 2] = np.uint32(0xffc00001).view(np.float32)
    s[-1] = np.nan
    got = run_metrics(gt, s)
    assert got["n_nan"] == 3 and (got["n_pos"], got["n_neg"]) == (int(gt.sum()), int(len(gt) - gt.sum()))
    record = []
    res = metrics_device(dev(s), _index(gt), record=record)
    want = host_metrics([int(v) for v in gt], s.astype(np.float64).tolist())
    assert set(res) == set(KEYS)
    for k in KEYS:                      # the same path: the same object values, NaN or fallback included
        assert res[k] == want[k] or (np.isnan(res[k]) and np.isnan(want[k])), (k, res[k], want[k])
    assert record[0].path == "host" and record[0].host_copy_floats == len(s) and record[0].fields["n_nan"] == 3


def test_one_class_list_launches_nothing_and_returns_the_host_fallbacks():
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import host_metrics, metrics_device
    s = dev(np.float32([0.1, 0.4, 0.9]))
    for label in (0, 1):
        record, called = [], []
        real = ops.trial_metrics
        ops.trial_metrics = lambda *a, **k: called.append(1) or real(*a, **k)
        try:
            res = metrics_device(s, _index([label] * 3), record=record)
        finally:
            ops.trial_metrics = real
        want = host_metrics([label] * 3, s.cpu().numpy().astype(np.float64).tolist())
        assert not called and (res["eer"], res["eer_threshold"]) == (1, 1337)      # the reference's "very bad score"
        for k in KEYS:                  # (calculate_mdc does not raise on one class: its NaN is the host's answer too)
            assert res[k] == want[k] or (np.isnan(res[k]) and np.isnan(want[k])), (k, res[k], want[k])
        assert record[0].path == "host" and record[0].host_copy_doubles == 0


def test_metrics_device_on_a_clean_list_copies_eight_doubles():
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import metrics_device
    gt, s, m, h = MC.cases()[1]
    record = []
    res = metrics_device(dev(s), _index(gt), record=record)
    MC.check_against_host(res, m, h)
    assert set(res) == set(KEYS) and all(isinstance(v, float) for v in res.values())
    assert record[0].path == "device" and record[0].host_copy_floats == 0 and record[0].host_copy_doubles == 8


@pytest.mark.parametrize("tag", ["_c", "_cl"])
def test_evaluate_bank_device_metrics_reproduce_the_reference_evaluator_on_g12(tag):
    """The centred branches of g12, as in test_scoring_gpu.py: their smallest target / non-target score gap (4.5e-4) is far
    above the scoring bound, so the order of the device scores is the reference's and EER / minDCF are its values to the
    bounds of the metrics; a threshold is a score or an interpolation of two, so it moves with the scores: by at most the
    device's scoring bound plus the golden scores' own distance from float64, on top of the metric's own."""
    from test_scoring_gpu import _g12_eval
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator
    g, c = SC.g12(), SC.g12_case(tag)
    keys, pairs = _g12_eval()
    centre, ln = SC.G12_BRANCHES[tag]
    ev = CosineDistanceEvaluator(centre, ln, 32)
    ev.mean, ev.std = torch.from_numpy(g["fit_mean"]), torch.from_numpy(g["fit_std"])
    res = ev.evaluate_bank_metrics(pairs, keys, dev(c["bank"]), metrics="device")
    rec = ev.last_bank_scoring
    assert rec.scores is None and rec.host_copy_floats == 0 and rec.bank_floats == 32 * 1536
    assert ev.last_bank_metrics.path == "device" and ev.last_bank_metrics.host_copy_doubles == 8
    m = MC.metrics_ref(c["gt"], rec.device_scores.cpu().numpy())
    want = {k: float(g[f"{k}{tag}"]) for k in KEYS}
    s_bound = c["bound_score"] + float(np.abs(g[f"scores{tag}"] - c["score"]).max())
    t_bound = s_bound + (MC.thr_bound(m) if m["kind"] != "vertical" and np.isfinite(m["thr_lo"]) else 0.0)
    print(f"metrics-parity: g12 evaluate_bank_metrics(metrics='device') {tag}: eer {res['eer']:.12f} vs the reference "
          f"{abs(res['eer'] - want['eer']):.2e}; eer_threshold {abs(res['eer_threshold'] - want['eer_threshold']):.2e} (bound "
          f"{t_bound:.2e}); mdc rel {abs(res['mdc'] - want['mdc']) / want['mdc']:.2e}; mdc_threshold "
          f"{abs(res['mdc_threshold'] - want['mdc_threshold']):.2e} (bound {s_bound:.2e})")
    assert abs(res["eer"] - want["eer"]) <= MC.EER_BOUND
    assert abs(res["eer_threshold"] - want["eer_threshold"]) <= t_bound
    assert abs(res["mdc"] - want["mdc"]) <= MC.MDC_REL * want["mdc"]
    assert abs(res["mdc_threshold"] - want["mdc_threshold"]) <= s_bound
    # ... and the host metrics of the same device scores, through the default path
    host = ev.evaluate_bank(pairs, keys, dev(c["bank"]))
    assert ev.last_bank_scoring.host_copy_floats == 496
    h = {**host, "n_thresholds": m["n_thresholds"]}
    MC.check_against_host(res, m, h, what=tag)


def test_evaluate_bank_device_metrics_on_a_frame_bank():
    import random
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EvaluationPair
    g = SC.g12()
    frames, offsets, trials = SC.g12_frames()
    keys = [f"np{i}" for i in range(6)]
    pairs = [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]
    ev = CosineDistanceEvaluator()
    random.seed(int(g["nonpooled_seed"]))
    host = ev.evaluate_bank(pairs, keys, dev(frames), frame_offsets=offsets)
    scores = ev.last_bank_scoring.scores
    random.seed(int(g["nonpooled_seed"]))
    res = ev.evaluate_bank_metrics(pairs, keys, dev(frames), frame_offsets=offsets, metrics="device")
    assert ev.last_bank_scoring.host_copy_floats == 0 and ev.last_bank_scoring.scores is None
    assert np.array_equal(ev.last_bank_scoring.device_scores.cpu().numpy().astype(np.float64), scores)
    gt = [int(t[0]) for t in trials]
    m = MC.metrics_ref(gt, scores.astype(np.float32))
    MC.check_against_host(res, m, {**host, "n_thresholds": m["n_thresholds"]}, what="frame bank")


def _xvector_case():
    from test_xvector_gpu import K, _module
    mod = _module()
    g = torch.Generator().manual_seed(2)
    lens = (12, 33, 57)
    return mod, {f"u{i}": torch.randn(lens[i % 3], K.MELS, generator=g) for i in range(6)}, \
        dict(quantum=10, max_batch_frames=120, max_batch=4)


@pytest.mark.parametrize("name", ["wav2vec2", "xvector"])
def test_evaluate_trials_device_metrics_agree_with_host_metrics(name):
    from test_scoring_gpu import _module_case
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    mod, inputs, kw = _module_case("wav2vec2") if name == "wav2vec2" else _xvector_case()
    keys = sorted(inputs)
    idx = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    gt = [int((i + j) % 3 == 0 or j == i + 1) for i, j in idx]             # both classes, overlapping scores
    pairs = [EvaluationPair(bool(t), keys[i], keys[j]) for t, (i, j) in zip(gt, idx)]
    host = mod.evaluate_trials(pairs, inputs, scoring="device", metrics="host", **kw)
    scores = mod.evaluator.last_bank_scoring.scores
    assert mod.evaluator.last_bank_scoring.host_copy_floats == 15
    got = mod.evaluate_trials(pairs, inputs, scoring="device", metrics="device", **kw)
    rec = mod.evaluator.last_bank_scoring
    assert rec.host_copy_floats == 0 and rec.scores is None and mod.evaluator.last_bank_metrics.path == "device"
    assert np.array_equal(rec.device_scores.cpu().numpy().astype(np.float64), scores)       # the same scores, twice
    m = MC.metrics_ref(gt, scores.astype(np.float32))
    f = MC.check_against_host(got, m, {**host, "n_thresholds": m["n_thresholds"]}, what=name)
    MC.check_mdc_threshold(got["mdc_threshold"], gt, scores.astype(np.float32))
    print(f"metrics-parity: {name} evaluate_trials(metrics='device') vs metrics='host' ({m['kind']}): eer {f['eer_host']:.2e}, "
          f"mdc rel {f['mdc_host']:.2e}")
    with pytest.raises(ValueError, match="needs scoring='device'"):
        mod.evaluate_trials(pairs, inputs, metrics="device", **kw)
