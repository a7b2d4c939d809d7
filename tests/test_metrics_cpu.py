"""CPU tests of the device trial metrics: the reference rule of tests/metrics_cases.py (what w2v2_trial_metrics
computes, restated in numpy int64 / float64) against the HOST metrics of eval_metrics.py within the bounds stated there,
the conditions on the committed case list, the tie-order pair, the C ABI of the new entries, and the argument errors of
``ops``, ``evaluate_bank_metrics(metrics=)`` and ``evaluate_trials(metrics=)`` that need no device.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

import metrics_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("eer", "eer_threshold", "mdc", "mdc_threshold")


def test_committed_case_list_meets_its_conditions():
    cs = MC.cases()
    kinds = Counter(m["kind"] for _, _, m, _ in cs)
    print(f"metrics-parity (cpu): {len(cs)} cases: {dict(kinds)}")
    assert len(cs) == MC.NUM_CASES == 400
    assert kinds["interior"] >= 0.60 * len(cs) and kinds["vertical"] >= 0.10 * len(cs)
    for gt, s, _, _ in cs:
        assert 4 <= len(s) < 300 and s.dtype == np.float32 and 0 < gt.sum() < len(gt) and s.min() >= 0 and s.max() <= 1


def test_reference_rule_against_the_host_metrics_on_the_committed_cases():
    worst = Counter()
    for n, (gt, s, m, h) in enumerate(MC.cases()):
        f = MC.check_against_host({k: m[k] for k in KEYS}, m, h, what=n)
        MC.check_mdc_threshold(m["mdc_threshold"], gt, s)
        assert m["n_thresholds"] == h["n_thresholds"], n           # the kept points are roc_curve's
        for k in ("eer_host", "mdc_host"):
            worst[k] = max(worst[k], f[k])
        if f["thr_bound"]:
            worst["thr / bound"] = max(worst["thr / bound"], f["thr"] / f["thr_bound"])
    print(f"metrics-parity (cpu): rule vs host over {MC.NUM_CASES} cases: eer {worst['eer_host']:.2e} (bound "
          f"{MC.EER_BOUND:.0e}); interior threshold at most {worst['thr / bound']:.2f} of its bound; mdc rel "
          f"{worst['mdc_host']:.2e} (bound {MC.MDC_REL:.2e})")


@pytest.mark.parametrize("name", sorted(MC.edge_cases(2048)))
def test_reference_rule_against_the_host_metrics_on_the_edges(name):
    from w2v2_speaker_amd import ops
    gt, s, p_target = MC.edge_cases(ops.SORT_TILE)[name]
    m, h = MC.metrics_ref(gt, s, p_target=p_target), MC.host_metrics(gt, s, p_target=p_target)
    MC.check_against_host({k: m[k] for k in KEYS}, m, h, what=name)
    MC.check_mdc_threshold(m["mdc_threshold"], gt, s, p_target=p_target)
    assert m["n_thresholds"] == h["n_thresholds"]
    if name == "collinear_run":         # more than a tile of dropped points between lo and hi
        assert m["hi"] - m["lo"] > ops.SORT_TILE and m["kind"] == "interior"
    if name.startswith("separated"):
        assert m["eer"] == 0 and m["kind"] == "vertical"
    if name == "separated_first_segment":
        assert (m["lo"], m["hi"]) == (0, 1) and m["eer_threshold"] == np.inf


def test_tie_order_decides_the_min_dcf():
    """The sweep of calculate_mdc attains its minimum inside the tie group at 0.5: the order inside the tie (the stable
    order of the input) decides both the cost and its threshold."""
    for gt, want in zip(MC.TIE_GT, MC.TIE_HOST):
        h = MC.host_metrics(gt, MC.TIE_SCORES, p_target=MC.TIE_P_TARGET)
        m = MC.metrics_ref(gt, MC.TIE_SCORES, p_target=MC.TIE_P_TARGET)
        assert h["mdc"] == pytest.approx(want[0], abs=1e-15) and h["mdc_threshold"] == float(np.float32(want[1]))
        assert abs(m["mdc"] - h["mdc"]) <= MC.MDC_REL * h["mdc"] and m["mdc_threshold"] == h["mdc_threshold"]
    assert sorted(MC.TIE_GT[0]) == sorted(MC.TIE_GT[1])


def test_sort_reference_orders_the_special_values_as_the_contract_says():
    keys = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, -np.nan, 1.0, -0.0], dtype=np.float32)
    keys[5] = np.uint32(0xffc00000).view(np.float32)
    assert MC.sort_ref(keys).tolist() == [4, 1, 2, 7, 6, 3, 0, 5]
    for kind in MC.SORT_KINDS:
        k = MC.sort_keys(kind, 300)
        assert k.dtype == np.float32 and k.shape == (300,)
    full = MC.sort_keys("full_range", 70001)
    bits = full.view(np.uint32)
    assert np.isnan(full[bits >> 31 == 0]).any() and np.isnan(full[bits >> 31 == 1]).any() and np.isinf(full).any()
    assert (bits == 0x80000000).any() and (bits == 0).any() and ((bits & 0x7f800000) == 0).sum() > 2
    assert len({int(b) & 0x00ffffff for b in MC.sort_keys("top_byte", 300).view(np.uint32)}) == 1
    assert len({int(b) >> 8 for b in MC.sort_keys("bottom_byte", 300).view(np.uint32)}) == 1


def _c_decl(hdr: str, name: str):
    """(result, parameter kinds) of ``name`` in the header: 'p' pointer, 'i64', 'i32', 'f32', 'f64'."""
    m = re.search(r"\b(int|int64_t) " + name + r"\(([^;]*?)\);", hdr, re.S)
    assert m, name
    kinds = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        if p == "void":
            continue
        kinds.append("p" if "*" in p else {"int64_t": "i64", "int": "i32", "float": "f32", "double": "f64"}[p.split(" ")[0]])
    return {"int": "i32", "int64_t": "i64"}[m.group(1)], kinds


def test_new_symbols_declared_exported_and_wrapped_with_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32", C.c_double: "f64"}
    for name in ("w2v2_sort_f32_index", "w2v2_trial_metrics", "w2v2_trial_metrics_workspace_bytes",
                 "w2v2_sort_f32_index_workspace_bytes", "w2v2_sort_tile"):
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        res, args = _lib._SIGS[name]
        assert (kind[res], [kind[a] for a in args]) == _c_decl(hdr, name), name
    assert "metrics.hip" in _build.SOURCES
    for cite in ("src/eval_metrics.py:54-79", ":90-206"):
        assert cite in hdr
    lib = _lib.load()
    T = lib.w2v2_sort_tile()
    assert T == ops.SORT_TILE and T % 256 == 0
    sort_b, met_b = lib.w2v2_sort_f32_index_workspace_bytes, lib.w2v2_trial_metrics_workspace_bytes
    # a tile more is a column of the digit x tile table more: 256 counters, beside the keys themselves
    assert sort_b(T + 1) - sort_b(T) >= 256 * 4 > sort_b(T) - sort_b(T - 16) > 0
    for P in (1, T, 579818):
        assert met_b(P) > sort_b(P) >= 16 * P and sort_b(P) % 16 == 0 and met_b(P) % 16 == 0
    assert met_b(579818) < 64 * 579818                         # tens of bytes a trial
    for bad in (0, -1, 2 ** 31):
        assert sort_b(bad) == -1 and met_b(bad) == -1
        with pytest.raises(ValueError, match="outside"):
            ops.trial_metrics_workspace(bad, "cpu")
    assert met_b(2 ** 31 - 1) > 0
    assert list(inspect.signature(ops.sort_f32_index).parameters) == ["keys", "order_out", "keys_out", "workspace"]
    assert list(inspect.signature(ops.trial_metrics).parameters) == ["scores", "labels", "c_miss", "c_fa", "p_target", "out",
                                                                     "workspace"]
    assert list(inspect.signature(ops.trial_metrics_workspace).parameters) == ["P", "device"]
    assert ops.trial_metrics_workspace(1000, "cpu").numel() == met_b(1000)
    assert ops.sort_f32_index_workspace(1000, "cpu").numel() == sort_b(1000)


def test_ops_argument_checks_need_no_device():
    from w2v2_speaker_amd import ops
    s, l = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    for kw, msg in ((dict(c_miss=0.5), "c_miss=0.5 should be >= 1"), (dict(c_fa=0), "c_fa=0 should be >= 1"),
                    (dict(p_target=1.5), "p_target=1.5 should be between 0 and 1"),
                    (dict(p_target=-0.1), "p_target=-0.1 should be between 0 and 1")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            ops.trial_metrics(s, l, **kw)
    for bad_s, bad_l in ((s.double(), l), (s, l.int()), (s[:0], l[:0]), (s, l[:3]), (torch.zeros(8)[::2], l),
                         (s.reshape(2, 2), l)):
        with pytest.raises(ValueError, match="trial_metrics"):
            ops.trial_metrics(bad_s, bad_l)
    with pytest.raises(ValueError, match="out is"):
        ops.trial_metrics(s, l, out=torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.trial_metrics(s, l)
    for bad in (s.double(), s[:0], torch.zeros(8)[::2], s.reshape(2, 2)):
        with pytest.raises(ValueError, match="sort_f32_index"):
            ops.sort_f32_index(bad)
    with pytest.raises(ValueError, match="order_out"):
        ops.sort_f32_index(s, order_out=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="keys_out"):
        ops.sort_f32_index(s, keys_out=torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sort_f32_index(s)


def test_metrics_argument_of_the_evaluator_and_of_the_modules():
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import CosineDistanceEvaluator, EvaluationPair
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import TrialIndex, score_trials_device
    from w2v2_speaker_amd.lightning_modules.speaker._optim_surface import EmbeddingEvaluation
    pairs, keys, bank = [EvaluationPair(True, "a", "b")], ["a", "b"], torch.zeros(2, 4)
    ev = CosineDistanceEvaluator()
    assert inspect.signature(ev.evaluate_bank_metrics).parameters["metrics"].default == "host"
    assert "metrics" not in inspect.signature(ev.evaluate_bank).parameters      # evaluate_bank is as it was: the host metrics
    with pytest.raises(ValueError, match="metrics='gpu'"):
        ev.evaluate_bank_metrics(pairs, keys, bank, metrics="gpu")
    with pytest.raises(NotImplementedError, match="combined on the host in the reference's Python-float order"):
        ev.evaluate_bank_metrics(pairs, keys, [bank, bank], metrics="device")
    with pytest.raises(NotImplementedError, match="combined on the host"):
        score_trials_device([bank, bank], TrialIndex(pairs, keys), keep_on_device=True)
    sig = inspect.signature(EmbeddingEvaluation.evaluate_trials).parameters
    assert sig["metrics"].default == "host" and sig["scoring"].default == "host"

    class Stub(EmbeddingEvaluation):
        def compute_speaker_embeddings(self, *a, **k):
            raise AssertionError("the arguments are checked before anything is embedded")
    with pytest.raises(ValueError, match="metrics='device' needs scoring='device'"):
        Stub().evaluate_trials(pairs, {}, metrics="device")
    with pytest.raises(ValueError, match="metrics='gpu'"):
        Stub().evaluate_trials(pairs, {}, scoring="device", metrics="gpu")
    # labels of a trial list: uint8, one per trial, cached per device
    idx = TrialIndex.from_rows([(0, 1), (1, 0), (0, 0)], [1, 0, 1], 2)
    lab = idx.device_labels("cpu")
    assert lab.dtype == torch.uint8 and lab.tolist() == [1, 0, 1] and idx.device_labels("cpu") is lab
    with pytest.raises(ValueError, match="not in the bank"):
        TrialIndex([EvaluationPair(True, "a", "zz")], keys).device_labels("cpu")
