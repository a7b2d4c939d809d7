"""CPU test of the argument checks that the evaluation wrappers of ops.py share: the ``pairs`` table, the mean / std pair,
the detection costs, the optional outputs and the one-label-per-trial rule.  Every wrapper that takes one of them is fed one
malformed value of it and must raise a ValueError that starts with the wrapper's own name -- for the costs, with the message
of the reference's calculate_mdc.  All of these checks run before the device check, so no library is loaded.  (The float32
outputs of embed_stats, score_pairs, score_frame_sets, rows_transform, topk_stats, score_pairs_norm and plda_score_pairs are
checked behind the device check: test_scoring_gpu.py, test_score_norm_gpu.py and test_backend_gpu.py reach those.)"""
import pytest
import torch

N, D, P = 8, 16, 5


def _bank(rows=N):
    return torch.zeros(rows, D)


def _pairs():
    return torch.zeros(P, 2, dtype=torch.int32)


def _f64(n):
    return torch.zeros(n, dtype=torch.float64)


def _scores():
    return torch.zeros(P)


def _labels(n=P):
    return torch.zeros(n, dtype=torch.uint8)


BAD_PAIRS = {"int64": lambda: torch.zeros(P, 2, dtype=torch.int64), "three columns": lambda: torch.zeros(P, 3, dtype=torch.int32),
             "one-dimensional": lambda: torch.zeros(2 * P, dtype=torch.int32), "empty": lambda: torch.zeros(0, 2, dtype=torch.int32),
             "strided": lambda: torch.zeros(P, 4, dtype=torch.int32)[:, ::2], "a list": lambda: [[0, 1]]}
BAD_CENTRING = {"mean alone": lambda: (torch.zeros(D), None), "std alone": lambda: (None, torch.ones(D)),
                "float64": lambda: (torch.zeros(D, dtype=torch.float64), torch.ones(D)),
                "short": lambda: (torch.zeros(D), torch.ones(D - 4)), "strided": lambda: (torch.zeros(2 * D)[::2], torch.ones(D))}
BAD_COSTS = {"c_miss=0.5 should be >= 1": dict(c_miss=0.5), "c_fa=0 should be >= 1": dict(c_fa=0),
             "p_target=1.5 should be between 0 and 1": dict(p_target=1.5),
             "p_target=-0.1 should be between 0 and 1": dict(p_target=-0.1)}
OPEN_PRIOR = {"p_target=0 should be strictly between 0 and 1": dict(p_target=0),
              "p_target=1 should be strictly between 0 and 1": dict(p_target=1)}

CASES = []
for _name, _bad in BAD_PAIRS.items():
    CASES += [("score_pairs", f"pairs {_name}", lambda ops, b=_bad: ops.score_pairs(_bank(), b()), "score_pairs: pairs is"),
              ("score_pairs_norm", f"pairs {_name}",
               lambda ops, b=_bad: ops.score_pairs_norm(_scores(), b(), torch.zeros(N), torch.ones(N)), "score_pairs_norm: pairs is"),
              ("plda_score_pairs", f"pairs {_name}", lambda ops, b=_bad: ops.plda_score_pairs(_bank(), b(), _f64(D), _f64(D), 0.0),
               "plda_score_pairs: pairs is")]
for _name, _bad in BAD_CENTRING.items():
    CASES += [("score_pairs", f"centring {_name}", lambda ops, b=_bad: ops.score_pairs(_bank(), _pairs(), *b()), "score_pairs: mean"),
              ("rows_transform", f"centring {_name}", lambda ops, b=_bad: ops.rows_transform(_bank(), *b()), "rows_transform: mean"),
              ("cohort_stats", f"centring {_name}", lambda ops, b=_bad: ops.cohort_stats(_bank(), _bank(4), 2, *b()),
               "cohort_stats: mean")]
for _msg, _kw in BAD_COSTS.items():
    CASES += [("trial_metrics", _msg, lambda ops, kw=_kw: ops.trial_metrics(_scores(), _labels(), **kw), _msg),
              ("calib_fit", _msg, lambda ops, kw=_kw: ops.calib_fit(_scores(), _labels(), **kw), _msg),
              ("llr_metrics", _msg, lambda ops, kw=_kw: ops.llr_metrics(_scores(), _labels(), **kw), _msg)]
for _msg, _kw in OPEN_PRIOR.items():
    CASES.append(("calib_fit", _msg, lambda ops, kw=_kw: ops.calib_fit(_scores(), _labels(), **kw), _msg))
CASES += [
    ("sort_f32_index", "order_out int64", lambda ops: ops.sort_f32_index(_scores(), order_out=torch.zeros(P, dtype=torch.int64)),
     "sort_f32_index: order_out is"),
    ("sort_f32_index", "order_out short", lambda ops: ops.sort_f32_index(_scores(), order_out=torch.zeros(P - 1, dtype=torch.int32)),
     "sort_f32_index: order_out is"),
    ("sort_f32_index", "keys_out float64", lambda ops: ops.sort_f32_index(_scores(), keys_out=_f64(P)), "sort_f32_index: keys_out is"),
    ("sort_f32_index", "keys_out strided", lambda ops: ops.sort_f32_index(_scores(), keys_out=torch.zeros(2 * P)[::2]),
     "sort_f32_index: keys_out is"),
    ("trial_metrics", "out float32", lambda ops: ops.trial_metrics(_scores(), _labels(), out=torch.zeros(8)), "trial_metrics: out is"),
    ("trial_metrics", "out short", lambda ops: ops.trial_metrics(_scores(), _labels(), out=_f64(7)), "trial_metrics: out is"),
    ("calib_fit", "record float32", lambda ops: ops.calib_fit(_scores(), _labels(), record=torch.zeros(ops.CALIB_RECORD_DOUBLES)),
     "calib_fit: record is"),
    ("calib_fit", "record short", lambda ops: ops.calib_fit(_scores(), _labels(), record=_f64(ops.CALIB_RECORD_DOUBLES - 1)),
     "calib_fit: record is"),
    ("calib_fit", "record a list", lambda ops: ops.calib_fit(_scores(), _labels(), record=[0.0] * ops.CALIB_RECORD_DOUBLES),
     "calib_fit: record is"),
    ("calib_apply", "out float64", lambda ops: ops.calib_apply(_scores(), _f64(2), out=_f64(P)), "calib_apply: out is"),
    ("calib_apply", "out short", lambda ops: ops.calib_apply(_scores(), _f64(2), out=torch.zeros(P - 1)), "calib_apply: out is"),
    ("llr_metrics", "out float32", lambda ops: ops.llr_metrics(_scores(), _labels(), out=torch.zeros(8)), "llr_metrics: out is"),
    ("llr_metrics", "out strided", lambda ops: ops.llr_metrics(_scores(), _labels(), out=_f64(16)[::2]), "llr_metrics: out is"),
    ("trial_metrics", "labels short", lambda ops: ops.trial_metrics(_scores(), _labels(P - 1)), "trial_metrics: one label per"),
    ("calib_fit", "labels short", lambda ops: ops.calib_fit(_scores(), _labels(P - 1)), "calib_fit: one label per"),
    ("llr_metrics", "labels short", lambda ops: ops.llr_metrics(_scores(), _labels(P - 1)), "llr_metrics: one label per"),
    ("trial_metrics", "labels int32", lambda ops: ops.trial_metrics(_scores(), torch.zeros(P, dtype=torch.int32)),
     "trial_metrics: labels is"),
    ("calib_fit", "labels int32", lambda ops: ops.calib_fit(_scores(), torch.zeros(P, dtype=torch.int32)), "calib_fit: labels is"),
    ("llr_metrics", "labels int32", lambda ops: ops.llr_metrics(_scores(), torch.zeros(P, dtype=torch.int32)), "llr_metrics: labels is"),
]


@pytest.mark.parametrize("wrapper,what,call,starts", CASES, ids=[f"{c[0]}-{c[1]}".replace(" ", "_") for c in CASES])
def test_shared_argument_checks_name_their_wrapper(wrapper, what, call, starts):
    from w2v2_speaker_amd import ops
    assert hasattr(ops, wrapper)
    with pytest.raises(ValueError) as e:
        call(ops)
    assert str(e.value).startswith(starts), str(e.value)
