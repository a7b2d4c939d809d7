"""Paired-input evaluation at unequal lengths, host side: the oracle's paired path against the reference golden, the trial
bucketing, the module's _evaluate and the new C-ABI symbol (no GPU needed)."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from oracle import w2v2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_pairs():
    """The four pairs of g20_paired_varlen.npz: ([left waveform [1, n]], [right], golden)."""
    g = np.load(os.path.join(GOLDEN, "g20_paired_varlen.npz"))
    wl, _ = O.synth_batch(4, 26000, 2, seed=21)
    wr, _ = O.synth_batch(4, 26000, 2, seed=22)
    left = [wl[b:b + 1, 0, :int(n)] for b, n in enumerate(g["left_lengths"])]
    right = [wr[b:b + 1, 0, :int(n)] for b, n in enumerate(g["right_lengths"])]
    return left, right, g


def oracle_pair_hidden(a, b, sd, ocfg, cls_c=1.0, sep_c=-1.0):
    """last_hidden_state of O.paired_equality_scores' sequence (the function itself returns the logits only)."""
    f1 = O.feature_projection(O.feature_extractor(a, sd, ocfg).transpose(1, 2), sd, ocfg)
    f2 = O.feature_projection(O.feature_extractor(b, sd, ocfg).transpose(1, 2), sd, ocfg)
    tok = lambda c: torch.full((a.shape[0], 1, f1.shape[2]), float(c), dtype=f1.dtype)
    return O.encoder(torch.cat([tok(cls_c), f1, tok(sep_c), f2, tok(sep_c)], dim=1), sd, ocfg)


def test_oracle_paired_path_matches_reference_golden_at_unequal_lengths():
    ocfg = O.OracleConfig.tiny()
    sd = O.make_state_dict(ocfg, 20211)
    left, right, g = golden_pairs()
    assert [int(n) for n in g["left_lengths"]] == [4000, 400, 2500, 26000]
    assert [int(n) for n in g["right_lengths"]] == [400, 4000, 3217, 26000]
    H = ocfg.hidden_size
    eye, zero = torch.eye(H), torch.zeros(H)
    with torch.no_grad():
        for b, (a, c) in enumerate(zip(left, right)):
            tok0 = O.paired_equality_scores(a, c, sd, ocfg, eye, zero)       # identity "linear": token 0 itself
            err = rel_l2(tok0[0], g["token0"][b])
            print(f"pair {b}: token 0 rel-L2 vs reference {err:.3e}")
            assert err < 2e-5, (b, err)
            if b == 2:
                h = oracle_pair_hidden(a, c, sd, ocfg)
                assert h.shape[1:] == g["pair2.last_hidden_state"].shape
                assert torch.allclose(h[:, 0], tok0, rtol=0, atol=1e-6)      # the helper is the function's sequence
                err = rel_l2(h[0], g["pair2.last_hidden_state"])
                print(f"pair 2: last_hidden_state rel-L2 vs reference {err:.3e}")
                assert err < 2e-5, err


@pytest.mark.parametrize("quantum,budget,max_batch", [(100, 66 * 301, 64), (50, 66 * 301, 64), (7, 900, 5), (1, 400, 3)])
def test_plan_pair_batches(quantum, budget, max_batch):
    from w2v2_speaker_amd.eval_batching import plan_batches, plan_pair_batches
    r = random.Random(5)
    left = [r.randint(1, 999) for _ in range(300)] + [1, 1, 2000]
    right = [r.randint(1, 999) for _ in range(300)] + [1, 999, 2000]
    out = plan_pair_batches(left, right, quantum, budget, max_batch)
    seen = [i for idx, _, _ in out for i in idx]
    assert sorted(seen) == list(range(len(left)))             # every trial exactly once
    for idx, padded, batch in out:
        assert padded % quantum == 0 and 1 <= len(idx) <= batch <= max_batch
        assert batch == 1 or batch * padded <= budget
        assert all(padded >= left[i] + right[i] + 3 for i in idx)
    assert plan_pair_batches(left, right, quantum, budget, max_batch) == out          # deterministic
    assert out == plan_batches([a + b + 3 for a, b in zip(left, right)], quantum, budget, max_batch)


def test_plan_pair_batches_defaults_and_errors():
    from w2v2_speaker_amd import eval_batching as E
    assert E.DEFAULT_PAIR_QUANTUM == 100 and E.DEFAULT_MAX_PAIR_BATCH_FRAMES == 66 * 301
    assert E.plan_pair_batches([149] * 70, [149] * 70)[0][1:] == (400, 49)
    for bad in (dict(quantum=0), dict(max_batch_frames=0), dict(max_batch=-1)):
        with pytest.raises(ValueError):
            E.plan_pair_batches([3], [4], **bad)
    with pytest.raises(ValueError):
        E.plan_pair_batches([0], [4])
    with pytest.raises(ValueError):
        E.plan_pair_batches([3, 4], [4])


def test_evaluate_matches_oracle_metrics_and_nan_rule():
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_paired_input import Wav2vec2PairedSpeakerModule as M
    r = np.random.default_rng(11)
    label = (r.random(200) < 0.4).astype(np.int64)
    logits = r.standard_normal(200) * 1.5 + (2 * label - 1) * 0.8
    # the shapes the step hooks return: [B, 1] logits per batch, a list of labels; and a bare int / float
    outputs = [{"prediction": logits[i:i + 8, None].tolist(), "label": label[i:i + 8].tolist()} for i in range(0, 192, 8)]
    outputs += [{"prediction": float(logits[i]), "label": int(label[i])} for i in range(192, 200)]
    got = M._evaluate(outputs)
    assert set(got) == {"eer", "eer_threshold", "mdc", "mdc_threshold"}
    scores = np.clip((logits + 1) / 2, 0, 1)
    eer, thr = O.calculate_eer(label, scores)
    mdc, mthr = O.calculate_mdc(label, scores)
    assert got["eer"] == pytest.approx(eer, abs=1e-12) and got["eer_threshold"] == pytest.approx(thr, abs=1e-12)
    assert got["mdc"] == pytest.approx(mdc, abs=1e-12) and got["mdc_threshold"] == pytest.approx(mthr, abs=1e-12)
    assert 0.0 < got["eer"] < 0.5
    nan = M._evaluate([{"prediction": [[float("nan")]] * 6, "label": [0, 1, 0, 1, 1, 0]}])
    assert nan["eer"] == 1


def test_pair_assemble_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _lib, ops
    assert "int w2v2_pair_assemble(" in hdr
    assert "w2v2_pair_assemble" in _lib._SIGS and len(_lib._SIGS["w2v2_pair_assemble"][1]) == 13
    assert callable(ops.pair_assemble)
    assert hasattr(_lib.load(), "w2v2_pair_assemble")


def test_pair_tables_validation_is_host_only():
    from w2v2_speaker_amd import ops
    t = ops.pair_tables([0, 5], [3, 1], [3, 0], torch.tensor([2, 5]), rows=6, T=11)
    assert t.dtype == torch.int32 and t.tolist() == [[0, 5], [3, 1], [3, 0], [2, 5]]
    for bad in (([0], [0], [1], [1]), ([0], [5], [0], [4]), ([4], [3], [0], [1]), ([0], [1], [-1], [1]), ([0], [1], [0], [1, 1])):
        with pytest.raises(ValueError):
            ops.pair_tables(*bad, rows=6, T=11)
