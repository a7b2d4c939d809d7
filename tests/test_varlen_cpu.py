"""Batched variable-length evaluation, host side: the length-bucketing planner, the length validation of
Plan.forward(lengths=) and the new C-ABI symbols (no GPU needed)."""
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["w2v2_conv0_stats_len", "w2v2_conv0_stats_mfma_len", "w2v2_posconv_regroup_len", "w2v2_softmax_fwd_len",
               "w2v2_attention_fwd_len", "w2v2_pool_fwd_len"]


def _lengths(n=300, seed=3):
    r = random.Random(seed)
    return [r.randint(4 * 16000, 20 * 16000) for _ in range(n)]


@pytest.mark.parametrize("quantum,budget,max_batch", [(32000, 66 * 48000, 64), (16000, 66 * 48000, 64),
                                                      (8000, 10 * 48000, 7), (1, 200000, 3)])
def test_plan_batches_covers_every_index_within_budget_and_quantum(quantum, budget, max_batch):
    from w2v2_speaker_amd.eval_batching import plan_batches
    lens = _lengths() + [250000, 400, 401, 320000]
    out = plan_batches(lens, quantum, budget, max_batch)
    seen = [i for idx, _, _ in out for i in idx]
    assert sorted(seen) == list(range(len(lens)))            # every index exactly once
    shapes = {}
    for idx, n, batch in out:
        assert n % quantum == 0 and 1 <= len(idx) <= batch <= max_batch
        assert batch == 1 or batch * n <= budget
        assert all(lens[i] <= n < lens[i] + quantum for i in idx)
        shapes.setdefault(n, set()).add(batch)
    assert all(len(b) == 1 for b in shapes.values())          # one plan shape per bucket
    pads = [n for _, n, _ in out]
    assert pads == sorted(pads)                               # buckets in length order: each plan built once
    # scattering the batches' rows back by index restores input order
    back = [None] * len(lens)
    for idx, n, _ in out:
        for i in idx:
            back[i] = lens[i]
    assert back == lens
    assert plan_batches(lens, quantum, budget, max_batch) == out          # deterministic


def test_plan_batches_long_utterance_runs_alone_and_defaults():
    from w2v2_speaker_amd.eval_batching import DEFAULT_MAX_BATCH_SAMPLES, min_samples, plan_batches
    from w2v2_speaker_amd.config import W2V2Config
    assert DEFAULT_MAX_BATCH_SAMPLES == 66 * 48000
    out = plan_batches([5_000_000, 16000, 16000], 16000, 1_000_000, 64)
    assert out[-1] == ((0,), 5_008_000, 1)
    assert out[0] == ((1, 2), 16000, 62)
    cfg = W2V2Config()
    assert min_samples(cfg.conv_kernel, cfg.conv_stride) == 400
    assert cfg.num_frames(400) == 1 and cfg.conv_lengths(399)[-1] < 1
    with pytest.raises(ValueError):
        plan_batches([0, 5], 16000, 1000, 4)


@pytest.mark.parametrize("feature_dims", [(), (3,)])
def test_padded_batches_fill_the_planned_batches(feature_dims):
    """1-D waveforms and [T, 3] features: every utterance sits in exactly one (batch, row), zero-padded to the planned
    length; unused rows are all zero and carry the fill length."""
    import torch
    from w2v2_speaker_amd.eval_batching import padded_batches, plan_batches
    lens, quantum, cap, max_batch, fill = [5, 12, 7, 12, 3], 4, 24, 2, 2
    g = torch.Generator().manual_seed(11)
    utts = [torch.rand(n, *feature_dims, generator=g) + 0.5 for n in lens]          # no zero inside an utterance
    planned = plan_batches(lens, quantum, cap, max_batch)
    got = list(padded_batches(utts, quantum, cap, max_batch, fill, "cpu"))
    assert len(got) == len(planned) >= 2
    placed, unused_rows = [], 0
    for (idx, padded, row_lens), (pidx, n, batch) in zip(got, planned):
        assert tuple(idx) == pidx and padded.shape == (batch, n) + feature_dims and padded.dtype == torch.float32
        assert len(row_lens) == batch == max_batch
        for j in range(batch):
            if j < len(idx):
                u = utts[idx[j]]
                assert row_lens[j] == lens[idx[j]] == u.shape[0]
                assert torch.equal(padded[j, :u.shape[0]], u) and not padded[j, u.shape[0]:].any()
                placed.append(idx[j])
            else:
                assert row_lens[j] == fill and not padded[j].any()
                unused_rows += 1
    assert sorted(placed) == list(range(5)) and len(placed) == 5        # a permutation of the inputs
    assert unused_rows == 1                                             # the bucket of the 3-sample utterance


def test_length_validation_errors():
    import torch
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.engine import valid_lengths
    cfg = W2V2Config()
    assert valid_lengths(cfg, [48000, 400], 2, 48000) == [48000, 400]
    assert valid_lengths(cfg, torch.tensor([48000, 1000]), 2, 48000) == [48000, 1000]
    with pytest.raises(ValueError):
        valid_lengths(cfg, [48001, 400], 2, 48000)            # longer than the plan
    with pytest.raises(ValueError):
        valid_lengths(cfg, [48000, 399], 2, 48000)            # no encoder frame
    with pytest.raises(ValueError):
        valid_lengths(cfg, [48000], 2, 48000)                 # one per row
    with pytest.raises(ValueError):
        valid_lengths(cfg, torch.tensor([1.0, 2.0]), 2, 48000)


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _lib
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in hdr, name
        assert name in _lib._SIGS, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
