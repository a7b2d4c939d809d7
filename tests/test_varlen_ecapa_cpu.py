"""Batched variable-length evaluation of ECAPA-TDNN, host side: the minimum utterance length, the validation of
EcapaPlan.embed(lengths=), the frame-bucket policy and the new C-ABI symbols (no GPU needed)."""
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["w2v2_im2col_reflect_len", "w2v2_im2col_reflect_sum_len", "w2v2_asp_context_len", "w2v2_asp_pool_fwd_len"]


def test_ecapa_min_frames():
    from w2v2_speaker_amd.ecapa import EcapaConfig, ecapa_min_frames
    assert ecapa_min_frames(EcapaConfig()) == 5               # k = 3, dilation 4: pad 4, and reflect needs pad < length
    assert ecapa_min_frames(EcapaConfig.tiny()) == 5          # the tiny model keeps the kernel sizes and dilations
    assert ecapa_min_frames(EcapaConfig(kernel_sizes=(5, 3, 3, 3, 1), dilations=(4, 2, 3, 4, 1))) == 9
    assert ecapa_min_frames(EcapaConfig(kernel_sizes=(1, 1, 1, 1, 1), dilations=(1, 1, 1, 1, 1))) == 1
    # torch's own rule for the same padding: F.pad(mode="reflect") accepts pad < length only
    import torch
    x = torch.zeros(1, 1, 5)
    torch.nn.functional.pad(x, (4, 4), mode="reflect")
    with pytest.raises(RuntimeError):
        torch.nn.functional.pad(x[:, :, :4], (4, 4), mode="reflect")


def test_frame_length_validation_errors():
    import torch
    from w2v2_speaker_amd.ecapa import EcapaConfig, valid_frame_lengths
    cfg = EcapaConfig()
    assert valid_frame_lengths(cfg, [300, 5], 2, 300) == [300, 5]
    assert valid_frame_lengths(cfg, torch.tensor([300, 17]), 2, 300) == [300, 17]
    with pytest.raises(ValueError):
        valid_frame_lengths(cfg, [301, 5], 2, 300)            # longer than the plan
    with pytest.raises(ValueError):
        valid_frame_lengths(cfg, [300, 4], 2, 300)            # shorter than the widest reflect padding allows
    with pytest.raises(ValueError):
        valid_frame_lengths(cfg, [300], 2, 300)               # one per row
    with pytest.raises(ValueError):
        valid_frame_lengths(cfg, torch.tensor([1.0, 2.0]), 2, 300)


def test_frame_bucket_policy_with_the_frame_defaults():
    from w2v2_speaker_amd.eval_batching import (DEFAULT_FRAME_QUANTUM, DEFAULT_MAX_BATCH, DEFAULT_MAX_BATCH_FRAMES,
                                                plan_batches)
    assert (DEFAULT_FRAME_QUANTUM, DEFAULT_MAX_BATCH_FRAMES, DEFAULT_MAX_BATCH) == (200, 66 * 300, 64)
    r = random.Random(20240)
    lens = [r.randint(400, 2000) for _ in range(512)] + [5, 200, 201, 30000]
    out = plan_batches(lens, DEFAULT_FRAME_QUANTUM, DEFAULT_MAX_BATCH_FRAMES, DEFAULT_MAX_BATCH)
    assert sorted(i for idx, _, _ in out for i in idx) == list(range(len(lens)))      # every index exactly once
    for idx, n, batch in out:
        assert n % DEFAULT_FRAME_QUANTUM == 0 and 1 <= len(idx) <= batch <= DEFAULT_MAX_BATCH
        assert batch == 1 or batch * n <= DEFAULT_MAX_BATCH_FRAMES                    # no batch over budget
        assert all(lens[i] <= n < lens[i] + DEFAULT_FRAME_QUANTUM for i in idx)
    assert out[-1] == ((len(lens) - 1,), 30000, 1)            # longer than the budget: alone
    assert len({(n, b) for _, n, b in out}) <= 2000 // DEFAULT_FRAME_QUANTUM + 2      # one plan shape per bucket


def test_module_signature_defaults():
    import inspect
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTdnnModule
    p = inspect.signature(EcapaTdnnModule.compute_speaker_embeddings).parameters
    assert (p["quantum"].default, p["max_batch_frames"].default, p["max_batch"].default) == (200, 66 * 300, 64)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("quantum", "max_batch_frames", "max_batch"))
    assert hasattr(EcapaTdnnModule, "evaluate_trials")


def test_new_symbols_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _lib, ops
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in hdr, name
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for fn in ("im2col_reflect_len", "asp_context_len", "asp_pool_fwd_len"):
        assert callable(getattr(ops, fn)), fn
