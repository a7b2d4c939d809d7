"""Host side of the triplet losses (no GPU needed): the triplet draw and the batch processor against what the reference
itself produced (tests/golden/g21_triplet.*, written by tests/golden/make_triplet_goldens.py), the float64 restatement
of tests/triplet_cases.py against the reference's losses and autograd gradients, the fairness of the GPU cases to f32,
the new C-ABI symbol, and the constructor errors of the module that fire before any device allocation."""
import inspect
import json
import os
import random

import numpy as np
import pytest
import torch

import triplet_cases as TC
from test_fbank_cpu import _c_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64


def golden():
    z = np.load(os.path.join(GOLDEN, "g21_triplet.npz"))
    with open(os.path.join(GOLDEN, "g21_triplet.json")) as f:
        return z, json.load(f)


def rel(got, ref):
    got, ref = torch.as_tensor(got, dtype=F64), torch.as_tensor(ref, dtype=F64)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def test_sample_triplets_reproduces_the_reference_draws():
    from w2v2_speaker_amd.heads import sample_triplets
    z, meta = golden()
    assert len(meta["seeds"]) == 3
    for seed in meta["seeds"]:
        random.seed(seed)
        pos, neg = sample_triplets(z[f"s{seed}_label"].tolist())
        assert pos == z[f"s{seed}_pos"].tolist() and neg == z[f"s{seed}_neg"].tolist(), seed
        # a private generator gives the same draws and leaves the global one alone
        state = random.getstate()
        assert sample_triplets(z[f"s{seed}_label"].tolist(), rng=random.Random(seed)) == (pos, neg)
        assert random.getstate() == state


def test_sample_triplets_rejects_batches_without_triplets():
    from w2v2_speaker_amd.heads import sample_triplets
    with pytest.raises(ValueError, match="occur once"):
        sample_triplets([0, 0, 1, 1, 2])            # a singleton label: no positive
    with pytest.raises(ValueError, match="single speaker"):
        sample_triplets([3, 3, 3, 3])               # one speaker: no negative
    pos, neg = sample_triplets([0, 1, 0, 1], rng=random.Random(0))
    assert pos == [2, 3, 0, 1] and all(n % 2 != i % 2 for i, n in enumerate(neg))


def test_float64_restatement_reproduces_the_reference_losses_and_gradients():
    z, meta = golden()
    for seed in meta["seeds"]:
        emb, pos, neg = torch.from_numpy(z[f"s{seed}_emb"]), z[f"s{seed}_pos"].tolist(), z[f"s{seed}_neg"].tolist()
        label, logits = torch.from_numpy(z[f"s{seed}_label"]), torch.from_numpy(z[f"s{seed}_logits"])
        for m in meta["margins"]:
            r = TC.triplet_ref(emb, pos, neg, m)
            assert abs(float(r["loss"]) - float(z[f"s{seed}_loss_m{m}"])) <= 1e-12 * abs(float(z[f"s{seed}_loss_m{m}"]))
            assert rel(r["demb"], z[f"s{seed}_demb_m{m}"]) < 1e-12, (seed, m)
        for c_ce, c_t in meta["coefs"]:
            r = TC.triplet_ref(emb, pos, neg, 1.0, coef=c_t)
            lg = logits.clone().requires_grad_(True)
            ce = torch.nn.functional.cross_entropy(lg, label)
            ce.backward()
            want = float(z[f"s{seed}_loss_ce{c_ce}{c_t}"])
            assert abs(c_ce * float(ce.detach()) + c_t * float(r["loss"]) - want) <= 1e-12 * abs(want)
            assert rel(r["demb"], z[f"s{seed}_demb_ce{c_ce}{c_t}"]) < 1e-12
            assert rel(c_ce * lg.grad, z[f"s{seed}_dlogits_ce{c_ce}{c_t}"]) < 1e-12


def all_cases():
    for B, E in TC.SHAPES:
        yield f"shape {B}x{E}", TC.shape_case(B, E)
    yield "fan-in", TC.fan_in_case()
    yield "all-inactive", TC.all_inactive_case()


def test_cases_keep_every_hinge_away_from_zero_and_are_fair_to_f32():
    """Every GPU case (built here exactly as the GPU tests build it): no row within HINGE_GAP of its hinge at either margin,
    and the kernel's arithmetic restated in f32 on the CPU stays inside the GPU bounds, so a miss on the GPU is the
    kernel's."""
    n = 0
    for name, (emb, pos, neg) in all_cases():
        for m in TC.MARGINS:
            ref = TC.triplet_ref(emb, pos, neg, m)
            assert float(ref["v"].abs().min()) > TC.HINGE_GAP, (name, m)
            e = TC.errors(TC.triplet_ref(emb, pos, neg, m, dtype=torch.float32), ref)
            print(f"triplet-parity: f32 restatement, {name} margin {m}: " +
                  ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in e.items()))
            assert TC.within_bounds(e), (name, m, e)
            n += 1
    assert n == 2 * (len(TC.SHAPES) + 2)
    emb, pos, neg = TC.all_inactive_case()
    ref = TC.triplet_ref(emb, pos, neg, 1.0)
    assert float(ref["loss"]) == 0.0 and float(ref["demb"].abs().max()) == 0.0


def test_reference_treats_a_hinge_at_zero_as_active():
    """torch's clamp_min backward passes the gradient where the input EQUALS the bound: the kernel's `>= 0`."""
    x = torch.tensor([-1.0, 0.0, 1.0], requires_grad=True)
    x.clamp_min(0).sum().backward()
    assert x.grad.tolist() == [0.0, 1.0, 1.0]


def stream(n_speakers, per_speaker, seq, seed):
    from w2v2_speaker_amd.data import SpeakerClassificationDataSample
    return TC.sample_stream(SpeakerClassificationDataSample, n_speakers, per_speaker, seq, seed)


def test_triplet_batch_processor_reproduces_the_reference_batches():
    from w2v2_speaker_amd.data import TripletSpeakerBatchProcessor
    _, meta = golden()
    assert len(meta["batch_processor"]) == 3 and any(c["ensure"] for c in meta["batch_processor"])
    for c in meta["batch_processor"]:
        random.seed(c["seed"])
        bp = TripletSpeakerBatchProcessor(c["max_batch_size"], c["max_queue_size"], ensure_all_samples_seen=c["ensure"])
        got = list(bp(stream(c["n_speakers"], c["per_speaker"], c["seq"], c["seed"])))
        assert [list(b.keys) for b in got] == c["batches"], c["seed"]
        for b, keys in zip(got, c["batches"]):
            assert b.ground_truth.tolist() == [int(k[2:5]) for k in keys]
        if c["ensure"]:       # the drain hands out every sample; its batches need not hold pairs
            assert sum(len(b) for b in c["batches"]) == c["n_speakers"] * c["per_speaker"]
            assert any(len(set(b.ground_truth.tolist())) * 2 != len(b.keys) for b in got)
        else:                 # every batch: anchor and positive of each of its speakers, side by side
            for b in got:
                gt = b.ground_truth.tolist()
                assert gt[0::2] == gt[1::2] and len(set(gt[0::2])) == len(gt) // 2 >= 2


def test_triplet_batch_processor_errors():
    from w2v2_speaker_amd.data import ShardDataset, TripletSpeakerBatchProcessor
    with pytest.raises(ValueError, match="even"):
        TripletSpeakerBatchProcessor(7, 32)
    bp = TripletSpeakerBatchProcessor(4, 3)          # six singleton speakers fill 2 * max_queue_size without a triplet
    with pytest.raises(ValueError, match="queue size"):
        list(bp(stream(8, 1, 1, 0)))
    with pytest.raises(ValueError, match="already been loaded"):
        list(TripletSpeakerBatchProcessor(4, 32)(list(stream(2, 2, 2, 0))[:1] * 2))
    assert isinstance(ShardDataset([], 4, batch_processing_mode="categorical_triplets").batcher, TripletSpeakerBatchProcessor)
    assert not isinstance(ShardDataset([], 4).batcher, TripletSpeakerBatchProcessor)
    with pytest.raises(ValueError, match="batch_processing_mode"):
        ShardDataset([], 4, batch_processing_mode="triplets")


def test_new_symbol_declared_exported_and_wrapped_with_a_matching_signature():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _lib, ops
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32"}
    name = "w2v2_triplet_fwd_bwd"
    assert name in _lib._SIGS and name in _lib.EXPORTS
    res, args = _lib._SIGS[name]
    assert res is C.c_int32 and [kind[a] for a in args] == _c_params(hdr, name)
    assert hasattr(_lib.load(), name)
    params = list(inspect.signature(ops.triplet_fwd_bwd).parameters)
    assert params == ["emb", "pos", "neg", "d_ap", "d_an", "loss_rows", "demb", "B", "E", "margin", "coef", "accumulate",
                      "loss_scale", "ld"]


def test_loss_modules_keep_the_reference_surface():
    from w2v2_speaker_amd.optim.loss import CrossEntropyLoss, TripletCrossEntropyLoss, TripletLoss
    assert TripletLoss().margin == 1 and TripletLoss(margin=0.3).margin == 0.3
    both = TripletCrossEntropyLoss()
    assert (both.c_ce, both.c_triplet, both.margin) == (1, 1, 1)
    assert isinstance(both, TripletLoss) and isinstance(both, CrossEntropyLoss)
    assert TripletCrossEntropyLoss(3, 2).c_ce == 3
    for bad in ((0, 1), (1, 0.5)):
        with pytest.raises(ValueError, match="at least 1"):
            TripletCrossEntropyLoss(*bad)
    TripletLoss.verify_labels([0, 0, 1, 1])
    with pytest.raises(AssertionError):
        TripletLoss.verify_labels([0, 0, 1])
    assert list(inspect.signature(TripletLoss.forward).parameters) == ["self", "embeddings", "label_indexes"]
    assert list(inspect.signature(TripletCrossEntropyLoss.forward).parameters) == ["self", "embeddings", "logits",
                                                                                   "label_indexes"]


def test_module_constructor_errors_fire_before_any_device_allocation():
    """The limits of the triplet modes: all raised from the configuration alone (device="cpu" never gets as far as an
    arena here)."""
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    from w2v2_speaker_amd.optim.loss import TripletCrossEntropyLoss
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: W2V2Config.tiny())
    mk = lambda loss, **kw: Wav2vec2FCModule.from_config(Wav2vec2FCModuleConfig(reset_weights=True, **kw), 4, loss=loss,
                                                         device="cpu")
    try:
        for loss in ("triplet", "triplet_ce"):
            with pytest.raises(ValueError, match="triplet loss does not support no_pooling"):
                mk(loss, stat_pooling_type="none")
            with pytest.raises(NotImplementedError, match="embedding_layer_idx"):
                mk(loss, hidden_fc_layers_out=[16], embedding_layer_idx=0)
        with pytest.raises(ValueError, match="nothing would be trainable"):
            mk("triplet", wav2vec_initially_frozen=True, num_frozen_steps=3)
        with pytest.raises(NotImplementedError, match="c_ce"):
            Wav2vec2FCModule(None, Wav2vec2FCModuleConfig(reset_weights=True), 4, lambda: TripletCrossEntropyLoss(2, 1),
                             device="cpu")
    finally:
        W2V2Config.from_huggingface_id = orig


def test_arena_layout_of_the_triplet_heads():
    """"triplet" owns no head parameter (empty head bucket, head_size 0); "triplet_ce" owns exactly what "ce" owns."""
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    mk = lambda head, **kw: ParamStore(cfg, "cpu", torch.float32, head=head, num_speakers=7, **kw)
    tri, tce, ce = mk("triplet"), mk("triplet_ce", hidden_fc=(16,)), mk("ce", hidden_fc=(16,))
    assert not [n for n in tri.shapes if not n.startswith("wav2vec.")]
    assert tri.head_size() == 0 and tri.grad_buckets()[0] == ("head", 0, 0)
    assert list(tce.shapes.items()) == list(ce.shapes.items()) and tce.offsets == ce.offsets
    assert tce.head_size() == ce.head_size() > 0 and tce.grad_buckets() == ce.grad_buckets()
    assert tce.reference_parameter_order() == ce.reference_parameter_order()
    assert tri.reference_parameter_order() == [n for n in ce.reference_parameter_order() if n.startswith("wav2vec.")]
    # a reference checkpoint carries the Linear the triplet loss never trains: ignored on load, absent on save
    sd = mk("ce").state_dict()
    assert "fc_list.0.0.weight" in sd
    tri.load_state_dict(sd, strict=True, prefix_model=False)
    assert not [k for k in tri.state_dict() if k.startswith("fc_list.")]
    with pytest.raises(NotImplementedError):
        mk("triplet", hidden_fc=(16,))
