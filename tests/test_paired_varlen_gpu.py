"""Paired-input evaluation at unequal lengths on the GPU: the assemble kernel, Plan.forward(pair_lengths=) against the
reference golden (g20_paired_varlen.npz), the oracle and batch-size-1 plans, the encoder-only plan over a feature bank, and the
module surface (compute_speaker_equality at N != M, score_trials, evaluate_trials, the step hooks)."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
LEFT, RIGHT = [4000, 400, 2500, 26000], [400, 4000, 3217, 26000]          # the golden's pairs
ORACLE_TOL = {torch.float32: 1e-4, torch.float16: 3e-3, torch.bfloat16: 4e-2}      # test_tiny_vs_oracle_at_own_lengths
INDEP_TOL = {torch.float32: 1e-5, torch.float16: 2e-3, torch.bfloat16: 3e-2}       # test_batch_independence_against_b1_plans


def _cfgs(name):
    from w2v2_speaker_amd.config import W2V2Config
    cfg, ocfg = W2V2Config.tiny(), O.OracleConfig.tiny()
    if name == "d64":             # head dimension 64: the fused attention kernels (16-bit)
        kw = dict(hidden_size=128, num_attention_heads=2)
        cfg, ocfg = dataclasses.replace(cfg, **kw), dataclasses.replace(ocfg, **kw)
    return cfg, ocfg


def _state(cfg, ocfg):
    sd = O.make_state_dict(ocfg, 20211)
    sd["linear.weight"] = O.synth_tensor("linear.weight", (1, cfg.hidden_size), 20211)
    sd["linear.bias"] = O.synth_tensor("linear.bias", (1,), 20211)
    return sd


def _store(cfg, ocfg, dtype):
    from w2v2_speaker_amd.params import ParamStore
    st = ParamStore(cfg, DEV, dtype, head="bce")
    st.load_state_dict(_state(cfg, ocfg))
    return st


def _waves():
    wl, _ = O.synth_batch(4, 26000, 2, seed=21)
    wr, _ = O.synth_batch(4, 26000, 2, seed=22)
    return wl[:, 0], wr[:, 0]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Token 0 [4, H] and logits [4] of the four pairs, each alone at its own lengths (computed once per configuration)."""
    cfg, ocfg = _cfgs(name)
    sd = _state(cfg, ocfg)
    wl, wr = _waves()
    eye, zero = torch.eye(cfg.hidden_size), torch.zeros(cfg.hidden_size)
    tok, logit = [], []
    with torch.no_grad():
        for b, (na, nb) in enumerate(zip(LEFT, RIGHT)):
            a, c = wl[b:b + 1, :na], wr[b:b + 1, :nb]
            tok.append(O.paired_equality_scores(a, c, sd, ocfg, eye, zero)[0])
            logit.append(O.paired_equality_scores(a, c, sd, ocfg, sd["linear.weight"], sd["linear.bias"])[0, 0])
    return torch.stack(tok), torch.stack(logit)


def _noise_pad(wav, lens, seed=1):
    """The padding of each row filled with N(0, 10^2) noise (finite in every dtype)."""
    g = torch.Generator().manual_seed(seed)
    out = wav.clone()
    for b, n in enumerate(lens):
        out[b, n:] = 10 * torch.randn(out.shape[1] - n, generator=g)
    return out


def _padded_batch(seed=1):
    wl, wr = _waves()
    return _noise_pad(torch.cat([wl, wr]), LEFT + RIGHT, seed).to(DEV)


def _logits(emb, sd):
    return (emb.float().cpu() @ sd["linear.weight"].t() + sd["linear.bias"])[:, 0]


# ------------------------------------------------------------------------------------------------ kernel
# (row, frames) of the utterances inside an 80-row feature matrix; rows 0, 17, 33, 35 and 76..79 belong to none
UTT = [(1, 16), (18, 15), (34, 1), (36, 17), (45, 31)]
# (left utterance, right utterance): utterance 0 in three pairs, pair 2 with left_row > right_row, pair 4 with itself
PAIRS = [(0, 1), (0, 3), (3, 0), (2, 4), (2, 2), (1, 3)]


@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_assemble_kernel(dtype, H):
    from w2v2_speaker_amd import ops
    R, T, B = 80, 40, len(PAIRS)
    g = torch.Generator().manual_seed(H)
    feat = torch.randn(R, H, generator=g)
    named = torch.zeros(R, dtype=torch.bool)
    for r, f in UTT:
        named[r:r + f] = True
    assert 0 < int((~named).sum()) < R
    feat[~named] = float("nan")
    feat = feat.to(dtype).to(DEV)
    lr, lf = [UTT[a][0] for a, _ in PAIRS], [UTT[a][1] for a, _ in PAIRS]
    rr, rf = [UTT[b][0] for _, b in PAIRS], [UTT[b][1] for _, b in PAIRS]
    assert all(a + b + 3 <= T for a, b in zip(lf, rf)) and {*lf, *rf} == {1, 15, 16, 17, 31}
    y = torch.full((B, T, H), 5.0, dtype=dtype, device=DEV)
    ops.pair_assemble(feat, y, lr, lf, rr, rf, 1.0, -1.0)
    tok = lambda c: torch.full((1, H), c, dtype=dtype, device=DEV)
    for b in range(B):
        ref = torch.cat([tok(1.0), feat[lr[b]:lr[b] + lf[b]], tok(-1.0), feat[rr[b]:rr[b] + rf[b]], tok(-1.0)])
        te = lf[b] + rf[b] + 3
        assert ref.shape[0] == te and torch.equal(y[b, :te], ref), b
        assert not y[b, te:].any(), b                          # exactly zero (NaN would count as nonzero)


def test_pair_assemble_rejects_bad_tables():
    from w2v2_speaker_amd import ops
    feat = torch.zeros(80, 64, device=DEV)
    y = torch.zeros(1, 40, 64, device=DEV)
    for lr, lf, rr, rf in (([0], [0], [10], [5]),              # ta = 0
                           ([0], [20], [20], [18]),            # ta + tb + 3 > T
                           ([70], [11], [0], [5]),             # left rows past R
                           ([0], [5], [78], [3])):             # right rows past R
        with pytest.raises(ValueError):
            ops.pair_assemble(feat, y, lr, lf, rr, rf, 1.0, -1.0)
    ops.pair_assemble(feat, y, [69], [11], [77], [3], 1.0, -1.0)            # the last rows are fine
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_lengths_vs_golden_and_oracle(dtype):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("tiny")
    st = _store(cfg, ocfg, dtype)
    sd = _state(cfg, ocfg)
    g = np.load(os.path.join(GOLDEN, "g20_paired_varlen.npz"))
    assert g["left_lengths"].tolist() == LEFT and g["right_lengths"].tolist() == RIGHT
    plan = Plan(st, 4, 26000, train=False, pooling="first", paired=True)
    emb = plan.embed(_padded_batch(1), pair_lengths=(LEFT, RIGHT)).clone()
    assert plan.frame_lengths == [cfg.num_frames(a) + cfg.num_frames(b) + 3 for a, b in zip(LEFT, RIGHT)] == [16, 16, 19, 165]
    otok, ologit = _oracle("tiny")
    for b in range(4):
        eg, eo = rel_l2(emb[b].cpu(), g["token0"][b]), rel_l2(emb[b].cpu(), otok[b])
        print(f"{dtype} pair {b}: token 0 rel-L2 vs reference {eg:.3e}, vs oracle {eo:.3e}")
        assert eg < ORACLE_TOL[dtype] and eo < ORACLE_TOL[dtype], (b, eg, eo)
    pred, pred_ref = torch.sigmoid(_logits(emb, sd)), torch.sigmoid(ologit)
    print(f"{dtype}: max |sigmoid difference| {float((pred - pred_ref).abs().max()):.3e}")
    assert torch.allclose(pred, pred_ref, rtol=0, atol=1e-5 if dtype == torch.float32 else 3e-2)
    emb2 = plan.embed(_padded_batch(2), pair_lengths=(torch.tensor(LEFT), torch.tensor(RIGHT)))
    assert torch.equal(emb, emb2)                              # the padding's content never reaches a result


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_pair_lengths_equal_fixed_length_path(dtype):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("tiny")
    st = _store(cfg, ocfg, dtype)
    sd = _state(cfg, ocfg)
    B, N = 3, 4000
    wl, wr = _waves()
    wav = torch.cat([wl[:B, :N], wr[:B, :N]]).to(DEV)
    plan = Plan(st, B, N, train=False, pooling="first", paired=True)
    a = _logits(plan.embed(wav), sd)
    b = _logits(plan.embed(wav, pair_lengths=([N] * B, [N] * B)), sd)
    assert plan.frame_lengths == [plan.T] * B
    c = _logits(plan.embed(wav), sd)                           # back on the fixed-length path
    assert plan.frame_lengths is None
    assert torch.equal(a, b) and torch.equal(a, c)


# Parent commit's fixed-length paired path at this configuration (B = 1, N = 26000 + 26000, i.e. the 165-frame tiled
# kernels) against the oracle, measured on an MI355X: see D64_PARENT_ERR below.  Where that is above the tiny bound the
# bound of the variable-length path is 1.5 x the parent's error (another M routes the GEMMs to other tiles).
D64_PARENT_ERR = {torch.float16: None, torch.bfloat16: None}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fused_and_tiled_attention_on_the_pair_path(dtype):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("d64")
    st = _store(cfg, ocfg, dtype)
    plan = Plan(st, 4, 26000, train=False, pooling="first", paired=True)
    assert plan.fused and cfg.head_dim == 64
    emb = plan.embed(_padded_batch(3), pair_lengths=(LEFT, RIGHT)).clone()
    assert plan.frame_lengths == [16, 16, 19, 165]
    wl, wr = _waves()
    otok, _ = _oracle("d64")
    bound = ORACLE_TOL[dtype]
    if D64_PARENT_ERR[dtype] is not None and D64_PARENT_ERR[dtype] > bound:
        bound = 1.5 * D64_PARENT_ERR[dtype]
    errs = []
    for b, (na, nb) in enumerate(zip(LEFT, RIGHT)):
        n = max(na, nb)
        w1 = torch.zeros(2, n)
        w1[0, :na], w1[1, :nb] = wl[b, :na], wr[b, :nb]
        p1 = Plan(st, 1, n, train=False, pooling="first", paired=True)
        ref = p1.embed(w1.to(DEV), pair_lengths=([na], [nb])).cpu()
        e1, eo = rel_l2(emb[b].cpu(), ref[0]), rel_l2(emb[b].cpu(), otok[b])
        print(f"d64 {dtype} pair {b}: rel-L2 vs batch-1 plan {e1:.3e}, vs oracle {eo:.3e} (bound {bound:.3e})")
        errs.append((b, e1, eo))
    for b, e1, eo in errs:
        assert e1 < {torch.float16: 2e-3, torch.bfloat16: 3e-2}[dtype], (b, e1)
        assert eo < bound, (b, eo)


@pytest.mark.parametrize("dtype", DTYPES)
def test_encoder_only_plan_equals_direct_path(dtype):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("tiny")
    st = _store(cfg, ocfg, dtype)
    direct = Plan(st, 4, 26000, train=False, pooling="first", paired=True)
    ref = direct.embed(_padded_batch(4), pair_lengths=(LEFT, RIGHT)).clone()
    lens = LEFT + RIGHT
    fplan = Plan(st, 8, 26000, train=False, pooling="first")
    feat, frames = fplan.features(_padded_batch(5), lengths=lens)
    assert feat.shape == (8, cfg.num_frames(26000), cfg.hidden_size) and frames == [cfg.num_frames(n) for n in lens]
    offset = np.concatenate([[0], np.cumsum(frames)]).tolist()
    bank = torch.full((offset[-1] + 3, cfg.hidden_size), float("nan"), dtype=dtype, device=DEV)    # 3 rows nobody names
    for i, f in enumerate(frames):
        bank[offset[i]:offset[i] + f].copy_(feat[i, :f])
    enc = Plan.pair_encoder(st, 4, 170)
    assert enc.T == 170 and not hasattr(enc, "conv") and not hasattr(enc, "h0")
    got = enc.embed_pairs(bank, offset[:4], frames[:4], offset[4:8], frames[4:])
    assert enc.frame_lengths == [16, 16, 19, 165]
    for b in range(4):
        err = rel_l2(got[b].cpu(), ref[b].cpu())
        print(f"{dtype} pair {b}: encoder-only plan vs pair_lengths path rel-L2 {err:.3e}")
        assert err < INDEP_TOL[dtype], (b, err)
    with pytest.raises(ValueError):
        enc.forward(_padded_batch(5))                          # no conv stack behind it
    with pytest.raises(ValueError):
        enc.embed_pairs(bank, offset[:4], frames[:4], offset[4:8], [f + 6 for f in frames[4:]])     # 171 frames > 170


# ------------------------------------------------------------------------------------------------ module
def _tiny_module(dtype):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_paired_input import (Wav2vec2PairedSpeakerModule,
                                                                                   Wav2vec2PairedSpeakerModuleConfig)
    cfg, ocfg = _cfgs("tiny")
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: cfg)
    try:
        mod = Wav2vec2PairedSpeakerModule(None, Wav2vec2PairedSpeakerModuleConfig(), device=DEV, act_dtype=dtype)
    finally:
        W2V2Config.from_huggingface_id = orig
    mod.store.load_state_dict(_state(cfg, ocfg))
    return mod


def _trial_set():
    from w2v2_speaker_amd.data.paired import EvaluationPair
    r = np.random.default_rng(17)
    lens = [400, 9000] + [int(n) for n in r.integers(401, 9000, 8)]
    audio = {f"u{i}": torch.randn(n, generator=torch.Generator().manual_seed(100 + i)) for i, n in enumerate(lens)}
    audio["u3"] = audio["u3"][None]                            # [1, N] is accepted too
    keys = list(audio)
    pairs = [EvaluationPair(bool(r.integers(0, 2)), keys[int(i)], keys[int(j)])
             for i, j in zip(r.integers(0, 10, 19), r.integers(0, 10, 19))]
    pairs.insert(5, EvaluationPair(True, "u4", "u4"))          # an utterance against itself
    assert len({k for p in pairs for k in (p.sample1_id, p.sample2_id)}) < 2 * len(pairs)         # utterances are reused
    return audio, pairs


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_trials_matches_per_trial_equality(dtype):
    mod = _tiny_module(dtype)
    audio, pairs = _trial_set()
    kw = dict(quantum=10, max_batch_frames=4 * 60, max_batch=4)
    got = mod.score_trials(pairs, audio, **kw)
    built = mod.bucket_plans_built
    assert len(got) == len(pairs) == 20 and built > 0 and mod.last_bank_bytes > 0
    sq = lambda w: w if w.dim() == 2 else w[None]
    ref = [float(mod.compute_speaker_equality(sq(audio[p.sample1_id]), sq(audio[p.sample2_id]))[0, 0]) for p in pairs]
    # the quantity with a bound is token 0; a logit is its inner product with one weight row, so the same relative
    # bound holds for the logits on the scale |w| |token 0| (Cauchy-Schwarz)
    w = mod.store.p("linear.weight").float().norm().item()
    scale = w * np.sqrt(mod.model_cfg.hidden_size)             # token 0 leaves a LayerNorm: |token 0| ~ sqrt(H)
    worst = max(abs(a - b) for a, b in zip(got, ref))
    print(f"{dtype}: max |logit difference| {worst:.3e} on the scale {scale:.3e}")
    assert worst < INDEP_TOL[dtype] * scale
    plans_before = mod.bucket_plans_built
    again = mod.score_trials(pairs, audio, **kw)
    assert mod.bucket_plans_built == plans_before and again == got       # plans are reused; same bits
    back = mod.score_trials(pairs[::-1], audio, **kw)                      # the order follows `pairs` (the utterances
    assert max(abs(x - y) for x, y in zip(back, got[::-1])) < INDEP_TOL[dtype] * scale     # then batch differently)
    assert len({round(v, 4) for v in got}) > len(got) // 2                # ... and the scores tell the trials apart
    with pytest.raises(ValueError, match="split"):
        mod.score_trials(pairs, audio, max_bank_bytes=1, **kw)
    if dtype == torch.float32:
        res = mod.evaluate_trials(pairs, audio, **kw)
        exp = mod._evaluate([{"prediction": ref, "label": [int(p.same_speaker) for p in pairs]}])
        assert set(res) == {"eer", "eer_threshold", "mdc", "mdc_threshold"}
        assert abs(float(res["eer"]) - float(exp["eer"])) <= 1.0 / len(pairs) + 1e-9
        assert float(res["mdc"]) == pytest.approx(float(exp["mdc"]), abs=1e-4)


def test_step_hooks_and_unequal_shapes():
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_paired_input import PairedSpeakerClassificationDataBatch
    mod = _tiny_module(torch.float32)
    wl, wr = _waves()
    a, b = wl[:2, :4000], wr[:2, :3217]
    s = mod.compute_speaker_equality(a, b)                     # [B, N] and [B, M]
    assert s.shape == (2, 1)
    pad = torch.zeros(2, 4000)
    pad[:, :3217] = b
    s2 = mod.compute_speaker_equality(a, pad, lengths=([4000, 4000], [3217, 3217]))
    assert torch.equal(s, s2)
    cfg, ocfg = _cfgs("tiny")
    sd = _state(cfg, ocfg)
    with torch.no_grad():
        ref = O.paired_equality_scores(a, b, sd, ocfg, sd["linear.weight"], sd["linear.bias"])
    assert torch.allclose(torch.sigmoid(s.cpu()), torch.sigmoid(ref), rtol=0, atol=1e-5)
    batch2 = PairedSpeakerClassificationDataBatch(2, ["a", "b"], a, ["c", "d"], b, torch.tensor([1, 0]))
    out = mod.validation_step(batch2)
    assert set(out) == {"prediction", "label"} and out["label"] == [1, 0]
    assert np.allclose(np.asarray(out["prediction"]), s.cpu().numpy())
    with pytest.raises(ValueError):
        mod.test_step(batch2)
    batch1 = PairedSpeakerClassificationDataBatch(1, ["a"], a[:1], ["c"], b[:1], torch.tensor([0]))
    outs = [mod.test_step(batch1), out]
    res = mod.test_epoch_end(outs)
    assert res == mod.validation_epoch_end(outs) == mod._evaluate(outs) and set(res) == {"eer", "eer_threshold", "mdc",
                                                                                            "mdc_threshold"}


# ------------------------------------------------------------------------------------------------ guards
def test_pair_lengths_guards():
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("tiny")
    st = _store(cfg, ocfg, torch.float32)
    wav2, wav4 = torch.randn(2, 4000, device=DEV), torch.randn(4, 4000, device=DEV)
    ok = ([4000, 3000], [500, 4000])
    with pytest.raises(NotImplementedError):
        Plan(st, 2, 4000, train=True, pooling="first", paired=True).forward(wav4, pair_lengths=ok)
    with pytest.raises(ValueError):
        Plan(st, 2, 4000, train=False).forward(wav2, pair_lengths=ok)
    plan = Plan(st, 2, 4000, train=False, pooling="first", paired=True)
    with pytest.raises(NotImplementedError, match="pair_lengths"):
        plan.forward(wav4, lengths=[4000, 3000])
    with pytest.raises(ValueError):
        plan.embed(wav4, pair_lengths=([4001, 3000], [500, 4000]))
    with pytest.raises(ValueError):
        plan.embed(wav4, pair_lengths=([4000, 3000], [399, 4000]))
    with pytest.raises(ValueError):
        plan.embed(wav4, pair_lengths=([4000, 3000], [500]))
    assert torch.isfinite(plan.embed(wav4, pair_lengths=ok)).all()
