"""Batched variable-length embedding extraction vs the per-utterance path, on the GPU only (fails without one).

A seeded set of utterances (default 512, uniform 4-20 s) is embedded (a) one at a time through compute_speaker_embedding
(batch 1, one plan per length -- how the reference's test loop runs) on a subset, and (b) with compute_speaker_embeddings
(length buckets, one variable-length forward per batch) on the full set.  Warm-up passes run first (plans built), every
timed region is bracketed by device synchronisation.  Prints one JSON line.
    python tools/varlen_eval_bench.py [--n 512] [--subset 64] [--dtype f16] [--min-s 4] [--max-s 20]
--model ecapa runs the same comparison on the full-width ECAPA-TDNN (C = 1024) over filterbank tensors of --min-frames to
--max-frames frames (default 400-2000, the 4-20 s of the wav2vec2 leg at the 10 ms hop); the per-utterance path is timed
twice, building its one-plan-per-length as it goes (what a first pass over a trial list costs) and with the plans cached.
    python tools/varlen_eval_bench.py --model ecapa [--dtype f32|bf16]
--model paired scores a seeded trial list (default 2048 trials over 256 utterances, uniform 4-20 s) with the paired-input
model three ways: (a) one trial at a time through compute_speaker_equality (batch 1; a subset), (b) score_trials (every
utterance through the conv stack once, trials batched through encoder-only plans), (c) score_trials with the feature reuse
switched off (each trial's two utterances through the conv stack on their own), so that batching and reuse can be told apart.
    python tools/varlen_eval_bench.py --model paired [--trials 2048] [--utts 256] [--subset 64] [--dtype f16]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def ecapa_main(a):
    from oracle import ecapa_oracle as E
    from w2v2_speaker_amd.eval_batching import DEFAULT_FRAME_QUANTUM, DEFAULT_MAX_BATCH, DEFAULT_MAX_BATCH_FRAMES, plan_batches
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTDNNModuleConfig, EcapaTdnnModule
    if a.dtype == "f16":
        raise SystemExit("the ECAPA path runs in f32 (the reference's precision) or bf16")
    dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[a.dtype]
    mod = EcapaTdnnModule.from_config(EcapaTDNNModuleConfig(), num_speakers=8, device="cuda", act_dtype=dtype)
    mod.store.load_state_dict(E.make_state_dict(E.EcapaConfig(), 20211), strict=False)
    n_mels = mod.cfg.input_mel_coefficients
    r = np.random.default_rng(a.seed)
    lens = [int(x) for x in r.integers(a.min_frames, a.max_frames + 1, a.n)]
    feats = [torch.from_numpy(r.standard_normal((n, n_mels)).astype(np.float32)) for n in lens]
    sub = list(range(min(a.subset, a.n)))
    q = a.quantum or DEFAULT_FRAME_QUANTUM
    for f in feats[-2:]:                                      # warm-up: plan machinery, kernels loaded
        mod.compute_speaker_embedding(f)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = [mod.compute_speaker_embedding(feats[i]) for i in sub]          # builds one plan per distinct frame count
    torch.cuda.synchronize()
    ta_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = [mod.compute_speaker_embedding(feats[i]) for i in sub]          # the same plans, cached
    torch.cuda.synchronize()
    ta = time.perf_counter() - t0
    per_utt_plans = len(mod._plans)
    mod._plans.clear()
    built0 = mod.bucket_plans_built
    mod.compute_speaker_embeddings(feats, quantum=q)          # warm-up pass builds the bucket plans
    torch.cuda.synchronize()
    built = mod.bucket_plans_built - built0
    t0 = time.perf_counter()
    got = mod.compute_speaker_embeddings(feats, quantum=q)
    torch.cuda.synchronize()
    tb = time.perf_counter() - t0
    err = max(float((got[i].float() - ref[j].float()).norm() / ref[j].float().norm()) for j, i in enumerate(sub))
    batches = plan_batches(lens, q, DEFAULT_MAX_BATCH_FRAMES, DEFAULT_MAX_BATCH)
    padded = sum(b * n for _, n, b in batches)
    fr_sub, fr = sum(lens[i] for i in sub), sum(lens)
    print(json.dumps({
        "metric": "varlen_eval_ecapa", "dtype": a.dtype, "channels": mod.cfg.channels[0], "n_utts": a.n, "subset": len(sub),
        "quantum_frames": q,
        "per_utt_first_pass_utt_per_s": round(len(sub) / ta_build, 2),
        "per_utt_first_pass_frames_per_s": round(fr_sub / ta_build, 1),
        "per_utt_utt_per_s": round(len(sub) / ta, 2), "per_utt_frames_per_s": round(fr_sub / ta, 1),
        "batched_utt_per_s": round(a.n / tb, 2), "batched_frames_per_s": round(fr / tb, 1),
        "speedup_utt_per_s": round((a.n / tb) / (len(sub) / ta), 2),
        "speedup_vs_first_pass": round((a.n / tb) / (len(sub) / ta_build), 2),
        "per_utt_plans_built": per_utt_plans, "bucket_plans_built": built, "batches": len(batches),
        "padded_over_valid_frames": round(padded / fr, 4),
        "max_rel_l2_batched_vs_per_utt": err,
    }))


def paired_main(a):
    from oracle import w2v2_oracle as O
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.data.paired import EvaluationPair
    from w2v2_speaker_amd.eval_batching import DEFAULT_PAIR_QUANTUM, plan_pair_batches
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_paired_input import (Wav2vec2PairedSpeakerModule,
                                                                                   Wav2vec2PairedSpeakerModuleConfig)
    dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[a.dtype]
    cfg = W2V2Config()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: cfg)
    try:
        mod = Wav2vec2PairedSpeakerModule(None, Wav2vec2PairedSpeakerModuleConfig(), device="cuda", act_dtype=dtype)
    finally:
        W2V2Config.from_huggingface_id = orig
    sd = O.make_state_dict(O.OracleConfig.base(), 20211)
    sd["linear.weight"] = O.synth_tensor("linear.weight", (1, cfg.hidden_size), 20211)
    sd["linear.bias"] = O.synth_tensor("linear.bias", (1,), 20211)
    mod.store.load_state_dict(sd)
    r = np.random.default_rng(a.seed)
    lens = [int(x) for x in r.integers(int(a.min_s * 16000), int(a.max_s * 16000) + 1, a.utts)]
    audio = {f"u{i}": torch.from_numpy(r.standard_normal(n).astype(np.float32)) for i, n in enumerate(lens)}
    ij = r.integers(0, a.utts, (a.trials, 2))
    pairs = [EvaluationPair(bool(i % 2), f"u{int(x)}", f"u{int(y)}") for i, (x, y) in enumerate(ij)]
    sub = list(range(min(a.subset, a.trials)))
    q = a.quantum or DEFAULT_PAIR_QUANTUM
    one = lambda i: mod.compute_speaker_equality(audio[pairs[i].sample1_id][None], audio[pairs[i].sample2_id][None])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    # (a) per trial at batch 1: the warm-up pass builds its plans (one per 2 s of the longer side), the timed pass reuses them
    b0 = mod.bucket_plans_built
    for i in sub:
        one(i)
    plans_a = mod.bucket_plans_built - b0 + len(mod._plans)
    b0 = mod.bucket_plans_built + len(mod._plans)
    ref, ta = timed(lambda: [float(one(i)[0, 0]) for i in sub])
    assert mod.bucket_plans_built + len(mod._plans) == b0, "the per-trial pass rebuilt plans inside the timed region"
    # (b) score_trials, (c) the same without the feature reuse; warm-up passes build the bucket plans
    b0 = mod.bucket_plans_built
    mod.score_trials(pairs, audio, quantum=q)
    plans_b = mod.bucket_plans_built - b0
    got, tb = timed(lambda: mod.score_trials(pairs, audio, quantum=q))
    assert mod.bucket_plans_built - b0 == plans_b, "score_trials rebuilt plans inside the timed region"
    bank_b = mod.last_bank_bytes
    mod.score_trials(pairs, audio, quantum=q, reuse_features=False)
    b0 = mod.bucket_plans_built
    got_c, tc = timed(lambda: mod.score_trials(pairs, audio, quantum=q, reuse_features=False))
    assert mod.bucket_plans_built == b0, "score_trials(reuse_features=False) rebuilt plans inside the timed region"
    bank_c = mod.last_bank_bytes
    fr = [cfg.num_frames(n) for n in lens]
    lf, rf = [fr[int(x)] for x, _ in ij], [fr[int(y)] for _, y in ij]
    batches = plan_pair_batches(lf, rf, q)
    valid = sum(x + y + 3 for x, y in zip(lf, rf))
    per_trial_a, per_trial_b, per_trial_c = ta / len(sub), tb / a.trials, tc / a.trials
    print(json.dumps({
        "metric": "varlen_eval_paired", "dtype": a.dtype, "trials": a.trials, "utterances": a.utts, "subset": len(sub),
        "quantum_frames": q,
        "per_trial_s": round(ta, 4), "per_trial_trials_per_s": round(1 / per_trial_a, 2),
        "score_trials_s": round(tb, 4), "score_trials_trials_per_s": round(1 / per_trial_b, 2),
        "score_trials_no_reuse_s": round(tc, 4), "score_trials_no_reuse_trials_per_s": round(1 / per_trial_c, 2),
        "speedup_score_trials_vs_per_trial": round(per_trial_a / per_trial_b, 2),
        "speedup_no_reuse_vs_per_trial": round(per_trial_a / per_trial_c, 2),
        "speedup_reuse_alone": round(tc / tb, 2),
        "per_trial_plans_built": plans_a, "bucket_plans_built": plans_b, "pair_batches": len(batches),
        "padded_over_valid_frames": round(sum(b * n for _, n, b in batches) / valid, 4),
        "bank_bytes": bank_b, "bank_bytes_no_reuse": bank_c,
        "max_abs_logit_diff_vs_per_trial": max(abs(got[i] - ref[j]) for j, i in enumerate(sub)),
        "max_abs_logit_diff_no_reuse_vs_per_trial": max(abs(got_c[i] - ref[j]) for j, i in enumerate(sub)),
        "max_abs_logit": max(abs(v) for v in ref),
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="w2v2", choices=["w2v2", "ecapa", "paired"])
    ap.add_argument("--trials", type=int, default=2048)
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--min-frames", type=int, default=400)
    ap.add_argument("--max-frames", type=int, default=2000)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--min-s", type=float, default=4.0)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=20240)
    ap.add_argument("--quantum", type=int, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("varlen_eval_bench needs the GPU")
    if a.model == "ecapa":
        return ecapa_main(a)
    if a.model == "paired":
        return paired_main(a)
    from oracle import w2v2_oracle as O
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.eval_batching import DEFAULT_QUANTUM, plan_batches
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[a.dtype]
    cfg = W2V2Config()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: cfg)
    try:
        mod = Wav2vec2FCModule.from_config(Wav2vec2FCModuleConfig(reset_weights=True), num_speakers=8, device="cuda",
                                           act_dtype=dtype)
    finally:
        W2V2Config.from_huggingface_id = orig
    sd = O.make_state_dict(O.OracleConfig.base(), 20211)
    mod.store.load_state_dict({"wav2vec.model." + k: v for k, v in sd.items()}, strict=False)
    r = np.random.default_rng(a.seed)
    lens = [int(x) for x in r.integers(int(a.min_s * 16000), int(a.max_s * 16000) + 1, a.n)]
    wavs = [torch.from_numpy(r.standard_normal(n).astype(np.float32)) for n in lens]
    sub = list(range(min(a.subset, a.n)))
    q = a.quantum or DEFAULT_QUANTUM
    # (a) per-utterance path; warm-up on two utterances of other lengths (plan machinery, kernels loaded)
    for w in wavs[-2:]:
        mod.compute_speaker_embedding(w)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = [mod.compute_speaker_embedding(wavs[i]) for i in sub]
    torch.cuda.synchronize()
    ta = time.perf_counter() - t0
    # (b) batched: a warm-up pass builds the bucket plans, the timed pass reuses them
    built0 = mod.bucket_plans_built
    mod.compute_speaker_embeddings(wavs, quantum=q)
    torch.cuda.synchronize()
    built = mod.bucket_plans_built - built0
    t0 = time.perf_counter()
    got = mod.compute_speaker_embeddings(wavs, quantum=q)
    torch.cuda.synchronize()
    tb = time.perf_counter() - t0
    err = max(float((got[i].float() - ref[j].float()).norm() / ref[j].float().norm()) for j, i in enumerate(sub))
    batches = plan_batches(lens, q)
    padded = sum(b * n for _, n, b in batches)
    audio_sub = sum(lens[i] for i in sub) / 16000
    audio = sum(lens) / 16000
    print(json.dumps({
        "metric": "varlen_eval", "dtype": a.dtype, "n_utts": a.n, "subset": len(sub), "quantum": q,
        "per_utt_utt_per_s": round(len(sub) / ta, 2), "per_utt_audio_s_per_s": round(audio_sub / ta, 1),
        "batched_utt_per_s": round(a.n / tb, 2), "batched_audio_s_per_s": round(audio / tb, 1),
        "speedup_utt_per_s": round((a.n / tb) / (len(sub) / ta), 2),
        "per_utt_plans_built": len(sub) + 2, "bucket_plans_built": built, "batches": len(batches),
        "padded_over_valid_samples": round(padded / sum(lens), 4),
        "max_rel_l2_batched_vs_per_utt": err,
    }))


if __name__ == "__main__":
    main()
