"""Batched variable-length embedding extraction vs the per-utterance path, on the GPU only (fails without one).

A seeded set of utterances (default 512, uniform 4-20 s) is embedded (a) one at a time through compute_speaker_embedding
(batch 1, one plan per length -- how the reference's test loop runs) on a subset, and (b) with compute_speaker_embeddings
(length buckets, one variable-length forward per batch) on the full set.  Warm-up passes run first (plans built), every
timed region is bracketed by device synchronisation.  Prints one JSON line.
    python tools/varlen_eval_bench.py [--n 512] [--subset 64] [--dtype f16] [--min-s 4] [--max-s 20]
--model ecapa runs the same comparison on the full-width ECAPA-TDNN (C = 1024) over filterbank tensors of --min-frames to
--max-frames frames (default 400-2000, the 4-20 s of the wav2vec2 leg at the 10 ms hop); the per-utterance path is timed
twice, building its one-plan-per-length as it goes (what a first pass over a trial list costs) and with the plans cached.
    python tools/varlen_eval_bench.py --model ecapa [--dtype f32|bf16]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="w2v2", choices=["w2v2", "ecapa"])
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
