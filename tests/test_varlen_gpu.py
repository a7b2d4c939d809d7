"""Batched variable-length evaluation on the GPU: the length-aware kernels against the same kernels on each utterance
alone, Plan.forward(lengths=) against the reference goldens, the oracle and the batch-size-1 plans, and the module
surface (compute_speaker_embeddings, evaluate_trials)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
EDGES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65]


def _i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device=DEV)


def _store(cfg, ocfg, dtype, seed=20211, head=None, C=1):
    from w2v2_speaker_amd.params import ParamStore
    st = ParamStore(cfg, DEV, dtype, head=head, num_speakers=C)
    st.load_state_dict(O.make_state_dict(ocfg, seed))
    return st


def _cfgs(name):
    from w2v2_speaker_amd.config import W2V2Config
    if name == "tiny":
        return W2V2Config.tiny(), O.OracleConfig.tiny()
    return W2V2Config(), O.OracleConfig.base()


def _assert_close(got, ref, tol, what=None):
    """rel-L2 within tol on the finite entries, and NaN in the same places (mean+std of a one-frame utterance: torch's
    unbiased std is NaN, and so is the kernel's)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan), what
    err = rel_l2(got[~nan], ref[~nan])
    assert err < tol, (what, err)


def _noise_pad(wav, lens, seed=1):
    """The padding of each row filled with N(0, 10^2) noise (finite in every dtype)."""
    g = torch.Generator().manual_seed(seed)
    out = wav.clone()
    for b, n in enumerate(lens):
        out[b, n:] = 10 * torch.randn(out.shape[1] - n, generator=g)
    return out


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("mfma", [False, True])
def test_conv0_stats_len_bit_identical_to_utterance_alone(mfma):
    from w2v2_speaker_amd import _lib, ops
    C, k, stride = 512, 10, 5
    frames = [1, 127, 128, 129, 639, 640, 641, 1400]
    N = (max(frames) - 1) * stride + k
    g = torch.Generator().manual_seed(4)
    wav = torch.randn(len(frames), N, generator=g).to(DEV)
    w = (0.3 * torch.randn(C, k, generator=g)).to(DEV)
    work = ops.conv0_workspace(len(frames), N, C, k, stride, DEV)
    work.fill_(float("nan"))                                  # skipped partials must never be read
    mr = ops.conv0_stats_len(wav, w, work, _i32(frames), k, stride, mfma).clone()
    fn = ops.lib().w2v2_conv0_stats_mfma if mfma else ops.lib().w2v2_conv0_stats
    for b, L in enumerate(frames):
        n = (L - 1) * stride + k
        x = wav[b:b + 1, :n].contiguous()
        wk = ops.conv0_workspace(1, n, C, k, stride, DEV)
        ref = wk[wk.numel() - C * 2:]
        _lib.check(fn(x.data_ptr(), w.data_ptr(), wk.data_ptr(), ref.data_ptr(), 1, n, C, k, stride, 1e-5,
                      ops.stream()), "conv0_stats")
        assert torch.equal(mr[b], ref.view(C, 2)), (mfma, L)


def test_conv0_stats_mfma_len_rejects_the_convolution_statistics_branch():
    from w2v2_speaker_amd import ops
    C, k, stride = 512, 8, 4                                  # k != 10: no window-moment path
    wav = torch.randn(2, 4000, device=DEV)
    w = torch.randn(C, k, device=DEV)
    work = ops.conv0_workspace(2, 4000, C, k, stride, DEV)
    with pytest.raises(RuntimeError):
        ops.conv0_stats_len(wav, w, work, _i32([100, 50]), k, stride, True)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_posconv_regroup_len(dtype):
    from w2v2_speaker_amd import ops
    B, T, H, G, K = 4, 70, 64, 4, 16
    lens = [1, 17, 64, 70]
    x = torch.randn(B, T, H, device=DEV).to(dtype)
    xg = torch.full((B, G, T + K - 1, H // G), 7.0, device=DEV, dtype=dtype)
    ops.posconv_regroup_len(x, xg, _i32(lens), B, T, H, G, K, K // 2)
    for b, L in enumerate(lens):
        ref = torch.empty(1, G, L + K - 1, H // G, device=DEV, dtype=dtype)
        ops.posconv_regroup(x[b:b + 1, :L].contiguous(), ref, 1, L, H, G, K, K // 2)
        assert torch.equal(xg[b, :, :L + K - 1], ref[0])
        assert not xg[b, :, L + K - 1:].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["mean+std", "mean", "max", "first", "last", "middle", "quantile"])
def test_pool_len_bit_identical(dtype, mode):
    from w2v2_speaker_amd import ops
    T, H = 70, 64
    lens = EDGES + [T]
    B = len(lens)
    m = ops.POOL_MODES[mode]
    x = torch.randn(B, T, H, device=DEV).to(dtype)
    W = ops.POOL_WIDTH.get(m, 1) * H
    out = torch.empty(B, W, device=DEV)
    ops.pool_fwd_len(x, out, _i32(lens), m)
    for b, L in enumerate(lens):
        ref = torch.empty(1, W, device=DEV)
        ops.pool_fwd(x[b:b + 1, :L].contiguous(), ref, m)
        assert torch.equal(out[b:b + 1].isnan(), ref.isnan())
        assert torch.equal(out[b:b + 1].nan_to_num(), ref.nan_to_num()), (mode, L)


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_len_bit_identical_and_padding_zero(dtype):
    from w2v2_speaker_amd import ops
    T, heads = 70, 3
    lens = EDGES + [T]
    B = len(lens)
    ld = (T + 7) // 8 * 8
    s = torch.randn(B * heads * T, ld, device=DEV) * 3
    p = torch.full((B * heads * T, ld), 5.0, device=DEV).to(dtype)
    ops.softmax_fwd_len(s, p, _i32(lens), B, heads, T, ld)
    p = p.view(B, heads, T, ld)
    sv = s.view(B, heads, T, ld)
    for b, L in enumerate(lens):
        sl = sv[b, :, :L, :L].contiguous().view(heads * L, L)
        ref = torch.empty(heads * L, L, dtype=dtype, device=DEV)
        ops.softmax_fwd(sl, ref, None, heads * L, L, L, 0.0, 0)
        assert torch.equal(p[b, :, :L, :L].reshape(heads * L, L), ref), L
        assert not p[b, :, :L, L:T].any() and not p[b, :, L:, :T].any()


@pytest.mark.parametrize("geom", ["32", "64"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_attention_len_bit_identical_under_forced_geometry(geom, dtype, monkeypatch):
    from w2v2_speaker_amd import ops
    monkeypatch.setenv("W2V2_ATTN_GEOM", geom)
    heads, d, T = 2, 64, 130
    lens = EDGES + [T]
    B = len(lens)
    H = heads * d
    qkv = (torch.randn(B, T, 3 * H, device=DEV)).to(dtype)
    for b, L in enumerate(lens):                              # padded rows hold garbage (inf / nan in 16 bits)
        qkv[b, L:] = float("nan") if b % 2 else float("inf")
    ctx = torch.full((B, T, H), 3.0, device=DEV, dtype=dtype)
    lse = torch.empty(B * heads * T, device=DEV)
    ops.attention_fwd_len(qkv, ctx, lse, _i32(lens), B, T, heads, d, d ** -0.5)
    for b, L in enumerate(lens):
        ref = torch.empty(1, L, H, device=DEV, dtype=dtype)
        rl = torch.empty(heads * L, device=DEV)
        ops.attention_fwd(qkv[b:b + 1, :L].contiguous(), ref, rl, 1, L, heads, d, d ** -0.5, 0.0, 0)
        assert torch.equal(ctx[b, :L], ref[0]), (geom, L)
        assert not ctx[b, L:].any()
        assert torch.equal(lse.view(B, heads, T)[b, :, :L], rl.view(heads, L))


def test_len_entries_at_full_lengths_equal_the_fixed_length_entries(monkeypatch):
    """The two forms of an operation are instantiations of one kernel body: with lens = [T] * B the variable-length
    entry must give the bits of the fixed-length entry, on shapes that cross the kernels' internal boundaries."""
    from w2v2_speaker_amd import _lib, ops
    g = torch.Generator().manual_seed(7)
    # layer-0 statistics, exact and window-moment route: five whole 128-frame chunks and a ragged one (two 640-frame
    # window-moment blocks, the second ragged)
    C, k, stride, B = 512, 10, 5, 2
    N = 5 * (128 * stride) + 37 * stride + k
    wav = torch.randn(B, N, generator=g).to(DEV)
    w = (0.3 * torch.randn(C, k, generator=g)).to(DEV)
    for mfma in (False, True):
        work = ops.conv0_workspace(B, N, C, k, stride, DEV)
        mr = ops.conv0_stats_len(wav, w, work, _i32([(N - k) // stride + 1] * B), k, stride, mfma).clone()
        wk = ops.conv0_workspace(B, N, C, k, stride, DEV)
        ref = wk[wk.numel() - B * C * 2:]
        fn = ops.lib().w2v2_conv0_stats_mfma if mfma else ops.lib().w2v2_conv0_stats
        _lib.check(fn(wav.data_ptr(), w.data_ptr(), wk.data_ptr(), ref.data_ptr(), B, N, C, k, stride, 1e-5,
                      ops.stream()), "conv0_stats")
        assert torch.equal(mr, ref.view(B, C, 2)), mfma
    for dtype in DTYPES:
        B, T, H, G, K = 2, 21, 64, 4, 8
        x = torch.randn(B, T, H, generator=g).to(DEV).to(dtype)
        xg = torch.full((B, G, T + K - 1, H // G), 7.0, device=DEV, dtype=dtype)
        ref = torch.full_like(xg, 5.0)
        ops.posconv_regroup_len(x, xg, _i32([T] * B), B, T, H, G, K, K // 2)
        ops.posconv_regroup(x, ref, B, T, H, G, K, K // 2)
        assert torch.equal(xg, ref), dtype
        # pooling: a partial 128-channel block, T no multiple of the 16 time lanes
        B, T, H = 3, 37, 136
        x = torch.randn(B, T, H, generator=g).to(DEV).to(dtype)
        for m in range(6):
            W = ops.POOL_WIDTH.get(m, 1) * H
            out, ref = torch.full((B, W), 7.0, device=DEV), torch.full((B, W), 5.0, device=DEV)
            ops.pool_fwd_len(x, out, _i32([T] * B), m)
            ops.pool_fwd(x, ref, m)
            assert torch.equal(out, ref), (dtype, m)
        # softmax without dropout: more than one 64-lane pass
        B, heads, T = 2, 2, 70
        ld = (T + 7) // 8 * 8
        s = (3 * torch.randn(B * heads * T, ld, generator=g)).to(DEV)
        p = torch.full((B * heads * T, ld), 7.0, device=DEV).to(dtype)
        ref = p.clone()
        ops.softmax_fwd_len(s, p, _i32([T] * B), B, heads, T, ld)
        ops.softmax_fwd(s, ref, None, B * heads * T, T, ld, 0.0, 0)
        assert torch.equal(p, ref), dtype
    # fused attention without dropout, every row valid: all of ctx and lse
    B, heads, d = 2, 2, 64
    for geom in ("32", "64"):
        monkeypatch.setenv("W2V2_ATTN_GEOM", geom)
        for dtype in (torch.float16, torch.bfloat16):
            for T in (70, 149):
                qkv = torch.randn(B, T, 3 * heads * d, generator=g).to(DEV).to(dtype)
                ctx = torch.full((B, T, heads * d), 7.0, device=DEV, dtype=dtype)
                ref = torch.full_like(ctx, 5.0)
                lse, rl = torch.full((B * heads * T,), 7.0, device=DEV), torch.full((B * heads * T,), 5.0, device=DEV)
                ops.attention_fwd_len(qkv, ctx, lse, _i32([T] * B), B, T, heads, d, d ** -0.5)
                ops.attention_fwd(qkv, ref, rl, B, T, heads, d, d ** -0.5, 0.0, 0)
                assert torch.equal(ctx, ref) and torch.equal(lse, rl), (geom, dtype, T)


# ------------------------------------------------------------------------------------------------ engine
def _golden_batch():
    """g2_base's two 3 s utterances and g13_long's 20 s one, in one batch padded to 20 s (weights seed 20211)."""
    w2, _ = O.synth_batch(2, 48000, 5994, seed=42133724)
    w13, _ = O.synth_batch(1, 320000, 5994, seed=90017)
    wav = torch.zeros(3, 320000)
    wav[0, :48000], wav[1, :48000], wav[2] = w2[0, 0], w2[1, 0], w13[0, 0]
    g2, g13 = np.load(os.path.join(GOLDEN, "g2_base.npz")), np.load(os.path.join(GOLDEN, "g13_long.npz"))
    ref = np.concatenate([g2["eval.mean+std"], g13["eval.mean+std"]])
    return wav, [48000, 48000, 320000], ref


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_pinned_padded_batch_and_padding_content_irrelevant(dtype):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("base")
    st = _store(cfg, ocfg, dtype)
    wav, lens, ref = _golden_batch()
    plan = Plan(st, 3, 320000, train=False)
    e = plan.embed(wav.to(DEV), lengths=lens).clone()
    assert plan.frame_lengths == [149, 149, 999]
    bound = {torch.float32: 1e-4, torch.float16: 1e-3, torch.bfloat16: 3e-2}[dtype]
    for b in range(3):
        err = rel_l2(e[b].cpu(), ref[b])
        print(f"{dtype} row {b}: rel-L2 vs reference {err:.3e}")
        assert err < bound, (b, err)
    e2 = plan.embed(_noise_pad(wav, lens).to(DEV), lengths=lens)
    assert torch.equal(e, e2)


@pytest.mark.parametrize("name", ["base", "tiny"])
def test_full_lengths_equal_fixed_length_path(name):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs(name)
    N = 48000 if name == "base" else 4000
    for dtype in DTYPES:
        st = _store(cfg, ocfg, dtype)
        wav, _ = O.synth_batch(2, N, 10, seed=5)
        plan = Plan(st, 2, N, train=False)
        a = plan.embed(wav.to(DEV)).clone()
        b = plan.embed(wav.to(DEV), lengths=[N, N]).clone()
        assert torch.equal(a, b), dtype
        c = plan.embed(wav.to(DEV)).clone()                     # back on the fixed-length path
        assert torch.equal(a, c)


POOLS = ["mean+std", "mean", "max", "first", "first+cls", "last", "middle", "quantile"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pooling", POOLS)
def test_tiny_vs_oracle_at_own_lengths(dtype, pooling):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("tiny")
    st = _store(cfg, ocfg, dtype)
    lens = [4000, 3217, 1600, 401]
    wav, _ = O.synth_batch(4, 4000, 10, seed=11)
    wav = wav[:, 0]
    cls = pooling == "first+cls"
    plan = Plan(st, 4, 4000, train=False, pooling=pooling, insert_cls_token=cls)
    e = plan.embed(_noise_pad(wav, lens).to(DEV), lengths=lens).cpu()
    assert plan.frame_lengths == [cfg.num_frames(n) + cls for n in lens] and plan.frame_lengths[3] == 1 + cls
    sd = O.make_state_dict(ocfg, 20211)
    tol = {torch.float32: 1e-4, torch.float16: 3e-3, torch.bfloat16: 4e-2}[dtype]
    for b, n in enumerate(lens):
        with torch.no_grad():
            ref = O.speaker_embedding(wav[b:b + 1, :n].unsqueeze(1), sd, ocfg, pooling)
        _assert_close(e[b:b + 1], ref, tol, (pooling, n))


def test_tiny_stable_family_vs_oracle_at_own_lengths():
    import dataclasses
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.engine import Plan
    kw = dict(num_hidden_layers=3, do_stable_layer_norm=True, feat_extract_norm="layer", conv_bias=True)  # as g19_tiny_stable
    cfg, ocfg = dataclasses.replace(W2V2Config.tiny(), **kw), dataclasses.replace(O.OracleConfig.tiny(), **kw)
    st = _store(cfg, ocfg, torch.float32)
    lens = [4000, 2500, 700]
    wav, _ = O.synth_batch(3, 4000, 10, seed=12)
    wav = wav[:, 0]
    plan = Plan(st, 3, 4000, train=False)
    e = plan.embed(_noise_pad(wav, lens).to(DEV), lengths=lens).cpu()
    sd = O.make_state_dict(ocfg, 20211)
    for b, n in enumerate(lens):
        with torch.no_grad():
            ref = O.speaker_embedding(wav[b:b + 1, :n].unsqueeze(1), sd, ocfg, "mean+std")
        _assert_close(e[b:b + 1], ref, 1e-4, n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_base_vs_oracle_at_two_cropped_lengths(dtype):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("base")
    st = _store(cfg, ocfg, dtype)
    lens = [36800, 113600]                                    # 2.3 s, 7.1 s
    wav, _ = O.synth_batch(2, 113600, 10, seed=13)
    wav = wav[:, 0]
    plan = Plan(st, 2, 113600, train=False)
    e = plan.embed(_noise_pad(wav, lens).to(DEV), lengths=lens).cpu()
    sd = O.make_state_dict(ocfg, 20211)
    for b, n in enumerate(lens):
        with torch.no_grad():
            ref = O.speaker_embedding(wav[b:b + 1, :n].unsqueeze(1), sd, ocfg, "mean+std")
        err = rel_l2(e[b:b + 1], ref)
        print(f"base {dtype} {n} samples: rel-L2 vs oracle {err:.3e}")
        assert err < {torch.float32: 1e-4, torch.float16: 1e-3}[dtype], (n, err)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_independence_against_b1_plans(dtype):
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("base")
    st = _store(cfg, ocfg, dtype)
    lens = [64000, 400, 20000, 52000, 33333]
    wav, _ = O.synth_batch(len(lens), 64000, 10, seed=14)
    wav = wav[:, 0]
    e = Plan(st, len(lens), 64000, train=False).embed(_noise_pad(wav, lens).to(DEV), lengths=lens).cpu()
    bound = {torch.float32: 1e-5, torch.float16: 2e-3, torch.bfloat16: 3e-2}[dtype]
    for b, n in enumerate(lens):
        ref = Plan(st, 1, n, train=False).embed(wav[b:b + 1, :n].contiguous().to(DEV)).cpu()
        _assert_close(e[b:b + 1], ref, bound, n)


def test_unsupported_configurations_raise():
    from w2v2_speaker_amd.engine import Plan
    cfg, ocfg = _cfgs("tiny")
    st = _store(cfg, ocfg, torch.float32)
    wav = torch.randn(2, 4000, device=DEV)
    with pytest.raises(NotImplementedError):
        Plan(st, 2, 4000, train=True).forward(wav, lengths=[4000, 3000])
    with pytest.raises(NotImplementedError):
        Plan(st, 2, 4000, train=False, paired=True).forward(torch.randn(4, 4000, device=DEV), lengths=[4000, 3000])
    for pooling in ("random", "none"):
        with pytest.raises(NotImplementedError):
            Plan(st, 2, 4000, train=False, pooling=pooling).embed(wav, lengths=[4000, 3000])
    plan = Plan(st, 2, 4000, train=False)
    with pytest.raises(ValueError):
        plan.embed(wav, lengths=[4001, 3000])
    with pytest.raises(ValueError):
        plan.embed(wav, lengths=[4000, 399])


# ------------------------------------------------------------------------------------------------ module surface
def _tiny_module(dtype=torch.float32, **cfg_kw):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    cfg, ocfg = W2V2Config.tiny(), O.OracleConfig.tiny()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: cfg)
    try:
        mod = Wav2vec2FCModule.from_config(Wav2vec2FCModuleConfig(reset_weights=True, **cfg_kw), num_speakers=6,
                                           device=DEV, act_dtype=dtype)
    finally:
        W2V2Config.from_huggingface_id = orig
    sd = O.make_state_dict(ocfg, 20211)
    mod.store.load_state_dict({"wav2vec.model." + k: v for k, v in sd.items()}, strict=False)
    return mod


@pytest.mark.parametrize("dtype", DTYPES)
def test_compute_speaker_embeddings_matches_per_utterance(dtype):
    from w2v2_speaker_amd.eval_batching import plan_batches
    mod = _tiny_module(dtype, hidden_fc_layers_out=[48, 128], embedding_layer_idx=0) if dtype == torch.float32 \
        else _tiny_module(dtype)
    r = np.random.default_rng(7)
    lens = [int(n) for n in r.integers(401, 9000, 40)]
    wavs = [torch.randn(n, generator=torch.Generator().manual_seed(i)) for i, n in enumerate(lens)]
    wavs[3] = wavs[3][None]                                   # [1, N] is accepted too
    kw = dict(quantum=1600, max_batch_samples=8 * 4000, max_batch=8)
    got = mod.compute_speaker_embeddings(wavs, **kw)
    assert mod.bucket_plans_built <= len({(n, b) for _, n, b in plan_batches(lens, **kw)})
    bound = {torch.float32: 1e-5, torch.float16: 2e-3, torch.bfloat16: 3e-2}[dtype]
    for w, e in zip(wavs, got):
        ref = mod.compute_speaker_embedding(w)
        assert e.shape == ref.shape
        _assert_close(e, ref, bound)


def test_evaluate_trials_matches_per_utterance_path():
    from w2v2_speaker_amd.data.synthetic import synth_trial_set
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    mod = _tiny_module()
    wav, _, keys, trials = synth_trial_set(n_speakers=4, utts_per_speaker=3, n_samples=8000)
    r = np.random.default_rng(3)
    audio = {k: torch.from_numpy(wav[i, :int(r.integers(1200, 8000))].copy()) for i, k in enumerate(keys)}
    pairs = [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]
    got = mod.evaluate_trials(pairs, audio, quantum=800, max_batch_samples=4 * 8000, max_batch=4)
    outs = [{"embedding": mod.compute_speaker_embedding(audio[k]).cpu(), "sample_id": [k]} for k in keys]
    ref = mod._evaluate_embeddings(outs, pairs)
    assert set(got) == set(ref)
    for k in ref:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        if "eer" in k.lower():
            assert abs(float(a) - float(b)) <= 1.0 / len(pairs) + 1e-9, k
        else:
            assert np.allclose(a, b, atol=1e-4), k
