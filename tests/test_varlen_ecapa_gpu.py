"""Batched variable-length evaluation of ECAPA-TDNN and of attentive statistics pooling on the GPU: the length-aware
kernels against the fixed-length kernels on each utterance alone, EcapaPlan.embed(lengths=) and
Plan.embed(lengths=, pooling="attentive") against the batch-size-1 plans and a float64 evaluation-mode restatement, and
the module surface (compute_speaker_embeddings, evaluate_trials)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import ecapa_oracle as E
from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
EDGES = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65]
# batch row against the (1, L_b) plan of the same build: the bounds of tests/test_varlen_gpu.py for this comparison
B1_BOUND = {torch.float32: 1e-5, torch.float16: 2e-3, torch.bfloat16: 3e-2}


def _i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device=DEV)


def _noise_pad(x, lens, seed=1):
    """[B, T, ...] with the frames past lens[b] of each row filled with N(0, 10^2) noise (finite in every dtype)."""
    g = torch.Generator().manual_seed(seed)
    out = x.clone()
    for b, n in enumerate(lens):
        out[b, n:] = 10 * torch.randn(out[b, n:].shape, generator=g)
    return out


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dil", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [3, 5])
def test_im2col_reflect_len_bit_identical_and_padding_rows_zero(dtype, k, dil):
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.ecapa import EcapaConfig, ecapa_min_frames
    T, C, ld = 150, 16, 48
    pad = dil * (k - 1) // 2
    lens = [T, max(ecapa_min_frames(EcapaConfig()), pad + 1), pad + 1, pad + 2, 23, 149]
    B = len(lens)
    g = torch.Generator().manual_seed(10 * k + dil)
    parent = _noise_pad(torch.randn(B, T, ld, generator=g), lens).to(DEV).to(dtype).view(B * T, ld)
    x, x2 = parent[:, 8:8 + C], parent[:, 32:32 + C]          # row-strided views, like the Res2Net slices
    for second in (None, x2):
        col = torch.full((B * T, k * C), 7.0, device=DEV, dtype=dtype)
        ops.im2col_reflect_len(x, ld, col, _i32(lens), B, T, C, k, dil, second, ld if second is not None else 0)
        col = col.view(B, T, k * C)
        for b, L in enumerate(lens):
            xs = x.view(B, T, C)[b, :L].contiguous()
            ref = torch.empty(L, k * C, device=DEV, dtype=dtype)
            if second is None:
                ops.im2col_reflect(xs, C, ref, 1, L, C, k, dil)
            else:
                ops.im2col_reflect(xs, C, ref, 1, L, C, k, dil, x2.view(B, T, C)[b, :L].contiguous(), C)
            assert torch.equal(col[b, :L], ref), (k, dil, L, second is not None)
            assert not col[b, L:].any(), (k, dil, L)


@pytest.mark.parametrize("dtype", DTYPES)
def test_asp_context_len_bit_identical(dtype):
    from w2v2_speaker_amd import ops
    T, C = 70, 72
    lens = EDGES + [T]
    B = len(lens)
    x = _noise_pad(torch.randn(B, T, C, generator=torch.Generator().manual_seed(2)), lens).to(DEV).to(dtype)
    ctx = torch.full((B, 2 * C), 5.0, device=DEV)
    ops.asp_context_len(x.view(B * T, C), ctx, _i32(lens), B, T, C)
    for b, L in enumerate(lens):
        ref = torch.empty(1, 2 * C, device=DEV)
        ops.asp_context(x[b, :L].contiguous(), ref, 1, L, C)
        assert torch.equal(ctx[b:b + 1], ref), L


@pytest.mark.parametrize("dtype", DTYPES)
def test_asp_pool_fwd_len_bit_identical(dtype):
    from w2v2_speaker_amd import ops
    T, C = 70, 72
    lens = EDGES + [T]
    B = len(lens)
    g = torch.Generator().manual_seed(3)
    x = _noise_pad(torch.randn(B, T, C, generator=g), lens).to(DEV).to(dtype)
    s = _noise_pad(3 * torch.randn(B, T, C, generator=g), lens, seed=2).to(DEV).to(dtype)
    out = torch.full((B, 2 * C), 5.0, device=DEV)
    stats = torch.full((B, C, 2), 5.0, device=DEV)
    ops.asp_pool_fwd_len(x.view(B * T, C), s.view(B * T, C), out, stats, _i32(lens), B, T, C)
    for b, L in enumerate(lens):
        ro, rs = torch.empty(1, 2 * C, device=DEV), torch.empty(1, C, 2, device=DEV)
        ops.asp_pool_fwd(x[b, :L].contiguous(), s[b, :L].contiguous(), ro, rs, 1, L, C)
        assert torch.equal(out[b:b + 1], ro), L
        assert torch.equal(stats[b:b + 1], rs), L


def test_len_entries_at_full_lengths_equal_the_fixed_length_entries():
    """The two forms of an operation are instantiations of one kernel body: with lens = [T] * B the variable-length
    entry must give the bits of the fixed-length entry."""
    from w2v2_speaker_amd import ops
    g = torch.Generator().manual_seed(7)
    for dtype in DTYPES:
        B, T, C = 2, 19, 72                                   # a partial 64-channel block, T no multiple of 8 time lanes
        lens = _i32([T] * B)
        x = torch.randn(B, T, C, generator=g).to(DEV).to(dtype)
        s = (3 * torch.randn(B, T, C, generator=g)).to(DEV).to(dtype)
        ctx, ref = torch.full((B, 2 * C), 7.0, device=DEV), torch.full((B, 2 * C), 5.0, device=DEV)
        ops.asp_context_len(x.view(B * T, C), ctx, lens, B, T, C)
        ops.asp_context(x.view(B * T, C), ref, B, T, C)
        assert torch.equal(ctx, ref), dtype
        out, ro = torch.full((B, 2 * C), 7.0, device=DEV), torch.full((B, 2 * C), 5.0, device=DEV)
        stats, rs = torch.full((B, C, 2), 7.0, device=DEV), torch.full((B, C, 2), 5.0, device=DEV)
        ops.asp_pool_fwd_len(x.view(B * T, C), s.view(B * T, C), out, stats, lens, B, T, C)
        ops.asp_pool_fwd(x.view(B * T, C), s.view(B * T, C), ro, rs, B, T, C)
        assert torch.equal(out, ro) and torch.equal(stats, rs), dtype
        B, T, C, k, dil = 2, 23, 32, 3, 2                     # more than one workgroup, the last one partial
        lens = _i32([T] * B)
        x = torch.randn(B * T, C, generator=g).to(DEV).to(dtype)
        x2 = torch.randn(B * T, C, generator=g).to(DEV).to(dtype)
        for second in (None, x2):
            col = torch.full((B * T, k * C), 7.0, device=DEV, dtype=dtype)
            ref = torch.full_like(col, 5.0)
            ops.im2col_reflect_len(x, C, col, lens, B, T, C, k, dil, second, C if second is not None else 0)
            ops.im2col_reflect(x, C, ref, B, T, C, k, dil, second, C if second is not None else 0)
            assert torch.equal(col, ref), (dtype, second is not None)


# ------------------------------------------------------------------------------------------------ ECAPA engine
def _running(name, C, seed=20211):
    """Seeded, non-trivial BatchNorm running statistics {mean[C], var[C]}."""
    return torch.cat([0.2 * O.synth_tensor(name + ".running_mean", (C,), seed),
                      0.5 + O.synth_tensor(name + ".running_var", (C,), seed).abs()])


def _ecapa_store(dtype, full=False, classes=9):
    from w2v2_speaker_amd.ecapa import EcapaConfig, EcapaStore
    cfg, ocfg = (EcapaConfig(), E.EcapaConfig()) if full else (EcapaConfig.tiny(), E.EcapaConfig.tiny())
    st = EcapaStore(cfg, DEV, dtype, num_speakers=classes)
    sd = E.make_state_dict(ocfg, 20211)
    full_sd = dict(sd)
    full_sd["loss_fn.fc_weights"] = O.synth_tensor("loss_fn.fc_weights", (classes, cfg.lin_neurons), 20211)
    st.load_state_dict(full_sd)
    run = {}
    for n, r in st.bn_running.items():
        run[n] = _running(n, r.numel() // 2)
        r.copy_(run[n].to(DEV))
    return cfg, ocfg, st, sd, run


def _feats(cfg, B, T, seed=3):
    return torch.randn(B, T, cfg.input_mel_coefficients, generator=torch.Generator().manual_seed(seed))


ECAPA_DTYPES = [torch.float32, torch.bfloat16]               # the two the ECAPA store accepts


@pytest.mark.parametrize("dtype", ECAPA_DTYPES)
def test_ecapa_padding_content_is_irrelevant_and_full_lengths_equal_fixed_path(dtype):
    from w2v2_speaker_amd.ecapa import EcapaPlan, ecapa_min_frames
    cfg, _, st, _, _ = _ecapa_store(dtype)
    B, T = 5, 120
    lens = [T, ecapa_min_frames(cfg), 6, 77, 119]
    feat = _feats(cfg, B, T)
    plan = EcapaPlan(st, B, T, train=False)
    zero_pad = feat.clone()
    for b, n in enumerate(lens):
        zero_pad[b, n:] = 0
    a = plan.embed(zero_pad.to(DEV), lengths=lens).clone()
    assert plan.frame_lengths == lens
    b_ = plan.embed(_noise_pad(feat, lens).to(DEV), lengths=torch.tensor(lens)).clone()
    assert torch.isfinite(a).all() and torch.equal(a, b_)
    fixed = plan.embed(feat.to(DEV)).clone()
    assert plan.frame_lengths is None
    full = plan.embed(feat.to(DEV), lengths=[T] * B).clone()
    assert torch.equal(fixed, full)
    assert torch.equal(fixed, plan.embed(feat.to(DEV)))         # back on the fixed-length path


def _check_rows_against_b1_plans(st, cfg, lens, T, dtype, seed=5):
    from w2v2_speaker_amd.ecapa import EcapaPlan
    B = len(lens)
    feat = _feats(cfg, B, T, seed)
    e = EcapaPlan(st, B, T, train=False).embed(_noise_pad(feat, lens).to(DEV), lengths=lens).cpu()
    for b, n in enumerate(lens):
        ref = EcapaPlan(st, 1, n, train=False).embed(feat[b:b + 1, :n].contiguous().to(DEV)).cpu()
        err = rel_l2(e[b:b + 1], ref)
        print(f"ecapa {dtype} row {b} ({n} of {T} frames): rel-L2 vs the (1, {n}) plan {err:.3e}")
        assert err < B1_BOUND[dtype], (n, err)


@pytest.mark.parametrize("dtype", ECAPA_DTYPES)
def test_ecapa_tiny_batch_independence_against_b1_plans(dtype):
    from w2v2_speaker_amd.ecapa import ecapa_min_frames
    cfg, _, st, _, _ = _ecapa_store(dtype)
    _check_rows_against_b1_plans(st, cfg, [200, ecapa_min_frames(cfg), 9, 64, 131, 199], 200, dtype)


@pytest.mark.parametrize("dtype", ECAPA_DTYPES)
def test_ecapa_full_width_batch_independence_against_b1_plans(dtype):
    cfg, _, st, _, _ = _ecapa_store(dtype, full=True)
    assert cfg.channels[0] == 1024
    _check_rows_against_b1_plans(st, cfg, [400, 100, 257, 333], 400, dtype)


# evaluation-mode restatement (BatchNorm1d.eval(): running statistics) of oracle/ecapa_oracle.py, whose BatchNorm is the
# training-mode one; the convolution, SE and tensor layout pieces are the oracle's own
def _bn_eval(x, gamma, beta, run):
    C = gamma.numel()
    return (x - run[:C]) / torch.sqrt(run[C:] + E.BN_EPS) * gamma + beta


def _tdnn_eval(x, sd, run, p, dil):
    y = E.conv1d_same_reflect(x, sd[p + "conv.conv.weight"], sd[p + "conv.conv.bias"], dil)
    return _bn_eval(F.relu(y), sd[p + "norm.norm.weight"], sd[p + "norm.norm.bias"], run[p + "norm.norm.weight"])


def _asp_eval(x_btc, sd, run, p="asp."):
    """oracle.attentive_stat_pool with the BatchNorm of the attention TDNN in evaluation mode."""
    x = x_btc.transpose(1, 2)
    T = x.shape[2]
    mean = x.mean(dim=2, keepdim=True)
    std = torch.sqrt(((x - mean) ** 2).mean(dim=2, keepdim=True).clamp(1e-12))
    a = F.conv1d(torch.cat([x, mean.expand(-1, -1, T), std.expand(-1, -1, T)], dim=1), sd[p + "tdnn.conv.conv.weight"],
                 sd[p + "tdnn.conv.conv.bias"])
    a = _bn_eval(F.relu(a).transpose(1, 2), sd[p + "tdnn.norm.norm.weight"], sd[p + "tdnn.norm.norm.bias"],
                 run[p + "tdnn.norm.norm.weight"]).transpose(1, 2)
    a = F.conv1d(torch.tanh(a), sd[p + "conv.conv.weight"], sd[p + "conv.conv.bias"])
    w = torch.softmax(a, dim=2)
    wmean = (w * x).sum(dim=2)
    wstd = torch.sqrt(((w * (x - wmean[:, :, None]) ** 2).sum(dim=2)).clamp(1e-12))
    return torch.cat([wmean, wstd], dim=1)


def _ecapa_eval_f64(feat, sd, run, ocfg):
    """[1, L, n_mels] -> (pooled [1, 2C], embedding [1, lin_neurons]) in float64, every BatchNorm on running statistics."""
    sd = {k: v.double() for k, v in sd.items()}
    run = {k: v.double() for k, v in run.items()}
    x = _tdnn_eval(feat.double(), sd, run, "blocks.0.", ocfg.dilations[0])
    outs = []
    for i in range(1, len(ocfg.channels) - 1):
        p = f"blocks.{i}."
        y = _tdnn_eval(x, sd, run, p + "tdnn1.", 1)
        ys, y_i = [], None
        for j, x_j in enumerate(torch.chunk(y, ocfg.res2net_scale, dim=2)):
            if j == 0:
                y_i = x_j
            else:
                y_i = _tdnn_eval(x_j if j == 1 else x_j + y_i, sd, run, p + f"res2net_block.blocks.{j - 1}.",
                                 ocfg.dilations[i])
            ys.append(y_i)
        y = _tdnn_eval(torch.cat(ys, dim=2), sd, run, p + "tdnn2.", 1)
        x = E.se_block(y, sd, p + "se_block.") + x
        outs.append(x)
    x = _tdnn_eval(torch.cat(outs, dim=2), sd, run, "mfa.", ocfg.dilations[-1])
    pooled = _asp_eval(x, sd, run)
    e = _bn_eval(pooled, sd["asp_bn.norm.weight"], sd["asp_bn.norm.bias"], run["asp_bn.norm.weight"])
    return pooled, e @ sd["fc.conv.weight"][:, :, 0].t() + sd["fc.conv.bias"]


def test_ecapa_f32_against_float64_restatement_at_own_lengths():
    """Tolerances: the f32 stage checks of tests/test_ecapa_gpu.py (pooled statistics 5e-5, embedding 1e-4)."""
    from w2v2_speaker_amd.ecapa import FE, EcapaPlan, ecapa_min_frames
    cfg, ocfg, st, sd, run = _ecapa_store(torch.float32)
    run = {n[len(FE):]: v for n, v in run.items()}
    T = 90
    lens = [T, ecapa_min_frames(cfg), 8, 41, 89]
    feat = _feats(cfg, len(lens), T, seed=8)
    plan = EcapaPlan(st, len(lens), T, train=False)
    e = plan.embed(_noise_pad(feat, lens).to(DEV), lengths=lens).cpu()
    pooled = plan.pooled.cpu()
    for b, n in enumerate(lens):
        with torch.no_grad():
            rp, re = _ecapa_eval_f64(feat[b:b + 1, :n], sd, run, ocfg)
        ep, ee = rel_l2(pooled[b:b + 1], rp), rel_l2(e[b:b + 1], re)
        print(f"ecapa f32 row {b} ({n} frames): pooled {ep:.3e}, embedding {ee:.3e} vs float64")
        assert ep < 5e-5 and ee < 1e-4, (n, ep, ee)


def test_ecapa_refusals():
    from w2v2_speaker_amd.ecapa import EcapaPlan, ecapa_min_frames
    cfg, _, st, _, _ = _ecapa_store(torch.float32)
    feat = _feats(cfg, 2, 50).to(DEV)
    with pytest.raises(NotImplementedError):
        EcapaPlan(st, 2, 50, train=True).embed(feat, lengths=[50, 40])
    plan = EcapaPlan(st, 2, 50, train=False)
    with pytest.raises(ValueError):
        plan.embed(feat, lengths=[50])
    with pytest.raises(ValueError):
        plan.embed(feat, lengths=[51, 40])
    with pytest.raises(ValueError):
        plan.embed(feat, lengths=[50, ecapa_min_frames(cfg) - 1])
    assert torch.isfinite(plan.embed(feat, lengths=[50, ecapa_min_frames(cfg)])).all()


# ------------------------------------------------------------------------------------------------ attentive wav2vec2
def _attentive_store(dtype):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    cfg, ocfg = W2V2Config.tiny(), O.OracleConfig.tiny()
    st = ParamStore(cfg, DEV, dtype, head=None, attentive_pool=True)
    st.init_weights(20211)                                    # (the six pooling tensors)
    st.load_state_dict({"wav2vec.model." + k: v for k, v in O.make_state_dict(ocfg, 20211).items()}, strict=False)
    st.asp_running.copy_(_running("asp", st.asp_running.numel() // 2).to(DEV))
    return cfg, st


@pytest.mark.parametrize("dtype", DTYPES)
def test_attentive_plan_padding_irrelevant_full_lengths_and_b1_plans(dtype):
    from w2v2_speaker_amd.engine import Plan
    cfg, st = _attentive_store(dtype)
    N = 4000
    lens = [4000, 3217, 1600, 401]
    wav, _ = O.synth_batch(4, N, 10, seed=11)
    wav = wav[:, 0]
    plan = Plan(st, 4, N, train=False, pooling="attentive")
    a = plan.embed(wav.to(DEV), lengths=lens).clone()
    assert plan.frame_lengths == [cfg.num_frames(n) for n in lens]
    b_ = plan.embed(_noise_pad(wav, lens).to(DEV), lengths=lens).clone()
    assert torch.isfinite(a).all() and torch.equal(a, b_)
    fixed = plan.embed(wav.to(DEV)).clone()
    assert torch.equal(fixed, plan.embed(wav.to(DEV), lengths=[N] * 4))
    for b, n in enumerate(lens):
        ref = Plan(st, 1, n, train=False, pooling="attentive").embed(wav[b:b + 1, :n].contiguous().to(DEV)).cpu()
        err = rel_l2(a[b:b + 1].cpu(), ref)
        print(f"attentive {dtype} row {b} ({n} samples): rel-L2 vs the (1, {n}) plan {err:.3e}")
        assert err < B1_BOUND[dtype], (n, err)


def test_wav2vec2_random_and_none_pooling_still_refuse_lengths():
    from w2v2_speaker_amd.engine import Plan
    _, st = _attentive_store(torch.float32)
    wav = torch.randn(2, 4000, device=DEV)
    for pooling in ("random", "none"):
        with pytest.raises(NotImplementedError):
            Plan(st, 2, 4000, train=False, pooling=pooling).embed(wav, lengths=[4000, 3000])
    with pytest.raises(NotImplementedError):
        Plan(st, 2, 4000, train=True, pooling="attentive").embed(wav, lengths=[4000, 3000])


# ------------------------------------------------------------------------------------------------ module surface
def _ecapa_module(dtype):
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTDNNModuleConfig, EcapaTdnnModule
    c = E.EcapaConfig.tiny()
    mcfg = EcapaTDNNModuleConfig(input_mel_coefficients=c.input_size, lin_neurons=c.lin_neurons, channels=list(c.channels),
                                 kernel_sizes=list(c.kernel_sizes), dilations=list(c.dilations),
                                 attention_channels=c.attention_channels, res2net_scale=c.res2net_scale,
                                 se_channels=c.se_channels)
    mod = EcapaTdnnModule.from_config(mcfg, num_speakers=6, device=DEV, act_dtype=dtype)
    mod.store.load_state_dict(E.make_state_dict(c, 20211), strict=False)
    for n, r in mod.store.bn_running.items():
        r.copy_(_running(n, r.numel() // 2).to(DEV))
    return mod


@pytest.mark.parametrize("dtype", ECAPA_DTYPES)
def test_ecapa_compute_speaker_embeddings_matches_per_utterance(dtype):
    from w2v2_speaker_amd.eval_batching import plan_batches
    mod = _ecapa_module(dtype)
    F_ = mod.cfg.input_mel_coefficients
    r = np.random.default_rng(7)
    lens = [int(n) for n in r.integers(5, 260, 40)]
    feats = [torch.randn(n, F_, generator=torch.Generator().manual_seed(i)) for i, n in enumerate(lens)]
    feats[3] = feats[3][None]                                 # [1, T, n_mels] is accepted too
    kw = dict(quantum=40, max_batch_frames=8 * 120, max_batch=8)
    got = mod.compute_speaker_embeddings(feats, **kw)
    assert mod.bucket_plans_built <= len({(n, b) for _, n, b in plan_batches(lens, 40, 8 * 120, 8)})
    for f, e in zip(feats, got):
        ref = mod.compute_speaker_embedding(f)
        assert e.shape == ref.shape
        err = rel_l2(e.cpu(), ref.cpu())
        assert err < B1_BOUND[dtype], (tuple(f.shape), err)


def _trial_set(make_input, lo, hi):
    from w2v2_speaker_amd.data.synthetic import synth_trial_set
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    wav, _, keys, trials = synth_trial_set(n_speakers=4, utts_per_speaker=3, n_samples=8000)
    r = np.random.default_rng(3)
    inputs = {k: make_input(torch.from_numpy(wav[i].copy()), int(r.integers(lo, hi))) for i, k in enumerate(keys)}
    return keys, inputs, [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]


def _assert_same_scores(got, ref, n_pairs):
    assert set(got) == set(ref)
    for k in ref:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        if "eer" in k.lower():
            assert abs(float(a) - float(b)) <= 1.0 / n_pairs + 1e-9, k
        else:
            assert np.allclose(a, b, atol=1e-4), k


def test_ecapa_evaluate_trials_matches_per_utterance_path():
    mod = _ecapa_module(torch.float32)
    F_ = mod.cfg.input_mel_coefficients
    keys, feats, pairs = _trial_set(lambda w, n: w[:n * F_].view(n, F_), 20, 400)     # frames cut out of the waveform
    got = mod.evaluate_trials(pairs, feats, quantum=50, max_batch_frames=4 * 400, max_batch=4)
    outs = [{"embedding": mod.compute_speaker_embedding(feats[k]).cpu(), "sample_id": [k]} for k in keys]
    _assert_same_scores(got, mod._evaluate_embeddings(outs, pairs), len(pairs))


def _attentive_module(dtype):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    cfg, ocfg = W2V2Config.tiny(), O.OracleConfig.tiny()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: cfg)
    try:
        mod = Wav2vec2FCModule.from_config(Wav2vec2FCModuleConfig(reset_weights=True, stat_pooling_type="attentive",
                                                                  test_stat_pooling_type="attentive"),
                                           num_speakers=6, device=DEV, act_dtype=dtype)
    finally:
        W2V2Config.from_huggingface_id = orig
    sd = O.make_state_dict(ocfg, 20211)
    mod.store.load_state_dict({"wav2vec.model." + k: v for k, v in sd.items()}, strict=False)
    mod.store.asp_running.copy_(_running("asp", mod.store.asp_running.numel() // 2).to(DEV))
    return mod


@pytest.mark.parametrize("dtype", DTYPES)
def test_attentive_module_compute_speaker_embeddings_matches_per_utterance(dtype):
    from w2v2_speaker_amd.eval_batching import plan_batches
    mod = _attentive_module(dtype)
    r = np.random.default_rng(7)
    lens = [int(n) for n in r.integers(401, 9000, 40)]
    wavs = [torch.randn(n, generator=torch.Generator().manual_seed(i)) for i, n in enumerate(lens)]
    kw = dict(quantum=1600, max_batch_samples=8 * 4000, max_batch=8)
    got = mod.compute_speaker_embeddings(wavs, **kw)
    assert mod.bucket_plans_built <= len({(n, b) for _, n, b in plan_batches(lens, **kw)})
    for w, e in zip(wavs, got):
        ref = mod.compute_speaker_embedding(w)
        assert e.shape == ref.shape
        err = rel_l2(e.cpu(), ref.cpu())
        assert err < B1_BOUND[dtype], (w.shape[0], err)


def test_attentive_module_evaluate_trials_matches_per_utterance_path():
    mod = _attentive_module(torch.float32)
    keys, audio, pairs = _trial_set(lambda w, n: w[:n], 1200, 8000)
    got = mod.evaluate_trials(pairs, audio, quantum=800, max_batch_samples=4 * 8000, max_batch=4)
    outs = [{"embedding": mod.compute_speaker_embedding(audio[k]).cpu(), "sample_id": [k]} for k in keys]
    _assert_same_scores(got, mod._evaluate_embeddings(outs, pairs), len(pairs))
