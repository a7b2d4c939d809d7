"""Device log-mel filterbank front-end (csrc/fbank.hip) on the GPU: both stages against a float64 restatement within ten
times the host f32 path's own error, the variable-length contract bit for bit, the output forms, and the waveform paths
of EcapaPlan, EcapaTrainer and EcapaTdnnModule against their filterbank-tensor paths.

Lines that start with ``fbank-parity:`` are the measured figures recorded in profiles/fbank_parity.txt."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_varlen_ecapa_gpu import B1_BOUND, _running

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOP, WIN, TILE = 160, 400, 16
KINDS = ["noise", "speech", "gap"]
# the lengths around the one- / two- / three-hop boundaries, and the three that straddle the kernel's frame tile
LENGTHS = [640, 799, 800, 801, 959, 960, 961, 1000, HOP * TILE - 1, HOP * TILE, HOP * TILE + 1, 4000, 48000]
VARLEN_N = 10400
VARLEN_LENS = [10400, 640, 801, 960, 4000, 10239, 10240, 10241]
FACTOR = 10.0                 # device error <= FACTOR x the host f32 path's error against the same float64 restatement
MIN_STD_DB = 1.0              # every mel channel of a test signal spreads at least this much over its frames (float64)

_FB = {}


def _fb(n_mels=40):
    from w2v2_speaker_amd.data.fbank import Fbank
    if n_mels not in _FB:
        _FB[n_mels] = Fbank(n_mels=n_mels)
    return _FB[n_mels]


# ------------------------------------------------------------------------------------------------ signals, references
def _znorm(x):
    return (x - x.mean()) / (x.std() + 1e-5)


def _raw_signal(kind, n, seed):
    """z-normalised like the pipeline's waveforms.  noise: white; speech: six harmonics between 130 and 3400 Hz under a 3 Hz
    squared-sine envelope + 5 % noise + a 1e-3 noise floor; gap: white noise with x[n // 3 : n // 2] = 0 exactly."""
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return _znorm(torch.randn(n, generator=g))
    if kind == "speech":
        t = torch.arange(n, dtype=torch.float64) / 16000.0
        x = sum(torch.sin(2 * math.pi * f * t + i) / (i + 1)
                for i, f in enumerate((130.0, 260.0, 520.0, 1100.0, 2300.0, 3400.0)))
        x = (x * torch.sin(2 * math.pi * 3.0 * t) ** 2).float()
        return _znorm(x + 0.05 * torch.randn(n, generator=g) + 1e-3 * torch.randn(n, generator=g))
    assert kind == "gap"
    x = torch.randn(n, generator=g)
    x[n // 3:n // 2] = 0.0
    x = _znorm(x)
    x[n // 3:n // 2] = 0.0
    return x


def _f64_stages(x, fb):
    """The float64 restatement: torch.stft in double on the CPU, then the lines of data/fbank.py and of
    InputNormalizer2D(True).  -> (dB before the clamp, clamped dB, normalised), all [F, n_mels] float64."""
    spec = torch.stft(x.double(), fb.n_fft, hop_length=fb.hop, win_length=fb.win, window=fb.window.double(), center=True,
                      pad_mode="constant", normalized=False, onesided=True, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2
    mel = power.t() @ fb.fbank.double()
    raw = 10.0 * torch.log10(torch.clamp(mel, min=fb.amin))
    db = torch.maximum(raw, raw.max() - fb.top_db)
    std, mean = torch.std_mean(db, dim=0)
    return raw, db, (db - mean) / (std + 1e-5)


def _host_f32_stages(x, fb):
    from w2v2_speaker_amd.data.pipeline import InputNormalizer2D
    db = fb(x)
    return db, InputNormalizer2D.normalize(db, True)[0]


def _signal(kind, n, n_mels=40, base=0):
    """The first seed (base + n, base + n + 1000, ...) whose float64 features spread >= MIN_STD_DB in every mel channel, so
    that 1 / (std + 1e-5) amplifies nothing; the choice looks at the float64 reference only.  -> (x, f64 stages)."""
    fb = _fb(n_mels)
    for k in range(40):
        x = _raw_signal(kind, n, base + n + 1000 * k)
        ref = _f64_stages(x, fb)
        if float(ref[1].std(dim=0).min()) >= MIN_STD_DB:
            return x, ref
    raise AssertionError(f"no {kind} signal of {n} samples with every channel spread >= {MIN_STD_DB} dB")


def _i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device=DEV)


def _front_end(wav, lens=None, n_mels=40, dtype=torch.float32, ldo=None, fill=0.0):
    """wav [B, N] (CPU) through the two kernels -> (dB before the clamp [B, T, n_mels], out [B, T, ldo]) on the CPU."""
    from w2v2_speaker_amd import ops
    assert ops.FBANK_TILE_FRAMES == TILE and (ops.FBANK_HOP, ops.FBANK_WIN) == (HOP, WIN)
    fb = _fb(n_mels)
    B, N = wav.shape
    T = 1 + N // HOP
    ldo = ldo or n_mels
    window, fbank = fb.window.to(DEV), fb.fbank.to(DEV)
    db = torch.full((B, T, n_mels), 3.0, device=DEV)
    pmax = ops.fbank_partial_max(B, T, DEV)
    ld = _i32(lens) if lens is not None else None
    ops.fbank_db(wav.to(DEV).contiguous(), ld, window, fbank, db, pmax)
    out = torch.full((B * T, ldo), fill, dtype=dtype, device=DEV)
    ops.fbank_normalize(db, pmax, ld, out, ldo)
    torch.cuda.synchronize()
    return db.cpu(), out.view(B, T, ldo).cpu()


def _clamp(db):
    return torch.maximum(db, db.max() - 80.0)


def _check_parity(tag, x, ref, n_mels=40):
    """Both stages of the device front-end on one utterance against the float64 restatement: max |error| <= FACTOR x the
    host f32 path's max |error| on the same input.  Prints the figures before it asserts."""
    fb = _fb(n_mels)
    _, ref_db, ref_norm = ref
    assert float(ref_db.std(dim=0).min()) >= MIN_STD_DB            # no (nearly) constant channel
    host_db, host_norm = _host_f32_stages(x, fb)
    dev_raw, dev_norm = _front_end(x[None], n_mels=n_mels)
    assert dev_raw.shape[1:] == ref_db.shape == host_db.shape
    e_host_db = float((host_db.double() - ref_db).abs().max())
    e_host_norm = float((host_norm.double() - ref_norm).abs().max())
    e_dev_db = float((_clamp(dev_raw[0]).double() - ref_db).abs().max())
    e_dev_norm = float((dev_norm[0].double() - ref_norm).abs().max())
    print(f"fbank-parity: {tag} n={x.numel()} n_mels={n_mels}: dB stage device {e_dev_db:.3e} host {e_host_db:.3e} "
          f"(x{e_dev_db / e_host_db:.2f}); normalised device {e_dev_norm:.3e} host {e_host_norm:.3e} "
          f"(x{e_dev_norm / e_host_norm:.2f})")
    assert e_host_db > 0 and e_host_norm > 0
    assert torch.isfinite(dev_raw).all() and torch.isfinite(dev_norm).all()
    assert e_dev_db <= FACTOR * e_host_db, (tag, x.numel(), e_dev_db, e_host_db)
    assert e_dev_norm <= FACTOR * e_host_norm, (tag, x.numel(), e_dev_norm, e_host_norm)


# ------------------------------------------------------------------------------------------------ 1: stage parity
@pytest.mark.parametrize("kind", KINDS)
def test_stage_parity_against_float64_within_ten_host_errors(kind):
    for n in LENGTHS:
        x, ref = _signal(kind, n)
        if kind == "gap":
            assert not x[n // 3:n // 2].any()
            share = float((ref[0] < ref[0].max() - 80.0).double().mean())
            print(f"fbank-parity: gap n={n}: {100 * share:.1f} % of the cells clamped")
            if n // 2 - n // 3 >= WIN + HOP:        # the gap holds a whole window: all-zero frames at the 1e-10 floor
                assert share > 0, n
        _check_parity(kind, x, ref)


# ------------------------------------------------------------------------------------------------ 2: variable length
def _varlen_batch(order):
    g = torch.Generator().manual_seed(77)
    utts = [_raw_signal(KINDS[i % 3], n, 500 + i) for i, n in enumerate(VARLEN_LENS)]
    wav = 10.0 * torch.randn(len(utts), VARLEN_N, generator=g)       # samples past n_b: N(0, 10^2)
    for row, i in enumerate(order):
        wav[row, :VARLEN_LENS[i]] = utts[i]
    return utts, wav, [VARLEN_LENS[i] for i in order]


def test_variable_length_rows_bit_identical_to_the_utterance_alone():
    B = len(VARLEN_LENS)
    order = list(range(B))
    utts, wav, lens = _varlen_batch(order)
    raw, out = _front_end(wav, lens, fill=5.0)
    utts_r, wav_r, lens_r = _varlen_batch(order[::-1])
    raw_r, out_r = _front_end(wav_r, lens_r, fill=5.0)
    for b, n in enumerate(VARLEN_LENS):
        F = 1 + n // HOP
        alone_raw, alone = _front_end(utts[b][None], fill=5.0)
        assert alone.shape[1] == F
        assert torch.isfinite(alone).all()
        assert torch.equal(raw[b, :F], alone_raw[0]), n
        assert torch.equal(out[b, :F], alone[0]), n
        assert not out[b, F:].any(), n
        rb = B - 1 - b
        assert torch.equal(out_r[rb], out[b]) and torch.equal(raw_r[rb, :F], raw[b, :F]), n
    # lens = N for every row is the call without lens
    full = torch.stack([_raw_signal("noise", 4000, s) for s in (1, 2)])
    assert torch.equal(_front_end(full, [4000, 4000])[1], _front_end(full)[1])


# ------------------------------------------------------------------------------------------------ 3: output forms
def test_bf16_output_is_the_f32_output_rounded():
    wav = torch.stack([_raw_signal(k, 4000, 9) for k in KINDS])
    lens = [4000, 2561, 640]
    _, f32 = _front_end(wav, lens)
    _, b16 = _front_end(wav, lens, dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and torch.equal(b16, f32.to(torch.bfloat16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_strided_output_leaves_the_other_columns_untouched(dtype):
    wav = torch.stack([_raw_signal(k, 4000, 9) for k in KINDS])
    lens = [4000, 2561, 640]
    _, dense = _front_end(wav, lens, dtype=dtype)
    _, wide = _front_end(wav, lens, dtype=dtype, ldo=48, fill=7.0)
    assert torch.equal(wide[:, :, :40], dense)
    assert bool((wide[:, :, 40:] == 7.0).all())


@pytest.mark.parametrize("kind", KINDS)
def test_eighty_mel_channels_parity(kind):
    for n in (640, HOP * TILE + 1, 4000):
        x, ref = _signal(kind, n, n_mels=80, base=7)
        _check_parity(kind, x, ref, n_mels=80)


# ------------------------------------------------------------------------------------------------ 4: plan
def _small_cfg():
    from w2v2_speaker_amd.ecapa import EcapaConfig
    return EcapaConfig(input_mel_coefficients=40, lin_neurons=24, channels=(64, 64, 64, 64, 192), attention_channels=16,
                       res2net_scale=4, se_channels=16)


def _store(dtype, seed=20211, classes=9):
    from w2v2_speaker_amd.ecapa import EcapaStore
    st = EcapaStore(_small_cfg(), DEV, dtype, num_speakers=classes)
    st.init_weights(seed)
    for n, r in st.bn_running.items():
        r.copy_(_running(n, r.numel() // 2).to(DEV))
    return st


def _read_back(plan):
    """The front-end's own output in the plan's feature buffer as a [B, T, n_mels] f32 tensor."""
    F_ = plan.cfg.input_mel_coefficients
    return plan.feat[:, :F_].float().reshape(plan.B, plan.T, F_).clone()


def _wavs(B, N, seed=0):
    return torch.stack([_raw_signal(KINDS[b % 3], N, seed + b) for b in range(B)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plan_embed_waveform_equals_embed_of_its_own_features(dtype):
    from w2v2_speaker_amd.ecapa import EcapaPlan, fbank_frames
    st = _store(dtype)
    B, N = 3, 8000
    plan = EcapaPlan(st, B, fbank_frames(N), train=False)
    wav = _wavs(B, N).to(DEV)
    e = plan.embed_waveform(wav).clone()
    feats = _read_back(plan)
    assert torch.isfinite(e).all() and feats.abs().max() > 0.5
    assert torch.equal(plan.embed(feats), e)
    assert torch.equal(plan.embed_waveform(wav), e)
    with pytest.raises(ValueError):
        plan.embed_waveform(wav[:, :N - 200])                     # one frame fewer than the plan's


def test_plan_embed_waveform_against_host_features():
    from w2v2_speaker_amd.ecapa import EcapaPlan, fbank_frames
    st = _store(torch.float32)
    B, N = 3, 8000
    plan = EcapaPlan(st, B, fbank_frames(N), train=False)
    wav = _wavs(B, N)
    fb = _fb()
    host = torch.stack([_host_f32_stages(w, fb)[1] for w in wav])
    f64 = torch.stack([_f64_stages(w, fb)[2] for w in wav]).float()
    e_host = plan.embed(host.to(DEV)).cpu().clone()
    e_f64 = plan.embed(f64.to(DEV)).cpu().clone()
    e_dev = plan.embed_waveform(wav.to(DEV)).cpu().clone()
    bound = FACTOR * rel_l2(e_host, e_f64)
    err = rel_l2(e_dev, e_host)
    print(f"fbank-parity: plan f32 B={B} N={N}: embed_waveform vs embed(host features) rel-L2 {err:.3e}; "
          f"embed(host f32 features) vs embed(float64 features) rel-L2 {bound / FACTOR:.3e} (bound x{FACTOR:.0f})")
    assert bound > 0 and err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plan_embed_waveform_lengths_against_b1_plans(dtype):
    from w2v2_speaker_amd.ecapa import EcapaPlan, fbank_frames
    st = _store(dtype)
    N, lens = 4000, [4000, 640, 801, HOP * TILE + 1]
    B = len(lens)
    utts = [_raw_signal(KINDS[b % 3], n, 40 + b) for b, n in enumerate(lens)]
    wav = 10.0 * torch.randn(B, N, generator=torch.Generator().manual_seed(4))
    for b, u in enumerate(utts):
        wav[b, :u.numel()] = u
    plan = EcapaPlan(st, B, fbank_frames(N), train=False)
    e = plan.embed_waveform(wav.to(DEV), lengths=lens).cpu().clone()
    assert plan.frame_lengths == [fbank_frames(n) for n in lens]
    assert torch.equal(plan.embed_waveform(wav.to(DEV), lengths=torch.tensor(lens)).cpu(), e)
    for b, n in enumerate(lens):
        ref = EcapaPlan(st, 1, fbank_frames(n), train=False).embed_waveform(utts[b][None].to(DEV)).cpu()
        err = rel_l2(e[b:b + 1], ref)
        print(f"fbank-parity: plan {dtype} row {b} ({n} of {N} samples): rel-L2 vs the (1, {fbank_frames(n)}) plan {err:.3e}")
        assert err < B1_BOUND[dtype], (n, err)
    plan.embed_waveform(wav.to(DEV))
    assert plan.frame_lengths is None                            # back on the fixed-length path
    with pytest.raises(ValueError):
        plan.embed_waveform(wav.to(DEV), lengths=[4000, 639, 801, 2561])
    with pytest.raises(ValueError):
        plan.embed_waveform(wav.to(DEV), lengths=[4001, 640, 801, 2561])
    with pytest.raises(NotImplementedError):
        EcapaPlan(st, B, fbank_frames(N), train=True).embed_waveform(wav.to(DEV), lengths=lens)


# ------------------------------------------------------------------------------------------------ 5: training
def _deterministic_f32_weight_gradients(monkeypatch):
    """Exact-f32 training gives the weight gradients of a block's Res2Net chunks to ONE batched split-K product that adds
    its partial sums with f32 atomics (ecapa.py, _SERes2Net), in an order that differs from launch to launch: two steps
    from the very same features then differ in the last bit.  The plans of the two f32 tests below are built with the
    engine's switch for the per-chunk products, which have no split at this token count (f32_dw_split: fewer than 256
    tokens per split), so that bit-equality says something about the input path.  bf16 plans (atomic-free grouped
    weight gradients) run as they are."""
    monkeypatch.setenv("W2V2_ECAPA_NO_BATCHED_DW", "1")


def _trainer(dtype, B, N, accumulate=1):
    from w2v2_speaker_amd.ecapa import EcapaPlan, EcapaTrainer, fbank_frames
    from w2v2_speaker_amd.optim.schedule import Constant
    st = _store(dtype)
    plan = EcapaPlan(st, B, fbank_frames(N), train=True)
    return st, plan, EcapaTrainer(st, plan, Constant(1e-3), accumulate_grad_batches=accumulate)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_step_from_waveforms_equals_train_step_from_its_features(dtype, monkeypatch):
    _deterministic_f32_weight_gradients(monkeypatch)
    B, N = 4, 8000
    wav = _wavs(B, N, seed=20).to(DEV)
    label = torch.tensor([0, 3, 8, 3], device=DEV)
    st_w, plan_w, tr_w = _trainer(dtype, B, N)
    st_f, _, tr_f = _trainer(dtype, B, N)
    assert torch.equal(st_w.flat, st_f.flat)
    before = st_w.flat.clone()
    loss_w, _ = tr_w.train_step(wav, label)
    feats = _read_back(plan_w)
    loss_f, _ = tr_f.train_step(feats, label)
    assert math.isfinite(float(loss_w)) and float(loss_w) == float(loss_f)
    assert tr_w.stepped and tr_f.stepped and not torch.equal(st_w.flat, before)
    assert torch.equal(st_w.flat, st_f.flat)
    for n in st_w.bn_running:
        assert torch.equal(st_w.bn_running[n], st_f.bn_running[n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_accumulated_train_step_from_waveforms_equals_features(dtype, monkeypatch):
    _deterministic_f32_weight_gradients(monkeypatch)
    B, N = 4, 8000
    label = torch.tensor([1, 7, 2, 2], device=DEV)
    st_w, plan_w, tr_w = _trainer(dtype, B, N, accumulate=2)
    st_f, _, tr_f = _trainer(dtype, B, N, accumulate=2)
    before = st_w.flat.clone()
    for micro in range(2):
        wav = _wavs(B, N, seed=30 + 10 * micro).to(DEV)
        loss_w, _ = tr_w.train_step(wav, label)
        loss_f, _ = tr_f.train_step(_read_back(plan_w), label)
        assert float(loss_w) == float(loss_f)
        assert tr_w.stepped == tr_f.stepped == (micro == 1)
        if micro == 0:
            assert torch.equal(st_w.flat, before)                 # the window is still open
    assert not torch.equal(st_w.flat, before) and torch.equal(st_w.flat, st_f.flat)


# ------------------------------------------------------------------------------------------------ 6: module
def _module(dtype=torch.float32, **kw):
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTDNNModuleConfig, EcapaTdnnModule
    c = _small_cfg()
    mcfg = EcapaTDNNModuleConfig(input_mel_coefficients=c.input_mel_coefficients, lin_neurons=c.lin_neurons,
                                 channels=list(c.channels), kernel_sizes=list(c.kernel_sizes), dilations=list(c.dilations),
                                 attention_channels=c.attention_channels, res2net_scale=c.res2net_scale,
                                 se_channels=c.se_channels)
    mod = EcapaTdnnModule.from_config(mcfg, num_speakers=6, device=DEV, act_dtype=dtype, **kw)
    for n, r in mod.store.bn_running.items():
        r.copy_(_running(n, r.numel() // 2).to(DEV))
    return mod


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_module_waveform_embeddings_match_per_utterance(dtype):
    from w2v2_speaker_amd.eval_batching import plan_batches
    mod = _module(dtype, input_features="waveform")
    lens = VARLEN_LENS[1:]                                        # the seven shorter than the batch of test 2
    wavs = [_raw_signal(KINDS[i % 3], n, 60 + i) for i, n in enumerate(lens)]
    wavs[2] = wavs[2][None]                                       # [1, N] is accepted too
    kw = dict(quantum=10, max_batch_frames=4 * 70, max_batch=4)
    got = mod.compute_speaker_embeddings(wavs, **kw)
    buckets = {(n, b) for _, n, b in plan_batches(lens, 10 * HOP, 4 * 70 * HOP, 4)}
    assert all(n % HOP == 0 for n, _ in buckets) and 0 < mod.bucket_plans_built <= len(buckets)
    for w, e in zip(wavs, got):
        ref = mod.compute_speaker_embedding(w)
        assert e.shape == ref.shape == (1, 24)
        err = rel_l2(e.cpu(), ref.cpu())
        print(f"fbank-parity: module {dtype} {w.numel()} samples: bucketed vs alone rel-L2 {err:.3e}")
        assert err < B1_BOUND[dtype], (w.numel(), err)
    # the three input forms of one batch
    x = _wavs(2, 1600, seed=3)
    a = mod.compute_speaker_embedding(x)
    assert torch.equal(mod.compute_speaker_embedding(x[:, None, :]), a)
    assert torch.equal(mod.compute_speaker_embedding(x[0]), mod.compute_speaker_embedding(x[0:1]))


def test_module_waveform_trials_score_like_the_fbank_module_on_host_features():
    """EER: identical unless two scores tie within the parity of test 4 (the seeds below leave the closest pair of scores
    orders of magnitude further apart than the two modules' scores are from each other; both figures are printed)."""
    from w2v2_speaker_amd.data.synthetic import score_trials, synth_trial_set
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    wav, _, keys, trials = synth_trial_set(n_speakers=4, utts_per_speaker=2, n_samples=8000, seed=52001)
    r = np.random.default_rng(3)
    audio = {k: torch.from_numpy(wav[i, :int(r.integers(1200, 8000))].copy()) for i, k in enumerate(keys)}
    pairs = [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]
    fb = _fb()
    feats = {k: _host_f32_stages(a, fb)[1] for k, a in audio.items()}
    mod_w, mod_f = _module(input_features="waveform"), _module()
    assert mod_f.input_features == "fbank" and torch.equal(mod_w.store.flat, mod_f.store.flat)
    kw = dict(quantum=10, max_batch_frames=4 * 50, max_batch=4)
    got = mod_w.evaluate_trials(pairs, audio, **kw)
    ref = mod_f.evaluate_trials(pairs, feats, **kw)
    e_w = torch.cat(mod_w.compute_speaker_embeddings([audio[k] for k in keys], **kw)).cpu().numpy()
    e_f = torch.cat(mod_f.compute_speaker_embeddings([feats[k] for k in keys], **kw)).cpu().numpy()
    s_w, s_f = np.array(score_trials(e_w, trials)[1]), np.array(score_trials(e_f, trials)[1])
    print(f"fbank-parity: module trials: {len(pairs)} pairs, eer waveform {got['eer']} fbank {ref['eer']}; closest two "
          f"scores {np.diff(np.sort(s_f)).min():.3e} apart, waveform vs fbank scores differ by <= {np.abs(s_w - s_f).max():.3e}")
    assert set(got) == set(ref) and 0.0 <= ref["eer"] <= 1.0
    assert got["eer"] == ref["eer"]
    assert np.allclose(s_w, s_f, atol=1e-4) and np.array_equal(np.argsort(s_w), np.argsort(s_f))


def test_module_fbank_mode_is_unchanged_and_unknown_modes_are_refused():
    mod = _module()
    assert mod.input_features == "fbank"
    feat = torch.randn(2, 30, 40, generator=torch.Generator().manual_seed(1))
    e = mod.compute_speaker_embedding(feat)
    assert e.shape == (2, 24) and torch.equal(mod.compute_speaker_embedding(feat[0]), mod.compute_speaker_embedding(feat[:1]))
    got = mod.compute_speaker_embeddings([feat[0], feat[1][None, :17]])
    assert rel_l2(got[0].cpu(), mod.compute_speaker_embedding(feat[0]).cpu()) < B1_BOUND[torch.float32]
    with pytest.raises(ValueError):
        mod.compute_speaker_embeddings([torch.randn(700)])        # a waveform is no filterbank tensor
    with pytest.raises((AssertionError, ValueError, RuntimeError, IndexError)):
        mod.compute_speaker_embedding(torch.randn(2, 700))         # ... nor is a batch of them
    with pytest.raises(ValueError):
        _module(input_features="mel")
    with pytest.raises(ValueError):
        _module(input_features="waveform").compute_speaker_embeddings([feat[0]])
