"""CPU tests of the waveform augmentation: the C ABI of the new entries, the host half of data/augment.py (seeded draws
in the reference's order of np.random calls, SpecAugmentBand's arithmetic, the Augmenter's flags, row order and key
suffixes), the designed filters in float64, the resampling oracle against scipy's upfirdn, the argument errors that need
no device and the module surface.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import augment_cases as AC
from test_metrics_cpu import _c_decl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000
NEW = ("w2v2_aug_time_dropout", "w2v2_aug_mix_uniform", "w2v2_aug_mix_bank", "w2v2_aug_fir", "w2v2_aug_fir_tile",
       "w2v2_aug_resample", "w2v2_aug_resample_tile")


def test_new_symbols_declared_exported_and_wrapped_with_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32", C.c_double: "f64"}
    for name in NEW:
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        res, args = _lib._SIGS[name]
        assert (kind[res], [kind[a] for a in args]) == _c_decl(hdr, name), name
        assert args == [] or args[-1] is C.c_void_p, name                   # void* stream last
    assert _c_decl(hdr, "w2v2_aug_mix_uniform") == ("i32", ["p", "i64", "i32", "p", "p", "i32", "p", "i64", "p"])
    assert "augment.hip" in _build.SOURCES
    assert "waveform augmentation" in hdr and "THIS COMMENT IS THE DEFINITION" in hdr
    assert f"#define W2V2_AUG_MAX_TAPS {ops.AUG_MAX_TAPS}" in hdr and ops.AUG_MAX_TAPS >= 2561 and ops.AUG_MAX_TAPS % 2 == 1
    lib = _lib.load()
    assert lib.w2v2_aug_fir_tile() == ops.AUG_FIR_TILE == AC.FIR_TILE
    assert lib.w2v2_aug_resample_tile() == ops.AUG_RESAMPLE_TILE == AC.RESAMPLE_TILE
    for name in ("aug_time_dropout", "aug_mix_uniform", "aug_mix_bank", "aug_fir", "aug_resample"):
        assert callable(getattr(ops, name))


def test_ops_argument_checks_need_no_device():
    from w2v2_speaker_amd import ops
    x, rows = torch.zeros(3, 16), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="2-D float32"):
        ops.aug_time_dropout(x.double(), rows, torch.zeros(2, 1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="spans"):
        ops.aug_time_dropout(x, rows, torch.zeros(3, 1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="rows"):
        ops.aug_time_dropout(x, rows.long(), torch.zeros(2, 1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="lens"):
        ops.aug_time_dropout(x, rows, torch.zeros(2, 1, 2, dtype=torch.int32), lens=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="coef"):
        ops.aug_mix_uniform(x, rows, torch.zeros(3), 1)
    with pytest.raises(ValueError, match="bank_lens"):
        ops.aug_mix_bank(x, rows, torch.zeros(2), torch.zeros(4, 8), torch.zeros(3, dtype=torch.int32), rows)
    with pytest.raises(ValueError, match="taps"):
        ops.aug_fir(x, torch.zeros(3, 16), rows, rows, torch.zeros(3, 5), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="share memory"):
        ops.aug_fir(x, x, rows, rows, torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="U = 0"):
        ops.aug_resample(x, torch.zeros(3, 16), rows, rows, 0, 1)
    with pytest.raises(ValueError, match="h is"):
        ops.aug_resample(x, torch.zeros(3, 16), rows, rows, 2, 1, torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.aug_resample(x, torch.zeros(3, 16), rows, rows, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.aug_time_dropout(x, rows, torch.zeros(2, 0, 2, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ seeded draws
class _Recorder:
    """Stands in for np.random inside data/augment.py: forwards to a RandomState and writes down every call."""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def __getattr__(self, name):
        fn = getattr(self.rs, name)

        def call(*a, **k):
            self.calls.append((name,) + tuple(a))
            return fn(*a, **k)
        return call


@pytest.fixture
def recorded(monkeypatch):
    from w2v2_speaker_amd.data import augment as A

    class _Np:
        def __init__(self, rec):
            self.random = rec

        def __getattr__(self, name):
            return getattr(np, name)
    rec = _Recorder(123)
    monkeypatch.setattr(A, "np", _Np(rec))
    return A, rec


def test_time_dropout_draws_count_then_length_then_start(recorded):
    A, rec = recorded
    a = A.TimeDropoutAugment(SR, 0.25, 2, 5)
    d = a.draw(48000)
    assert rec.calls[0] == ("randint", 2, 6) and len(rec.calls) == 1 + 2 * len(d.spans) and 2 <= len(d.spans) <= 5
    for s, (start, length) in enumerate(d.spans):
        assert rec.calls[1 + 2 * s] == ("randint", 0, 4000)
        assert rec.calls[2 + 2 * s] == ("randint", 0, max(48000 - length, 1))
        assert 0 <= length < 4000 and 0 <= start < max(48000 - length, 1)
    rec.calls.clear()
    d = a.draw(10)                                               # an utterance shorter than the span: start is drawn from [0, 1)
    assert all(c == ("randint", 0, 1) for c, (_, l) in zip(rec.calls[2::2], d.spans) if l >= 10)


def test_time_dropout_under_np_random_seed_is_the_stated_sequence_of_calls():
    from w2v2_speaker_amd.data.augment import TimeDropoutAugment
    np.random.seed(7)
    got = TimeDropoutAugment(SR, 0.25, 0, 5).draw(48000).spans
    np.random.seed(7)
    want = []
    for _ in range(np.random.randint(0, 6)):
        length = np.random.randint(0, 4000)
        want.append((np.random.randint(0, max(48000 - length, 1)), length))
    assert got == want


def test_frequency_dropout_draws_count_then_two_uniforms_per_band(recorded):
    A, rec = recorded
    d = A.FrequencyDropoutAugment(SR, 1, 5, 1).draw(48000)
    top = A.SpecAugmentBand.freq2mel(SR / 2)
    assert rec.calls[0] == ("randint", 1, 6) and len(rec.calls) == 1 + 2 * len(d.bands)
    for s, (lo, hi) in enumerate(d.bands):
        w, f0 = rec.calls[1 + 2 * s], rec.calls[2 + 2 * s]
        assert w[:2] == ("uniform", 0) and w[2] == pytest.approx(top * 27.0 / 256.0)
        assert f0[:2] == ("uniform", 0) and 0 <= lo <= hi <= SR / 2
    assert d.taps.size == len(d.bands) * 512 + 1


def test_speed_and_noise_draw_one_call_each(recorded):
    A, rec = recorded
    d = A.ChoiceSpeedAugment(SR, [0.95, 1, 1.05]).draw(100)
    assert [c[0] for c in rec.calls] == ["choice"] and (d.U, d.D) in ((20, 19), (1, 1), (20, 21))
    rec.calls.clear()
    d = A.UniformSpeedAugment(SR, 0.9, 1.1).draw(100)
    assert rec.calls == [("uniform", 0.9, 1.1)] and d.D <= 64 and abs(d.U / d.D - 1 / d.speed) < 1 / 64
    rec.calls.clear()
    d = A.ChoiceRandomNoiseAugment(SR, [15, 20, 100]).draw(100)
    assert [c[0] for c in rec.calls] == ["choice"] and d.coef == A.snr_to_coef(d.snr)
    rec.calls.clear()
    a = A.ChoiceRirsNoiseAugment(SR, [15], [torch.zeros(5), torch.zeros(9)])
    assert [a.draw(100).bank_row for _ in range(3)] == [0, 1, 0] and [c[0] for c in rec.calls] == ["choice"] * 3
    assert a.bank.shape == (2, 9) and a.bank_lens.tolist() == [5, 9]
    rec.calls.clear()
    r = A.ReverbAugment(SR, room_scale_min=0, room_scale_max=100)
    assert rec.calls == [("randint", 50, 51), ("randint", 50, 51), ("randint", 0, 101)]
    assert (r.reverberance, r.damping) == (50, 50) and 0 <= r.room_scale <= 100 and r.name == "add_reverb"


def test_snr_to_coef_and_names():
    from w2v2_speaker_amd.data import augment as A
    assert A.snr_to_coef(0) == 0.5 and A.snr_to_coef(10) == pytest.approx(10 / 11)
    assert np.float32(A.snr_to_coef(100)) == np.float32(1.0) and np.float32(A.snr_to_coef(15)) < 1
    names = [A.TimeDropoutAugment(SR, 0.25, 0, 5).name, A.FrequencyDropoutAugment(SR, 0, 5, 1).name,
             A.ChoiceSpeedAugment(SR, [1]).name, A.UniformSpeedAugment(SR, 0.9, 1.1).name,
             A.ChoiceRandomNoiseAugment(SR, [15]).name, A.ChoiceRirsNoiseAugment(SR, [15], [torch.zeros(3)]).name]
    assert names == ["time_dropout", "frequency_dropout", "choice_speed", "uniform_speed", "uniform_noise",
                     "rirs_background_noise"]
    # the reference's constructor keywords
    for cls, kw in ((A.TimeDropoutAugment, ["sample_rate", "max_dropout_length_seconds", "min_drop_count", "max_drop_count"]),
                    (A.FrequencyDropoutAugment, ["sample_rate", "min_drop_count", "max_drop_count", "band_scaling"]),
                    (A.ChoiceSpeedAugment, ["sample_rate", "possible_speed_factors"]),
                    (A.UniformSpeedAugment, ["sample_rate", "min_speed_factor", "max_speed_factor"]),
                    (A.ChoiceRandomNoiseAugment, ["sample_rate", "snr_choices"]),
                    (A.ChoiceRirsNoiseAugment, ["sample_rate", "snr_choices", "noise_bank"]),
                    (A.ReverbAugment, ["sample_rate", "reverberance_min", "reverberance_max", "damping_min", "damping_max",
                                       "room_scale_min", "room_scale_max"])):
        pos = [n for n, p in inspect.signature(cls.__init__).parameters.items()
               if n != "self" and p.kind is p.POSITIONAL_OR_KEYWORD]
        assert pos == kw, cls.__name__


def test_spec_augment_band_formula_on_fixed_draws(monkeypatch):
    from w2v2_speaker_amd.data import augment as A
    draws = iter([0.25, 0.5])
    seen = []

    def uniform(lo, hi):
        seen.append((lo, hi))
        return lo + next(draws) * (hi - lo)
    monkeypatch.setattr(np.random, "uniform", uniform)
    band = A.SpecAugmentBand(SR, 1)
    text = band()
    top = 2595.0 * np.log10(1 + 8000 / 700)
    width = 0.25 * top * 27.0 / 256.0
    f0 = 0.5 * (top - width)
    low, high = (10.0 ** (f0 / 2595.0) - 1) * 700, (10.0 ** ((f0 + width) / 2595.0) - 1) * 700
    assert seen == [(0, top * 27.0 / 256.0), (0, top - width)]
    assert text == f"{high}-{low}"
    assert A.SpecAugmentBand.mel2freq(A.SpecAugmentBand.freq2mel(1234.5)) == pytest.approx(1234.5)


# ------------------------------------------------------------------------------------------------ the Augmenter's host half
def _augs():
    from w2v2_speaker_amd.data import augment as A
    return [A.TimeDropoutAugment(SR, 0.01, 1, 2), A.FrequencyDropoutAugment(SR, 1, 2, 1, taps=33),
            A.ChoiceSpeedAugment(SR, [0.95, 1.05]), A.ChoiceRandomNoiseAugment(SR, [15])]


def test_augmenter_flags_row_order_and_key_suffixes():
    from w2v2_speaker_amd.data.augment import Augmenter, resampled_length
    with pytest.raises(ValueError, match="at least stack augmentations or yield intermediate"):
        Augmenter(_augs(), False, False, True)
    names = ["time_dropout", "frequency_dropout", "choice_speed", "uniform_noise"]
    # the shipped configuration: six-fold with five augmenters, here 1 + 4
    a = Augmenter(_augs(), stack_augmentations=False, yield_intermediate_augmentations=True, yield_unaugmented=True)
    assert a.rows_per_sample() == 5 and a.output_shape(3, 1600) == (15, resampled_length(1600, 20, 19))
    np.random.seed(3)
    draws, keys, lens, source, _ = a.plan([1600, 1500], ["a", "b"], 1685)
    assert keys == ["a"] + [f"a/{n}" for n in names] + ["b"] + [f"b/{n}" for n in names]
    assert source == [0] * 5 + [1] * 5
    for b, n in enumerate((1600, 1500)):
        sp = draws[b][2]
        assert lens[5 * b:5 * b + 5] == [n, n, n, resampled_length(n, sp.U, sp.D), n]
    # no unaugmented row
    a = Augmenter(_augs(), False, True, False)
    assert a.rows_per_sample() == 4 and a.plan([100], ["k"], 200)[1] == [f"k/{n}" for n in names]
    # stacked: the suffixes pile up and the lengths follow the speed change
    a = Augmenter(_augs(), True, True, True)
    draws, keys, lens, _, stage = a.plan([1600], ["k"], 4000)
    assert keys == ["k", "k/time_dropout", "k/time_dropout/frequency_dropout", "k/time_dropout/frequency_dropout/choice_speed",
                    "k/time_dropout/frequency_dropout/choice_speed/uniform_noise"]
    n2 = resampled_length(1600, draws[0][2].U, draws[0][2].D)
    assert lens == [1600, 1600, 1600, n2, n2] and [s[0] for s in stage] == [1600, 1600, n2, n2]
    assert a.max_samples(1600) == resampled_length(1600, 20, 19)
    # stacked without intermediates: the reference returns the last sample alone, whatever yield_unaugmented says
    a = Augmenter(_augs(), True, False, True)
    assert a.rows_per_sample() == 1
    assert a.plan([1600], ["k"], 4000)[1] == ["k/time_dropout/frequency_dropout/choice_speed/uniform_noise"]
    # a crop
    assert Augmenter(_augs(), False, True, True).plan([1600], ["k"], 1000)[2] == [1000] * 5


def test_augmenter_draws_sample_by_sample_in_augmenter_order(recorded):
    A, rec = recorded
    augs = [A.ChoiceSpeedAugment(SR, [0.95, 1.05]), A.ChoiceRandomNoiseAugment(SR, [15, 20])]
    A.Augmenter(augs, False, True, True).plan([100, 100, 100], ["a", "b", "c"], 200)
    assert [c[0] for c in rec.calls] == ["choice"] * 6
    assert [tuple(c[1]) for c in rec.calls] == [(0.95, 1.05), (15, 20)] * 3


def test_reverb_raises_on_the_device_path_and_module_surface_checks():
    from w2v2_speaker_amd.data.augment import Augmenter, ReverbAugment
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTdnnModule, FilterbankSpeakerModule
    from w2v2_speaker_amd.lightning_modules.speaker.xvector import XVectorModule
    r = ReverbAugment(SR)
    with pytest.raises(NotImplementedError, match="recursive"):
        r.draw(100)
    with pytest.raises(NotImplementedError, match="recursive"):
        Augmenter([r], False, True, True)._check_device_forms()
    aug = Augmenter(_augs(), False, True, True)
    for bad in ("fbank",):
        with pytest.raises(ValueError, match="augmenter= needs input_features='waveform'"):
            FilterbankSpeakerModule._check_augmenter(aug, bad)
    FilterbankSpeakerModule._check_augmenter(aug, "waveform")
    FilterbankSpeakerModule._check_augmenter(None, "fbank")
    with pytest.raises(ValueError, match="Augmenter"):
        FilterbankSpeakerModule._check_augmenter(object(), "waveform")
    for cls in (EcapaTdnnModule, XVectorModule):
        p = inspect.signature(cls.__init__).parameters["augmenter"]
        assert p.default is None and p.kind is p.KEYWORD_ONLY
    # the constructors refuse it before anything touches a device
    from w2v2_speaker_amd.lightning_modules.speaker.xvector import XVectorModuleConfig
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTDNNModuleConfig
    with pytest.raises(ValueError, match="augmenter= needs input_features='waveform'"):
        XVectorModule.from_config(XVectorModuleConfig(), 4, device="cpu", input_features="fbank", augmenter=aug)
    with pytest.raises(ValueError, match="augmenter= needs input_features='waveform'"):
        EcapaTdnnModule.from_config(EcapaTDNNModuleConfig(), 4, device="cpu", input_features="fbank", augmenter=aug)


# ------------------------------------------------------------------------------------------------ designed filters (f64)
def _gain_db(h, f_hz):
    n = np.arange(h.size)
    return 20 * np.log10(np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(f_hz) / SR, n)) @ h) + 1e-300)


@pytest.mark.parametrize("low,high", [(1000.0, 2000.0), (300.0, 900.0), (5000.0, 5600.0), (0.0, 700.0), (7000.0, 8000.0)])
def test_band_reject_depth_and_pass_band(low, high):
    from w2v2_speaker_amd.data.augment import band_reject_taps, kaiser_transition_hz
    h = band_reject_taps(low, high, SR)
    tr = kaiser_transition_hz(513, SR)
    assert h.size == 513 and 200 < tr < 300 and high - low > 2 * tr
    assert _gain_db(h, np.array([(low + high) / 2]))[0] <= -100.0
    f = np.linspace(0, SR / 2, 1601)
    passband = f[(f < low - tr) | (f > high + tr)]
    assert passband.size and np.abs(_gain_db(h, passband)).max() <= 0.01


def test_composed_taps_equal_the_convolution_of_the_stages():
    from w2v2_speaker_amd.data.augment import AUG_MAX_TAPS, band_reject_taps, compose_taps
    st = [band_reject_taps(lo, hi, SR) for lo, hi in ((500, 900), (2000, 2100), (3000, 4500), (100, 101), (6000, 7900))]
    h = compose_taps(st)
    want = st[0]
    for s in st[1:]:
        want = np.convolve(want, s)
    assert h.size == 5 * 512 + 1 == AUG_MAX_TAPS and np.array_equal(h, want)
    assert np.array_equal(compose_taps([]), np.ones(1)) and np.array_equal(compose_taps(st[:1]), st[0])
    x = np.random.RandomState(0).standard_normal(9000)          # away from the ends, one pass = the passes in turn
    one, turn = np.convolve(x, h, "same"), x
    for s in st:
        turn = np.convolve(turn, s, "same")
    assert np.abs(one - turn)[1300:-1300].max() < 1e-12


def test_speed_ratios_are_the_stated_fractions():
    from w2v2_speaker_amd.data.augment import resample_prototype, resampled_length, speed_ratio
    assert speed_ratio(0.95) == (20, 19) and speed_ratio(1.05) == (20, 21) and speed_ratio(1) == (1, 1)
    assert speed_ratio(0.5) == (2, 1) and speed_ratio(2.0) == (1, 2)
    assert resampled_length(48000, 20, 19) == 50527 and resampled_length(48000, 20, 21) == 45715
    h = resample_prototype(20, 21)
    assert h.size == 2 * 32 * 21 + 1 and h.sum() == pytest.approx(1.0) and np.array_equal(h, h[::-1])
    for ph in range(20):                                        # every polyphase branch has the gain 1 / U
        assert h[ph::20].sum() * 20 == pytest.approx(1.0, abs=1e-3)


@pytest.mark.parametrize("U,D", [r for r in AC.RESAMPLE_RATIOS if r != (1, 1)])
def test_resampling_oracle_agrees_with_upfirdn(U, D):
    from scipy.signal import upfirdn
    from w2v2_speaker_amd.data.augment import resample_prototype
    h = resample_prototype(U, D)
    half = (h.size - 1) // 2
    for n in (1, 50, 257):
        x = AC.wave(1, n, n)[0]
        N_out = -(-n * U // D) + 3
        y, bound, out_len = AC.resample_ref(x, n, U, D, h, N_out)
        # upfirdn: full[k] = sum_j g[k D - j U] x[j].  With g = p zeros in front of U h, p = -half mod D, the output m of
        # the definition (tap index m D - j U + half) is full[m + (half + p) / D]
        p = -half % D
        full = upfirdn(np.concatenate([np.zeros(p), U * h]), x.astype(np.float64), U, D)
        k0 = (half + p) // D
        want = full[k0:k0 + out_len]
        assert out_len == -(-n * U // D) and want.size == out_len and np.abs(y[:out_len] - want).max() <= 1e-12
        assert not y[out_len:].any() and (bound[:out_len] > 0).any()


def test_uniform_stream_restatement_is_a_24_bit_uniform():
    u = AC.uniform_stream(1234, 3, 1 << 16)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    assert np.array_equal(u, np.round(u * 2 ** 24) / 2 ** 24)
    assert abs(u.astype(np.float64).mean() - 0.5) < 4 / np.sqrt(12 * (1 << 16))
    assert not np.array_equal(u, AC.uniform_stream(1234, 4, 1 << 16))
    assert np.array_equal(u, AC.uniform_stream(1234, 3, 1 << 16))
