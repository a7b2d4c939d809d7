"""CPU tests of the reverb augmentation: the parameter arithmetic of data/augment.py reverb_parameters against the values
the definition tabulates, the oracles of tests/reverb_cases.py on a unit impulse, the C ABI of the new entry, the argument
errors that need no device, and ReverbAugment's two forms.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import reverb_cases as RC
from test_augment_cpu import _Recorder
from test_metrics_cpu import _c_decl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000


# ------------------------------------------------------------------------------------------------ the parameters
def test_reverb_parameters_give_the_tabulated_delays_and_coefficients():
    from w2v2_speaker_amd.data.augment import reverb_parameters
    for rev, fb in ((0, 0.3000), (50, 0.8817), (100, 0.9800)):
        p = reverb_parameters(SR, rev, 50, 50)
        assert p.feedback.dtype == np.float32 and abs(float(p.feedback) - fb) < 5e-5, (rev, float(p.feedback))
    for damping, damp in ((0, 0.20), (50, 0.35), (100, 0.50)):
        assert reverb_parameters(SR, 50, damping, 50).damp == np.float32(damp)
    for room, a0, a1 in ((0, [40, 43], [41, 43]), (37, [175, 187], [177, 185]), (100, [405, 431], [409, 427])):
        p = reverb_parameters(SR, 50, 50, room)
        assert p.comb_delays.shape == (2, 8) and p.comb_delays.dtype == np.int32
        assert p.comb_delays[0, :2].tolist() == a0 and p.comb_delays[1, :2].tolist() == a1, room
        assert p.allpass_delays.tolist() == [[82, 124, 160, 202], [86, 119, 164, 197]]      # no room scale in the all-passes
        assert p.wet_gain == np.float32(0.015) and p.dry_gain == np.float32(1.0)
    p = reverb_parameters(SR, 50, 50, 37)
    row = p.row()
    assert row.dtype == np.int32 and row.shape == (RC.PARAMS,)
    assert row[:16].tolist() == p.comb_delays.reshape(-1).tolist() and row[16:24].tolist() == p.allpass_delays.reshape(-1).tolist()
    assert row[24:].view(np.float32).tolist() == [p.feedback, np.float32(0.35), np.float32(0.015), np.float32(1.0)]
    assert np.array_equal(row, RC.table_row(p.comb_delays, p.allpass_delays, p.feedback, p.damp, p.wet_gain, p.dry_gain))


def test_reverb_parameters_sign_pattern_and_the_sample_rates_that_fit():
    from w2v2_speaker_amd.data.augment import REVERB_MAX_DELAY, reverb_parameters
    p = reverb_parameters(22050, 50, 50, 100)                   # r = 1/2, scale = 1: delays are half the 44.1 kHz lengths
    combs = np.array([1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617])
    sign = np.array([1, -1, 1, -1, 1, -1, 1, -1])
    assert p.comb_delays[0].tolist() == [int(0.5 * c + 0.5) for c in combs]
    assert p.comb_delays[1].tolist() == [int(0.5 * (c + 12 * s) + 0.5) for c, s in zip(combs, sign)]
    aps = np.array([225, 341, 441, 556])
    assert p.allpass_delays[1].tolist() == [int(0.5 * (a + 12 * s) + 0.5) for a, s in zip(aps, sign[:4])]
    # the header's statement: room scale 100 fits up to 27,940 Hz; at 32 kHz up to room scale 85, at 44.1 kHz up to 59
    assert REVERB_MAX_DELAY == RC.MAX_DELAY
    assert reverb_parameters(27940, 50, 50, 100).comb_delays.max() == RC.MAX_DELAY
    for rate, room in ((27941, 100), (32000, 86), (44100, 60)):
        with pytest.raises(ValueError, match=r"outside \[1, 1024\]"):
            reverb_parameters(rate, 50, 50, room)
    reverb_parameters(32000, 50, 50, 85)
    reverb_parameters(44100, 50, 50, 59)


# ------------------------------------------------------------------------------------------------ the oracles
def test_oracle_on_a_unit_impulse_is_silent_up_to_the_smallest_comb_delay_then_wet_gain_per_comb():
    from w2v2_speaker_amd.data.augment import reverb_parameters
    x = np.zeros(300, np.float32)
    x[0] = 1.0
    wg = float(np.float32(RC.WET_GAIN))
    # both arrays alike, three combs share the smallest delay: y = 0.5 (3 wg + 3 wg); the four all-passes have sign +1
    row = RC.table_row([[5, 5, 9, 5, 11, 13, 17, 19]] * 2, [[23, 29, 31, 37]] * 2, 0.5, 0.3, RC.WET_GAIN, 0.0)
    for dt in (np.float64, np.float32):
        y = RC.reverb_ref(x, 300, row, 300, dt)
        assert not y[:5].any() and float(y[5]) == pytest.approx(3 * wg, rel=1e-6), dt
        assert not y[6:9].any() and float(y[9]) == pytest.approx(wg, rel=1e-6)
    # the reference's parameters at room scale 0: delay 40 is in array 0 alone, once
    p = reverb_parameters(SR, 50, 50, 0)
    p.dry_gain = np.float32(0.0)
    y = RC.reverb_ref(x, 300, p.row(), 300)
    assert not y[:40].any() and y[40] == pytest.approx(0.5 * wg, rel=1e-12) and y[41] == pytest.approx(0.5 * wg, rel=1e-12)
    p.dry_gain = np.float32(1.0)
    y = RC.reverb_ref(x, 300, p.row(), 300)
    assert y[0] == 1.0 and not y[1:40].any()                    # the dry signal, (1 + 1) / 2


def test_oracle_in_blocks_equals_the_sample_by_sample_definition():
    """The oracles walk a filter in blocks of its delay; this is the definition's per-sample loop, in float64."""
    r = np.random.RandomState(0)
    x = r.standard_normal(200)
    D, fb, damp = 7, 0.9, 0.3
    line, store, p, want = np.zeros(D), 0.0, 0, np.zeros(200)
    for n in range(200):
        o = line[p]
        store = o + (store - o) * damp
        line[p] = x[n] + store * fb
        want[n] = o
        p = (p + 1) % D
    assert np.array_equal(RC._comb(x, D, np.float64(fb), np.float64(damp), np.float64), want)
    line, p = np.zeros(D), 0
    for n in range(200):
        o = line[p]
        line[p] = x[n] + 0.5 * o
        want[n] = o - x[n]
        p = (p + 1) % D
    assert np.array_equal(RC._allpass(x, D, np.float64), want)
    # a length shorter than the row, and a crop: zeros behind, a prefix in front
    x32 = RC.wave(1, 100, 3)[0]
    row = RC.edge_row(0, 0.8817, 0.2, 1.0)
    full = RC.reverb_ref(x32, 100, row, 100)
    assert np.array_equal(RC.reverb_ref(x32, 60, row, 100)[:60], full[:60]) and not RC.reverb_ref(x32, 60, row, 100)[60:].any()
    assert np.array_equal(RC.reverb_ref(x32, 100, row, 40), full[:40])
    y64, bound, seq = RC.reverb_refs(x32, 100, row, 100)
    assert 0 < seq < 1e-6 and bound == max(4 * seq, 2.0 ** -22 * np.abs(y64).max())


def test_cases_hold_every_edge_the_definition_names():
    assert RC.DELAY_EDGES == [1, 2, 63, 64, 65, 127, 128, 129, 1024] and len(RC.COEFS) == 12
    for k in range(12):
        row = RC.edge_row(k, 0.3, 0.2, 0.0)
        assert set(row[:16].tolist()) == set(RC.DELAY_EDGES) and set(row[16:24].tolist()) <= set(RC.DELAY_EDGES)
    assert {RC.edge_row(k, 0.3, 0.2, 0.0)[16 + j] for k in range(12) for j in range(8)} == set(RC.DELAY_EDGES)
    for v in (0, 1, 2, 3, 62, 66, 126, 130, 511, 512, 513, 1023, 1024, 1025, 1027):
        assert v in RC.LENGTHS
    assert max(RC.LENGTHS) == RC.N_MAX == 2 * RC.CHUNK + 3


# ------------------------------------------------------------------------------------------------ the C ABI and ops
def test_reverb_symbol_is_declared_exported_and_wrapped_with_a_matching_signature():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    from w2v2_speaker_amd.data import augment as A
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32", C.c_double: "f64"}
    for name in ("w2v2_aug_reverb", "w2v2_aug_reverb_chunk"):
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        res, args = _lib._SIGS[name]
        assert (kind[res], [kind[a] for a in args]) == _c_decl(hdr, name), name
    assert _c_decl(hdr, "w2v2_aug_reverb") == ("i32", ["p", "i64", "i32", "p", "p", "p", "i64", "i32", "p", "i32", "p", "p"])
    assert _lib._SIGS["w2v2_aug_reverb"][1][:10] == _lib._SIGS["w2v2_aug_fir"][1][:10]      # src / dst as in w2v2_aug_fir
    assert "reverb.hip" in _build.SOURCES and "reverb.hip" not in _build.EXTRA_FLAGS
    assert f"#define W2V2_AUG_REVERB_MAX_DELAY {ops.AUG_REVERB_MAX_DELAY}" in hdr
    assert f"#define W2V2_AUG_REVERB_PARAMS {ops.AUG_REVERB_PARAMS}" in hdr
    assert ops.AUG_REVERB_MAX_DELAY == A.REVERB_MAX_DELAY == RC.MAX_DELAY == 1024
    assert ops.AUG_REVERB_PARAMS == A.REVERB_PARAMS == RC.PARAMS == 2 * 8 + 2 * 4 + 4
    assert _lib.load().w2v2_aug_reverb_chunk() == ops.AUG_REVERB_CHUNK == RC.CHUNK
    assert callable(ops.aug_reverb)


def test_ops_aug_reverb_argument_checks_need_no_device():
    from w2v2_speaker_amd import ops
    x, y, rows = torch.zeros(3, 16), torch.zeros(3, 16), torch.zeros(2, dtype=torch.int32)
    good = torch.zeros(2, ops.AUG_REVERB_PARAMS, dtype=torch.int32)
    with pytest.raises(ValueError, match="2-D float32"):
        ops.aug_reverb(x.double(), y, rows, rows, good)
    with pytest.raises(ValueError, match="rows"):
        ops.aug_reverb(x, y, rows.long(), rows, good)
    with pytest.raises(ValueError, match="name 2 rows each"):
        ops.aug_reverb(x, y, rows, torch.zeros(3, dtype=torch.int32), good)
    with pytest.raises(ValueError, match="lens"):
        ops.aug_reverb(x, y, rows, rows, good, lens=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="share memory"):
        ops.aug_reverb(x, x, rows, rows, good)
    for bad in (torch.zeros(3, ops.AUG_REVERB_PARAMS, dtype=torch.int32), torch.zeros(2, ops.AUG_REVERB_PARAMS - 1, dtype=torch.int32),
                torch.zeros(2, ops.AUG_REVERB_PARAMS), torch.zeros(2 * ops.AUG_REVERB_PARAMS, dtype=torch.int32),
                torch.zeros(2, 2 * ops.AUG_REVERB_PARAMS, dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match=r"params is a contiguous int32 \[2, 28\]"):
            ops.aug_reverb(x, y, rows, rows, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.aug_reverb(x, y, rows, rows, good)


# ------------------------------------------------------------------------------------------------ ReverbAugment
@pytest.fixture
def recorded(monkeypatch):
    from w2v2_speaker_amd.data import augment as A

    class _Np:
        def __init__(self, rec):
            self.random = rec

        def __getattr__(self, name):
            return getattr(np, name)
    rec = _Recorder(321)
    monkeypatch.setattr(A, "np", _Np(rec))
    return A, rec


def test_on_device_reverb_makes_the_three_construction_draws_and_none_in_draw(recorded):
    A, rec = recorded
    r = A.ReverbAugment(SR, 40, 60, 30, 70, 0, 100, on_device=True)
    assert rec.calls == [("randint", 40, 61), ("randint", 30, 71), ("randint", 0, 101)]
    rec.calls.clear()
    d = r.draw(48000)
    assert rec.calls == [] and r.draw(1) is d and r.max_length(777) == 777 and r.name == "add_reverb" and r.kind == "reverb"
    want = A.reverb_parameters(SR, r.reverberance, r.damping, r.room_scale)
    assert isinstance(d, A.ReverbDraw) and np.array_equal(d.row(), want.row()) and d.dry_gain == np.float32(1.0)
    aug = A.Augmenter([A.ChoiceSpeedAugment(SR, [0.95, 1.05]), r, A.ChoiceRandomNoiseAugment(SR, [15])], True, True, True)
    aug._check_device_forms()
    rec.calls.clear()
    draws, keys, lens, source, stage = aug.plan([1600, 900], ["a", "b"], 4000)
    assert [c[0] for c in rec.calls] == ["choice"] * 4                          # speed and noise per row, nothing for the reverb
    n = A.resampled_length(1600, draws[0][0].U, draws[0][0].D)
    assert keys[:4] == ["a", "a/choice_speed", "a/choice_speed/add_reverb", "a/choice_speed/add_reverb/uniform_noise"]
    assert lens[:4] == [1600, n, n, n] and draws[0][1] is d and aug.max_samples(1600) == A.resampled_length(1600, 20, 19)
    # the keyword is keyword-only, and a sample rate at which the room does not fit is refused at construction
    with pytest.raises(TypeError):
        A.ReverbAugment(SR, 50, 50, 50, 50, 0, 100, True)
    with pytest.raises(ValueError, match="outside"):
        A.ReverbAugment(44100, room_scale_min=100, room_scale_max=100, on_device=True)


def test_default_reverb_still_raises_and_the_modules_take_the_device_form():
    from w2v2_speaker_amd.data.augment import Augmenter, ReverbAugment
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import FilterbankSpeakerModule
    r = ReverbAugment(SR)
    assert r.on_device is False
    with pytest.raises(NotImplementedError, match="recursive"):
        r.draw(100)
    with pytest.raises(NotImplementedError, match="recursive"):
        Augmenter([r], False, True, True)._check_device_forms()
    assert ReverbAugment(44100, room_scale_min=100, room_scale_max=100).room_scale == 100      # (the default form checks nothing)
    aug = Augmenter([ReverbAugment(SR, on_device=True)], False, True, True)
    aug._check_device_forms()
    FilterbankSpeakerModule._check_augmenter(aug, "waveform")
    assert aug.rows_per_sample() == 2 and aug.plan([100], ["k"], 100)[1] == ["k", "k/add_reverb"]
