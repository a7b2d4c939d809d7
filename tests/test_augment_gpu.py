"""The waveform augmentation on the device (csrc/augment.hip, data/augment.py) against the float64 oracles of
tests/augment_cases.py, within the bounds derived there; dropout, the copy ratio and the uniform stream bit for bit.

Every launch works on buffers with a guard band in front and behind and padding columns behind N, all prefilled with a
sentinel, and next to two rows that are not listed: whatever is not a listed row's first N columns must keep its bits.
Each case runs with 16-byte aligned rows (the vector forms) and with an odd row stride (the scalar forms).  The worst
error over its bound is printed before it is asserted (``pytest -s``; profiles/augment_parity.txt)."""
import numpy as np
import pytest
import torch

import augment_cases as AC
from w2v2_speaker_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                      # floats in front of and behind every buffer
SENT = -77.25                   # the sentinel: no case produces it
STRIDES = ["aligned", "odd"]


class Buf:
    """A [rows, N] f32 view with row stride ld inside a flat sentinel-filled buffer."""

    def __init__(self, rows, N, stride, fill=None):
        self.rows, self.N = rows, N
        self.ld = (N + 3) // 4 * 4 + 4 if stride == "aligned" else (N + 3) | 1
        self.flat = torch.full((2 * GUARD + rows * self.ld,), SENT, dtype=torch.float32, device=DEV)
        self.t = self.flat[GUARD:GUARD + rows * self.ld].view(rows, self.ld)[:, :N]
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)))
        self.before = self.flat.clone()

    def check_untouched(self, listed):
        """Everything but the first N columns of the listed rows has the bits it had."""
        mask = torch.ones_like(self.flat, dtype=torch.bool)
        body = mask[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)
        for r in listed:
            body[r, :self.N] = False
        assert torch.equal(self.flat.view(torch.int32)[mask], self.before.view(torch.int32)[mask])

    def np(self):
        return self.t.cpu().numpy()


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def f32(v):
    return torch.tensor(np.asarray(v, np.float32), device=DEV)


def within(tag, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    print(f"augment-parity: {tag}: max |err| {err.max():.3e}, worst err / bound {ratio:.3f}")
    assert (err <= bound).all(), (tag, float(err.max()), ratio)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("case", AC.DROPOUT_CASES, ids=[c[0] for c in AC.DROPOUT_CASES])
def test_time_dropout_is_exact(case, stride):
    _, spans, n = case
    N = AC.DROPOUT_N
    x = AC.wave(4, N, 1)
    buf = Buf(4, N, stride, x)
    lens = [N, n or N, N, (n or N) - 7]
    listed = [3, 1]
    other = [(N - 1 - s - l, l) for s, l in spans]              # row 3 takes the mirrored spans
    S = len(spans)
    table = np.zeros((2, S, 2), np.int32)
    table[0], table[1] = np.asarray(other, np.int32).reshape(S, 2), np.asarray(spans, np.int32).reshape(S, 2)
    ops.aug_time_dropout(buf.t, i32(listed), i32(table).view(2, S, 2), lens=i32(lens) if n else None)
    got = buf.np()
    for r, sp in zip(listed, (other, spans)):
        want = AC.dropout_ref(x[r], lens[r] if n else N, sp)
        assert np.array_equal(got[r].view(np.int32), want.view(np.int32)), (r, sp)
    buf.check_untouched(listed)


# ------------------------------------------------------------------------------------------------ mixes
def _coef(snr):
    from w2v2_speaker_amd.data.augment import snr_to_coef
    return np.float32(snr_to_coef(snr))


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("snr", AC.MIX_SNRS)
def test_mix_uniform_against_float64_and_the_restated_stream(snr, stride):
    N, seed = 257, 0x1234_5678_9ABC
    x = AC.wave(4, N, 2)
    lens, listed = [N, 200, N, 131], [1, 2]
    c = _coef(snr)
    assert (c == 1.0) == (snr == 100)
    for use_lens in (False, True):
        buf = Buf(4, N, stride, x)
        ops.aug_mix_uniform(buf.t, i32(listed), f32([c, c]), seed, lens=i32(lens) if use_lens else None)
        got = buf.np()
        for r in listed:
            n = lens[r] if use_lens else N
            y, bound = AC.mix_ref(x[r], n, c, AC.uniform_stream(seed, r, N))
            within(f"mix_uniform snr={snr} {stride} row {r} len {n}", got[r], y, bound)
            assert not got[r, n:].any()
            if snr == 100:                                       # c == 1.0f: the signal itself
                assert np.array_equal(got[r, :n], x[r, :n])
        buf.check_untouched(listed)
        again = Buf(4, N, stride, x)
        ops.aug_mix_uniform(again.t, i32(listed), f32([c, c]), seed, lens=i32(lens) if use_lens else None)
        assert torch.equal(again.flat.view(torch.int32), buf.flat.view(torch.int32))     # the same seed twice


def test_uniform_stream_is_the_numpy_restatement_bit_for_bit():
    """c = 0 over zeros leaves u itself: fma(0, 0, 1 * u).  Bounds, mean and lag-1 correlation are those of the restated
    stream because the arrays are equal."""
    N, seed = 1 << 16, 20211
    buf = Buf(4, N, "aligned", np.zeros((4, N), np.float32))
    ops.aug_mix_uniform(buf.t, i32([0, 2]), f32([0.0, 0.0]), seed)
    got = buf.np()
    for r in (0, 2):
        u = AC.uniform_stream(seed, r, N)
        assert np.array_equal(got[r].view(np.int32), u.view(np.int32)), r
        d = got[r].astype(np.float64)
        lag1 = np.corrcoef(d[:-1], d[1:])[0, 1]
        print(f"augment-parity: uniform stream row {r}: min {d.min():.3e} max {d.max():.9f} mean {d.mean():.6f} lag-1 {lag1:+.5f}")
        assert d.min() >= 0.0 and d.max() < 1.0
        assert d.mean() == u.astype(np.float64).mean() and lag1 == np.corrcoef(u[:-1].astype(np.float64), u[1:])[0, 1]
    assert not np.array_equal(got[0], got[2])                   # two rows under one seed
    buf.check_untouched([0, 2])
    other = Buf(4, N, "aligned", np.zeros((4, N), np.float32))
    ops.aug_mix_uniform(other.t, i32([0]), f32([0.0]), seed + 1)
    assert not np.array_equal(other.np()[0], got[0])            # another seed


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("snr", AC.MIX_SNRS)
def test_mix_bank_repeats_the_noise_to_the_rows_length(snr, stride):
    N = 257
    x = AC.wave(6, N, 3)
    L = AC.MIX_BANK_LENS
    bank = Buf(len(L), max(L), stride, AC.wave(len(L), max(L), 4))
    noise = bank.np().copy()
    lens, listed, bank_row = [N, 256, N, 100, 3, N], [5, 0, 3, 1], [3, 0, 1, 2]
    c = _coef(snr)
    for use_lens in (False, True):
        buf = Buf(6, N, stride, x)
        ops.aug_mix_bank(buf.t, i32(listed), f32([c] * 4), bank.t, i32(L), i32(bank_row), lens=i32(lens) if use_lens else None)
        got = buf.np()
        for r, m in zip(listed, bank_row):
            n = lens[r] if use_lens else N
            y, bound = AC.mix_ref(x[r], n, c, AC.bank_noise(noise[m], L[m], N))
            within(f"mix_bank snr={snr} {stride} row {r} len {n} noise len {L[m]}", got[r], y, bound)
            assert not got[r, n:].any()
        buf.check_untouched(listed)
    bank.check_untouched([])
    # a bank row out of range is not read: that row is NaN, the other is right
    buf = Buf(6, N, stride, x)
    ops.aug_mix_bank(buf.t, i32([2, 4]), f32([c, c]), bank.t, i32(L), i32([len(L), 1]))
    got = buf.np()
    assert np.isnan(got[2]).all()
    within("mix_bank next to a bad bank row", got[4], *AC.mix_ref(x[4], N, c, AC.bank_noise(noise[1], L[1], N)))
    buf.check_untouched([2, 4])


# ------------------------------------------------------------------------------------------------ FIR
_FIR_TAPS = {K: AC.fir_taps(K, 0) for K in AC.FIR_TAPS_IN_ONE_LAUNCH}


def _fir_launch(x, lens, src_rows, dst_rows, Ks, N_out, stride, use_lens=True):
    ldt = max(Ks) + 3
    taps = np.full((len(Ks), ldt), np.nan, np.float32)          # what lies behind a row's taps is never read
    for r, K in enumerate(Ks):
        taps[r, :K] = _FIR_TAPS[K]
    src, dst = Buf(x.shape[0], x.shape[1], stride, x), Buf(6, N_out, stride)
    ops.aug_fir(src.t, dst.t, i32(src_rows), i32(dst_rows), f32(taps), i32(Ks), lens=i32(lens) if use_lens else None)
    return src, dst


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("N", AC.FIR_N)
def test_fir_against_float64_every_tap_count_in_one_launch(N, stride):
    Ks = AC.FIR_TAPS_IN_ONE_LAUNCH
    x = AC.wave(6, N, 5)
    src_rows, dst_rows = [4, 0, 2, 5], [1, 5, 0, 3]
    for lens in (None, [max(N - 1, 0), N, N // 2, N, max(N - 3, 0), N // 3]):
        src, dst = _fir_launch(x, lens, src_rows, dst_rows, Ks, N, stride, lens is not None)
        got = dst.np()
        for s, d, K in zip(src_rows, dst_rows, Ks):
            n = lens[s] if lens else N
            y, bound = AC.fir_ref(x[s], n, _FIR_TAPS[K], N)
            within(f"fir N={N} {stride} K={K} len {n}", got[d], y, bound)
            assert not got[d, n:].any()
            # the row alone: B = 1, N = len, one listed row
            if n > 0:
                a_src, a_dst = Buf(1, n, stride, x[s:s + 1, :n]), Buf(1, n, stride)
                ops.aug_fir(a_src.t, a_dst.t, i32([0]), i32([0]), f32(_FIR_TAPS[K][None]), i32([K]))
                assert np.array_equal(a_dst.np()[0].view(np.int32), got[d, :n].view(np.int32)), (K, n)
        dst.check_untouched(dst_rows)
        src.check_untouched([])


@pytest.mark.parametrize("stride", STRIDES)
def test_fir_crops_and_pads_to_the_output_width_and_refuses_bad_tap_counts(stride):
    N = AC.FIR_TILE + 1
    x = AC.wave(6, N, 6)
    Ks, src_rows, dst_rows = [513, 3, AC.MAX_TAPS, 1], [0, 1, 2, 3], [2, 3, 4, 5]
    lens = [N, 700, N, 5, N, N]
    for N_out in (1000, N + 300):
        src, dst = _fir_launch(x, lens, src_rows, dst_rows, Ks, N_out, stride)
        got = dst.np()
        for s, d, K in zip(src_rows, dst_rows, Ks):
            y, bound = AC.fir_ref(x[s], lens[s], _FIR_TAPS[K], N_out)
            within(f"fir N_in={N} N_out={N_out} {stride} K={K} len {lens[s]}", got[d], y, bound)
            assert not got[d, min(lens[s], N_out):].any()
        dst.check_untouched(dst_rows)
    # an even count, zero, and one above the cap: NaN rows, nothing read; the good row next to them is right
    src, dst = Buf(6, N, stride, x), Buf(6, N, stride)
    taps = np.zeros((4, 8), np.float32)
    taps[3, :3] = _FIR_TAPS[3]
    ops.aug_fir(src.t, dst.t, i32([0, 1, 2, 3]), i32([0, 1, 2, 3]), f32(taps), i32([4, 0, AC.MAX_TAPS + 2, 3]))
    got = dst.np()
    assert np.isnan(got[:3]).all()
    within("fir next to bad tap counts", got[3], *AC.fir_ref(x[3], N, _FIR_TAPS[3], N))
    dst.check_untouched([0, 1, 2, 3])


# ------------------------------------------------------------------------------------------------ resample
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("U,D", AC.RESAMPLE_RATIOS, ids=[f"{u}/{d}" for u, d in AC.RESAMPLE_RATIOS])
def test_resample_against_float64(U, D, stride):
    from w2v2_speaker_amd.data.augment import resample_prototype
    h = resample_prototype(U, D).astype(np.float32)
    lens = AC.resample_lens(D)
    R, N_in = len(lens), max(lens)
    x = AC.wave(R + 2, N_in, 7)
    all_lens = lens + [N_in, 3]
    src_rows, dst_rows = list(range(R)), [R + 1 - i for i in range(R)]       # dst rows 0 and 1 stay untouched
    full = -(-N_in * U // D)
    for N_out in (full + 5, max(full // 2, 1)):                             # zero padding; a cropped row
        src, dst = Buf(R + 2, N_in, stride, x), Buf(R + 2, N_out, stride)
        out_lens = torch.full((R + 2,), -7, dtype=torch.int32, device=DEV)
        ops.aug_resample(src.t, dst.t, i32(src_rows), i32(dst_rows), U, D, f32(h), lens=i32(all_lens), out_lens=out_lens)
        got, got_lens = dst.np(), out_lens.cpu().tolist()
        assert got_lens[:2] == [-7, -7]
        for s, d in zip(src_rows, dst_rows):
            n = all_lens[s]
            y, bound, out_len = AC.resample_ref(x[s], n, U, D, h, N_out)
            assert got_lens[d] == out_len == min(-(-n * U // D), N_out)
            if (U, D) == (1, 1):
                assert np.array_equal(got[d].view(np.int32), y.astype(np.float32).view(np.int32))
            else:
                within(f"resample {U}/{D} {stride} len {n} N_out {N_out}", got[d], y, bound)
            assert not got[d, out_len:].any()
            a_src, a_dst = Buf(1, n, stride, x[s:s + 1, :n]), Buf(1, max(out_len, 1), stride)      # the row alone
            ops.aug_resample(a_src.t, a_dst.t, i32([0]), i32([0]), U, D, f32(h))
            assert np.array_equal(a_dst.np()[0, :out_len].view(np.int32), got[d, :out_len].view(np.int32)), (n, N_out)
        dst.check_untouched(dst_rows)
        src.check_untouched([])


# ------------------------------------------------------------------------------------------------ end to end
SR = 16000


def _bank():
    return [torch.from_numpy(AC.wave(1, n, 40 + n)[0]).to(DEV) for n in (700, 2500)]


def _five(bank):
    from w2v2_speaker_amd.data import augment as A
    return [A.TimeDropoutAugment(SR, 0.02, 1, 3), A.FrequencyDropoutAugment(SR, 1, 2, 1), A.ChoiceSpeedAugment(SR, [0.95, 1, 1.05]),
            A.ChoiceRandomNoiseAugment(SR, [15, 20]), A.ChoiceRirsNoiseAugment(SR, [15], bank)]


@pytest.mark.parametrize("lengths", [None, [1600, 1500, 901]])
def test_augmenter_process_batch_against_the_oracles(lengths):
    from w2v2_speaker_amd.data import augment as A
    B, N = 3, 1600
    x = AC.wave(B, N, 8)
    bank = _bank()
    aug = A.Augmenter(_five(bank), stack_augmentations=False, yield_intermediate_augmentations=True, yield_unaugmented=True,
                      seed=5)
    np.random.seed(11)
    gt = torch.tensor([4, 2, 9], device=DEV)
    out = aug.process_batch(torch.from_numpy(x).to(DEV), gt, keys=["a", "b", "c"], lengths=lengths)
    No = -(-N * 20 // 19)
    assert out.network_input.shape == (B * 6, No) and out.ground_truth.tolist() == [4] * 6 + [2] * 6 + [9] * 6
    assert out.source_row.tolist() == [0] * 6 + [1] * 6 + [2] * 6 and out.lengths.cpu().tolist() == out.lengths_host
    assert out.keys[6:12] == ["b", "b/time_dropout", "b/frequency_dropout", "b/choice_speed", "b/uniform_noise",
                              "b/rirs_background_noise"]
    got = out.network_input.cpu().numpy()
    for b in range(B):
        n = lengths[b] if lengths else N
        d_drop, d_band, d_speed, d_noise, d_rirs = out.draws[b]
        r0 = 6 * b
        assert out.lengths_host[r0:r0 + 6] == [n, n, n, A.resampled_length(n, d_speed.U, d_speed.D), n, n]
        assert np.array_equal(got[r0, :n], x[b, :n]) and not got[r0, n:].any()
        want = np.zeros(No, np.float32)
        want[:N] = AC.dropout_ref(x[b], n, d_drop.spans)
        assert np.array_equal(got[r0 + 1], want) and 1 <= len(d_drop.spans) <= 3
        within(f"augmenter row {b} frequency_dropout ({d_band.taps.size} taps)", got[r0 + 2],
               *AC.fir_ref(x[b], n, d_band.taps.astype(np.float32), No))
        h = A.resample_prototype(d_speed.U, d_speed.D).astype(np.float32)
        y, bound, out_len = AC.resample_ref(x[b], n, d_speed.U, d_speed.D, h, No)
        within(f"augmenter row {b} choice_speed {d_speed.U}/{d_speed.D}", got[r0 + 3], y, bound)
        xpad = np.zeros(No, np.float32)
        xpad[:N] = x[b]
        u = AC.uniform_stream(aug.noise_seed(0, 3), r0 + 4, No)
        within(f"augmenter row {b} uniform_noise", got[r0 + 4], *AC.mix_ref(xpad, n, np.float32(d_noise.coef), u))
        m = d_rirs.bank_row
        nz = bank[m].cpu().numpy()
        within(f"augmenter row {b} rirs_background_noise", got[r0 + 5],
               *AC.mix_ref(xpad, n, np.float32(d_rirs.coef), AC.bank_noise(nz, nz.size, No)))
        assert m == b % 2
    # a second step: the staging buffers take turns, the noise seed moves on
    np.random.seed(11)
    again = aug.process_batch(torch.from_numpy(x).to(DEV), gt, lengths=lengths)
    a = again.network_input.cpu().numpy()
    rows = np.arange(B * 6)
    same = rows[(rows % 6 != 4) & (rows % 6 != 5)]
    assert np.array_equal(a[same], got[same]) and not np.array_equal(a[4], got[4]) and again.keys[1] == "0/time_dropout"


def test_augmenter_stacked_chain_of_exact_stages():
    """Stacking: dropout -> speed 1 (a copy) -> noise at 100 dB (c = 1.0f) is the dropout, bit for bit, in every row the
    chain yields; an output narrower than the input crops."""
    from w2v2_speaker_amd.data import augment as A
    B, N = 2, 900
    x = AC.wave(B, N, 9)
    augs = [A.TimeDropoutAugment(SR, 0.01, 2, 2), A.ChoiceSpeedAugment(SR, [1]), A.ChoiceRandomNoiseAugment(SR, [100])]
    for inter, No in ((True, None), (False, None), (True, 500)):
        aug = A.Augmenter(augs, True, inter, True)
        np.random.seed(2)
        out = aug.process_batch(torch.from_numpy(x).to(DEV), torch.arange(B, device=DEV), lengths=[900, 850], out_samples=No)
        got, per = out.network_input.cpu().numpy(), (4 if inter else 1)
        W = No or N
        assert got.shape == (B * per, W)
        for b, n in enumerate((900, 850)):
            want = AC.dropout_ref(x[b], n, out.draws[b][0].spans)[:W]
            first = b * per + (1 if inter else 0)
            for r in range(first, (b + 1) * per):
                assert np.array_equal(got[r], want), (inter, No, r)
            if inter:
                assert np.array_equal(got[b * per, :min(n, W)], x[b, :min(n, W)])
        assert out.keys[-1] == "1/time_dropout/choice_speed/uniform_noise"


def _xvector(**kw):
    import xvector_cases as K
    from w2v2_speaker_amd.lightning_modules.speaker import XVectorModule, XVectorModuleConfig
    cfg = XVectorModuleConfig(tdnn_channels=list(K.CHANNELS), lin_neurons=K.LIN, in_channels=40)
    return XVectorModule.from_config(cfg, K.SPEAKERS, max_lr=1e-2, max_steps=100, **kw)


def test_xvector_module_trains_through_the_augmenter_and_none_changes_nothing():
    import xvector_cases as K
    from w2v2_speaker_amd.data import augment as A
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    B, N = 3, 4800
    wav = torch.from_numpy(AC.wave(B, N, 10))
    label = torch.tensor([0, 1, K.SPEAKERS - 1])
    batch = SpeakerClassificationDataBatch(B, ["a", "b", "c"], wav, label)
    aug = A.Augmenter(_five(_bank()), False, True, True)
    mod = _xvector(input_features="waveform", augmenter=aug)
    np.random.seed(3)
    before = mod.store.flat.clone()
    out = mod.training_step(batch)
    loss = float(out["loss"])
    print(f"augment-parity: x-vector training step on the augmented batch [{B * 6}, {aug.max_samples(N)}]: loss {loss:.4f}")
    assert np.isfinite(loss) and loss > 0 and out["prediction"].shape == (B * 6, K.SPEAKERS)
    assert torch.isfinite(mod.store.flat).all() and not torch.equal(before, mod.store.flat) and aug.step == 1
    # augmenter=None is the module built without the keyword, bit for bit
    plain, none = _xvector(input_features="waveform"), _xvector(input_features="waveform", augmenter=None)
    o1, o2 = plain.training_step(batch), none.training_step(batch)
    assert torch.equal(o1["loss"], o2["loss"]) and torch.equal(o1["prediction"], o2["prediction"])
    assert torch.equal(plain.store.flat, none.store.flat)
    with pytest.raises(ValueError, match="augmenter= needs input_features='waveform'"):
        _xvector(input_features="fbank", augmenter=aug)
