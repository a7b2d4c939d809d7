"""The reverb augmentation on the device (csrc/reverb.hip, data/augment.py) against the two oracles of
tests/reverb_cases.py: per row  max |y_dev - y_f64| <= max(4 max |y_seq32 - y_f64|, 2^-22 max |y_f64|),  the yardstick
being the f32 sequential loop's own error.  Rows are Gaussian of amplitude 0.1.

Every launch works on the guarded, sentinel-filled buffers of tests/test_augment_gpu.py next to rows that are not listed;
the source holds NaN behind every row's length.  The errors are printed next to their bounds before they are asserted
(``pytest -s``; profiles/augment_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

import augment_cases as AC
import reverb_cases as RC
from test_augment_gpu import DEV, SR, Buf, i32, within
from w2v2_speaker_amd import ops

pytestmark = pytest.mark.gpu
STRIDES = ["aligned", "odd"]


def poisoned(x, lens):
    x = np.array(x, np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan                                       # zero by index: never read
    return x


def launch(x, lens, src_rows, dst_rows, table, N_out, stride, dst_total, use_lens=True):
    """-> (src Buf, dst Buf) after one w2v2_aug_reverb; src is NaN behind every length."""
    src = Buf(x.shape[0], x.shape[1], stride, poisoned(x, lens))
    dst = Buf(dst_total, N_out, stride)
    ops.aug_reverb(src.t, dst.t, i32(src_rows), i32(dst_rows), torch.from_numpy(np.ascontiguousarray(table)).to(DEV),
                   lens=i32(lens) if use_lens else None)
    torch.cuda.synchronize()
    src.check_untouched([])
    dst.check_untouched(dst_rows)
    return src, dst


def check_row(tag, got, ref):
    """One row against (y_f64, bound, seq_err) of RC.reverb_refs: finite and within the bound."""
    y64, bound, seq = ref
    err = float(np.abs(got.astype(np.float64) - y64).max()) if got.size else 0.0
    print(f"augment-parity: reverb {tag}: max |y| {np.abs(y64).max():.3e}, sequential f32 loop {seq:.3e}, device {err:.3e}, "
          f"bound {bound:.3e}, device / bound {err / bound if bound else 0.0:.3f}")
    assert np.isfinite(got).all() and err <= bound, (tag, err, bound)


@functools.lru_cache(maxsize=None)
def edge_case():
    """Every length of RC.LENGTHS in one launch: row r has length LENGTHS[r], the coefficients COEFS[r % 12] and the delay
    edges dealt from edge r.  -> (x, lens, table, refs), the oracles computed once."""
    lens = list(RC.LENGTHS)
    R = len(lens)
    x = RC.wave(R, RC.N_MAX, 1)
    table = np.stack([RC.edge_row(r, *RC.COEFS[r % len(RC.COEFS)]) for r in range(R)])
    refs = [RC.reverb_refs(x[r], lens[r], table[r], RC.N_MAX) for r in range(R)]
    return x, lens, table, refs


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("stride", STRIDES)
def test_every_delay_edge_coefficient_and_length_in_one_launch(stride):
    x, lens, table, refs = edge_case()
    R = len(lens)
    src_rows = list(range(R))
    dst_rows = [(5 * r + 3) % (R + 2) for r in range(R)]           # a scattered list, two rows of the buffer not named
    assert len(set(dst_rows)) == R and dst_rows != src_rows
    _, dst = launch(x, lens, src_rows, dst_rows, table, RC.N_MAX, stride, R + 2)
    got = dst.np()
    for r in range(R):
        f, d, g = RC.COEFS[r % len(RC.COEFS)]
        check_row(f"edges len {lens[r]} feedback {f} damp {d} dry {g} ({stride})", got[dst_rows[r]], refs[r])
        assert not got[dst_rows[r], lens[r]:].any()                 # columns [len, N_out) are zeros, bit for bit


@pytest.mark.parametrize("N", [n for n in RC.LENGTHS if n >= 1])
def test_buffer_widths_at_the_delay_and_chunk_edges_without_lens(N):
    stride = STRIDES[N % 2]
    x = RC.wave(2, N, 100 + N)
    table = np.stack([RC.edge_row(N, 0.8817, 0.2, 0.0), RC.edge_row(N + 1, 0.98, 0.5, 1.0)])
    _, dst = launch(x, [N, N], [0, 1], [1, 0], table, N, stride, 3, use_lens=False)
    got = dst.np()
    for r in range(2):
        check_row(f"N {N} row {r} ({stride})", got[1 - r], RC.reverb_refs(x[r], N, table[r], N))


@pytest.mark.parametrize("stride", STRIDES)
def test_crops_at_a_narrower_output_and_pads_a_wider_one(stride):
    x, lens = RC.wave(3, RC.N_MAX, 7), [RC.N_MAX, 700, 3]
    table = np.stack([RC.edge_row(r, *RC.COEFS[4 + r]) for r in range(3)])
    for N_out in (600, RC.N_MAX + 70):
        _, dst = launch(x, lens, [0, 1, 2], [2, 0, 1], table, N_out, stride, 4)
        got = dst.np()
        for r, d in enumerate((2, 0, 1)):
            check_row(f"N_out {N_out} len {lens[r]} ({stride})", got[d], RC.reverb_refs(x[r], lens[r], table[r], N_out))
            assert not got[d, min(lens[r], N_out):].any()


def test_a_row_is_bit_identical_to_the_call_on_the_row_alone_and_a_launch_to_its_repeat():
    x, lens, table, _ = edge_case()
    R = len(lens)
    rows = list(range(R))
    first = launch(x, lens, rows, rows, table, RC.N_MAX, "aligned", R)[1].np()
    again = launch(x, lens, rows, rows, table, RC.N_MAX, "odd", R)[1].np()
    assert np.array_equal(first.view(np.int32), again.view(np.int32))
    for n in (3, 65, 128, RC.CHUNK + 1, RC.N_MAX):
        r = lens.index(n)
        for N in (n, n + 5):                                    # the row alone: B = 1, R = 1, any N >= len
            xr = np.zeros((1, N), np.float32)
            xr[0, :n] = x[r, :n]
            alone = launch(xr, [n], [0], [0], table[r:r + 1], N, "odd", 1)[1].np()
            assert np.array_equal(alone[0, :n].view(np.int32), first[r, :n].view(np.int32)), (r, N)
            assert not alone[0, n:].any()
    # a crop is a prefix, bit for bit
    crop = launch(x, lens, rows, rows, table, 600, "aligned", R)[1].np()
    assert np.array_equal(crop.view(np.int32), first[:, :600].view(np.int32))


def test_a_bad_table_gives_a_nan_row_and_leaves_its_neighbours_correct():
    x, lens = RC.wave(5, 300, 9), [300, 300, 200, 300, 300]
    table = np.stack([RC.edge_row(r, 0.8817, 0.35, 1.0) for r in range(5)])
    table[1, 3] = 0                                             # a comb delay of 0
    table[2, 20] = RC.MAX_DELAY + 1                             # an all-pass delay beyond the maximum
    table[3, 15] = -7
    _, dst = launch(x, lens, [0, 1, 2, 3, 4], [4, 3, 2, 1, 0], table, 300, "aligned", 6)
    got = dst.np()
    for r in (1, 2, 3):
        assert np.isnan(got[4 - r]).all(), r                     # the whole row, as w2v2_aug_fir does
    for r in (0, 4):
        check_row(f"next to a bad table, row {r}", got[4 - r], RC.reverb_refs(x[r], lens[r], table[r], 300))


@pytest.mark.parametrize("room", RC.ROOMS)
def test_reference_parameters_at_16_khz(room):
    from w2v2_speaker_amd.data.augment import reverb_parameters
    N = 3000
    x = RC.wave(2, N, 20 + room)
    rows = []
    for dry in (1.0, 0.0):
        p = reverb_parameters(SR, 50, 50, room)
        p.dry_gain = np.float32(dry)
        rows.append(p.row())
    table = np.stack(rows)
    _, dst = launch(x, [N, N - 1], [0, 1], [0, 1], table, N, STRIDES[room % 2], 2)
    got = dst.np()
    for r, dry in enumerate((1.0, 0.0)):
        check_row(f"reverb 50 50 {room} at 16 kHz, dry gain {dry}", got[r], RC.reverb_refs(x[r], N - r, table[r], N))


# ------------------------------------------------------------------------------------------------ end to end
def _three():
    from w2v2_speaker_amd.data import augment as A
    np.random.seed(4)
    return [A.ChoiceSpeedAugment(SR, [0.95, 1.05]), A.ReverbAugment(SR, on_device=True), A.ChoiceRandomNoiseAugment(SR, [15, 20])]


@pytest.mark.parametrize("stack", [False, True])
def test_augmenter_with_reverb_between_speed_and_noise(stack):
    from w2v2_speaker_amd.data import augment as A
    B, N, lengths = 3, 1600, [1600, 1500, 901]
    x = RC.wave(B, N, 30)
    augs = _three()
    aug = A.Augmenter(augs, stack_augmentations=stack, yield_intermediate_augmentations=True, yield_unaugmented=True, seed=6)
    np.random.seed(12)
    out = aug.process_batch(torch.from_numpy(x).to(DEV), torch.tensor([4, 2, 9], device=DEV), keys=["a", "b", "c"], lengths=lengths)
    No = A.resampled_length(N, 20, 19)
    got = out.network_input.cpu().numpy()
    assert got.shape == (B * 4, No) and out.source_row.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert out.ground_truth.tolist() == [4] * 4 + [2] * 4 + [9] * 4 and out.lengths.cpu().tolist() == out.lengths_host
    names = ["choice_speed", "add_reverb", "uniform_noise"]
    for b, key in enumerate("abc"):
        n, r0 = lengths[b], 4 * b
        d_speed, d_rev, d_noise = out.draws[b]
        n_speed = A.resampled_length(n, d_speed.U, d_speed.D)
        if stack:
            assert out.keys[r0:r0 + 4] == [key] + [key + "".join("/" + s for s in names[:k + 1]) for k in range(3)]
            assert out.lengths_host[r0:r0 + 4] == [n, n_speed, n_speed, n_speed]
        else:
            assert out.keys[r0:r0 + 4] == [key] + [f"{key}/{s}" for s in names]
            assert out.lengths_host[r0:r0 + 4] == [n, n_speed, n, n]
        assert d_rev is augs[1].parameters and d_rev.dry_gain == np.float32(1.0)
        assert np.array_equal(got[r0, :n], x[b, :n]) and not got[r0, n:].any()
        h = A.resample_prototype(d_speed.U, d_speed.D).astype(np.float32)
        y, bound, _ = AC.resample_ref(x[b], n, d_speed.U, d_speed.D, h, No)
        within(f"augmenter (stack {stack}) row {b} choice_speed {d_speed.U}/{d_speed.D}", got[r0 + 1], y, bound)
        xpad = np.zeros(No, np.float32)
        xpad[:N] = x[b]
        # stacked, a stage reads what the stage before it wrote on the device, and the noise is keyed by the row of its own buffer
        rev_in, rev_n = (got[r0 + 1], n_speed) if stack else (xpad, n)
        check_row(f"augmenter (stack {stack}) row {b} add_reverb room {augs[1].room_scale}", got[r0 + 2],
                  RC.reverb_refs(rev_in, rev_n, d_rev.row(), No))
        assert not got[r0 + 2, rev_n:].any()
        mix_in, mix_n, mix_row = (got[r0 + 2], n_speed, b) if stack else (xpad, n, r0 + 3)
        u = AC.uniform_stream(aug.noise_seed(0, 2), mix_row, No)
        within(f"augmenter (stack {stack}) row {b} uniform_noise", got[r0 + 3], *AC.mix_ref(mix_in, mix_n, np.float32(d_noise.coef), u))


def test_xvector_module_trains_through_the_five_augmenters_of_xvector_all_augment():
    import xvector_cases as K
    from test_augment_gpu import _xvector
    from w2v2_speaker_amd.data import augment as A
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    B, N = 3, 4800
    wav = torch.from_numpy(RC.wave(B, N, 10))
    batch = SpeakerClassificationDataBatch(B, ["a", "b", "c"], wav, torch.tensor([0, 1, K.SPEAKERS - 1]))
    np.random.seed(5)
    aug = A.Augmenter([A.TimeDropoutAugment(SR, 0.25, 0, 5), A.FrequencyDropoutAugment(SR, 0, 5, 1), A.ChoiceSpeedAugment(SR, [0.95, 1, 1.05]),
                       A.ReverbAugment(SR, room_scale_min=0, room_scale_max=100, on_device=True),
                       A.ChoiceNoiseAugment(SR, [15, 20, 100])], False, True, True)
    mod = _xvector(input_features="waveform", augmenter=aug)
    before = mod.store.flat.clone()
    out = mod.training_step(batch)
    loss = float(out["loss"])
    print(f"augment-parity: x-vector training step through the five augmenters [{B * aug.rows_per_sample()}, {aug.max_samples(N)}]: "
          f"loss {loss:.4f}")
    assert aug.rows_per_sample() == 6 and out["prediction"].shape == (B * aug.rows_per_sample(), K.SPEAKERS)
    assert np.isfinite(loss) and loss > 0 and torch.isfinite(mod.store.flat).all() and not torch.equal(before, mod.store.flat)
    assert aug.step == 1
