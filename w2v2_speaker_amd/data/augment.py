"""The ``augmenter`` stage of the reference's training pipelines on the device (ref: src/data/preprocess/augment.py,
config/data/pipeline/xvector_*augment*.yaml: selector -> augmenter -> filterbank -> normalizer).

The host draws every row's parameters with the reference's ``np.random`` calls in the reference's order -- sample by
sample, augmenter by augmenter -- and designs the filters in numpy; each draw is a small record, no sample is touched on
the host.  The records of a step go up as ONE table through two pinned staging buffers used in turn, and the kernels of
csrc/augment.hip and csrc/reverb.hip (include/w2v2_hip.h, "waveform augmentation": the definition of the six operations)
do the work on the [B, N] waveforms where they lie.  The reference runs the effects through WavAugment / libsox; what is
restated from memory of that library is marked "as recollected" here and listed in DESIGN.md 7.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

AUG_MAX_TAPS = 2561                 # ops.AUG_MAX_TAPS: five composed 513-tap stages
SINC_ATTENUATION_DB = 120.0         # the reference's `sinc -a 120`
RESAMPLE_ATTENUATION_DB = 80.0      # the resampling prototype's Kaiser window (this module's choice)
RESAMPLE_ZEROS = 32                 # zero crossings of the prototype on either side: half = 32 max(U, D)
REVERB_MAX_DELAY = 1024             # ops.AUG_REVERB_MAX_DELAY
REVERB_PARAMS = 28                  # ops.AUG_REVERB_PARAMS
REVERB_COMB_LENGTHS = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)      # at 44.1 kHz (sox reverb.c, as recollected)
REVERB_ALLPASS_LENGTHS = (225, 341, 441, 556)
REVERB_STEREO_ADJUST = 12
REVERB_WET_GAIN = 0.015             # 0 dB wet gain, no pre-delay


# ------------------------------------------------------------------------------------------------ filter design (numpy, f64)
def kaiser_beta(attenuation_db: float) -> float:
    """Kaiser's beta for a stop-band attenuation above 50 dB: 0.1102 (A - 8.7)."""
    return 0.1102 * (attenuation_db - 8.7)


def kaiser_transition_hz(taps: int, sample_rate: float, attenuation_db: float = SINC_ATTENUATION_DB) -> float:
    """Width of the transition band of a Kaiser-windowed sinc: (A - 7.95) / (2.285 (taps - 1)) rad per sample."""
    return (attenuation_db - 7.95) / (2.285 * (taps - 1)) * sample_rate / (2.0 * math.pi)


@functools.lru_cache(maxsize=16)
def _kaiser_window(taps: int, beta: float) -> Tuple[np.ndarray, np.ndarray]:
    """(tap positions about the centre, Kaiser window), f64, computed once per (taps, beta): the Bessel function is
    most of a stage's design time."""
    n, w = np.arange(taps, dtype=np.float64) - (taps - 1) / 2, np.kaiser(taps, beta)
    n.setflags(write=False)
    w.setflags(write=False)
    return n, w


def _lowpass(fc: float, n: np.ndarray, window: np.ndarray) -> np.ndarray:
    """Windowed-sinc low-pass with its -6 dB point at fc (in cycles per sample), f64."""
    return 2.0 * fc * np.sinc(2.0 * fc * n) * window


def band_reject_taps(low_hz: float, high_hz: float, sample_rate: float, taps: int = 513,
                     attenuation_db: float = SINC_ATTENUATION_DB) -> np.ndarray:
    """One `sinc -a 120 high-low` stage: a low-pass at ``low_hz`` plus a high-pass at ``high_hz`` (the unit impulse minus
    a low-pass), both Kaiser-windowed sincs of ``taps`` (odd) taps.  f64, centre tap at (taps - 1) / 2."""
    if taps < 3 or taps % 2 == 0:
        raise ValueError(f"taps={taps}: an odd count of at least 3")
    if not 0.0 <= low_hz <= high_hz <= sample_rate / 2:
        raise ValueError(f"band [{low_hz}, {high_hz}] Hz outside [0, {sample_rate / 2}] or reversed")
    n, w = _kaiser_window(taps, kaiser_beta(attenuation_db))
    h = _lowpass(low_hz / sample_rate, n, w) - _lowpass(high_hz / sample_rate, n, w)
    h[(taps - 1) // 2] += 1.0
    return h


def compose_taps(stages: Sequence[np.ndarray]) -> np.ndarray:
    """The one filter that equals the stages applied in turn to an unbounded signal: their convolution (f64).  No stage
    gives the unit impulse.  Against truncated passes the result differs only within a filter's half-width of a row's
    ends, where an intermediate pass would have cut the tail the next one reads."""
    h = np.ones(1, dtype=np.float64)
    for s in stages:
        h = np.convolve(h, np.asarray(s, dtype=np.float64))
    return h


def speed_ratio(speed: float, max_denominator: int = 64) -> Tuple[int, int]:
    """(U, D) with U / D the closest fraction to 1 / speed under ``max_denominator``: 0.95 -> 20/19, 1.05 -> 20/21."""
    if not speed > 0:
        raise ValueError(f"speed factor {speed!r} must be positive")
    f = Fraction(1.0 / float(speed)).limit_denominator(max_denominator)
    if f.numerator < 1:
        raise ValueError(f"speed factor {speed!r} is too large for max_denominator={max_denominator}")
    return f.numerator, f.denominator


def resample_prototype(U: int, D: int, attenuation_db: float = RESAMPLE_ATTENUATION_DB) -> np.ndarray:
    """The low-pass of w2v2_aug_resample at the U-times-oversampled rate: a Kaiser-windowed sinc with its cutoff at
    1 / max(U, D) of that rate's Nyquist frequency and half = 32 max(U, D) taps on either side, scaled to unit DC gain."""
    m = max(int(U), int(D))
    half = RESAMPLE_ZEROS * m
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(n / m) * np.kaiser(2 * half + 1, kaiser_beta(attenuation_db))
    return h / h.sum()


def resampled_length(n: int, U: int, D: int) -> int:
    return -(-int(n) * int(U) // int(D))


def snr_to_coef(snr_db: float) -> float:
    """additive_noise, as recollected: r = 10^(snr / 10), the signal's weight is r / (1 + r)."""
    r = 10.0 ** (float(snr_db) / 10.0)
    return r / (1.0 + r)


# ------------------------------------------------------------------------------------------------ the draws' records
@dataclass
class DropoutDraw:
    spans: List[Tuple[int, int]]                # (start, length) per span, in draw order


@dataclass
class BandDraw:
    bands: List[Tuple[float, float]]            # (low, high) Hz per stage, in draw order
    taps: np.ndarray                            # the composed filter, f64


@dataclass
class SpeedDraw:
    speed: float
    U: int
    D: int


@dataclass
class NoiseDraw:
    snr: float
    coef: float
    bank_row: int = -1                          # ChoiceRirsNoiseAugment: which noise of the bank


@dataclass
class ReverbDraw:
    """One row of w2v2_aug_reverb's table: delays [array][filter], coefficients already rounded to f32."""
    comb_delays: np.ndarray                     # int32 [2, 8]
    allpass_delays: np.ndarray                  # int32 [2, 4]
    feedback: np.float32
    damp: np.float32
    wet_gain: np.float32
    dry_gain: np.float32 = np.float32(1.0)

    def row(self) -> np.ndarray:
        """int32 [REVERB_PARAMS]: the delays, then the f32 coefficients by their bits."""
        coef = np.asarray([self.feedback, self.damp, self.wet_gain, self.dry_gain], np.float32).view(np.int32)
        return np.concatenate([self.comb_delays.reshape(-1), self.allpass_delays.reshape(-1), coef]).astype(np.int32)


def reverb_parameters(sample_rate: float, reverberance: float, damping: float, room_scale: float) -> ReverbDraw:
    """sox's `reverb <reverberance> <damping> <room_scale>` on a mono input (stereo depth 100: two filter arrays), as
    recollected from reverb.c and stated in include/w2v2_hip.h; the arithmetic in float64.  ValueError when a delay leaves
    [1, REVERB_MAX_DELAY]."""
    r = float(sample_rate) / 44100.0
    scale = float(room_scale) / 100.0 * 0.9 + 0.1
    combs, allpasses = np.zeros((2, 8), np.int32), np.zeros((2, 4), np.int32)
    for w in range(2):
        sign = 1.0                                      # flips after every filter, through the combs and on through the all-passes
        for i, length in enumerate(REVERB_COMB_LENGTHS):
            combs[w, i] = int(scale * r * (length + REVERB_STEREO_ADJUST * sign * w) + 0.5)
            sign = -sign
        for j, length in enumerate(REVERB_ALLPASS_LENGTHS):
            allpasses[w, j] = int(r * (length + REVERB_STEREO_ADJUST * sign * w) + 0.5)
            sign = -sign
    lo, hi = min(combs.min(), allpasses.min()), max(combs.max(), allpasses.max())
    if lo < 1 or hi > REVERB_MAX_DELAY:
        raise ValueError(f"reverb at {sample_rate} Hz, room scale {room_scale}: delays {lo} .. {hi} outside "
                         f"[1, {REVERB_MAX_DELAY}]")
    a = -1.0 / math.log(1.0 - 0.3)
    b = 100.0 / (math.log(1.0 - 0.98) * a + 1.0)
    feedback = 1.0 - math.exp((float(reverberance) - b) / (a * b))
    damp = float(damping) / 100.0 * 0.3 + 0.2
    return ReverbDraw(combs, allpasses, np.float32(feedback), np.float32(damp), np.float32(REVERB_WET_GAIN))


# ------------------------------------------------------------------------------------------------ the reference's classes
class SpecAugmentBand:
    """ref: augment.py:246-269.  Two uniform draws on the mel scale, width first, then the lower edge; ``__call__``
    returns the reference's "<high>-<low>" string, ``draw`` the same two numbers as (low, high)."""

    def __init__(self, sampling_rate, scalar):
        self.sampling_rate = sampling_rate
        self.scalar = scalar

    @staticmethod
    def freq2mel(f):
        return 2595.0 * np.log10(1 + f / 700)

    @staticmethod
    def mel2freq(m):
        return (10.0 ** (m / 2595.0) - 1) * 700

    def draw(self) -> Tuple[float, float]:
        width_limit = 27.0 * self.scalar
        mel_top = self.freq2mel(self.sampling_rate / 2)
        mel_width = np.random.uniform(0, mel_top * width_limit / 256.0)
        mel_low = np.random.uniform(0, mel_top - mel_width)
        return self.mel2freq(mel_low), self.mel2freq(mel_low + mel_width)

    def __call__(self):
        low, high = self.draw()
        return f"{high}-{low}"


class WaveAugment:
    """What every augmentation has: ``sample_rate``, the reference's ``name`` (the key suffix), and ``draw(n)`` -- this
    row's parameters for an input of ``n`` samples, with the reference's np.random calls in the reference's order."""
    kind = ""

    def __init__(self, sample_rate: int, name: str):
        self.sample_rate = sample_rate
        self.name = name

    def draw(self, n: int):
        raise NotImplementedError

    def max_length(self, n: int) -> int:
        """The longest output an input of n samples can give."""
        return n


def _count(lo: int, hi: int) -> int:
    return int(np.random.randint(lo, hi + 1))


class TimeDropoutAugment(WaveAugment):
    """ref: augment.py:216-239: a count in [min_drop_count, max_drop_count], then that many time_dropout effects.  Each,
    as recollected: length = randint(0, max_frames), start = randint(0, max(n - length, 1)), x[start : start + length] = 0
    with max_frames = int(max_seconds * sample_rate)."""
    kind = "dropout"

    def __init__(self, sample_rate: int, max_dropout_length_seconds: float, min_drop_count: int, max_drop_count: int):
        super().__init__(sample_rate, "time_dropout")
        self.max_dropout_length_seconds = max_dropout_length_seconds
        self.min_drops = min_drop_count
        self.max_drops = max_drop_count
        self.max_frames = int(max_dropout_length_seconds * sample_rate)
        if self.max_frames < 1:
            raise ValueError("max_dropout_length_seconds * sample_rate must be at least one sample")

    def draw(self, n: int) -> DropoutDraw:
        spans = []
        for _ in range(_count(self.min_drops, self.max_drops)):
            length = int(np.random.randint(0, self.max_frames))
            spans.append((int(np.random.randint(0, max(n - length, 1))), length))
        return DropoutDraw(spans)


class FrequencyDropoutAugment(WaveAugment):
    """ref: augment.py:272-297: a count, then that many `sinc -a 120 <band>` stages, every band from SpecAugmentBand.
    ``taps`` (this module's; sox derives its own count from a transition width) is the length of one stage; the stages
    of a row are composed into one filter of at most count * (taps - 1) + 1 taps."""
    kind = "fir"

    def __init__(self, sample_rate: int, min_drop_count: int, max_drop_count: int, band_scaling: float, *, taps: int = 513):
        super().__init__(sample_rate, "frequency_dropout")
        self.min_drops = min_drop_count
        self.max_drops = max_drop_count
        self.band_scaling = band_scaling
        self.taps = int(taps)
        if self.taps < 3 or self.taps % 2 == 0 or max_drop_count * (self.taps - 1) + 1 > AUG_MAX_TAPS:
            raise ValueError(f"taps={taps}: odd, at least 3, and max_drop_count * (taps - 1) + 1 <= {AUG_MAX_TAPS}")

    def draw(self, n: int) -> BandDraw:
        band = SpecAugmentBand(self.sample_rate, self.band_scaling)
        bands = [band.draw() for _ in range(_count(self.min_drops, self.max_drops))]
        return BandDraw(bands, compose_taps([band_reject_taps(lo, hi, self.sample_rate, self.taps) for lo, hi in bands]))


class _SpeedAugment(WaveAugment):
    kind = "speed"

    def __init__(self, sample_rate: int, name: str, max_denominator: int):
        super().__init__(sample_rate, name)
        self.max_denominator = int(max_denominator)

    def _speed(self) -> float:
        raise NotImplementedError

    def _speeds(self) -> Sequence[float]:
        raise NotImplementedError

    def draw(self, n: int) -> SpeedDraw:
        s = float(self._speed())
        return SpeedDraw(s, *speed_ratio(s, self.max_denominator))

    def max_length(self, n: int) -> int:
        return max(resampled_length(n, *speed_ratio(s, self.max_denominator)) for s in self._speeds())


class ChoiceSpeedAugment(_SpeedAugment):
    """ref: augment.py:195-209: `speed <np.random.choice(factors)>` then `rate`: the row resampled by U / D ~ 1 / factor."""

    def __init__(self, sample_rate: int, possible_speed_factors: List[float], *, max_denominator: int = 64):
        super().__init__(sample_rate, "choice_speed", max_denominator)
        self.choices = possible_speed_factors

    def _speed(self):
        return np.random.choice(self.choices)

    def _speeds(self):
        return self.choices


class UniformSpeedAugment(_SpeedAugment):
    """ref: augment.py:175-192: the factor is np.random.uniform(min, max); it is QUANTISED to the closest U / D with
    D <= max_denominator (one launch per distinct ratio of a batch)."""

    def __init__(self, sample_rate: int, min_speed_factor: float, max_speed_factor: float, *, max_denominator: int = 64):
        super().__init__(sample_rate, "uniform_speed", max_denominator)
        self.min_speed = min_speed_factor
        self.max_speed = max_speed_factor

    def _speed(self):
        return np.random.uniform(self.min_speed, self.max_speed)

    def _speeds(self):
        return (self.min_speed, self.max_speed)           # the length is monotone in the factor


class ChoiceRandomNoiseAugment(WaveAugment):
    """ref: augment.py:304-329: uniform [0, 1) noise at an SNR of np.random.choice(snr_choices)."""
    kind = "mix_uniform"

    def __init__(self, sample_rate: int, snr_choices: List[int]):
        super().__init__(sample_rate, "uniform_noise")
        self.snr_choices = snr_choices

    def draw(self, n: int) -> NoiseDraw:
        snr = float(np.random.choice(self.snr_choices))
        return NoiseDraw(snr, snr_to_coef(snr))


ChoiceNoiseAugment = ChoiceRandomNoiseAugment      # the name config/data/pipeline/xvector_all_augment_pipeline.yaml uses


class ChoiceRirsNoiseAugment(WaveAugment):
    """ref: augment.py:340-411: a point-source noise, repeated until it covers the utterance, added at an SNR of
    np.random.choice(snr_choices); nothing is convolved.  ``noise_bank`` stands where the reference takes
    ``shards_folder``: a list of 1-D float32 device tensors, or a ([M, L] float32 device tensor, lengths) pair.  The
    noises are taken in the bank's order, round and round (the reference's shuffle buffer of 10 is not restated; it
    draws nothing from np.random)."""
    kind = "mix_bank"

    def __init__(self, sample_rate: int, snr_choices: List[int], noise_bank):
        super().__init__(sample_rate, "rirs_background_noise")
        self.snr_choices = snr_choices
        if isinstance(noise_bank, (tuple, list)) and len(noise_bank) == 2 and isinstance(noise_bank[0], torch.Tensor) \
                and noise_bank[0].dim() == 2:
            bank, lens = noise_bank[0], [int(v) for v in noise_bank[1]]
        else:
            rows = [t.reshape(-1) for t in noise_bank]
            if not rows:
                raise ValueError("noise_bank is empty")
            lens = [int(t.numel()) for t in rows]
            bank = torch.zeros(len(rows), max(lens), dtype=torch.float32, device=rows[0].device)
            for i, t in enumerate(rows):
                bank[i, :lens[i]] = t.to(torch.float32)
        if bank.dtype != torch.float32 or len(lens) != bank.shape[0] or min(lens) < 1 or max(lens) > bank.shape[1]:
            raise ValueError("noise_bank: float32 [M, L] with 1 <= lengths[m] <= L")
        self.bank = bank.contiguous()
        self.bank_lens_host = lens
        self.bank_lens = torch.tensor(lens, dtype=torch.int32).to(bank.device)
        self._next = 0

    def draw(self, n: int) -> NoiseDraw:
        row = self._next
        self._next = (row + 1) % len(self.bank_lens_host)
        snr = float(np.random.choice(self.snr_choices))
        return NoiseDraw(snr, snr_to_coef(snr), row)


class ReverbAugment(WaveAugment):
    """ref: augment.py:418-458: `reverb <reverberance> <damping> <room_scale>` then `channels`.  The constructor and its
    three draws (reverberance, damping, room scale, once, at construction) are the reference's.  ``on_device=True`` asks
    for the device form (w2v2_aug_reverb): ``draw`` then returns the one record the three values give and makes no
    np.random call.  Without it ``draw`` raises as it did before the device had the effect."""
    kind = "reverb"

    def __init__(self, sample_rate: int, reverberance_min: int = 50, reverberance_max: int = 50, damping_min: int = 50,
                 damping_max: int = 50, room_scale_min: int = 0, room_scale_max: int = 100, *, on_device: bool = False):
        super().__init__(sample_rate, "add_reverb")
        self.reverberance_min, self.reverberance_max = reverberance_min, reverberance_max
        self.damping_min, self.damping_max = damping_min, damping_max
        self.room_scale_min, self.room_scale_max = room_scale_min, room_scale_max
        self.reverberance = _count(reverberance_min, reverberance_max)
        self.damping = _count(damping_min, damping_max)
        self.room_scale = _count(room_scale_min, room_scale_max)
        self.on_device = bool(on_device)
        self.parameters = reverb_parameters(sample_rate, self.reverberance, self.damping, self.room_scale) if on_device else None

    def draw(self, n: int) -> ReverbDraw:
        if not self.on_device:
            raise NotImplementedError("ReverbAugment has no device form: sox's reverb is a recursive filter bank, sequential "
                                      "in time; leave it out of the augmenter's list")
        return self.parameters


# ------------------------------------------------------------------------------------------------ the augmenter
@dataclass
class AugmentedBatch:
    network_input: torch.Tensor         # [B', N'] f32 on the device, zero behind every row's length
    lengths: torch.Tensor               # [B'] int32 on the device
    ground_truth: torch.Tensor          # [B']
    keys: List[str]
    source_row: torch.Tensor            # [B'] int64 (host): the input row every output row came from
    lengths_host: List[int]
    draws: List[List[object]]           # per input row, one record per augmenter


class _Table:
    """The step's parameter tables as one int32 array (f32 sections are stored by their bits), every section 16-byte
    aligned; ``add`` returns the section's (offset, count)."""

    def __init__(self):
        self.parts: List[np.ndarray] = []
        self.size = 0

    def add(self, a: np.ndarray) -> Tuple[int, int, bool]:
        a = np.ascontiguousarray(a)
        is_f = a.dtype == np.float32
        assert is_f or a.dtype == np.int32
        flat = a.reshape(-1).view(np.int32)
        pad = -flat.size % 4
        off = self.size
        self.parts.append(flat)
        if pad:
            self.parts.append(np.zeros(pad, np.int32))
        self.size += flat.size + pad
        return off, flat.size, is_f


class Augmenter:
    """ref: augment.py:78-143, on a whole device batch.  ``process_batch`` gives the rows ``process`` would give for
    every sample of the batch, in the reference's order: per input row the unaugmented row (``yield_unaugmented``), then
    one row per augmenter (``yield_intermediate_augmentations``) or the last one only; with ``stack_augmentations`` an
    augmenter reads what the one before it wrote."""

    def __init__(self, augmenters: List[WaveAugment], stack_augmentations: bool, yield_intermediate_augmentations: bool,
                 yield_unaugmented: bool, *, seed: int = 0):
        if not stack_augmentations and not yield_intermediate_augmentations:
            raise ValueError("augmenter must at least stack augmentations or yield intermediate augmentations")
        self.augmenters = list(augmenters)
        self.stack_augmentations = stack_augmentations
        self.yield_intermediate_augmentations = yield_intermediate_augmentations
        self.yield_unaugmented = yield_unaugmented
        self.seed = int(seed)
        self.step = 0
        self._dev: Optional[torch.Tensor] = None
        self._stage: List[Optional[torch.Tensor]] = [None, None]
        self._copied: List[Optional[torch.cuda.Event]] = [None, None]
        self._turn = 0
        self._protos: Dict[Tuple[int, int], torch.Tensor] = {}

    # -- shapes ---------------------------------------------------------------------------------
    def rows_per_sample(self) -> int:
        if not self.yield_intermediate_augmentations:       # (the reference returns the last sample alone)
            return 1
        return int(bool(self.yield_unaugmented)) + len(self.augmenters)

    def _check_device_forms(self) -> None:
        for a in self.augmenters:
            if a.kind == "reverb":
                a.draw(0)                               # raises NotImplementedError unless it was built with on_device=True

    def max_samples(self, n: int) -> int:
        """The longest row an input of n samples can give: nothing is cropped at this width."""
        top = cur = int(n)
        for a in self.augmenters:
            m = a.max_length(cur if self.stack_augmentations else int(n))
            top = max(top, m)
            cur = m
        return top

    def output_shape(self, batch: int, samples: int, out_samples: Optional[int] = None) -> Tuple[int, int]:
        return batch * self.rows_per_sample(), int(out_samples) if out_samples is not None else self.max_samples(samples)

    # -- the host half: draws and row plan ------------------------------------------------------------
    def plan(self, lengths: Sequence[int], keys: Sequence[str], out_samples: int):
        """Draw every row's parameters (np.random, the reference's order) -> (draws, out_keys, out_lengths, source_row,
        stage_lengths) with stage_lengths[k][b] the length augmenter k leaves for input row b (before cropping)."""
        K, per = len(self.augmenters), self.rows_per_sample()
        draws, out_keys, out_lens, source = [], [], [], []
        stage_lens = [[0] * len(lengths) for _ in range(K)]
        for b, n0 in enumerate(lengths):
            cur_n, cur_key, row_draws = int(n0), keys[b], []
            inter = self.yield_intermediate_augmentations
            rows: List[Tuple[str, int]] = [(cur_key, cur_n)] if self.yield_unaugmented and inter else []
            for k, a in enumerate(self.augmenters):
                d = a.draw(cur_n)
                row_draws.append(d)
                n_new = min(resampled_length(cur_n, d.U, d.D), out_samples) if a.kind == "speed" else min(cur_n, out_samples)
                stage_lens[k][b] = n_new
                key_new = cur_key + f"/{a.name}"
                if self.yield_intermediate_augmentations:
                    rows.append((key_new, n_new))
                if self.stack_augmentations:
                    cur_n, cur_key = n_new, key_new
            if not inter:
                rows = [(cur_key, cur_n)]
            assert len(rows) == per
            draws.append(row_draws)
            for key, n in rows:
                out_keys.append(key)
                out_lens.append(min(n, out_samples))
                source.append(b)
        return draws, out_keys, out_lens, source, stage_lens

    # -- the upload -----------------------------------------------------------------------------------
    def _upload(self, table: np.ndarray, device: torch.device) -> torch.Tensor:
        n = table.size
        if self._dev is None or self._dev.numel() < n or self._dev.device != device:
            cap = max(1024, 1 << (n - 1).bit_length())
            self._dev = torch.zeros(cap, dtype=torch.int32, device=device)
            torch.cuda.synchronize(device)              # (a new buffer, not every step: uploads still in flight read the old stagings)
            self._stage = [torch.zeros(cap, dtype=torch.int32, pin_memory=True) for _ in range(2)]
            self._copied = [None, None]
        t = self._turn
        self._turn = 1 - t
        if self._copied[t] is not None:
            self._copied[t].synchronize()               # the upload of two steps ago has left this staging buffer
        self._stage[t][:n].copy_(torch.from_numpy(table))
        self._dev[:n].copy_(self._stage[t][:n], non_blocking=True)
        self._copied[t] = torch.cuda.Event()
        self._copied[t].record()
        return self._dev

    def _prototype(self, U: int, D: int, device) -> torch.Tensor:
        h = self._protos.get((U, D))
        if h is None:                                   # once per ratio, kept
            h = torch.from_numpy(resample_prototype(U, D).astype(np.float32)).to(device)
            self._protos[(U, D)] = h
        return h

    # -- the device half ------------------------------------------------------------------------------
    def process_batch(self, wav: torch.Tensor, ground_truth: torch.Tensor, keys: Optional[Sequence[str]] = None,
                      lengths=None, out_samples: Optional[int] = None) -> AugmentedBatch:
        from .. import ops
        if not isinstance(wav, torch.Tensor) or wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_cuda:
            raise ValueError("process_batch: wav is a float32 [B, N] tensor on the device")
        self._check_device_forms()
        B, N = wav.shape
        if isinstance(lengths, torch.Tensor):
            if lengths.is_cuda:
                raise ValueError("lengths must be Python ints or a CPU integer tensor")
            lengths = lengths.reshape(-1).tolist()
        lens0 = [N] * B if lengths is None else [int(v) for v in lengths]
        if len(lens0) != B or min(lens0) < 0 or max(lens0) > N:
            raise ValueError(f"lengths: {B} values in [0, {N}]")
        keys = [f"{i}" for i in range(B)] if keys is None else list(keys)
        if len(keys) != B or ground_truth.shape[0] != B:
            raise ValueError(f"keys / ground_truth: one per row of a batch of {B}")
        Bo, No = self.output_shape(B, N, out_samples)
        if No < 1:
            raise ValueError(f"out_samples={out_samples}")
        K, per, stack = len(self.augmenters), self.rows_per_sample(), self.stack_augmentations
        draws, out_keys, out_lens, source, stage_lens = self.plan(lens0, keys, No)
        dev = wav.device

        # ---- the table: lengths, row lists, and every stage's parameters
        tb = _Table()
        s_lens0 = tb.add(np.asarray(lens0, np.int32))
        s_out_lens = tb.add(np.asarray(out_lens, np.int32))
        s_iota = tb.add(np.arange(B, dtype=np.int32))
        last_only = not self.yield_intermediate_augmentations
        first = int(bool(self.yield_unaugmented and not last_only) or (last_only and K == 0))
        s_unaug = tb.add(np.arange(B, dtype=np.int32) * per) if first else None
        stages = []
        for k, a in enumerate(self.augmenters):
            st = {"kind": a.kind, "aug": a}
            yielded = self.yield_intermediate_augmentations or k == K - 1
            slot = 0 if last_only else first + k
            st["out_rows"] = tb.add(np.arange(B, dtype=np.int32) * per + slot) if yielded else None
            if stack:
                st["lens"] = tb.add(np.asarray(stage_lens[k], np.int32))
            ds = [draws[b][k] for b in range(B)]
            if a.kind == "dropout":
                S = max(len(d.spans) for d in ds)
                sp = np.zeros((B, S, 2), np.int32)
                for b, d in enumerate(ds):
                    for s, span in enumerate(d.spans):
                        sp[b, s] = span
                st["spans"], st["S"] = tb.add(sp), S
            elif a.kind == "fir":
                ldt = (max(d.taps.size for d in ds) + 3) // 4 * 4
                tp = np.zeros((B, ldt), np.float32)
                for b, d in enumerate(ds):
                    tp[b, :d.taps.size] = d.taps
                st["taps"], st["ldt"] = tb.add(tp), ldt
                st["ntaps"] = tb.add(np.asarray([d.taps.size for d in ds], np.int32))
            elif a.kind == "speed":
                groups: Dict[Tuple[int, int], List[int]] = {}
                for b, d in enumerate(ds):
                    groups.setdefault((d.U, d.D), []).append(b)
                st["groups"] = [(ud, tb.add(np.asarray(bs, np.int32)), bs) for ud, bs in sorted(groups.items())]
                if yielded:
                    st["group_out"] = [tb.add(np.asarray(bs, np.int32) * per + slot) for _, _, bs in st["groups"]]
            elif a.kind in ("mix_uniform", "mix_bank"):
                st["coef"] = tb.add(np.asarray([d.coef for d in ds], np.float32))
                if a.kind == "mix_bank":
                    st["bank_row"] = tb.add(np.asarray([d.bank_row for d in ds], np.int32))
            elif a.kind == "reverb":
                st["params"] = tb.add(np.stack([d.row() for d in ds]))
            else:
                raise NotImplementedError(f"augmenter kind {a.kind!r}")
            stages.append(st)
        table = np.concatenate(tb.parts) if tb.parts else np.zeros(0, np.int32)
        tdev = self._upload(table, dev)

        def sec(s):
            off, n, is_f = s
            v = tdev[off:off + n]
            return v.view(torch.float32) if is_f else v

        out = torch.empty(Bo, No, dtype=torch.float32, device=dev)
        lens0_d, out_lens_d, iota = sec(s_lens0), sec(s_out_lens), sec(s_iota)
        if first:
            ops.aug_resample(wav, out, iota, sec(s_unaug), 1, 1, lens=lens0_d)
        tmp: List[Optional[torch.Tensor]] = [None, None]
        src, src_lens = wav, lens0_d
        for k, st in enumerate(stages):
            a = st["aug"]
            if stack:                                   # a stage writes a buffer of its own; what is yielded is copied out
                if tmp[k % 2] is None:
                    tmp[k % 2] = torch.empty(B, No, dtype=torch.float32, device=dev)
                dst, dst_rows, dst_lens = tmp[k % 2], iota, sec(st["lens"])
            else:
                dst, dst_rows, dst_lens = out, sec(st["out_rows"]), out_lens_d
            kind = st["kind"]
            if kind == "fir":
                ops.aug_fir(src, dst, iota, dst_rows, sec(st["taps"]).view(B, st["ldt"]), sec(st["ntaps"]), lens=src_lens)
            elif kind == "speed":
                for g, ((U, D), s_rows, _) in enumerate(st["groups"]):
                    g_dst = sec(s_rows) if stack else sec(st["group_out"][g])
                    ops.aug_resample(src, dst, sec(s_rows), g_dst, U, D, None if U == D else self._prototype(U, D, dev),
                                     lens=src_lens)
            elif kind == "reverb":
                ops.aug_reverb(src, dst, iota, dst_rows, sec(st["params"]).view(B, REVERB_PARAMS), lens=src_lens)
            else:
                ops.aug_resample(src, dst, iota, dst_rows, 1, 1, lens=src_lens)
                if kind == "dropout":
                    ops.aug_time_dropout(dst, dst_rows, sec(st["spans"]).view(B, st["S"], 2), lens=dst_lens)
                elif kind == "mix_uniform":
                    ops.aug_mix_uniform(dst, dst_rows, sec(st["coef"]), self.noise_seed(self.step, k), lens=dst_lens)
                else:
                    ops.aug_mix_bank(dst, dst_rows, sec(st["coef"]), a.bank, a.bank_lens, sec(st["bank_row"]), lens=dst_lens)
            if stack:
                if st["out_rows"] is not None:
                    ops.aug_resample(dst, out, iota, sec(st["out_rows"]), 1, 1, lens=dst_lens)
                src, src_lens = dst, dst_lens
        self.step += 1
        gt = torch.repeat_interleave(ground_truth, per, dim=0)
        return AugmentedBatch(out, out_lens_d.clone(), gt, out_keys, torch.tensor(source, dtype=torch.int64), out_lens, draws)

    def noise_seed(self, step: int, k: int) -> int:
        """The seed of augmenter k's uniform noise in step ``step``: distinct per (seed, step, augmenter)."""
        return ((self.seed * 1_000_003 + step) * 64 + k) & (2 ** 63 - 1)
