"""Length bucketing for batched variable-length evaluation, the padded batches cut by it and the cache of the static
plans that run them (no kernels: testable on the CPU).

Utterances are sorted by length, each is given a padded length (its length rounded up to ``quantum`` samples; all
utterances with the same padded length form a bucket) and every bucket is cut into batches of at most
``min(max_batch, max_batch_samples // padded_n)`` rows -- at least one, so an utterance longer than the sample budget runs
alone.  Every batch of a bucket has the same shape (the last, partial one included: the caller fills its unused rows
with dummy audio and drops their outputs), so one static plan serves the whole bucket, and buckets come in length order.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import torch

DEFAULT_QUANTUM = 32000                      # 2 s at 16 kHz
DEFAULT_MAX_BATCH_SAMPLES = 66 * 48000       # the benchmark's training batch: an eval plan never holds more audio
DEFAULT_MAX_BATCH = 64
# the same policy over filterbank frames (ECAPA-TDNN: lengths in frames of the 10 ms hop of data/fbank.py)
DEFAULT_FRAME_QUANTUM = 200                  # 2 s
DEFAULT_MAX_BATCH_FRAMES = 66 * 300          # the benchmark's ECAPA training batch
# ... and over encoder frames of the paired-input model (20 ms per frame; a trial is [CLS] left [SEP] right [SEP])
DEFAULT_PAIR_QUANTUM = 100                   # 2 s
DEFAULT_MAX_PAIR_BATCH_FRAMES = 66 * 301     # the paired training batch at 3 s + 3 s: 2 * 149 + 3 frames per pair


def plan_batches(lengths: Sequence[int], quantum: int = DEFAULT_QUANTUM,
                 max_batch_samples: int = DEFAULT_MAX_BATCH_SAMPLES,
                 max_batch: int = DEFAULT_MAX_BATCH) -> List[Tuple[Tuple[int, ...], int, int]]:
    """-> [(indices, padded_n, batch)] in ascending padded length: `indices` (positions in `lengths`, at most `batch` of
    them, ascending length, ties in input order) run in one forward of a plan of shape (batch, padded_n).
    Deterministic; every index appears exactly once."""
    if quantum < 1 or max_batch_samples < 1 or max_batch < 1:
        raise ValueError("plan_batches: quantum, max_batch_samples and max_batch must be positive")
    lens = [int(n) for n in lengths]
    if any(n < 1 for n in lens):
        raise ValueError("plan_batches: every length must be positive")
    order = sorted(range(len(lens)), key=lambda i: (lens[i], i))
    out: List[Tuple[Tuple[int, ...], int, int]] = []
    i = 0
    while i < len(order):
        padded = -(-lens[order[i]] // quantum) * quantum
        j = i
        while j < len(order) and lens[order[j]] <= padded:
            j += 1
        batch = max(1, min(max_batch, max_batch_samples // padded))
        for k in range(i, j, batch):
            out.append((tuple(order[k:min(k + batch, j)]), padded, batch))
        i = j
    return out


def padded_batches(utterances: Sequence[torch.Tensor], quantum: int, max_batch_samples: int, max_batch: int, fill: int,
                   device) -> Iterator[Tuple[Tuple[int, ...], torch.Tensor, List[int]]]:
    """The batches of plan_batches over ``utterances`` (1-D waveforms [N], or [T, F] features: the length is dim 0, in
    the unit of ``quantum`` and ``max_batch_samples``), filled: -> (indices, padded, lens) per batch, ``padded`` the zero
    f32 batch [batch, padded_n, ...] on ``device`` with utterance indices[j] copied into row j, ``lens`` its valid
    length per row.  Unused rows of a bucket's last batch stay zero and get ``fill``, the shortest length the model
    takes; the caller drops their outputs."""
    for idx, n, batch in plan_batches([x.shape[0] for x in utterances], quantum, max_batch_samples, max_batch):
        padded = torch.zeros(batch, n, *utterances[idx[0]].shape[1:], dtype=torch.float32, device=device)
        lens = [fill] * batch
        for j, i in enumerate(idx):
            padded[j, :utterances[i].shape[0]].copy_(utterances[i])
            lens[j] = utterances[i].shape[0]
        yield idx, padded, lens


class PlanCache(OrderedDict):
    """Static plans by shape key, least recently used first.  ``bound``: how many are kept (None: all of them);
    ``on_evict(key)`` is told which plan went; ``built`` counts the misses."""

    def __init__(self, bound: Optional[int] = None, on_evict: Optional[Callable] = None):
        super().__init__()
        self.bound, self.on_evict, self.built = bound, on_evict, 0

    def lookup(self, key, build: Callable):
        if key in self:
            self.move_to_end(key)
            return self[key]
        plan = self[key] = build()
        self.built += 1
        while self.bound is not None and len(self) > self.bound:
            old, _ = self.popitem(last=False)
            if self.on_evict is not None:
                self.on_evict(old)
        return plan


def plan_pair_batches(left_frames: Sequence[int], right_frames: Sequence[int], quantum: int = DEFAULT_PAIR_QUANTUM,
                      max_batch_frames: int = DEFAULT_MAX_PAIR_BATCH_FRAMES,
                      max_batch: int = DEFAULT_MAX_BATCH) -> List[Tuple[Tuple[int, ...], int, int]]:
    """plan_batches for the trials of the paired-input model, in encoder frames: trial i occupies
    ``left_frames[i] + right_frames[i] + 3`` frames of a sequence.  -> [(indices, padded_frames, batch)]."""
    if quantum < 1 or max_batch_frames < 1 or max_batch < 1:
        raise ValueError("plan_pair_batches: quantum, max_batch_frames and max_batch must be positive")
    left, right = [int(n) for n in left_frames], [int(n) for n in right_frames]
    if len(left) != len(right):
        raise ValueError(f"plan_pair_batches: {len(left)} left and {len(right)} right frame counts")
    if any(n < 1 for n in left + right):
        raise ValueError("plan_pair_batches: every side of a trial needs at least one frame")
    return plan_batches([a + b + 3 for a, b in zip(left, right)], quantum, max_batch_frames, max_batch)


def min_samples(conv_kernel: Sequence[int], conv_stride: Sequence[int]) -> int:
    """Fewest samples that give one frame out of the conv stack (400 for wav2vec2's): the length of dummy rows."""
    n = 1
    for k, s in reversed(list(zip(conv_kernel, conv_stride))):
        n = (n - 1) * s + k
    return n
