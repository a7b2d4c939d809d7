"""ref: src/evaluation/speech/wer.py -- the word error rate, which the reference takes from jiwer: the word-level edit
distance (substitutions + deletions + insertions) summed over all sentences, over the number of reference words summed
over all sentences.  Words are what ``str.split()`` gives."""
from typing import List, Sequence


def _edit_distance(ref: Sequence[str], hyp: Sequence[str]) -> int:
    prev = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        cur = [i] + [0] * len(hyp)
        for j, h in enumerate(hyp, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (r != h))
        prev = cur
    return prev[-1]


def calculate_wer(transcriptions: List[str], ground_truths: List[str]) -> float:
    if isinstance(transcriptions, str):
        transcriptions = [transcriptions]
    if isinstance(ground_truths, str):
        ground_truths = [ground_truths]
    if len(transcriptions) != len(ground_truths):
        raise ValueError(f"wer: {len(transcriptions)} transcriptions for {len(ground_truths)} ground truths")
    errors = words = 0
    for hyp, ref in zip(transcriptions, ground_truths):
        r, h = ref.split(), hyp.split()
        errors += _edit_distance(r, h)
        words += len(r)
    if words == 0:
        raise ValueError("wer: the ground truths hold no word")
    return errors / words
