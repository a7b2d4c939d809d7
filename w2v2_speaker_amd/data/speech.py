"""ref: src/data/modules/speech/training_batch_speech.py -- the sample and batch of the speech recognition path and their
collate: waveforms and transcripts of different lengths right-padded with zeros to the longest of the batch, the lengths
before padding and the transcript strings kept beside them.  (Token 0 is the CTC blank, so a padded transcript row ends in
blanks nobody reads: the loss takes ``ground_truth_sequence_length``.)"""
import dataclasses
from typing import Dict, List, Optional

import torch


@dataclasses.dataclass
class SpeechRecognitionDataSample:
    key: str
    ground_truth: torch.Tensor                      # [SEQUENCE_LENGTH] token ids, 0 = blank
    ground_truth_string: str
    network_input: torch.Tensor                     # [NUM_FRAMES] (or [1, NUM_FRAMES]) waveform
    input_length: int                               # NUM_FRAMES before padding
    ground_truth_sequence_length: torch.Tensor      # the length of ``ground_truth``
    side_info: Optional[object] = None


@dataclasses.dataclass
class SpeechRecognitionDataBatch:
    batch_size: int
    keys: List[str]
    network_input: torch.Tensor                     # [BATCH_SIZE, MAX_NUM_FRAMES]
    input_lengths: List[int]
    ground_truth: torch.Tensor                      # [BATCH_SIZE, MAX_SEQUENCE_LENGTH]
    ground_truth_strings: List[str]
    ground_truth_sequence_length: torch.Tensor      # [BATCH_SIZE]
    side_info: Dict[str, object] = dataclasses.field(default_factory=dict)

    def __len__(self):
        return self.batch_size

    def to(self, device) -> "SpeechRecognitionDataBatch":
        return SpeechRecognitionDataBatch(self.batch_size, self.keys, self.network_input.to(device), self.input_lengths,
                                          self.ground_truth.to(device), self.ground_truth_strings,
                                          self.ground_truth_sequence_length, self.side_info)


def _pad_right(rows: List[torch.Tensor]) -> torch.Tensor:
    """ref: src/data/collating.py ``collate_append_constant`` for 1-D rows: zeros appended up to the longest."""
    if not rows:
        raise ValueError("expected non-empty list")
    width = max(int(r.shape[0]) for r in rows)
    out = torch.zeros(len(rows), width, dtype=rows[0].dtype)
    for i, r in enumerate(rows):
        out[i, :r.shape[0]] = r
    return out


def speech_collate_fn(lst: List[SpeechRecognitionDataSample]) -> SpeechRecognitionDataBatch:
    """ref: training_batch_speech.py:105-137 (``default_collate_fn``), without its squeeze of a batch of one: the batch
    dimension stays."""
    wav = _pad_right([s.network_input.reshape(-1) for s in lst])
    gt = _pad_right([s.ground_truth.reshape(-1) for s in lst])
    lengths = torch.tensor([int(s.ground_truth_sequence_length) for s in lst], dtype=torch.int64)
    return SpeechRecognitionDataBatch(
        batch_size=len(lst), keys=[s.key for s in lst], network_input=wav,
        input_lengths=[int(s.input_length) for s in lst], ground_truth=gt,
        ground_truth_strings=[s.ground_truth_string for s in lst], ground_truth_sequence_length=lengths,
        side_info={s.key: s.side_info for s in lst})
