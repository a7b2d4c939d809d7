"""ref: src/tokenizer/tokenizer_wav2vec2.py -- the letter tokenizer of wav2vec2's CTC head.  The reference wraps
``transformers.Wav2Vec2CTCTokenizer.from_pretrained("facebook/wav2vec2-base-960h")``; here the vocabulary is a file (or a
dict) and the two operations the speech module needs are restated: a transcript becomes one id per character with ``|``
for the space and ``<unk>`` for anything outside the vocabulary, and a sequence of per-frame argmaxes becomes a string the
way ``Wav2Vec2CTCTokenizer.decode`` makes it -- runs of equal tokens grouped, ``<pad>`` (the CTC blank) dropped, ``|`` turned
into a space, joined and stripped.  ``decode_ids`` takes what the device decoder (``ops.ctc_greedy_decode``) has already
collapsed and freed of blanks.  ``letter_vocab.json`` is the 32-entry vocabulary of that checkpoint written from memory:
it could not be compared with the hub's file."""
import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import torch

from .base import BaseTokenizer

LETTER_VOCAB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "letter_vocab.json")


@dataclass
class Wav2vec2TokenizerConfig:
    tokenizer_huggingface_id: str = "facebook/wav2vec2-base-960h"
    vocab: Optional[Union[str, Dict[str, int]]] = None        # a vocab.json path or a dict; None = the packaged letters


class Wav2vec2Tokenizer(BaseTokenizer):
    PAD, BOS, EOS, UNK, WORD_DELIMITER = "<pad>", "<s>", "</s>", "<unk>", "|"

    def __init__(self, cfg: Optional[Wav2vec2TokenizerConfig] = None, vocab: Optional[Union[str, Dict[str, int]]] = None):
        vocab = vocab if vocab is not None else (cfg.vocab if cfg is not None else None)
        if vocab is None:
            vocab = LETTER_VOCAB_PATH
        if isinstance(vocab, (str, os.PathLike)):
            with open(vocab, encoding="utf-8") as f:
                vocab = json.load(f)
        self.vocab: Dict[str, int] = {str(k): int(v) for k, v in vocab.items()}
        if sorted(self.vocab.values()) != list(range(len(self.vocab))):
            raise ValueError("tokenizer: the vocabulary's ids must be 0 .. size - 1, each once")
        for tok in (self.PAD, self.UNK, self.WORD_DELIMITER):
            if tok not in self.vocab:
                raise ValueError(f"tokenizer: the vocabulary has no {tok!r}")
        self.ids: List[str] = [t for t, _ in sorted(self.vocab.items(), key=lambda kv: kv[1])]
        self.pad_id, self.unk_id = self.vocab[self.PAD], self.vocab[self.UNK]

    def encode_string(self, string: str) -> torch.Tensor:
        text = string.replace(" ", self.WORD_DELIMITER)
        return torch.IntTensor([self.vocab.get(ch, self.unk_id) for ch in text])

    def _to_string(self, tokens: Sequence[int], group: bool) -> str:
        chars, prev = [], None
        for i in tokens:
            i = int(i)
            if group and i == prev:
                continue
            prev = i
            if i == self.pad_id:
                continue
            tok = self.ids[i]
            chars.append(" " if tok == self.WORD_DELIMITER else tok)
        return "".join(chars).strip()

    def decode_tensor(self, token_tensor: torch.Tensor) -> str:
        """Per-frame argmaxes [T] -> text: what ``Wav2Vec2CTCTokenizer.decode`` returns."""
        assert len(token_tensor.shape) == 1
        return self._to_string(token_tensor.tolist(), group=True)

    def decode_ids(self, tokens, counts) -> List[str]:
        """The device decoder's output -- tokens [B, T] (the first counts[b] of row b, runs already collapsed and blanks
        already dropped) and counts [B], host tensors or lists -> one string per utterance.  Nothing is grouped again:
        `A A` after a blank stays two letters."""
        tokens = tokens.tolist() if hasattr(tokens, "tolist") else tokens
        counts = counts.tolist() if hasattr(counts, "tolist") else counts
        return [self._to_string(row[:int(n)], group=False) for row, n in zip(tokens, counts)]

    def vocabulary_dictionary(self) -> Dict[str, int]:
        return dict(self.vocab)

    def vocabulary_size(self) -> int:
        return len(self.vocab)

    def special_tokens_dictionary(self) -> Dict[str, str]:
        """HF's ``special_tokens_map`` (token role -> token string), as the reference returns it under its pinned
        ``transformers`` (newer releases add ``word_delimiter_token``)."""
        roles = {"bos_token": self.BOS, "eos_token": self.EOS, "unk_token": self.UNK, "pad_token": self.PAD}
        return {r: t for r, t in roles.items() if t in self.vocab}

    def blank_token_id(self) -> int:
        return 0
