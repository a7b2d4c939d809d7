"""Tokenizers of the speech recognition path (ref: src/tokenizer/)."""
from .base import BaseTokenizer  # noqa: F401
from .tokenizer_wav2vec2 import LETTER_VOCAB_PATH, Wav2vec2Tokenizer, Wav2vec2TokenizerConfig  # noqa: F401
