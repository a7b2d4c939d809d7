"""ref: src/tokenizer/base.py -- the tokenizer API of the speech modules."""
from abc import abstractmethod
from typing import Dict

import torch


class BaseTokenizer:
    @abstractmethod
    def encode_string(self, string: str) -> torch.Tensor:
        pass

    @abstractmethod
    def decode_tensor(self, token_tensor: torch.Tensor):
        pass

    @abstractmethod
    def vocabulary_dictionary(self) -> Dict[str, int]:
        pass

    @abstractmethod
    def vocabulary_size(self) -> int:
        pass

    @abstractmethod
    def special_tokens_dictionary(self) -> Dict[str, int]:
        pass

    @abstractmethod
    def blank_token_id(self) -> int:
        pass
