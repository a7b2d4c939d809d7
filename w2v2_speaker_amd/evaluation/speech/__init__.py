from .wer import calculate_wer  # noqa: F401
