from .wav2vec2_fc_letter import Wav2vec2FcLetterRecognizer, Wav2vec2FcLetterRecognizerConfig  # noqa: F401
