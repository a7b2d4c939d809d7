from .xvector import XVectorModule, XVectorModuleConfig  # noqa: F401
from .wav2spk import Wav2SpkModule, Wav2SpkModuleConfig  # noqa: F401
from .wav2vec2_ecapa import Wav2vec2EcapaModule, Wav2vec2EcapaModuleConfig  # noqa: F401
