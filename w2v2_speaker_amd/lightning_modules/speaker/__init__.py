from .xvector import XVectorModule, XVectorModuleConfig  # noqa: F401
from .wav2spk import Wav2SpkModule, Wav2SpkModuleConfig  # noqa: F401
