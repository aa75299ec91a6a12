from .config import SqueezeWaveConfig, WNConfig  # noqa: F401
from .modules import SqueezeWave  # noqa: F401
from .loss import SqueezeWaveLoss, validation_loss  # noqa: F401
from .training import VocoderTrainer  # noqa: F401
from .corpus import SegmentSampler, VocoderCorpus  # noqa: F401
from .denoiser import Denoiser  # noqa: F401
