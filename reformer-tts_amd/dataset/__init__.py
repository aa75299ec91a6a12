from .utils import BatchPrefetcher, custom_sequence_padder  # noqa: F401
from .corpus import TTSCorpus, batch_plan, variable_batch_plan  # noqa: F401
