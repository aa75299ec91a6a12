from .trainer import Trainer, build_model, synthetic_batch, trim_attention_matrices  # noqa: F401
