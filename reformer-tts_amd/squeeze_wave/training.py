"""Vocoder training: the optimisation loop of the reference's ``LitSqueezeWave`` (``training/wrappers.py:327-418``) without
the Lightning plumbing.

``training_step`` is ``SqueezeWave.nll_backward`` (forward with batch-statistics BatchNorm, ``SqueezeWaveLoss``, backward: the
HIP path of ``squeeze_wave/modules.py``) between ``zero_grad`` and ``step`` of ``torch.optim.Adam(model.parameters(),
learning_rate)`` -- exactly ``configure_optimizers`` (:414-418).  The optimiser is plumbing and stays PyTorch."""
from __future__ import annotations

from typing import Dict, Iterable, Tuple

import torch

from . import loss as _loss
from .modules import SqueezeWave


class VocoderTrainer:
    def __init__(self, model: SqueezeWave, learning_rate: float = 4e-4, loss_sigma: float = 1.0):
        self.model, self.loss_sigma = model, float(loss_sigma)
        self.optimizer = torch.optim.Adam(model.parameters(), learning_rate)

    def training_step(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """``batch['spectrogram']`` (B, n_mel, Lm) and ``batch['audio']`` (B, 256 * Lm) on the model's device, as the
        reference's batches carry them (``wrappers.py:350-359``) -> the loss of this step (0-dim fp32 on the device)."""
        self.model.train()
        self.optimizer.zero_grad()
        loss = self.model.nll_backward(batch["spectrogram"], batch["audio"], sigma=self.loss_sigma)
        self.optimizer.step()
        return loss

    def validation_loss(self, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]]) -> torch.Tensor:
        """``val_loss`` (``wrappers.py:361-368``) in eval mode (running-statistics BatchNorm); the model's mode is restored."""
        was_training = self.model.training
        self.model.eval()
        try:
            return _loss.validation_loss(self.model, batches, sigma=self.loss_sigma)
        finally:
            self.model.train(was_training)
