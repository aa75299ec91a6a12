"""The SqueezeWave likelihood loss (reference ``reformer_tts/squeeze_wave/loss.py:14-31``) and the validation mean
of ``LitSqueezeWave`` (``training/wrappers.py:361-368``).

``SqueezeWaveLoss`` is the reference's arithmetic on the tuple ``SqueezeWave.forward`` returns, in float64 on whatever
device the tuple lives on; ``SqueezeWave.nll`` computes the same number without materialising the ``log_s`` list."""
from __future__ import annotations

from typing import Iterable, Tuple

import torch
from torch import nn


class SqueezeWaveLoss(nn.Module):
    def __init__(self, sigma: float = 1.0):
        super().__init__()
        self.sigma = sigma

    def forward(self, model_output) -> torch.Tensor:
        """(z (B, C, L), log_s_list, log_det_W_list) -> 0-dim fp32:
        [sum z^2 / (2 sigma^2) - sum_k sum log_s_k - sum_k log_det_W_k] / (B * C * L)."""
        z, log_s_list, log_det_w_list = model_output
        if len(log_s_list) != len(log_det_w_list):
            raise ValueError(f"SqueezeWaveLoss: {len(log_s_list)} log_s tensors for {len(log_det_w_list)} log-determinants")
        z = z.double()
        total = torch.sum(z * z) / (2.0 * float(self.sigma) ** 2)
        for log_s, log_det_w in zip(log_s_list, log_det_w_list):
            total = total - torch.sum(log_s.double()) - torch.as_tensor(log_det_w, device=z.device).double()
        return (total / z.numel()).float()


@torch.no_grad()
def validation_loss(model, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], sigma: float = 1.0) -> torch.Tensor:
    """``val_loss`` of the reference's vocoder training (``training/wrappers.py:361-368``): the mean over ``batches`` of
    (mel (B, n_mel, Lm), audio (B, 256 * Lm)) of ``SqueezeWaveLoss(sigma)(model((mel, audio)))``, each computed by
    ``model.nll`` -> 0-dim fp32 on the device.  The number the reference's checkpoints are named by."""
    losses = [model.nll(mel, audio, sigma=sigma) for mel, audio in batches]
    if not losses:
        raise ValueError("validation_loss: no batches")
    return torch.stack(losses).double().mean().float()
