"""Vocoder training: the optimisation loop of the reference's ``LitSqueezeWave`` (``training/wrappers.py:327-418``) without
the Lightning plumbing.

``training_step`` is ``SqueezeWave.nll_backward`` (forward with batch-statistics BatchNorm, ``SqueezeWaveLoss``, backward: the
HIP path of ``squeeze_wave/modules.py``) between ``zero_grad`` and ``step`` of ``torch.optim.Adam(model.parameters(),
learning_rate)`` -- exactly ``configure_optimizers`` (:414-418).  The optimiser is plumbing and stays PyTorch."""
from __future__ import annotations

from typing import Dict, Iterable, Tuple

import torch

from .. import _lib
from .._graphs import warm_capture
from . import loss as _loss
from .modules import SqueezeWave


class VocoderTrainer:
    def __init__(self, model: SqueezeWave, learning_rate: float = 4e-4, loss_sigma: float = 1.0, logdet: str = "host"):
        """``logdet``: where a step factors the invertible 1x1 convolutions (``SqueezeWave.nll_backward``).  ``"host"``: float64
        LAPACK with a device -> host copy per step.  ``"device"``: ``rtts_sw_inv1x1_factor``, and Adam with ``capturable=True``
        (its step count lives on the device) -- a step then touches the host nowhere and ``capture`` can record it."""
        if logdet not in ("host", "device"):
            raise ValueError(f"logdet must be 'host' or 'device' (got {logdet!r})")
        self.model, self.loss_sigma, self.logdet = model, float(loss_sigma), logdet
        self.optimizer = torch.optim.Adam(model.parameters(), learning_rate, **({"capturable": True} if logdet == "device" else {}))

    def training_step(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """``batch['spectrogram']`` (B, n_mel, Lm) and ``batch['audio']`` (B, 256 * Lm) on the model's device, as the
        reference's batches carry them (``wrappers.py:350-359``) -> the loss of this step (0-dim fp32 on the device)."""
        self.model.train()
        self.optimizer.zero_grad()
        loss = self.model.nll_backward(batch["spectrogram"], batch["audio"], sigma=self.loss_sigma, logdet=self.logdet)
        self.optimizer.step()
        return loss

    def check_determinants(self) -> None:
        """``SqueezeWave.check_determinants``: a device-mode step raises nothing for a determinant that is not positive (its loss
        is NaN or inf); this reads the signs back and raises by flow."""
        self.model.check_determinants()

    def capture(self, batch: int, mel_len: int):
        """-> ``run(batch_dict) -> loss``: the whole ``training_step`` for one (batch, mel_len) shape -- zeroing the gradients,
        re-fold with the device factorisation, forward, loss, backward, Adam -- as ONE hipGraph, replayed without host work.
        Needs ``logdet="device"`` and a model on the GPU in ``.train()``.  ``run`` copies ``batch['spectrogram']`` (B, n_mel, Lm)
        and ``batch['audio']`` (B, 256 * Lm) into the graph's input buffers (other shapes are refused by name, before anything
        is touched), replays, and returns the graph's 0-dim fp32 loss buffer: copy it before the next call.  Capturing does not
        advance training: the warm-up step ``warm_capture`` makes is undone (parameters, buffers, gradients, Adam state).  A
        replay changes the parameters in place without raising their version counters, so ``run`` drops the model's cached
        inference fold itself.  The graph writes the ``.grad`` tensors that exist when it is recorded: do not mix ``run`` with the
        eager ``training_step`` on one trainer -- its ``zero_grad()`` sets the gradients to None, after which ``p.grad`` no longer
        shows what a replay computed (the replays themselves stay consistent)."""
        model = self.model
        dev = model._device("VocoderTrainer.capture")
        if self.logdet != "device":
            raise _lib.RttsError("VocoderTrainer.capture needs logdet='device': with logdet='host' every step copies the 1x1 weights "
                                 "to the host and waits for them, which no graph can replay")
        if not model.training:
            raise _lib.RttsError("VocoderTrainer.capture needs training mode (call .train()): the graph keeps the mode it was captured in")
        batch, mel_len = int(batch), int(mel_len)
        if batch < 1 or mel_len < 1:
            raise ValueError(f"VocoderTrainer.capture: batch and mel_len must be positive (got {batch}, {mel_len})")
        spectrogram = torch.zeros(batch, model._n_mel(), mel_len, device=dev)
        audio = torch.zeros(batch, model.samples_per_frame() * mel_len, device=dev)
        params = list(model.parameters())
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        opt = self.optimizer

        def step():
            opt.zero_grad(set_to_none=False)
            loss = model.nll_backward(spectrogram, audio, sigma=self.loss_sigma, logdet="device")
            opt.step()
            return loss

        # the warm-up is a real step: everything it changes in place is put back once the graph is recorded
        kept = [t for p in params for t in (p.data, p.grad)] + list(model.buffers())
        saved = [t.clone() for t in kept]
        had = {id(p): {k: v.clone() for k, v in opt.state[p].items() if torch.is_tensor(v)} for p in params if p in opt.state and opt.state[p]}
        graph, loss = warm_capture(step)
        with torch.no_grad():
            for t, s in zip(kept, saved):
                t.copy_(s)
            for p in params:
                for k, v in opt.state[p].items():
                    if torch.is_tensor(v):
                        v.copy_(had[id(p)][k]) if id(p) in had else v.zero_()
        model._folded, model._folded_key = None, None

        def run(b: Dict[str, torch.Tensor]) -> torch.Tensor:
            for name, buf in (("spectrogram", spectrogram), ("audio", audio)):
                t = b[name]
                if not torch.is_tensor(t) or tuple(t.shape) != tuple(buf.shape):
                    raise ValueError(f"VocoderTrainer.capture graph for {name} {tuple(buf.shape)}: got {tuple(getattr(t, 'shape', ()))}")
                model._on_device(t, dev, "VocoderTrainer.capture", name)
            if not model.training:
                raise _lib.RttsError("VocoderTrainer.capture: the graph was captured in training mode; call .train()")
            spectrogram.copy_(b["spectrogram"], non_blocking=True)
            audio.copy_(b["audio"], non_blocking=True)
            graph.replay()
            model._folded, model._folded_key = None, None      # the parameters changed in place, their _version did not
            return loss
        run.graph, run.batch, run.mel_len = graph, batch, mel_len
        return run

    def validation_loss(self, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]]) -> torch.Tensor:
        """``val_loss`` (``wrappers.py:361-368``) in eval mode (running-statistics BatchNorm); the model's mode is restored."""
        was_training = self.model.training
        self.model.eval()
        try:
            return _loss.validation_loss(self.model, batches, sigma=self.loss_sigma)
        finally:
            self.model.train(was_training)
