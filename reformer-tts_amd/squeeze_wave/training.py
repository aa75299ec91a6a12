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
        dev = self._capture_device("capture")
        batch, mel_len = int(batch), int(mel_len)
        if batch < 1 or mel_len < 1:
            raise ValueError(f"VocoderTrainer.capture: batch and mel_len must be positive (got {batch}, {mel_len})")
        spectrogram = torch.zeros(batch, model._n_mel(), mel_len, device=dev)
        audio = torch.zeros(batch, model.samples_per_frame() * mel_len, device=dev)
        graph, loss = self._capture_step(lambda: model.nll_backward(spectrogram, audio, sigma=self.loss_sigma, logdet="device"))

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

    def _capture_device(self, what: str) -> torch.device:
        model = self.model
        dev = model._device(f"VocoderTrainer.{what}")
        if self.logdet != "device":
            raise _lib.RttsError(f"VocoderTrainer.{what} needs logdet='device': with logdet='host' every step copies the 1x1 weights "
                                 "to the host and waits for them, which no graph can replay")
        if not model.training:
            raise _lib.RttsError(f"VocoderTrainer.{what} needs training mode (call .train()): the graph keeps the mode it was captured in")
        return dev

    def _capture_step(self, forward_backward, also_kept=()):
        """zero_grad + ``forward_backward()`` (-> the loss) + Adam, warmed up and recorded as one graph -> (graph, its loss buffer).
        The warm-up is a real step: everything it changes in place -- parameters, gradients, buffers, Adam state, and the tensors
        of ``also_kept`` -- is put back once the graph is recorded, and the model's cached fold is dropped."""
        model, opt = self.model, self.optimizer
        params = list(model.parameters())
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)

        def step():
            opt.zero_grad(set_to_none=False)
            loss = forward_backward()
            opt.step()
            return loss

        kept = [t for p in params for t in (p.data, p.grad)] + list(model.buffers()) + list(also_kept)
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
        return graph, loss

    def capture_corpus(self, sampler):
        """-> ``run() -> loss``: ``capture`` with the batch drawn inside the graph.  The graph holds ``sampler.draw()`` -- the
        ``rtts_sw_draw_segments`` launch that writes the rows of a fresh batch from the device-resident corpus, and the add that
        advances the cursor -- followed by the whole step on those rows (``SqueezeWave.nll_backward_rows``), so a replay takes
        nothing from the host: no batch to assemble, no copy, no permute.  ``run.picks`` is the sampler's int32 (B, 2) buffer of
        the {utterance, hop} the last replay used (copy it before the next one); ``sampler.start_epoch`` between replays
        reshuffles without a recapture.  Everything ``capture`` says about the warm-up being undone, the fold cache and the
        gradients holds here; the warm-up's draw is undone too (the cursor is restored)."""
        from .corpus import SegmentSampler
        model = self.model
        dev = self._capture_device("capture_corpus")
        if not isinstance(sampler, SegmentSampler):
            raise TypeError(f"VocoderTrainer.capture_corpus takes a SegmentSampler (got {type(sampler).__name__})")
        if sampler.corpus.device != dev:
            raise _lib.RttsError(f"VocoderTrainer.capture_corpus runs on the GPU only: the corpus is on {sampler.corpus.device}, the model on {dev}")
        if (sampler.corpus.hop != model.samples_per_frame() or sampler.n_audio_channels != model.n_audio_channels
                or sampler.corpus.n_mel != model._n_mel()):
            raise ValueError(f"VocoderTrainer.capture_corpus: the sampler draws hop {sampler.corpus.hop}, {sampler.n_audio_channels} audio "
                             f"channels, {sampler.corpus.n_mel} mel channels; the model takes {model.samples_per_frame()}, "
                             f"{model.n_audio_channels}, {model._n_mel()}")
        batch, mel_len = sampler.batch, sampler.mel_len

        def forward_backward():
            mel_rows, audio_rows, _ = sampler.draw()
            return model.nll_backward_rows(mel_rows, audio_rows, batch, mel_len, sigma=self.loss_sigma, logdet="device")

        graph, loss = self._capture_step(forward_backward, also_kept=(sampler.state,))

        def run() -> torch.Tensor:
            if not model.training:
                raise _lib.RttsError("VocoderTrainer.capture_corpus: the graph was captured in training mode; call .train()")
            graph.replay()
            model._folded, model._folded_key = None, None      # the parameters changed in place, their _version did not
            return loss
        run.graph, run.batch, run.mel_len, run.picks, run.sampler = graph, batch, mel_len, sampler.picks, sampler
        return run

    def fit_corpus(self, sampler, epochs: int, log_every: int = 0, run=None):
        """``epochs`` epochs of ``sampler.steps_per_epoch`` replays of ``capture_corpus(sampler)`` (``run``: an earlier capture of
        this sampler to reuse), ``sampler.start_epoch(e)`` in front of each, continuing after the sampler's last epoch -> the
        loss of every step as host floats (read back once per epoch; ``log_every`` > 0 prints every that many steps)."""
        if run is None:
            run = self.capture_corpus(sampler)
        elif getattr(run, "sampler", None) is not sampler:
            raise ValueError("VocoderTrainer.fit_corpus: run was not captured from this sampler")
        first = 0 if sampler.epoch is None else sampler.epoch + 1
        losses = []
        for e in range(first, first + int(epochs)):
            sampler.start_epoch(e)
            kept = []
            for _ in range(sampler.steps_per_epoch):
                kept.append(run().clone())
            vals = torch.stack(kept).tolist() if kept else []
            for k, v in enumerate(vals):
                if log_every and (len(losses) + k + 1) % log_every == 0:
                    print(f"epoch {e} step {len(losses) + k + 1}: loss {v:.6f}", flush=True)
            losses += vals
        return losses

    def validation_loss(self, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]]) -> torch.Tensor:
        """``val_loss`` (``wrappers.py:361-368``) in eval mode (running-statistics BatchNorm); the model's mode is restored."""
        was_training = self.model.training
        self.model.eval()
        try:
            return _loss.validation_loss(self.model, batches, sigma=self.loss_sigma)
        finally:
            self.model.train(was_training)
