"""The denoiser that ends inference in the WaveGlow / SqueezeWave family: take the vocoder's own bias spectrum off the STFT
magnitudes of generated audio and resynthesise with the original phase.  The bias spectrum is the magnitude spectrum of what
the vocoder emits for an all-zero mel with an all-zero latent; subtracting a little of it removes the constant hum of a flow
vocoder.

One utterance x of n samples, w the periodic Hann of n_fft, X = stft(x, center=True, pad_mode="reflect"):

    g[k][t] = max(|X[k][t]| - strength * bias[k], 0) / |X[k][t]|        (0 where |X| = 0)
    y       = istft(g * X, center=True, length=n)

A ragged batch is one launch of ``rtts_denoise`` (csrc/denoise.hip) on packed audio: the layout ``SqueezeWave.infer_ragged`` /
``capture_ragged`` return and ``dataset.audio`` reads."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from .. import _lib, ops
from ..dataset.audio import MEL_MAX_SEGMENTS, _GpuOnly, _OffsetTables, _host_array, _offsets, _utterances, dft_basis, idft_basis

DENOISE_N_FFT, DENOISE_HOP = 1024, 256        # the one shape of rtts_denoise


def first_frame_magnitudes(audio: torch.Tensor, n_fft: int = DENOISE_N_FFT, win_length: int = DENOISE_N_FFT) -> torch.Tensor:
    """|X[k][0]|, k = 0 .. n_fft/2, of a 1-D waveform in float64: the reflect-padded first frame times the float64
    ``dft_basis`` (a matrix-vector product on the host; made once per denoiser)."""
    x = audio.detach().reshape(-1).to("cpu", torch.float64)
    half = n_fft // 2
    if x.numel() <= half:
        raise ValueError(f"the bias audio has {x.numel()} samples; reflect padding needs more than n_fft / 2 = {half}")
    frame = torch.cat([x[1:half + 1].flip(0), x[:half]])           # xpad[0 .. n_fft): x[n_fft/2] .. x[1], x[0] .. x[n_fft/2 - 1]
    cols = frame @ dft_basis(n_fft, win_length, dtype=torch.float64)
    mag = torch.empty(half + 1, dtype=torch.float64)
    mag[1:half] = torch.sqrt(cols[1:half] ** 2 + cols[half + 1:] ** 2)
    mag[0], mag[half] = cols[0].abs(), cols[half].abs()            # the two real bins share the column pair
    return mag


class DenoiseTables(_OffsetTables):
    """Offset tables of one ragged call: utterance lengths -> sample offsets, as a host array and a device tensor, and the plan
    of the call: maximal runs of consecutive utterances longer than n_fft / 2 (one launch each: ``runs`` of (first, count)) and
    the sample ranges of the shorter ones between them (``copies``), which pass through.  Build it once to replay a captured
    call on new audio of the same lengths."""

    def __init__(self, lengths: Sequence[int], n_fft: int, device):
        self.lengths = [int(n) for n in lengths]
        if not 1 <= len(self.lengths) <= MEL_MAX_SEGMENTS or min(self.lengths) < 0:
            raise ValueError(f"a denoiser call takes 1..{MEL_MAX_SEGMENTS} utterances of non-negative lengths (got {self.lengths})")
        self.sample_offsets = _offsets(self.lengths)
        self.runs: List[Tuple[int, int]] = []
        self.copies: List[Tuple[int, int]] = []
        i, b = 0, len(self.lengths)
        while i < b:
            long = self.lengths[i] > n_fft // 2
            j = i
            while j < b and (self.lengths[j] > n_fft // 2) == long:
                j += 1
            if long:
                self.runs.append((i, j - i))
            elif self.sample_offsets[j] > self.sample_offsets[i]:
                self.copies.append((self.sample_offsets[i], self.sample_offsets[j]))
            i = j
        # a run's host table is its own array: the entry point reads count + 1 values from its start
        self.soff_host = [_host_array(self.sample_offsets[first:first + cnt + 1]) for first, cnt in self.runs]
        self._upload(device, self.sample_offsets)


class Denoiser(_GpuOnly, nn.Module):
    """``Denoiser(vocoder)``: the bias spectrum of ``vocoder`` -- frame 0 of the STFT magnitudes of what it emits for a zero mel of
    ``n_bias_frames`` frames at ``sigma = 0`` -- as the f32 buffer ``bias_spec`` (n_fft/2 + 1,), computed once in float64.  The
    reference's ``infer`` scales every latent draw by sigma except the first (``modules.py:340-368``), so the zero latent that
    ``sigma = 0`` stands for in this family is passed explicitly: every draw is zero and the bias audio is deterministic
    (``Denoiser.bias_audio``).  ``Denoiser(bias_spec=...)`` takes a spectrum as given (tests, saved denoisers).

    Supported: n_fft = win_length = 1024, hop_length = 256 (the one shape of ``rtts_denoise``)."""

    _anchor = "bias_spec"

    def __init__(self, vocoder=None, *, bias_spec: Optional[torch.Tensor] = None, n_fft: int = 1024, hop_length: int = 256,
                 win_length: int = 1024, n_bias_frames: int = 88):
        super().__init__()
        if n_fft != DENOISE_N_FFT or hop_length != DENOISE_HOP or win_length != n_fft:
            raise ValueError(f"supported: n_fft = win_length = {DENOISE_N_FFT}, hop_length = {DENOISE_HOP} "
                             f"(got n_fft={n_fft}, win_length={win_length}, hop_length={hop_length})")
        if (vocoder is None) == (bias_spec is None):
            raise ValueError("Denoiser takes a vocoder or a bias_spec, not both and not neither")
        self.n_fft, self.hop_length, self.win_length, self.n_bias_frames = n_fft, hop_length, win_length, int(n_bias_frames)
        if vocoder is not None:
            bias_spec = first_frame_magnitudes(self.bias_audio(vocoder, self.n_bias_frames), n_fft, win_length)
        bias = torch.as_tensor(bias_spec).detach().reshape(-1)
        if bias.numel() != n_fft // 2 + 1:
            raise ValueError(f"bias_spec must hold n_fft / 2 + 1 = {n_fft // 2 + 1} magnitudes (got {bias.numel()})")
        device = bias.device if vocoder is None else vocoder._device("infer")
        self.register_buffer("bias_spec", bias.to(device, torch.float32).contiguous())
        self.register_buffer("dft_basis", dft_basis(n_fft, win_length).to(device), persistent=False)
        self.register_buffer("idft_basis", idft_basis(n_fft, win_length).to(device), persistent=False)

    @staticmethod
    @torch.no_grad()
    def bias_audio(vocoder, n_bias_frames: int = 88) -> torch.Tensor:
        """What ``vocoder`` emits for a zero mel of ``n_bias_frames`` frames with a zero latent -> (256 * n_bias_frames,) f32."""
        dev = vocoder._device("infer")
        mel = torch.zeros(1, vocoder._n_mel(), int(n_bias_frames), device=dev)
        noise = [torch.zeros(s, device=dev) for s in vocoder.noise_shapes(1, int(n_bias_frames))]
        return vocoder.infer(mel, sigma=0.0, noise=noise).reshape(-1)

    def tables(self, lengths: Sequence[int]) -> DenoiseTables:
        return DenoiseTables(lengths, self.n_fft, self._device("tables"))

    @torch.no_grad()
    def forward_packed(self, audio: torch.Tensor, lengths: Optional[Sequence[int]] = None, *, tables: Optional[DenoiseTables] = None,
                       strength: float = 0.1, out: Optional[torch.Tensor] = None):
        """``audio``: the utterances end to end, a flat f32 device tensor; ``lengths``: their sample counts (host ints), or
        ``tables`` from an earlier ``self.tables(lengths)`` -> (the denoised utterances over the same offsets, flat f32; the sample
        offsets).  ``out`` must not overlap ``audio``.  One launch per run of consecutive utterances longer than n_fft / 2 -- one
        launch when all are -- stream-ordered.  Utterances of at most n_fft / 2 samples cannot be reflect-padded
        (``torch.stft`` refuses them too): they are COPIED THROUGH UNCHANGED; a batch of only such utterances launches nothing."""
        dev = self._device("forward_packed")
        if tables is None:
            if lengths is None:
                raise ValueError("forward_packed needs lengths or tables")
            tables = self.tables(lengths)
        if not (torch.is_tensor(audio) and audio.is_cuda and audio.device == dev):
            where = audio.device if torch.is_tensor(audio) else type(audio).__name__
            raise _lib.RttsError(f"{type(self).__name__}.forward_packed runs on the GPU only: audio is on {where}, the bias on {dev}")
        total = tables.sample_offsets[-1]
        if audio.dim() != 1 or audio.dtype != torch.float32 or audio.numel() < total:
            raise ValueError(f"forward_packed: audio must be flat f32 of at least {total} samples (got {audio.dtype} {tuple(audio.shape)})")
        if out is None:
            out = torch.empty(total, dtype=torch.float32, device=dev)
        elif not (out.is_cuda and out.device == dev and out.dim() == 1 and out.dtype == torch.float32 and out.numel() >= total):
            raise ValueError(f"forward_packed: out must be flat f32 of at least {total} samples on {dev}")
        for (first, cnt), host in zip(tables.runs, tables.soff_host):
            ops.denoise(audio, host, tables.device_table[first:first + cnt + 1], cnt, self.dft_basis, self.idft_basis, self.bias_spec,
                        strength, self.n_fft, self.hop_length, out)
        for a, b in tables.copies:
            out[a:b].copy_(audio[a:b])
        return out, list(tables.sample_offsets)

    @torch.no_grad()
    def forward(self, audio, lengths=None, strength: float = 0.1):
        """``audio``: a list of 1-D device tensors -> the list of denoised utterances; or a padded (B, N) device tensor with
        ``lengths`` (host ints or a tensor) -> (B, N) f32, utterance i in [i, :lengths[i]] and zero behind it.  Utterances of at
        most n_fft / 2 samples come back unchanged (see ``forward_packed``); empty ones stay empty."""
        dev = self._device("forward")
        parts, lens = _utterances(audio, lengths, type(self).__name__)
        flat = torch.cat([p.to(dev, torch.float32) for p in parts])
        packed, off = self.forward_packed(flat, lens, strength=strength)
        waves = [packed[off[i]:off[i + 1]] for i in range(len(lens))]
        if not torch.is_tensor(audio):
            return waves
        res = torch.zeros(audio.shape, dtype=torch.float32, device=dev)
        for i, wv in enumerate(waves):
            res[i, :lens[i]] = wv
        return res
