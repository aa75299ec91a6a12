"""Griffin-Lim vocoding: log-mel spectrograms -> audio without a trained vocoder, for a ragged batch on the GPU.

What NVIDIA tacotron2's ``audio_processing.griffin_lim``, librosa's ``mel_to_audio`` and torchaudio's ``InverseMelScale`` +
``GriffinLim`` are for: listening to a spectrogram model before any vocoder has been trained, and a vocoder-independent number for
``synthesis.mel_round_trip_error``.  One utterance of L mel frames gives 256 L samples (the vocoder's contract); w is the periodic
Hann of n_fft, STFT / iSTFT are ``torch.stft(center=True, pad_mode="reflect")`` / ``torch.istft(center=True, length=n)``:

    M[k][t] = max(0, sum_m P[k][m] exp(mel[m][t]))^(1/power),  P = pinv(mel_basis);  column L repeats column L - 1
    x_0     = iSTFT(M e^{i phi})                                phi from the counter hash of the seed, or zero
    x_{k+1} = iSTFT(M R / |R|),  R = STFT(x_k - beta x_{k-1})   beta = momentum / (1 + momentum), k = 0 .. n_iter - 1

``momentum = 0`` is tacotron2's loop, ``momentum = 0.99`` librosa's and torchaudio's default (fast Griffin-Lim; by linearity the
momentum goes through the signal, so no spectrogram is kept between the iterations).  A call is ``1 + 1 + n_iter`` launches
(``rtts_gl_magnitudes``, ``rtts_gl_init``, ``rtts_gl_step`` of csrc/griffin_lim.hip) on three rotating audio buffers, with no host
synchronisation and no allocation between them: it can be captured into a hipGraph and replayed on a new mel of the same lengths.
Utterances of fewer than three frames cannot be reflect-padded: their samples are zeros."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib, ops
from .dataset.audio import MEL_MAX_SEGMENTS, _GpuOnly, _OffsetTables, _offsets, dft_basis, idft_basis
from .squeeze_wave.modules import host_lengths, segment_offsets

GL_N_FFT, GL_HOP = 1024, 256          # the one shape of rtts_gl_init / rtts_gl_step


def mel_pseudo_inverse(mel_basis: torch.Tensor) -> torch.Tensor:
    """(n_mels, bins) mel matrix -> its pseudo-inverse (bins, n_mels), computed in float64 on the host and rounded once to f32."""
    return torch.linalg.pinv(mel_basis.detach().to("cpu", torch.float64)).to(torch.float32).contiguous()


class GriffinLimTables(_OffsetTables):
    """Offset tables of one ragged call: mel frame counts L_i -> sample offsets (256 L_i samples each), the column offsets of the
    magnitudes (L_i + 1 columns each: the frame offsets ``MelTables`` gives for lengths 256 L_i) and the first frames of a packed
    (n_mels, sum L) mel, as host arrays and as one device tensor.  Build it once to replay a captured call on a new mel of the same
    lengths."""

    def __init__(self, frames: Sequence[int], device, hop_length: int = GL_HOP):
        self.frames = [int(n) for n in frames]
        if not 1 <= len(self.frames) <= MEL_MAX_SEGMENTS or min(self.frames) < 0:
            raise ValueError(f"a Griffin-Lim call takes 1..{MEL_MAX_SEGMENTS} utterances of non-negative frame counts (got {self.frames})")
        self.lengths = [hop_length * n for n in self.frames]
        self.sample_offsets = _offsets(self.lengths)
        self.col_offsets = _offsets([n + 1 for n in self.frames])
        self.mel_offsets = _offsets(self.frames)
        self._upload(device, [self.sample_offsets, self.col_offsets, self.mel_offsets, [0] * len(self.col_offsets)],
                     soff_host=self.sample_offsets, coff_host=self.col_offsets)


class GriffinLim(_GpuOnly, nn.Module):
    """``GriffinLim(creator)``: ``creator`` is the ``dataset.audio`` spectrogram module whose log-mels are to be inverted
    (``Tacotron2Spectrogram``: magnitude mels, power 1; ``MelSpectrogram``: power mels, power 2); it gives the mel matrix, the power,
    n_fft and the hop.  The object goes where a vocoder goes: ``synthesis.vocode_trimmed(gl, spectrogram, stop)``,
    ``synthesis.synthesize(tts, gl, phonemes)``.

    Supported: n_fft = win_length = 1024, hop_length = 256 (the one shape of the kernels)."""

    _anchor = "pinv"

    def __init__(self, creator, n_iter: int = 32, momentum: float = 0.99, phase: str = "hash", seed: int = 0):
        super().__init__()
        shape = tuple(getattr(creator, k, None) for k in ("n_fft", "win_length", "hop_length"))
        if shape != (GL_N_FFT, GL_N_FFT, GL_HOP):
            raise ValueError(f"creator: supported are n_fft = win_length = {GL_N_FFT}, hop_length = {GL_HOP} "
                             f"(got n_fft={shape[0]}, win_length={shape[1]}, hop_length={shape[2]})")
        if int(creator.power) not in (1, 2):
            raise ValueError(f"creator: power must be 1 or 2 (got {creator.power})")
        if int(n_iter) < 0:
            raise ValueError(f"n_iter must not be negative (got {n_iter})")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"momentum must be in [0, 1) (got {momentum})")
        if phase not in ("hash", "zero"):
            raise ValueError(f"phase must be 'hash' or 'zero' (got {phase!r})")
        self.n_fft, self.hop_length, self.n_mels, self.power = GL_N_FFT, GL_HOP, int(creator.n_mels), int(creator.power)
        self.n_iter, self.momentum, self.phase, self.seed = int(n_iter), float(momentum), phase, int(seed) & 0xFFFFFFFF
        device = creator.mel_basis.device
        self.register_buffer("pinv", mel_pseudo_inverse(creator.mel_basis).to(device), persistent=False)
        self.register_buffer("dft_basis", dft_basis(GL_N_FFT, GL_N_FFT).to(device), persistent=False)
        self.register_buffer("idft_basis", idft_basis(GL_N_FFT, GL_N_FFT).to(device), persistent=False)

    def tables(self, frames: Sequence[int]) -> GriffinLimTables:
        return GriffinLimTables(frames, self._device("tables"), self.hop_length)

    @torch.no_grad()
    def forward_packed(self, mel: torch.Tensor, frames=None, *, tables: Optional[GriffinLimTables] = None) -> Tuple[torch.Tensor, List[int]]:
        """``mel``: log-mel on the device, (B, n_mels, >= max frames) of any strides, or packed (n_mels, sum frames) as a creator's
        ``forward_packed`` returns it; ``frames``: the B frame counts (host ints), or ``tables`` from an earlier
        ``self.tables(frames)`` -> (the utterances end to end, flat f32 of 256 sum(frames) samples; the sample offsets).  The
        buffers are allocated up front; then 2 + n_iter launches, stream-ordered."""
        dev = self._device("forward_packed")
        if tables is None:
            if frames is None:
                raise ValueError("forward_packed needs frames or tables")
            tables = self.tables(host_lengths(frames))
        if not (torch.is_tensor(mel) and mel.is_cuda and mel.device == dev):
            where = mel.device if torch.is_tensor(mel) else type(mel).__name__
            raise _lib.RttsError(f"{type(self).__name__}.forward_packed runs on the GPU only: mel is on {where}, the bases on {dev}")
        if mel.dtype != torch.float32:
            mel = mel.float()
        nseg, total = len(tables.frames), tables.sample_offsets[-1]
        if total == 0:
            return torch.empty(0, dtype=torch.float32, device=dev), list(tables.sample_offsets)
        packed = mel.dim() == 2
        mel_start_host = tables.mel_offsets if packed else [0] * nseg
        offsets = tables.device_table[:2]
        mag = torch.empty(self.n_fft // 2 + 1, tables.col_offsets[-1], dtype=torch.float32, device=dev)
        audio = torch.empty(3, total, dtype=torch.float32, device=dev)
        ops.gl_magnitudes(mel, mel_start_host, tables.device_table[2 if packed else 3], tables.coff_host, offsets, nseg, self.pinv,
                          self.power, self.n_fft, mag)
        ops.gl_init(mag, tables.coff_host, tables.soff_host, offsets, nseg, self.dft_basis, self.idft_basis, self.phase, self.seed,
                    self.n_fft, self.hop_length, audio[0])
        beta = self.momentum / (1.0 + self.momentum)
        for k in range(self.n_iter):                               # x_k in audio[k % 3], x_{k-1} in audio[(k - 1) % 3]
            prev = audio[(k - 1) % 3] if k > 0 and beta > 0.0 else None
            ops.gl_step(audio[k % 3], prev, beta, mag, tables.coff_host, tables.soff_host, offsets, nseg, self.dft_basis, self.idft_basis,
                        self.n_fft, self.hop_length, audio[(k + 1) % 3])
        return audio[self.n_iter % 3], list(tables.sample_offsets)

    @torch.no_grad()
    def forward(self, mel: torch.Tensor, frames) -> List[torch.Tensor]:
        """-> the list of B waveforms, 256 frames_i f32 samples each, on the device."""
        packed, off = self.forward_packed(mel, frames)
        return [packed[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    @staticmethod
    def split_packed(audio: torch.Tensor, moff_host: List[int]) -> List[torch.Tensor]:
        """Packed audio -> the per-utterance views (256 samples per mel frame) of the FRAME offsets ``moff_host``, as the vocoder's."""
        flat = audio.view(-1)
        return [flat[GL_HOP * moff_host[i]:GL_HOP * moff_host[i + 1]] for i in range(len(moff_host) - 1)]

    @torch.no_grad()
    def infer_ragged(self, spectrogram: torch.Tensor, frames, sigma=None, noise=None):
        """The vocoder's ragged call: spectrogram (B, n_mels, Lmax), ``frames`` (B,) host ints -> (packed audio, the B views of
        256 frames_i samples).  Griffin-Lim draws nothing: ``sigma`` is ignored and ``noise`` must be None."""
        if noise is not None:
            raise ValueError("noise: Griffin-Lim draws no latent (its start phases come from seed); pass noise=None")
        dev = self._device("infer_ragged")
        lens = host_lengths(frames)
        packed, _ = self.forward_packed(spectrogram.to(dev), lens)
        return packed, self.split_packed(packed, segment_offsets(lens))
