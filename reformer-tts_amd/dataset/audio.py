"""Audio -> log-mel spectrograms on the GPU: the spectrogram creators of the reference's ``dataset/convert.py:34-123``
(``MelSpectrogramCreator``, ``Tacotron2SpectrogramCreator``, ``spectrogram_to_log_scale``) and the loop of
``dataset/preprocess.py:89-108``, batched.

The reference goes through torchaudio (``Spectrogram(pad=0)`` = ``torch.stft(center=True, pad_mode="reflect")`` with a periodic
Hann window) and librosa (``filters.mel``: Slaney scale, Slaney norm), one file at a time on the CPU.  Here a ragged batch of
utterances is one launch of ``rtts_mel_spectrogram`` (csrc/mel.hip): framing, the windowed DFT, the mel matrix and the log are
fused, in f32 throughout.  The window and the DFT live in one basis matrix built here in float64 and rounded once; the mel
matrix is ``mel_filterbank``, the triangular-ramp construction librosa and torchaudio share."""
from __future__ import annotations

import ctypes
import math
import os
import wave
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from .. import _lib, ops

MEL_MAX_SEGMENTS = 65535        # utterances of one launch (the grid's second dimension)
SUPPORTED_N_FFT = (512, 1024, 2048)


def _hz_to_mel(f: np.ndarray, mel_scale: str) -> np.ndarray:
    f = np.asarray(f, dtype=np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    if mel_scale != "slaney":
        raise ValueError(f"mel_scale must be 'htk' or 'slaney' (got {mel_scale!r})")
    logstep = math.log(6.4) / 27.0
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / logstep, f / (200.0 / 3.0))


def _mel_to_hz(m: np.ndarray, mel_scale: str) -> np.ndarray:
    m = np.asarray(m, dtype=np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    logstep = math.log(6.4) / 27.0
    return np.where(m >= 15.0, 1000.0 * np.exp(logstep * (m - 15.0)), m * (200.0 / 3.0))


def mel_filterbank(sample_rate: int, n_fft: int, n_mels: int, f_min: float = 0.0, f_max: Optional[float] = None,
                   mel_scale: str = "htk", norm: Optional[str] = None) -> torch.Tensor:
    """float64 (n_mels, n_fft/2 + 1) triangular mel filters: bin frequencies ``linspace(0, sr/2, n_fft/2 + 1)``, corner
    frequencies ``linspace(mel(f_min), mel(f_max), n_mels + 2)`` mapped back to Hz, weight = max(0, min(rising ramp, falling
    ramp)).  ``mel_scale``: "htk" (``2595 log10(1 + f/700)``) or "slaney" (linear below 1 kHz, logarithmic above);
    ``norm``: None or "slaney" (each filter scaled by 2 / its bandwidth).  librosa.filters.mel = ("slaney", "slaney")."""
    if norm not in (None, "slaney"):
        raise ValueError(f"norm must be None or 'slaney' (got {norm!r})")
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    if not 0.0 <= f_min < f_max:
        raise ValueError(f"need 0 <= f_min < f_max (got {f_min}, {f_max})")
    freqs = np.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1)
    m_lo, m_hi = (float(_hz_to_mel(np.array(f), mel_scale)) for f in (f_min, f_max))
    f_pts = _mel_to_hz(np.linspace(m_lo, m_hi, n_mels + 2), mel_scale)
    f_diff = np.diff(f_pts)
    slopes = f_pts[:, None] - freqs[None, :]                      # (n_mels + 2, bins)
    rising = -slopes[:-2] / f_diff[:-1, None]
    falling = slopes[2:] / f_diff[1:, None]
    fb = np.maximum(0.0, np.minimum(rising, falling))
    if norm == "slaney":
        fb = fb * (2.0 / (f_pts[2:] - f_pts[:-2]))[:, None]
    return torch.from_numpy(fb)


def hann_window(win_length: int, n_fft: int) -> np.ndarray:
    """float64 periodic Hann of ``win_length``, zero padded and centred to ``n_fft`` as ``torch.stft`` pads its window."""
    if not 1 <= win_length <= n_fft:
        raise ValueError(f"need 1 <= win_length <= n_fft (got {win_length}, {n_fft})")
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    return w


def dft_basis(n_fft: int, win_length: int) -> torch.Tensor:
    """f32 (n_fft, n_fft), the ``dft_basis`` of ``rtts_mel_spectrogram``: row n = sample of the frame, window folded in;
    column k < n_fft/2 = w[n] cos(2 pi n k / n_fft), column n_fft/2 + k = w[n] sin(2 pi n k / n_fft) (1 <= k < n_fft/2), column
    n_fft/2 = w[n] cos(pi n), the Nyquist bin.  Built in float64 with the angle reduced in integers ((n k) mod n_fft, so every
    argument lies in [0, 2 pi)), rounded once to f32."""
    half = n_fft // 2
    n = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(half, dtype=np.int64)[None, :]
    ang = (2.0 * np.pi / n_fft) * ((n * k) % n_fft).astype(np.float64)
    basis = np.empty((n_fft, n_fft), dtype=np.float64)
    basis[:, :half] = np.cos(ang)
    basis[:, half:] = np.sin(ang)
    basis[:, half] = 1.0 - 2.0 * (np.arange(n_fft) % 2)           # cos(pi n), exactly
    basis *= hann_window(win_length, n_fft)[:, None]
    return torch.from_numpy(basis.astype(np.float32))


def mel_frames(n_samples: int, hop_length: int) -> int:
    """Frames of an utterance of ``n_samples``: ``n_samples // hop_length + 1`` (``rtts_mel_frames``)."""
    lib = _lib.load()
    t = lib.rtts_mel_frames(int(n_samples), int(hop_length))
    if t < 0:
        raise _lib.RttsError(lib.rtts_last_error().decode())
    return int(t)


def _check_pcm16_mono(f, path) -> None:
    if f.getnchannels() != 1 or f.getsampwidth() != 2 or f.getcomptype() != "NONE":
        raise ValueError(f"{path}: expected 16-bit PCM mono, got {f.getnchannels()} channel(s) of {8 * f.getsampwidth()} bits "
                         f"({f.getcomptype()})")


def wav_info(path) -> Tuple[int, int]:
    """(samples, sample rate) of a 16-bit PCM mono WAV from its header alone; any other encoding raises."""
    with wave.open(os.fspath(path), "rb") as f:
        _check_pcm16_mono(f, path)
        return f.getnframes(), f.getframerate()


def read_wav(path) -> Tuple[torch.Tensor, int]:
    """16-bit PCM mono WAV -> (f32 samples in [-1, 1), sample rate): int16 / 32768, what ``torchaudio.load`` returns for such
    a file.  Any other encoding raises."""
    with wave.open(os.fspath(path), "rb") as f:
        _check_pcm16_mono(f, path)
        rate = f.getframerate()
        raw = f.readframes(f.getnframes())
    pcm = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    return torch.from_numpy(pcm), rate


def _offsets(counts: Sequence[int]) -> List[int]:
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    return off


class MelTables:
    """Offset tables of one ragged call: utterance lengths -> sample / frame offsets, as host arrays (validated by the entry
    point) and as one device tensor (read by the kernel).  Build it once to replay a captured call on new audio of the same
    lengths."""

    def __init__(self, lengths: Sequence[int], hop_length: int, device):
        self.lengths = [int(n) for n in lengths]
        if not 1 <= len(self.lengths) <= MEL_MAX_SEGMENTS:
            raise ValueError(f"a mel call takes 1..{MEL_MAX_SEGMENTS} utterances (got {len(self.lengths)})")
        self.frames = [n // hop_length + 1 for n in self.lengths]
        self.sample_offsets, self.frame_offsets = _offsets(self.lengths), _offsets(self.frames)
        n1 = len(self.lengths) + 1
        self.soff_host = (ctypes.c_int64 * n1)(*self.sample_offsets)
        self.foff_host = (ctypes.c_int64 * n1)(*self.frame_offsets)
        host = torch.tensor([self.sample_offsets, self.frame_offsets], dtype=torch.int64).pin_memory()
        self.device_table = host.to(device, non_blocking=True)    # enqueued, not waited for
        self._pinned = host                                       # alive until the copy has run


class _LogMel(nn.Module):
    """Shared body of the two creators: bases as non-persistent device buffers, ragged launches, padding, file I/O."""

    def __init__(self, sample_rate: int, n_fft: int, win_length: int, hop_length: int, n_mels: int, *, power: int, mel_scale: str,
                 norm: Optional[str], f_min: float = 0.0, f_max: float = 8000.0, clip: float = 1e-5):
        super().__init__()
        if n_fft not in SUPPORTED_N_FFT or hop_length != n_fft // 4 or not 1 <= n_mels <= 128:
            raise ValueError(f"supported: n_fft in {SUPPORTED_N_FFT}, hop_length = n_fft / 4, 1 <= n_mels <= 128 "
                             f"(got n_fft={n_fft}, hop_length={hop_length}, n_mels={n_mels})")
        self.sample_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels = sample_rate, n_fft, win_length, hop_length, n_mels
        self.power, self.clip = int(power), float(clip)
        self.register_buffer("dft_basis", dft_basis(n_fft, win_length), persistent=False)
        fb = mel_filterbank(sample_rate, n_fft, n_mels, f_min, f_max, mel_scale, norm)
        self.register_buffer("mel_basis", fb.to(torch.float32).contiguous(), persistent=False)

    @property
    def log_clip(self) -> float:
        """log(clip) rounded to f32: the value of padding frames (and, to the last bit or so, of silence)."""
        return float(np.float32(math.log(float(np.float32(self.clip)))))

    def _device(self, what: str) -> torch.device:
        dev = self.dft_basis.device
        if dev.type != "cuda":
            raise _lib.RttsError(f"{type(self).__name__}.{what} runs on the GPU only (no CPU fallback for the HIP path)")
        return dev

    def tables(self, lengths: Sequence[int]) -> MelTables:
        return MelTables(lengths, self.hop_length, self._device("tables"))

    @torch.no_grad()
    def forward_packed(self, audio: torch.Tensor, lengths: Optional[Sequence[int]] = None, *, tables: Optional[MelTables] = None,
                       out: Optional[torch.Tensor] = None):
        """``audio``: the utterances end to end, a flat f32 device tensor; ``lengths``: their sample counts (host ints), or
        ``tables`` from an earlier ``self.tables(lengths)`` -> (mel (n_mels, total frames) f32, frame offsets: utterance i owns
        columns [offsets[i], offsets[i+1]), the reference's (n_mels, T) of that utterance).  One launch, stream-ordered."""
        dev = self._device("forward_packed")
        if tables is None:
            if lengths is None:
                raise ValueError("forward_packed needs lengths or tables")
            tables = self.tables(lengths)
        if not (audio.is_cuda and audio.device == dev):
            raise _lib.RttsError(f"{type(self).__name__}.forward_packed runs on the GPU only: audio is on {audio.device}, the bases on {dev}")
        total = tables.frame_offsets[-1]
        if out is None:
            out = torch.empty(self.n_mels, total, dtype=torch.float32, device=dev)
        ops.mel_spectrogram(audio, tables.soff_host, tables.foff_host, tables.device_table, len(tables.lengths), self.dft_basis,
                            self.mel_basis, self.n_fft, self.hop_length, self.power, self.clip, out)
        return out, list(tables.frame_offsets)

    def _gather(self, audio, lengths) -> Tuple[torch.Tensor, List[int]]:
        dev = self._device("forward")
        if torch.is_tensor(audio):
            if audio.dim() != 2 or lengths is None:
                raise ValueError("forward takes a list of 1-D tensors, or a padded (B, N) tensor with lengths")
            if not audio.is_cuda:
                raise _lib.RttsError(f"{type(self).__name__}.forward runs on the GPU only (no CPU fallback for the HIP path)")
            if torch.is_tensor(lengths):
                lengths = lengths.tolist()
            lens = [int(n) for n in lengths]
            if len(lens) != audio.shape[0] or max(lens) > audio.shape[1]:
                raise ValueError(f"lengths {lens} do not fit audio of shape {tuple(audio.shape)}")
            parts = [audio[i, :n] for i, n in enumerate(lens)]
        else:
            parts = list(audio)
            if any(not torch.is_tensor(p) or p.dim() != 1 for p in parts):
                raise ValueError("forward takes a list of 1-D tensors, or a padded (B, N) tensor with lengths")
            if any(not p.is_cuda for p in parts):
                raise _lib.RttsError(f"{type(self).__name__}.forward runs on the GPU only (no CPU fallback for the HIP path)")
            lens = [int(p.numel()) for p in parts]
        if not parts:
            raise ValueError("forward: no utterances")
        short = [n for n in lens if n <= self.n_fft // 2]
        if short:
            raise ValueError(f"utterances of {short} samples: reflect padding needs more than n_fft / 2 = {self.n_fft // 2}")
        return torch.cat([p.to(dev, torch.float32) for p in parts]), lens

    @torch.no_grad()
    def forward(self, audio, lengths=None):
        """``audio``: a list of 1-D device tensors, or a padded (B, N) device tensor with ``lengths`` (host ints or a tensor)
        -> (log-mel (B, n_mels, T_max) f32, frames (B,) int64 on the device).  Utterance i fills [:, :frames_i]; frames past it
        hold log(clip), the value silence gets."""
        flat, lens = self._gather(audio, lengths)
        packed, foff = self.forward_packed(flat, lens)
        frames = [foff[i + 1] - foff[i] for i in range(len(lens))]
        mel = torch.full((len(lens), self.n_mels, max(frames)), self.log_clip, dtype=torch.float32, device=packed.device)
        for i, t in enumerate(frames):
            mel[i, :, :t] = packed[:, foff[i]:foff[i + 1]]
        return mel, torch.tensor(frames, dtype=torch.int64).to(packed.device, non_blocking=True)

    def _check_rate(self, rate: int, path) -> None:
        """The mel matrix is built for ``sample_rate``: audio at another rate would give wrong spectrograms without a sign."""
        if rate != self.sample_rate:
            raise ValueError(f"{path}: sample rate {rate} Hz, this creator was built for {self.sample_rate} Hz (resample first)")

    def audio_to_mel_spectrogram(self, input_path, output_path) -> None:
        """The reference's per-file call (``convert.py:53-64`` / ``:100-112``): 16-bit PCM mono WAV -> ``torch.save`` of the
        (1, n_mels, T) log-mel, a CPU tensor."""
        waveform, rate = read_wav(input_path)
        self._check_rate(rate, input_path)
        mel, _ = self.forward([waveform.to(self._device("audio_to_mel_spectrogram"))])
        torch.save(mel.cpu(), os.fspath(output_path))


class Tacotron2Spectrogram(_LogMel):
    """``Tacotron2SpectrogramCreator`` (``convert.py:67-112``): log of the mel-weighted STFT MAGNITUDES (power 2, then sqrt),
    librosa's mel matrix (Slaney scale and norm), 0 - 8000 Hz, clip 1e-5, natural log."""

    def __init__(self, sample_rate: int, n_fft: int, win_length: int, hop_length: int, n_mels: int):
        super().__init__(sample_rate, n_fft, win_length, hop_length, n_mels, power=1, mel_scale="slaney", norm="slaney")


class MelSpectrogram(_LogMel):
    """``MelSpectrogramCreator`` (``convert.py:34-64``): log of the mel-weighted POWER spectrogram, torchaudio's default mel
    matrix (HTK scale, no norm), 0 - 8000 Hz, same clip and log."""

    def __init__(self, sample_rate: int, n_fft: int, win_length: int, hop_length: int, n_mels: int):
        super().__init__(sample_rate, n_fft, win_length, hop_length, n_mels, power=2, mel_scale="htk", norm=None)


def preprocess_directory(audio_dir, mel_dir, creator: _LogMel, max_batch_samples: int = 1 << 24, suffix: str = ".wav") -> List[str]:
    """The loop of ``preprocess.py:100-108``, batched: every ``*.wav`` of ``audio_dir`` -> ``mel_dir/<stem>.pt`` (the
    reference's file format).  Files are sorted by length and packed into ragged launches of at most ``max_batch_samples``
    samples (one file alone may exceed it); only one batch of audio is in host memory at a time.  A file whose sample rate is
    not the creator's raises.  -> the written paths, in the order of the sorted input names."""
    dev = creator._device("preprocess_directory")
    names = sorted(f for f in os.listdir(audio_dir) if f.endswith(suffix))
    os.makedirs(mel_dir, exist_ok=True)
    samples = {}
    for name in names:                                             # headers only: the audio is decoded batch by batch
        samples[name], rate = wav_info(os.path.join(audio_dir, name))
        creator._check_rate(rate, os.path.join(audio_dir, name))
    order = sorted(names, key=lambda name: (samples[name], name))
    written = {}
    i = 0
    while i < len(order):
        batch, count = [], 0
        while i < len(order) and len(batch) < MEL_MAX_SEGMENTS and (not batch or count + samples[order[i]] <= max_batch_samples):
            batch.append(order[i])
            count += samples[order[i]]
            i += 1
        waves = [read_wav(os.path.join(audio_dir, name))[0] for name in batch]
        packed, foff = creator.forward_packed(torch.cat(waves).to(dev), [w.numel() for w in waves])
        host = packed.cpu()
        for j, name in enumerate(batch):
            path = os.path.join(mel_dir, name[:-len(suffix)] + ".pt")
            torch.save(host[:, foff[j]:foff[j + 1]].unsqueeze(0).clone(), path)
            written[name] = path
    return [written[name] for name in names]
