"""Audio -> log-mel spectrograms on the GPU: the spectrogram creators of the reference's ``dataset/convert.py:34-123``
(``MelSpectrogramCreator``, ``Tacotron2SpectrogramCreator``, ``spectrogram_to_log_scale``) and the loop of
``dataset/preprocess.py:89-108``, batched.

The reference goes through torchaudio (``Spectrogram(pad=0)`` = ``torch.stft(center=True, pad_mode="reflect")`` with a periodic
Hann window) and librosa (``filters.mel``: Slaney scale, Slaney norm), one file at a time on the CPU.  Here a ragged batch of
utterances is one launch of ``rtts_mel_spectrogram`` (csrc/mel.hip): framing, the windowed DFT, the mel matrix and the log are
fused, in f32 throughout.  The window and the DFT live in one basis matrix built here in float64 and rounded once; the mel
matrix is ``mel_filterbank``, the triangular-ramp construction librosa and torchaudio share.

In front of it, ``Resample`` / ``resample_wav`` are the reference's ``resample_wav`` (``convert.py:131-146``:
``torchaudio.transforms.Resample``, keep channel 0) as one ragged launch of ``rtts_resample`` (csrc/resample.hip), whose packed
output is the packed input of the mel launch: ``preprocess_directory(resample=True)`` uploads raw PCM and runs the two."""
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
RESAMPLE_TILE = 1024            # outputs of one workgroup of rtts_resample (RTTS_RESAMPLE_TILE of include/rtts.h)
RESAMPLE_MAX_TAPS = 256         # RTTS_RESAMPLE_MAX_TAPS
RESAMPLE_MAX_TABLE = 1 << 22    # RTTS_RESAMPLE_MAX_TABLE: coefficients of one table (new_red * taps)


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


def dft_basis(n_fft: int, win_length: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """f32 (n_fft, n_fft), the ``dft_basis`` of ``rtts_mel_spectrogram``: row n = sample of the frame, window folded in;
    column k < n_fft/2 = w[n] cos(2 pi n k / n_fft), column n_fft/2 + k = w[n] sin(2 pi n k / n_fft) (1 <= k < n_fft/2), column
    n_fft/2 = w[n] cos(pi n), the Nyquist bin.  Built in float64 with the angle reduced in integers ((n k) mod n_fft, so every
    argument lies in [0, 2 pi)), rounded once to f32 (``dtype=torch.float64``: the unrounded matrix)."""
    half = n_fft // 2
    n = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(half, dtype=np.int64)[None, :]
    ang = (2.0 * np.pi / n_fft) * ((n * k) % n_fft).astype(np.float64)
    basis = np.empty((n_fft, n_fft), dtype=np.float64)
    basis[:, :half] = np.cos(ang)
    basis[:, half:] = np.sin(ang)
    basis[:, half] = 1.0 - 2.0 * (np.arange(n_fft) % 2)           # cos(pi n), exactly
    basis *= hann_window(win_length, n_fft)[:, None]
    return torch.from_numpy(basis.astype(np.float32)) if dtype == torch.float32 else torch.from_numpy(basis).to(dtype)


def idft_basis(n_fft: int, win_length: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """f32 (n_fft, n_fft), the ``idft_basis`` of ``rtts_denoise``: the inverse of the real DFT in the column order of ``dft_basis``,
    with the synthesis window folded in.  Row = column of ``dft_basis``, column m = sample of the frame: row 0 = w[m] / n_fft,
    row n_fft/2 = w[m] cos(pi m) / n_fft (the Nyquist bin), row k = 2 w[m] cos(2 pi k m / n_fft) / n_fft and row n_fft/2 + k =
    2 w[m] sin(2 pi k m / n_fft) / n_fft for 1 <= k < n_fft/2.  So ``dft_basis @ idft_basis = diag(w) diag(w)``: a frame goes
    through both windows and nothing else.  Angles reduced in integers, float64, rounded once to f32, as ``dft_basis``
    (``dtype=torch.float64``: the unrounded matrix)."""
    half = n_fft // 2
    m = np.arange(n_fft, dtype=np.int64)[None, :]
    k = np.arange(half, dtype=np.int64)[:, None]
    ang = (2.0 * np.pi / n_fft) * ((k * m) % n_fft).astype(np.float64)
    inv = np.empty((n_fft, n_fft), dtype=np.float64)
    inv[:half] = 2.0 * np.cos(ang)
    inv[half:] = 2.0 * np.sin(ang)
    inv[0] = 1.0
    inv[half] = 1.0 - 2.0 * (np.arange(n_fft) % 2)                # cos(pi m), exactly
    inv *= hann_window(win_length, n_fft)[None, :] / n_fft
    return torch.from_numpy(inv.astype(np.float32)) if dtype == torch.float32 else torch.from_numpy(inv).to(dtype)


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


def _utterances(audio, lengths, who: str) -> Tuple[List[torch.Tensor], List[int]]:
    """The two input forms of the modules' ``forward`` -- a list of 1-D device tensors, or a padded (B, N) device tensor with
    ``lengths`` -- as (the utterances, their lengths)."""
    if torch.is_tensor(audio):
        if audio.dim() != 2 or lengths is None:
            raise ValueError("forward takes a list of 1-D tensors, or a padded (B, N) tensor with lengths")
        if not audio.is_cuda:
            raise _lib.RttsError(f"{who}.forward runs on the GPU only (no CPU fallback for the HIP path)")
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
            raise _lib.RttsError(f"{who}.forward runs on the GPU only (no CPU fallback for the HIP path)")
        lens = [int(p.numel()) for p in parts]
    if not parts:
        raise ValueError("forward: no utterances")
    return parts, lens


class _GpuOnly:
    """``_device(what)`` of the modules below: the device of the buffer named by ``_anchor``, which has to be a GPU."""

    _anchor: str

    def _device(self, what: str) -> torch.device:
        dev = getattr(self, self._anchor).device
        if dev.type != "cuda":
            raise _lib.RttsError(f"{type(self).__name__}.{what} runs on the GPU only (no CPU fallback for the HIP path)")
        return dev


def _host_array(offsets: Sequence[int]):
    return (ctypes.c_int64 * len(offsets))(*offsets)


class _OffsetTables:
    """What the tables of a ragged call share: offset lists as host arrays (validated by the entry point) and as one device
    tensor (read by the kernel)."""

    def _upload(self, device, rows=None, **host_arrays) -> None:
        """Attribute ``name`` = the ``c_int64`` array of each ``name=offsets``; ``device_table`` = int64 ``rows`` (default: those
        offset lists in order), copied from pinned memory when ``device`` is a GPU, without waiting."""
        for name, offsets in host_arrays.items():
            setattr(self, name, _host_array(offsets))
        host = torch.tensor(list(host_arrays.values()) if rows is None else rows, dtype=torch.int64)
        if torch.device(device).type == "cuda":
            host = host.pin_memory()
        self.device_table = host.to(device, non_blocking=True)    # enqueued, not waited for
        self._pinned = host                                       # alive until the copy has run


class MelTables(_OffsetTables):
    """Offset tables of one ragged call: utterance lengths -> sample / frame offsets, as host arrays (validated by the entry
    point) and as one device tensor (read by the kernel).  Build it once to replay a captured call on new audio of the same
    lengths."""

    def __init__(self, lengths: Sequence[int], hop_length: int, device):
        self.lengths = [int(n) for n in lengths]
        if not 1 <= len(self.lengths) <= MEL_MAX_SEGMENTS:
            raise ValueError(f"a mel call takes 1..{MEL_MAX_SEGMENTS} utterances (got {len(self.lengths)})")
        self.frames = [n // hop_length + 1 for n in self.lengths]
        self.sample_offsets, self.frame_offsets = _offsets(self.lengths), _offsets(self.frames)
        self._upload(device, soff_host=self.sample_offsets, foff_host=self.frame_offsets)


class _LogMel(_GpuOnly, nn.Module):
    """Shared body of the two creators: bases as non-persistent device buffers, ragged launches, padding, file I/O."""

    _anchor = "dft_basis"

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
        parts, lens = _utterances(audio, lengths, type(self).__name__)
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


def resample_tables(orig: int, new: int) -> Tuple[torch.Tensor, torch.Tensor, int, int, int]:
    """The tables of ``rtts_resample`` for ``orig`` -> ``new`` Hz -> (first int32 (new',), coefficients f32 (taps, new'), orig',
    new', taps), the rates reduced by their gcd.  Output k = j new' + p is sum_t x[j orig' + first[p] + t] * coefficients[t, p],
    with coefficients[t, p] = h((first[p] + t) / orig - p / new) for the filter
        h(d) = (1 + cos(2 pi c d / L)) / 2 * sin(2 pi c d) / (pi d) / orig  for |d| < W, else 0    (2 c / orig at d = 0),
        c = 0.99 * min(orig, new) / 2,  L = 6,  W = L / (2 c)
    (torchaudio's Resample: Kaldi's LinearResample, lowpass_filter_width 6).  first[p] = ceil(p orig' / new' - W orig); taps is the
    largest number of inputs within W of any phase, and shorter phases end in zeros.  The coefficient matrix is stored
    [tap][phase]: the lanes of a wave, consecutive outputs, read consecutive words.  Phase centres, the support and first[] are
    exact integer arithmetic (d = (i new' - p orig') / (orig' new' g), W = 200 / (33 min(orig, new))); h is evaluated in float64
    and rounded once to f32."""
    orig, new = int(orig), int(new)
    if orig < 1 or new < 1 or orig == new:
        raise ValueError(f"resample_tables: the rates must be positive and different (got {orig}, {new})")
    g = math.gcd(orig, new)
    o, w, lo = orig // g, new // g, min(orig, new)
    den, reach = 33 * lo * w, 200 * orig * w                      # p o / w -+ W orig = (33 lo p o -+ 200 orig w) / (33 lo w)
    first = [-((reach - 33 * lo * p * o) // den) for p in range(w)]
    last = [(33 * lo * p * o + reach) // den for p in range(w)]
    taps = max(b - a + 1 for a, b in zip(first, last))
    if taps > RESAMPLE_MAX_TAPS or w * taps > RESAMPLE_MAX_TABLE:
        raise ValueError(f"resample_tables: {orig} -> {new} Hz needs {taps} taps for {w} phases; supported are up to "
                         f"{RESAMPLE_MAX_TAPS} taps and {RESAMPLE_MAX_TABLE} coefficients")
    first_a = np.array(first, dtype=np.int64)
    num = (first_a[None, :] + np.arange(taps, dtype=np.int64)[:, None]) * w - np.arange(w, dtype=np.int64)[None, :] * o
    inside = np.abs(num) * (33 * lo) < 200 * (o * w * g)          # |d| < W
    d = num.astype(np.float64) / float(o * w * g)
    c = 0.495 * lo
    safe = np.where(num == 0, 1.0, d)
    sinc = np.where(num == 0, 2.0 * c, np.sin(2.0 * np.pi * c * safe) / (np.pi * safe))
    h = np.where(inside, 0.5 * (1.0 + np.cos(2.0 * np.pi * c * d / 6.0)) * sinc / orig, 0.0)
    return torch.tensor(first, dtype=torch.int32), torch.from_numpy(h.astype(np.float32)), o, w, taps


def resample_len(n_samples: int, orig: int, new: int) -> int:
    """Samples of an utterance of ``n_samples`` after ``orig`` -> ``new`` Hz: ceil(n_samples * new / orig) (``rtts_resample_len``)."""
    lib = _lib.load()
    m = lib.rtts_resample_len(int(n_samples), int(orig), int(new))
    if m < 0:
        raise _lib.RttsError(lib.rtts_last_error().decode())
    return int(m)


class ResampleTables(_OffsetTables):
    """Offset tables of one ragged ``rtts_resample`` call: utterance lengths in frames -> input / output offsets, as host arrays
    and as one device tensor, like ``MelTables``.  ``out_lengths`` / ``out_offsets`` are the lengths / sample offsets of the mel
    call that takes the output."""

    def __init__(self, lengths: Sequence[int], orig: int, new: int, device):
        self.lengths = [int(n) for n in lengths]
        if not 1 <= len(self.lengths) <= MEL_MAX_SEGMENTS:
            raise ValueError(f"a resample call takes 1..{MEL_MAX_SEGMENTS} utterances (got {len(self.lengths)})")
        if min(self.lengths) < 1:
            raise ValueError(f"utterances need at least one sample (got lengths {self.lengths})")
        self.out_lengths = [-((-n * new) // orig) for n in self.lengths]
        self.in_offsets, self.out_offsets = _offsets(self.lengths), _offsets(self.out_lengths)
        self._upload(device, ioff_host=self.in_offsets, ooff_host=self.out_offsets)


class Resample(_GpuOnly, nn.Module):
    """``torchaudio.transforms.Resample(orig_freq, new_freq)`` as the reference uses it (``convert.py:137``), for ragged batches on
    the GPU: one ``rtts_resample`` launch per call.  ``orig_freq == new_freq`` returns its input unchanged, as torchaudio's does."""

    _anchor = "first"

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        if self.orig_freq < 1 or self.new_freq < 1:
            raise ValueError(f"the rates must be positive (got {orig_freq}, {new_freq})")
        if self.orig_freq == self.new_freq:
            first, coef, self.orig_red, self.new_red, self.taps = torch.zeros(1, dtype=torch.int32), torch.ones(1, 1), 1, 1, 1
        else:
            first, coef, self.orig_red, self.new_red, self.taps = resample_tables(self.orig_freq, self.new_freq)
        self.register_buffer("first", first, persistent=False)
        self.register_buffer("coefficients", coef.contiguous(), persistent=False)

    def tables(self, lengths: Sequence[int]) -> ResampleTables:
        return ResampleTables(lengths, self.orig_red, self.new_red, self._device("tables"))

    @torch.no_grad()
    def forward_packed(self, audio: torch.Tensor, lengths: Optional[Sequence[int]] = None, *, tables: Optional[ResampleTables] = None,
                       channels: int = 1, out: Optional[torch.Tensor] = None):
        """``audio``: the utterances end to end, a flat device tensor, f32 (mono) or int16 (``channels`` interleaved: a WAV payload
        as it is; channel 0 / 32768 is resampled); ``lengths``: their frame counts (host ints), or ``tables`` from an earlier
        ``self.tables(lengths)`` -> (flat f32 of the resampled utterances, output offsets: utterance i owns
        [offsets[i], offsets[i+1])).  One launch, stream-ordered; the result is the packed input of a creator's
        ``forward_packed`` with lengths ``offsets[i+1] - offsets[i]``."""
        dev = self._device("forward_packed")
        if not (audio.is_cuda and audio.device == dev):
            raise _lib.RttsError(f"{type(self).__name__}.forward_packed runs on the GPU only: audio is on {audio.device}, the tables on {dev}")
        if self.orig_freq == self.new_freq:
            if audio.dtype != torch.float32 or lengths is None:
                raise ValueError("orig_freq == new_freq passes f32 audio with lengths through; there is nothing to launch")
            return audio, _offsets(lengths)
        if tables is None:
            if lengths is None:
                raise ValueError("forward_packed needs lengths or tables")
            tables = self.tables(lengths)
        if out is None:
            out = torch.empty(tables.out_offsets[-1], dtype=torch.float32, device=dev)
        ops.resample(audio, tables.ioff_host, tables.ooff_host, tables.device_table, len(tables.lengths), self.first, self.coefficients,
                     self.orig_red, self.new_red, out, channels=channels)
        return out, list(tables.out_offsets)

    @torch.no_grad()
    def forward(self, audio, lengths=None):
        """``audio``: a list of 1-D device tensors, or a padded (B, N) device tensor with ``lengths`` (host ints or a tensor)
        -> (resampled (B, M_max) f32, zero behind each utterance's M_i = ceil(N_i new / orig) samples; M (B,) int64 on the
        device)."""
        if self.orig_freq == self.new_freq:
            return audio, lengths
        dev = self._device("forward")
        parts, lens = _utterances(audio, lengths, type(self).__name__)
        packed, ooff = self.forward_packed(torch.cat([p.to(dev, torch.float32) for p in parts]), lens)
        m = [ooff[i + 1] - ooff[i] for i in range(len(lens))]
        res = torch.zeros(len(lens), max(m), dtype=torch.float32, device=dev)
        for i, n in enumerate(m):
            res[i, :n] = packed[ooff[i]:ooff[i + 1]]
        return res, torch.tensor(m, dtype=torch.int64).to(dev, non_blocking=True)


def pcm_info(path) -> Tuple[int, int, int]:
    """(frames, sample rate, channels) of a 16-bit PCM WAV from its header alone; any other sample format raises."""
    with wave.open(os.fspath(path), "rb") as f:
        if f.getsampwidth() != 2 or f.getcomptype() != "NONE":
            raise ValueError(f"{path}: expected 16-bit PCM, got {8 * f.getsampwidth()} bits ({f.getcomptype()})")
        return f.getnframes(), f.getframerate(), f.getnchannels()


def read_pcm(path) -> Tuple[torch.Tensor, int]:
    """16-bit PCM WAV of any channel count -> (int16 (frames, channels), sample rate): the payload as it is."""
    with wave.open(os.fspath(path), "rb") as f:
        if f.getsampwidth() != 2 or f.getcomptype() != "NONE":
            raise ValueError(f"{path}: expected 16-bit PCM, got {8 * f.getsampwidth()} bits ({f.getcomptype()})")
        rate, channels = f.getframerate(), f.getnchannels()
        raw = f.readframes(f.getnframes())
    pcm = np.frombuffer(raw, dtype="<i2").astype(np.int16).reshape(-1, channels)
    return torch.from_numpy(pcm), rate


def write_wav(path, samples: torch.Tensor, rate: int) -> None:
    """f32 samples (any shape, flattened) -> 16-bit PCM mono WAV: round(x * 32768), ties to even, clipped to [-32768, 32767]
    (the inverse of ``read_wav`` on every value a 16-bit file can hold)."""
    x = samples.detach().reshape(-1).to("cpu", torch.float64).numpy()
    pcm = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(os.fspath(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(rate))
        f.writeframes(pcm.tobytes())


def resample_wav(input_path, output_path, sampling_rate: int = 22050, device="cuda") -> None:
    """The reference's ``resample_wav`` (``convert.py:131-146``): channel 0 of a 16-bit PCM WAV, resampled to ``sampling_rate``
    on ``device``, saved as 16-bit mono.  A file already at the rate keeps its channel 0 bit for bit."""
    pcm, rate = read_pcm(input_path)
    if rate == sampling_rate:
        write_wav(output_path, pcm[:, 0].to(torch.float32) / 32768.0, rate)
        return
    resampler = Resample(rate, sampling_rate).to(device)
    out, _ = resampler.forward_packed(pcm.reshape(-1).to(resampler._device("resample_wav")), [pcm.shape[0]], channels=pcm.shape[1])
    write_wav(output_path, out, sampling_rate)


def group_by_format(info: dict) -> dict:
    """{name: (frames, rate, channels)} -> {(rate, channels): names sorted by (frames, name)}, keys in ascending order: the launches
    of ``preprocess_directory(resample=True)`` share a rate and a channel count."""
    groups = {}
    for name, (_, rate, channels) in info.items():
        groups.setdefault((rate, channels), []).append(name)
    return {key: sorted(groups[key], key=lambda name: (info[name][0], name)) for key in sorted(groups)}


def _batches(order: Sequence[str], size: dict, max_batch_samples: int):
    """Consecutive runs of ``order`` of at most ``max_batch_samples`` samples and MEL_MAX_SEGMENTS files (one file alone may
    exceed the former)."""
    i = 0
    while i < len(order):
        batch, count = [], 0
        while i < len(order) and len(batch) < MEL_MAX_SEGMENTS and (not batch or count + size[order[i]] <= max_batch_samples):
            batch.append(order[i])
            count += size[order[i]]
            i += 1
        yield batch


def _save_batch(packed: torch.Tensor, foff: Sequence[int], batch: Sequence[str], mel_dir, suffix: str, written: dict) -> None:
    host = packed.cpu()
    for j, name in enumerate(batch):
        path = os.path.join(mel_dir, name[:-len(suffix)] + ".pt")
        torch.save(host[:, foff[j]:foff[j + 1]].unsqueeze(0).clone(), path)
        written[name] = path


def _read_channel0(path) -> torch.Tensor:
    pcm, _ = read_pcm(path)
    return torch.from_numpy(pcm[:, 0].numpy().astype(np.float32) / 32768.0)


def preprocess_directory(audio_dir, mel_dir, creator: _LogMel, max_batch_samples: int = 1 << 24, suffix: str = ".wav",
                         resample: bool = False) -> List[str]:
    """The loop of ``preprocess.py:100-108``, batched: every ``*.wav`` of ``audio_dir`` -> ``mel_dir/<stem>.pt`` (the
    reference's file format).  Files are sorted by length and packed into ragged launches of at most ``max_batch_samples``
    samples (one file alone may exceed it); only one batch of audio is in host memory at a time.  A file whose sample rate is
    not the creator's raises -- unless ``resample`` is set: then the reference's ``resample_wav`` step (``preprocess.py:81-87``)
    runs in front, on the GPU.  16-bit PCM files of any rate and channel count are grouped by (rate, channels); a batch of a
    group is uploaded as raw PCM, channel 0 is resampled to ``creator.sample_rate`` by one ``rtts_resample`` launch, and its
    packed output feeds the mel launch without leaving the device (``max_batch_samples`` counts input frames).  Mono files
    already at the rate take the path above.  -> the written paths, in the order of the sorted input names."""
    dev = creator._device("preprocess_directory")
    names = sorted(f for f in os.listdir(audio_dir) if f.endswith(suffix))
    os.makedirs(mel_dir, exist_ok=True)
    written = {}
    if not resample:
        samples = {}
        for name in names:                                         # headers only: the audio is decoded batch by batch
            samples[name], rate = wav_info(os.path.join(audio_dir, name))
            creator._check_rate(rate, os.path.join(audio_dir, name))
        for batch in _batches(sorted(names, key=lambda name: (samples[name], name)), samples, max_batch_samples):
            waves = [read_wav(os.path.join(audio_dir, name))[0] for name in batch]
            packed, foff = creator.forward_packed(torch.cat(waves).to(dev), [w.numel() for w in waves])
            _save_batch(packed, foff, batch, mel_dir, suffix, written)
        return [written[name] for name in names]
    info = {name: pcm_info(os.path.join(audio_dir, name)) for name in names}
    frames = {name: info[name][0] for name in names}
    for (rate, channels), order in group_by_format(info).items():
        resampler = None if rate == creator.sample_rate else Resample(rate, creator.sample_rate).to(dev)
        for name in order:
            m = frames[name] if resampler is None else resample_len(frames[name], rate, creator.sample_rate)
            if m <= creator.n_fft // 2:
                raise ValueError(f"{os.path.join(audio_dir, name)}: {m} samples at {creator.sample_rate} Hz; reflect padding needs "
                                 f"more than n_fft / 2 = {creator.n_fft // 2}")
        for batch in _batches(order, frames, max_batch_samples):
            paths = [os.path.join(audio_dir, name) for name in batch]
            if resampler is None:                                  # at the rate already: channel 0, decoded on the host as read_wav does
                waves = [read_wav(p)[0] if channels == 1 else _read_channel0(p) for p in paths]
                packed, foff = creator.forward_packed(torch.cat(waves).to(dev), [w.numel() for w in waves])
            else:
                raw = torch.cat([read_pcm(p)[0].reshape(-1) for p in paths]).to(dev)
                audio, ooff = resampler.forward_packed(raw, [frames[name] for name in batch], channels=channels)
                packed, foff = creator.forward_packed(audio, [ooff[j + 1] - ooff[j] for j in range(len(batch))])
            _save_batch(packed, foff, batch, mel_dir, suffix, written)
    return [written[name] for name in names]
