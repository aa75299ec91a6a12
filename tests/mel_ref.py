"""float64 restatement of the log-mel pipeline (the oracle of tests/test_mel_cpu.py and tests/test_mel_hip.py).

A different algorithm from the kernel's on purpose: ``torch.stft`` (an FFT) in float64 for the spectrum, and a mel filter
bank written out here, filter by filter, that does not import the product's ``mel_filterbank``."""
import math

import torch

CLIP = 1e-5


def hz_to_mel(f: float, scale: str) -> float:
    if scale == "htk":
        return 2595.0 * math.log10(1.0 + f / 700.0)
    assert scale == "slaney"
    if f < 1000.0:
        return f / (200.0 / 3.0)
    return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def mel_to_hz(m: float, scale: str) -> float:
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    assert scale == "slaney"
    if m < 15.0:
        return m * (200.0 / 3.0)
    return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def filterbank(sample_rate, n_fft, n_mels, f_min, f_max, scale, norm) -> torch.Tensor:
    """(n_mels, n_fft/2 + 1) float64, one scalar at a time."""
    bins = n_fft // 2 + 1
    lo, hi = hz_to_mel(f_min, scale), hz_to_mel(f_max, scale)
    pts = [mel_to_hz(lo + (hi - lo) * i / (n_mels + 1), scale) for i in range(n_mels + 2)]
    fb = torch.zeros(n_mels, bins, dtype=torch.float64)
    for m in range(n_mels):
        left, centre, right = pts[m], pts[m + 1], pts[m + 2]
        for k in range(bins):
            f = (sample_rate / 2.0) * k / (bins - 1)
            w = max(0.0, min((f - left) / (centre - left), (right - f) / (right - centre)))
            if norm == "slaney":
                w *= 2.0 / (right - left)
            else:
                assert norm is None
            fb[m, k] = w
    return fb


def window(n_fft: int, win_length: int) -> torch.Tensor:
    """The float64 periodic Hann of win_length as torch.stft pads it to n_fft (centred)."""
    w = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
    return w


def magnitudes(x: torch.Tensor, n_fft: int, hop: int, win_length: int) -> torch.Tensor:
    """|STFT| (n_fft/2 + 1, T) float64 of a 1-D signal."""
    return torch.stft(x.double(), n_fft, hop, win_length, torch.hann_window(win_length, periodic=True, dtype=torch.float64), center=True,
                      pad_mode="reflect", return_complex=True).abs()


def mel_linear(x: torch.Tensor, fb: torch.Tensor, n_fft: int, hop: int, win_length: int, power: int, clip: float = CLIP) -> torch.Tensor:
    """max(fb @ |STFT|^power, clip) (n_mels, T) float64: the quantity whose log the product stores."""
    return torch.clamp(fb @ magnitudes(x, n_fft, hop, win_length) ** power, min=clip)


def frame_l1(x: torch.Tensor, n_fft: int, hop: int, win_length: int) -> torch.Tensor:
    """L1_t = sum_n |x_n w_n| of every frame (T,) float64: the scale of the kernel's rounding error."""
    xp = torch.nn.functional.pad(x.double().view(1, 1, -1), (n_fft // 2, n_fft // 2), mode="reflect").view(-1)
    frames = xp.unfold(0, n_fft, hop)                              # (T, n_fft)
    return (frames * window(n_fft, win_length)).abs().sum(1)
