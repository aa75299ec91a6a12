"""The denoiser of rtts_denoise restated on the host, written out from its definition (include/rtts.h) with explicit DFT matrices,
an explicit overlap-add and an explicit envelope -- no FFT, no torch.stft:

    X[k][t] = sum_m w[m] xpad[t hop + m] exp(-2 pi i k m / n_fft)                 k = 0 .. n_fft / 2
    g[k][t] = max(|X[k][t]| - strength * bias[k], 0) / |X[k][t]|                  (0 where |X| = 0)
    f[t][m] = irfft(g[.][t] X[.][t])[m]
    y[p]    = sum_t w[q - t hop] f[t][q - t hop] / sum_t w[q - t hop]^2,   q = p + n_fft / 2

``denoise_f64`` is the truth the tests compare against.  ``denoise_f32_twin`` does the two transforms as float32 matmuls with the
package's own two f32 bases and everything between them in float32: the CPU stand-in for the kernel's arithmetic, whose distance
from ``denoise_f64`` sets the kernel's error bound."""
import numpy as np
import torch

N_FFT, HOP = 1024, 256


def hann(n_fft=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def frames_of(x, n_fft=N_FFT, hop=HOP):
    """(T, n_fft) frames of the reflect-padded utterance, T = n // hop + 1."""
    x = np.asarray(x)
    n = x.shape[0]
    assert n > n_fft // 2, "reflect padding needs more than n_fft / 2 samples"
    xpad = np.concatenate([x[1:n_fft // 2 + 1][::-1], x, x[n - 1 - n_fft // 2:n - 1][::-1]])
    t = n // hop + 1
    return np.stack([xpad[i * hop:i * hop + n_fft] for i in range(t)])


def spectrum_f64(x, n_fft=N_FFT, hop=HOP):
    """(re, im), each (T, n_fft/2 + 1) float64."""
    m = np.arange(n_fft)[:, None]
    k = np.arange(n_fft // 2 + 1)[None, :]
    ang = 2.0 * np.pi * ((m * k) % n_fft) / n_fft
    fw = frames_of(np.asarray(x, dtype=np.float64), n_fft, hop) * hann(n_fft)[None, :]
    return fw @ np.cos(ang), -(fw @ np.sin(ang))


def gain(mag, bias, strength):
    safe = np.where(mag > 0, mag, 1)
    return np.where(mag > 0, np.maximum(mag - strength * bias[None, :], 0) / safe, 0)


def overlap_add(fr, w, n, n_fft=N_FFT, hop=HOP):
    """fr (T, n_fft) already multiplied by the synthesis window; frames summed in ascending order, in fr's dtype."""
    t = fr.shape[0]
    acc = np.zeros((t - 1) * hop + n_fft, dtype=fr.dtype)
    env = np.zeros_like(acc)
    w2 = (w * w).astype(fr.dtype)
    for i in range(t):
        acc[i * hop:i * hop + n_fft] += fr[i]
        env[i * hop:i * hop + n_fft] += w2
    sl = slice(n_fft // 2, n_fft // 2 + n)
    assert env[sl].min() > 0, "the window envelope must be positive over the utterance"
    return acc[sl] / env[sl]


def denoise_f64(x, bias, strength, n_fft=N_FFT, hop=HOP):
    x = np.asarray(x, dtype=np.float64)
    bias = np.asarray(bias, dtype=np.float64)
    re, im = spectrum_f64(x, n_fft, hop)
    g = gain(np.sqrt(re * re + im * im), bias, float(strength))
    re, im = g * re, g * im
    # irfft written out: (1/N) [X_0 + (-1)^m X_{N/2} + 2 sum_{0<k<N/2} (Re X_k cos(2 pi k m / N) - Im X_k sin(2 pi k m / N))]
    half = n_fft // 2
    k = np.arange(1, half)[:, None]
    m = np.arange(n_fft)[None, :]
    ang = 2.0 * np.pi * ((k * m) % n_fft) / n_fft
    f = (re[:, :1] + re[:, half:half + 1] * (1.0 - 2.0 * (np.arange(n_fft) % 2))[None, :]
         + 2.0 * (re[:, 1:half] @ np.cos(ang) - im[:, 1:half] @ np.sin(ang))) / n_fft
    w = hann(n_fft)
    return overlap_add(f * w[None, :], w, x.shape[0], n_fft, hop)


def first_frame_magnitudes_f64(x, n_fft=N_FFT, hop=HOP):
    re, im = spectrum_f64(np.asarray(x, dtype=np.float64)[:n_fft], n_fft, hop)    # frame 0 reads samples 0 .. n_fft / 2 only
    return np.sqrt(re[0] ** 2 + im[0] ** 2)


def denoise_f32_twin(x, bias, strength, dft32, idft32, n_fft=N_FFT, hop=HOP):
    """float32 throughout, the transforms as matmuls with the package's f32 bases (``dataset.audio.dft_basis`` / ``idft_basis``,
    numpy arrays): what the kernel computes, up to the order of its sums."""
    half = n_fft // 2
    x = np.asarray(x, dtype=np.float32)
    bias = np.asarray(bias, dtype=np.float32)
    s = np.float32(strength)
    cols = (torch.from_numpy(np.ascontiguousarray(frames_of(x, n_fft, hop))) @ torch.from_numpy(dft32)).numpy()     # (T, n_fft) f32
    mag = np.sqrt(cols[:, :half] ** 2 + cols[:, half:] ** 2, dtype=np.float32)
    mag[:, 0] = np.abs(cols[:, 0])
    g = gain(mag, bias[:half], s).astype(np.float32)
    mn = np.abs(cols[:, half])
    gn = gain(mn[:, None], bias[half:], s).astype(np.float32)[:, 0]
    z = np.empty_like(cols)
    z[:, :half] = g * cols[:, :half]
    z[:, half:] = g * cols[:, half:]
    z[:, half] = gn * cols[:, half]
    fr = (torch.from_numpy(z) @ torch.from_numpy(idft32)).numpy()                  # synthesis window folded into the basis
    return overlap_add(fr, dft32[:, 0].copy(), x.shape[0], n_fft, hop)
