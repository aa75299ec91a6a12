"""Griffin-Lim as include/rtts.h defines it (rtts_gl_magnitudes / rtts_gl_init / rtts_gl_step), restated on the host with explicit
DFT matrices and an explicit overlap-add -- no FFT, no torch.stft (TEST INFRASTRUCTURE; numpy on the CPU, no project kernel):

    M[k][t]  = max(0, sum_m P[k][m] exp(mel[m][t]))^(1/power),  t < L;  column L repeats column L - 1
    x_0      = iSTFT(M e^{i phi}),  phi[k][t] = 2 pi (drop_hash(seed, t (n_fft/2 + 1) + k) >> 8) / 2^24  ("hash") or 0 ("zero")
    x_{k+1}  = iSTFT(M R / |R|),    R = STFT(x_k - beta x_{k-1}),  beta = momentum / (1 + momentum),  R / |R| = 1 where |R| = 0

The ``*_f64`` functions are the truth the tests compare against.  The ``*_f32_twin`` functions do the transforms as float32 matmuls
with the package's own two f32 bases and everything between them in float32: the CPU stand-in for the kernels' arithmetic, whose
distance from float64 sets the kernels' error bounds.  Spectra are (T, bins) here, as in denoise_ref.py; M is passed and returned
bin-major (bins, T), the layout of the kernels."""
import numpy as np
import torch

from denoise_ref import HOP, N_FFT, frames_of, hann, overlap_add, spectrum_f64
from edges_ref import drop_hash

BINS = N_FFT // 2 + 1
_CACHE = {}


def _inverse_angles():
    if "ang" not in _CACHE:
        k = np.arange(1, N_FFT // 2)[:, None]
        m = np.arange(N_FFT)[None, :]
        ang = 2.0 * np.pi * ((k * m) % N_FFT) / N_FFT
        _CACHE["ang"] = (np.cos(ang), np.sin(ang))
    return _CACHE["ang"]


# ------------------------------------------------------------------ step 1: magnitudes
def magnitudes_f64(mel, pinv, power):
    """mel (n_mels, L) log-mel, pinv (bins, n_mels) -> (A, M), each (bins, L + 1) float64; L = 0 gives one zero column."""
    mel = np.asarray(mel, dtype=np.float64)
    pinv = np.asarray(pinv, dtype=np.float64)
    if mel.shape[1] == 0:
        z = np.zeros((pinv.shape[0], 1))
        return z, z.copy()
    a = np.maximum(pinv @ np.exp(mel), 0.0)
    a = np.concatenate([a, a[:, -1:]], axis=1)
    return a, a ** (1.0 / power)


def magnitude_bound(mel, pinv):
    """Elementwise bound on |A_f32 - A| for an ascending fmaf chain over n_mels terms in f32 (unit roundoff u = 2^-24): n_mels u for
    the chain (Higham, gamma_n to first order), 4 u for exp evaluated to 2 ulp and 4 u more of margin, times sum_m |P| exp(mel);
    (bins, L + 1)."""
    mel = np.asarray(mel, dtype=np.float64)
    s = np.abs(np.asarray(pinv, dtype=np.float64)) @ np.exp(mel)
    s = np.concatenate([s, s[:, -1:]], axis=1)
    return (mel.shape[0] + 8) * 2.0 ** -24 * s


def log_mel_f64(x, mel_basis, power, clip=1e-5):
    """(n_mels, T) float64 log-mel of an utterance as dataset.audio defines it: log(max(clip, mel_basis @ |X|^power))."""
    re, im = spectrum_f64(x)
    mag = np.sqrt(re * re + im * im).T
    return np.log(np.maximum(np.asarray(mel_basis, dtype=np.float64) @ (mag ** power), clip))


# ------------------------------------------------------------------ phases
def phases(phase, seed, t):
    """(t, bins) float64: the hash phases of frames 0 .. t - 1 of an utterance, or zeros."""
    if phase == "zero":
        return np.zeros((t, BINS))
    assert phase == "hash"
    idx = (np.arange(t, dtype=np.uint64)[:, None] * np.uint64(BINS) + np.arange(BINS, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)
    h = drop_hash(int(seed) & 0xFFFFFFFF, idx)
    return 2.0 * np.pi * (h >> np.uint64(8)).astype(np.float64) / 2.0 ** 24


# ------------------------------------------------------------------ float64 truth
def synth_f64(re, im, n):
    """iSTFT of the spectrum (re, im), each (T, bins): irfft written out (the imaginary part of bins 0 and n_fft/2 is not read), the
    synthesis window, the overlap-add over ascending frames and the window envelope."""
    half = N_FFT // 2
    cos, sin = _inverse_angles()
    f = (re[:, :1] + re[:, half:half + 1] * (1.0 - 2.0 * (np.arange(N_FFT) % 2))[None, :]
         + 2.0 * (re[:, 1:half] @ cos - im[:, 1:half] @ sin)) / N_FFT
    w = hann(N_FFT)
    return overlap_add(f * w[None, :], w, n)


def init_f64(mag, phase="hash", seed=0):
    """mag (bins, L + 1) -> x_0, 256 L samples; zeros for L < 3."""
    mag = np.asarray(mag, dtype=np.float64).T
    n = HOP * (mag.shape[0] - 1)
    if n <= N_FFT // 2:
        return np.zeros(n)
    phi = phases(phase, seed, mag.shape[0])
    return synth_f64(mag * np.cos(phi), mag * np.sin(phi), n)


def project_f64(mag_t, re, im):
    """M R / |R| for R = (re, im), (T, bins); R / |R| = 1 where |R| = 0."""
    a = np.sqrt(re * re + im * im)
    safe = np.where(a > 0, a, 1.0)
    return np.where(a > 0, mag_t * re / safe, mag_t), np.where(a > 0, mag_t * im / safe, 0.0)


def step_f64(mag, cur, prev=None, beta=0.0):
    mag_t = np.asarray(mag, dtype=np.float64).T
    cur = np.asarray(cur, dtype=np.float64)
    n = cur.shape[0]
    if n <= N_FFT // 2:
        return np.zeros(n)
    y = cur if prev is None or beta == 0.0 else cur - beta * np.asarray(prev, dtype=np.float64)
    re, im = spectrum_f64(y)
    return synth_f64(*project_f64(mag_t, re, im), n)


def griffin_lim_f64(mag, n_iter, momentum=0.99, phase="hash", seed=0, start=None):
    """-> [x_0, x_1, .. x_n_iter], the momentum carried through the signal; ``start`` replaces x_0."""
    beta = momentum / (1.0 + momentum)
    xs = [init_f64(mag, phase, seed) if start is None else np.asarray(start, dtype=np.float64)]
    for k in range(n_iter):
        xs.append(step_f64(mag, xs[-1], xs[-2] if k > 0 else None, beta))
    return xs


def griffin_lim_spectrogram_form_f64(mag, n_iter, momentum=0.99, phase="hash", seed=0):
    """The iteration as librosa and torchaudio write it, with the previous REBUILT SPECTROGRAM kept: c_k = STFT(x_k),
    R = c_k - beta c_{k-1}.  -> [x_0 .. x_n_iter].  Equal to ``griffin_lim_f64`` by the linearity of the STFT."""
    beta = momentum / (1.0 + momentum)
    mag_t = np.asarray(mag, dtype=np.float64).T
    xs = [init_f64(mag, phase, seed)]
    n = xs[0].shape[0]
    prev = None
    for _ in range(n_iter):
        re, im = spectrum_f64(xs[-1])
        r = (re, im) if prev is None else (re - beta * prev[0], im - beta * prev[1])
        prev = (re, im)
        xs.append(synth_f64(*project_f64(mag_t, *r), n))
    return xs


def spectral_error(x, mag):
    """d = || |STFT(x)| - M || / || M ||, float64."""
    re, im = spectrum_f64(np.asarray(x, dtype=np.float64))
    mag_t = np.asarray(mag, dtype=np.float64).T
    return float(np.linalg.norm(np.sqrt(re * re + im * im) - mag_t) / np.linalg.norm(mag_t))


# ------------------------------------------------------------------ float32 twin
def magnitudes_f32_twin(mel, pinv32, power):
    mel = np.asarray(mel, dtype=np.float32)
    if mel.shape[1] == 0:
        return np.zeros((pinv32.shape[0], 1), dtype=np.float32)
    a = np.maximum((torch.from_numpy(np.ascontiguousarray(pinv32)) @ torch.from_numpy(np.exp(mel))).numpy(), np.float32(0))
    a = np.concatenate([a, a[:, -1:]], axis=1)
    return np.sqrt(a) if power == 2 else a


def _synth_f32(z, idft32, dft32, n):
    fr = (torch.from_numpy(np.ascontiguousarray(z)) @ torch.from_numpy(idft32)).numpy()      # synthesis window folded into the basis
    return overlap_add(fr, dft32[:, 0].copy(), n)


def init_f32_twin(mag32, dft32, idft32, phase="hash", seed=0):
    """The columns of ``dft_basis``: cosine parts at k, +sum w x sin = -Im X at n_fft/2 + k, the Nyquist bin at n_fft/2."""
    half = N_FFT // 2
    mag_t = np.ascontiguousarray(np.asarray(mag32, dtype=np.float32).T)
    n = HOP * (mag_t.shape[0] - 1)
    if n <= half:
        return np.zeros(n, dtype=np.float32)
    phi = phases(phase, seed, mag_t.shape[0])
    co, si = np.cos(phi).astype(np.float32), np.sin(phi).astype(np.float32)
    z = np.empty((mag_t.shape[0], N_FFT), dtype=np.float32)
    z[:, :half] = mag_t[:, :half] * co[:, :half]
    z[:, half + 1:] = -(mag_t[:, 1:half] * si[:, 1:half])
    z[:, half] = mag_t[:, half] * co[:, half]
    return _synth_f32(z, idft32, dft32, n)


def step_f32_twin(mag32, cur, prev, beta, dft32, idft32):
    half = N_FFT // 2
    mag_t = np.ascontiguousarray(np.asarray(mag32, dtype=np.float32).T)
    cur = np.asarray(cur, dtype=np.float32)
    n = cur.shape[0]
    if n <= half:
        return np.zeros(n, dtype=np.float32)
    y = cur if prev is None or beta == 0.0 else cur - np.float32(beta) * np.asarray(prev, dtype=np.float32)
    cols = (torch.from_numpy(np.ascontiguousarray(frames_of(y))) @ torch.from_numpy(dft32)).numpy()       # (T, n_fft) f32
    a = np.sqrt(cols[:, :half] ** 2 + cols[:, half:] ** 2, dtype=np.float32)
    a[:, 0] = np.abs(cols[:, 0])
    an = np.abs(cols[:, half])
    safe = np.where(a > 0, a, np.float32(1))
    g = (mag_t[:, :half] / safe).astype(np.float32)
    z = np.empty_like(cols)
    z[:, :half] = np.where(a > 0, g * cols[:, :half], mag_t[:, :half])
    z[:, half:] = np.where(a > 0, g * cols[:, half:], np.float32(0))
    z[:, half] = np.where(an > 0, mag_t[:, half] / np.where(an > 0, an, np.float32(1)) * cols[:, half], mag_t[:, half])
    return _synth_f32(z, idft32, dft32, n)


def griffin_lim_f32_twin(mag32, n_iter, momentum, dft32, idft32, phase="hash", seed=0, start=None):
    beta = momentum / (1.0 + momentum)
    xs = [init_f32_twin(mag32, dft32, idft32, phase, seed) if start is None else np.asarray(start, dtype=np.float32)]
    for k in range(n_iter):
        xs.append(step_f32_twin(mag32, xs[-1], xs[-2] if k > 0 else None, beta, dft32, idft32))
    return xs


# ------------------------------------------------------------------ the convergence signal of the tests
def voiced_signal(n, seed, sample_rate=22050):
    """A vowel-like test signal: fundamental 120 + 40 sin(2 pi 1.3 t + phi) Hz, harmonics 1..29 at amplitude 1/k with random phases,
    times 0.5 + 0.5 sin^2(2 pi 3 t), times 0.1, plus 0.003 N(0, 1); float64."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / sample_rate
    f0 = 120.0 + 40.0 * np.sin(2.0 * np.pi * 1.3 * t + rng.uniform(0, 2 * np.pi))
    inst = 2.0 * np.pi * np.cumsum(f0) / sample_rate
    x = np.zeros(n)
    for k in range(1, 30):
        x += np.sin(k * inst + rng.uniform(0, 2 * np.pi)) / k
    x *= (0.5 + 0.5 * np.sin(2.0 * np.pi * 3.0 * t) ** 2) * 0.1
    return x + 0.003 * rng.standard_normal(n)
