"""float64 oracle of the sample-rate conversion, straight from its definition (no phases, no tables, no reduced ratio):

    c = 0.99 * 0.5 * min(orig, new),  L = 6,  W = L / (2 c)
    M = ceil(N new / orig)
    out[k] = sum_i x[i] h(i / orig - k / new),    0 <= k < M,   x zero outside [0, N)
    h(d)   = 0                                                      if |d| >= W
           = (1 + cos(2 pi c d / L)) / 2 * sin(2 pi c d) / (pi d) / orig   otherwise   (2 c / orig at d = 0)

``resample`` returns out and A_k = sum_i |x[i]| |h(.)|, the scale of the f32 rounding error of output k.  ``dense=True`` sums
over every i of the utterance; the default visits, per output, the inputs within W + 3 samples of its centre k orig / new --
outside, h is zero by its first line, so the two hold the same non-zero terms (tests/test_resample_cpu.py compares them)."""
import math

import numpy as np

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99


def cutoff(orig: int, new: int) -> float:
    return ROLLOFF * 0.5 * min(orig, new)


def h(d, orig: int, new: int) -> np.ndarray:
    """The filter at time differences ``d`` (seconds, float64 array)."""
    d = np.asarray(d, dtype=np.float64)
    c = cutoff(orig, new)
    width = LOWPASS_FILTER_WIDTH / (2.0 * c)
    safe = np.where(d == 0.0, 1.0, d)
    sinc = np.where(d == 0.0, 2.0 * c, np.sin(2.0 * np.pi * c * safe) / (np.pi * safe))
    window = 0.5 * (1.0 + np.cos(2.0 * np.pi * c * d / LOWPASS_FILTER_WIDTH))
    return np.where(np.abs(d) >= width, 0.0, window * sinc / orig)


def out_len(n: int, orig: int, new: int) -> int:
    return -((-n * new) // orig)


def resample(x, orig: int, new: int, dense: bool = False, chunk: int = 2048):
    """x: 1-D array -> (out float64 (M,), A float64 (M,))."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    m = out_len(n, orig, new)
    out, scale = np.zeros(m), np.zeros(m)
    reach = int(math.ceil(LOWPASS_FILTER_WIDTH / (2.0 * cutoff(orig, new)) * orig)) + 3
    for k0 in range(0, m, chunk):
        k = np.arange(k0, min(k0 + chunk, m), dtype=np.float64)
        if dense:
            i = np.broadcast_to(np.arange(n, dtype=np.int64)[None, :], (k.size, n))
        else:
            centre = np.floor(k * orig / new).astype(np.int64)
            i = centre[:, None] + np.arange(-reach, reach + 1, dtype=np.int64)[None, :]
        valid = (i >= 0) & (i < n)
        xi = np.where(valid, x[np.clip(i, 0, n - 1)], 0.0)
        w = h(i.astype(np.float64) / orig - k[:, None] / new, orig, new)
        out[k0:k0 + k.size] = (xi * w).sum(1)
        scale[k0:k0 + k.size] = (np.abs(xi) * np.abs(w)).sum(1)
    return out, scale
