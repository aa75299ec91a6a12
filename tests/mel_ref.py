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


# ---- shared by tests/test_mel_bins_cpu.py and tests/test_mel_bins_hip.py: inputs that reach every DFT bin, tile path and mel width ----

SIZES = ((512, 512), (1024, 1024), (2048, 2048), (1024, 800))      # (n_fft, win_length) of the per-bin tests
DENSE_WIDTHS_1024 = (1, 31, 32, 33, 64, 65, 96, 127, 128)          # n_mels around every 32-row wave tile of the mel product
# (n_fft, n_mels, power) of the dense-matrix test
DENSE_CASES = tuple((1024, m, 1) for m in DENSE_WIDTHS_1024) + tuple((n_fft, m, p) for n_fft in (512, 2048) for m in (33, 128) for p in (1, 2))


def frames_per_tile(n_fft: int) -> int:
    """FT of csrc/mel.hip: frames of one workgroup."""
    return 16 if n_fft == 2048 else 32


def noise(n: int) -> torch.Tensor:
    """Uniform noise in [-0.5, 0.5) of n samples, seeded by n."""
    return torch.rand(n, generator=torch.Generator().manual_seed(n)) - 0.5


def tile_frame_counts(n_fft: int):
    ft = frames_per_tile(n_fft)
    return [3, ft - 1, ft, ft + 1, 2 * ft, 2 * ft + 1, 3 * ft + 2]


def tile_lengths(n_fft: int):
    """The 14 utterance lengths of one ragged launch: for every frame count around the tile boundaries both ends of its length
    range, (f - 1) hop and f hop - 1 (raised to the n_fft/2 + 1 samples reflect padding needs).  The two 3-frame utterances come
    last, behind the longest: all their workgroups but the first exit at ``t0 >= frames``."""
    hop = n_fft // 4
    counts = tile_frame_counts(n_fft)
    out = []
    for f in counts[1:] + counts[:1]:
        for n in ((f - 1) * hop, f * hop - 1):
            n = max(n, n_fft // 2 + 1)
            assert n // hop + 1 == f
            out.append(n)
    return out


def one_hot_groups(n_fft: int):
    """[(first bin, rows)]: the bins 0 .. n_fft/2 in launches of at most 128 one-hot rows; the last one has a single row."""
    bins = n_fft // 2 + 1
    return [(b, min(128, bins - b)) for b in range(0, bins, 128)]


def one_hot(n_fft: int, rows) -> torch.Tensor:
    """f32 (len(rows), n_fft/2 + 1): row i reads bin rows[i] alone."""
    m = torch.zeros(len(rows), n_fft // 2 + 1)
    m[torch.arange(len(rows)), torch.as_tensor(list(rows))] = 1.0
    return m


def dense_matrix(n_mels: int, n_fft: int) -> torch.Tensor:
    """f32 (n_mels, n_fft/2 + 1), uniform in [0, 1) / bins: no column is zero, the first and the last included."""
    bins = n_fft // 2 + 1
    g = torch.Generator().manual_seed(1000 * n_mels + n_fft)
    return (torch.rand(n_mels, bins, dtype=torch.float64, generator=g) / bins).float()


def single_column_matrix(n_mels: int, n_fft: int, column: int) -> torch.Tensor:
    """f32 (n_mels, n_fft/2 + 1) whose only non-zero column is ``column`` (values in [0.5, 1.5))."""
    m = torch.zeros(n_mels, n_fft // 2 + 1)
    m[:, column] = torch.rand(n_mels, generator=torch.Generator().manual_seed(n_mels + column)) + 0.5
    return m


def error_over_bound(got_log: torch.Tensor, linear_ref: torch.Tensor, l1: torch.Tensor, row_sums: torch.Tensor, power: int,
                     clip: float = CLIP) -> torch.Tensor:
    """|exp(out) - ref| / (c L1_t^power S_m + 2^-18 ref) per element, ref = max(linear_ref, clip), c = 2^-20 (power 1) or 2^-19
    (power 2): the criterion of tests/test_mel_hip.py holds where this is <= 1.  got_log (rows, T) f32, linear_ref (rows, T)
    float64 before the clamp, l1 (T,), row_sums (rows,)."""
    assert tuple(got_log.shape) == tuple(linear_ref.shape) == (row_sums.numel(), l1.numel())
    ref = linear_ref.double().clamp_min(clip)
    bound = (2.0 ** -20 if power == 1 else 2.0 ** -19) * row_sums.double()[:, None] * (l1.double() ** power)[None, :] + 2.0 ** -18 * ref
    return (torch.exp(got_log.double()) - ref).abs() / bound


def frames_f32(x: torch.Tensor, n_fft: int, hop: int) -> torch.Tensor:
    """(T, n_fft) f32: the reflect-padded frames of a 1-D f32 signal."""
    xp = torch.nn.functional.pad(x.float().view(1, 1, -1), (n_fft // 2, n_fft // 2), mode="reflect").view(-1)
    return xp.unfold(0, n_fft, hop)


def twin_magnitudes(x: torch.Tensor, basis: torch.Tensor, n_fft: int, hop: int, power: int) -> torch.Tensor:
    """|X|^power (n_fft/2 + 1, T) in f32 through the kernel's own basis layout: frames @ basis, columns k and n_fft/2 + k the real
    and imaginary part of bin k for 1 <= k < n_fft/2, column 0 bin 0 and column n_fft/2 the Nyquist bin, both real."""
    half = n_fft // 2
    d = frames_f32(x, n_fft, hop) @ basis.float()                  # (T, n_fft)
    re, im = d[:, :half], d[:, half:]
    p2 = re * re + im * im
    p2[:, 0] = re[:, 0] * re[:, 0]
    p2 = torch.cat([p2, (im[:, 0] * im[:, 0])[:, None]], 1)
    return (p2 if power == 2 else p2.sqrt()).t().contiguous()


def twin_log_mel(mags: torch.Tensor, mel_basis: torch.Tensor, clip: float = CLIP) -> torch.Tensor:
    """log(max(M @ mags, clip)) in f32."""
    return torch.log(torch.clamp(mel_basis.float() @ mags, min=float(clip)))


def log_mel_f32(x: torch.Tensor, basis: torch.Tensor, mel_basis: torch.Tensor, n_fft: int, hop: int, power: int, clip: float = CLIP) -> torch.Tensor:
    """The float32 twin of rtts_mel_spectrogram on the host (n_mels, T): what a correct reading of the basis layout computes."""
    return twin_log_mel(twin_magnitudes(x, basis, n_fft, hop, power), mel_basis, clip)
