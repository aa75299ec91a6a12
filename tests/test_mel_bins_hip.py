"""rtts_mel_spectrogram (csrc/mel.hip) on every DFT bin, every tile path of its three instances and every mel width, against the
float64 oracle of tests/mel_ref.py.  tests/test_mel_hip.py sees the DFT through the product's filter banks only, which weigh bin 0
and the bins above 8 kHz with zero (tests/test_mel_bins_cpu.py); here the mel matrices are made by the tests, and every call goes
through ``ops.mel_spectrogram`` with the basis of ``dataset.audio.dft_basis``.

Criterion, per element and with nothing excluded (that of test_mel_hip.py):
    |exp(out) - ref| <= c L1_t^power S_m + 2^-18 ref,    c = 2^-20 (power 1) / 2^-19 (power 2),    ref clamped at clip = 1e-5,
L1_t = sum_n |x_n w_n| (``mel_ref.frame_l1``), S_m the row sum of the mel matrix used (1 for a one-hot row); and |out| < 16.
Inputs: ``mel_ref.tile_lengths`` -- 14 noise utterances in one ragged launch, of 3, FT - 1, FT, FT + 1, 2 FT, 2 FT + 1 and 3 FT + 2
frames (FT = 16 at n_fft 2048, else 32), each at the shortest and the longest length that has that many frames, the 3-frame ones
behind the longest.

  case                                         the kernel line it is there for
  test_every_bin_on_its_own                    one-hot rows over the bins 0 .. n_fft/2 in launches of 128, 128, ..., 1 rows: the
                                               accumulators of every wave (``acc[2j]``, ``acc[2j + 1]`` -> ``mag[bin * FT + c]``), the
                                               ``bin == 0`` branch (bin 0 from ``re``, the Nyquist bin from ``im``, basis column n_fft/2),
                                               the last product ``mrow && h == 0 ? a : 0.f`` with the zero row; both powers, the three
                                               instances and win 800 in a 1024 frame; ``t0 > 0``, the right-edge reflection in a later
                                               tile, ``t0 >= frames``, ``tcol = c & (FT - 1)``; n_mels = 1
  test_known_spectra                           a constant (all of it in bin 0, through ``fabsf(re)``), an alternating sign (all of it in
                                               the Nyquist bin, through ``fabsf(im)``), a sine on bin 450 (wave 7, argmax over 384..511)
  test_dense_matrix_every_width                ``if (w * 32 >= n_mels) return``, ``m < n_mels ? m : n_mels - 1``, ``mrow``, ``row < n_mels``
                                               at n_mels 1, 31, 32, 33, 64, 65, 96, 127, 128; every column of M non-zero
  test_single_column_matrices                  the first column alone (k = 0, h = 0 of the first pair) and the last alone (the pair
                                               (Nyquist bin, zero row))
  test_tile_paths_bitwise                      an utterance alone, in the batch, in the reversed batch and in a second run; a frame and
                                               the same samples one frame earlier in the tile and across a tile boundary (the header's
                                               "a frame's values do not depend on its place in the tile")
  test_audio_outside_the_utterance_is_not_read NaN in front of, behind and between the utterances: ``(s >= 0 && s < n) ? x[s] : 0.f``
                                               and the two reflections; the only check that sees a read at a zero window weight
                                               (w[0] = 0; 112 zeros on each side at win 800)
  test_output_outside_the_frames_is_not_written  ``c < FT && t < frames``, ``row < n_mels``, ``op[row * ld_out]`` with ld_out wider than the
                                               frames, guard rows, a lead and slack columns in every slot

Measured on one MI355X (worst error / bound over the launch set, as the tests print it; the bound is 1):
  per bin            n_fft 512     1024     2048     1024 / win 800        bin 0 (512, 1024, 2048, 800)   bin n_fft/2
  power 1            0.167         0.144    0.207    0.153                 0.082  0.118  0.131  0.102     0.120  0.144  0.085  0.106
  power 2            0.042         0.024    0.021    0.040                 0.037  0.022  0.014  0.017     0.039  0.024  0.009  0.015
  dense matrices     0.044 - 0.061 at n_fft 1024 (nine widths), 0.043 / 0.050 at 512, 0.049 / 0.051 at 2048; power 2: 0.002 / 0.001
  single column      first 0.113 / 0.135 / 0.135, last 0.120 / 0.161 / 0.104 (n_fft 512 / 1024 / 2048, the worse of the two powers)
At most 4 of the 167,564 - 340,300 references of a configuration lie below the clip (0.1 % is allowed).  The bitwise checks hold
as written, the place in the tile included.  The float32 host twin of test_mel_bins_cpu.py gives 0.05 - 0.14 per bin at power 1
on the same inputs: the kernel errs like a k-ordered f32 chain and no more.  The 41 cases take 2.9 s on the MI355X, the start of the process included.

What no test here can see, by the kernel's own arithmetic: ``s < n`` in the staging loop never fails (a sample with s >= n has been
reflected to 2 (n - 1) - s <= n - 2 one line earlier, and -s <= n_fft/2 < n), and ``s >= 0`` fails only for samples that frames
past the utterance's last alone read, which are never stored; ``w * 32 > n_mels`` in place of ``>=`` lets one more wave run with
``mrow`` false and every store masked by ``row < n_mels``.  Both are second guards, and removing either changes no output.
"""
import ctypes
import functools
import math

import pytest
import torch

import mel_ref

pytestmark = pytest.mark.gpu

CLIP = mel_ref.CLIP
SENTINEL = -7.0
DEVICE = "cuda:0"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device(DEVICE)


@functools.lru_cache(maxsize=None)
def _basis(n_fft, win):
    from reformer_tts_amd.dataset.audio import dft_basis
    return dft_basis(n_fft, win).to(DEVICE)


def _offsets(counts, lead=0):
    off = [lead]
    for n in counts:
        off.append(off[-1] + int(n))
    return off


def _launch(audio, soff, foff, n_fft, win, mel_basis, power, out):
    """One rtts_mel_spectrogram launch with offset tables of the caller's making; audio and out on the device."""
    from reformer_tts_amd import ops
    nseg = len(soff) - 1
    table = torch.tensor([soff, foff], dtype=torch.int64).to(audio.device)
    ops.mel_spectrogram(audio, (ctypes.c_int64 * (nseg + 1))(*soff), (ctypes.c_int64 * (nseg + 1))(*foff), table, nseg, _basis(n_fft, win),
                        mel_basis.to(audio.device).contiguous(), n_fft, n_fft // 4, power, CLIP, out)
    return out


def _run(utts, n_fft, win, mel_basis, power, gpu):
    """The utterances as one packed ragged launch -> [(n_mels, frames_i) f32 on the host]."""
    hop = n_fft // 4
    soff = _offsets(u.numel() for u in utts)
    foff = _offsets(u.numel() // hop + 1 for u in utts)
    out = torch.full((mel_basis.shape[0], foff[-1]), float("nan"), device=gpu)
    _launch(torch.cat(utts).to(gpu), soff, foff, n_fft, win, mel_basis, power, out)
    host = out.cpu()
    return [host[:, foff[i]:foff[i + 1]] for i in range(len(utts))]


@functools.lru_cache(maxsize=None)
def _batch(n_fft, win):
    """The 14 utterances of tile_lengths, their float64 magnitudes and frame scales: computed once, read by several tests."""
    hop = n_fft // 4
    utts = [mel_ref.noise(n) for n in mel_ref.tile_lengths(n_fft)]
    return utts, [mel_ref.magnitudes(x, n_fft, hop, win) for x in utts], [mel_ref.frame_l1(x, n_fft, hop, win) for x in utts]


def _hold(got, linear_ref, l1, row_sums, power, tag):
    """Assert the criterion on one utterance -> the (rows, T) error / bound ratios."""
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) < 16, tag
    ratio = mel_ref.error_over_bound(got, linear_ref, l1, row_sums, power)
    bad = ratio > 1
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} elements over the bound, worst {float(ratio.max()):.3f} of it at {divmod(int(ratio.argmax()), ratio.shape[1])}"
    return ratio


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("n_fft,win", mel_ref.SIZES)
def test_every_bin_on_its_own(gpu, n_fft, win, power):
    utts, mags, l1 = _batch(n_fft, win)
    worst = torch.zeros(n_fft // 2 + 1, dtype=torch.float64)
    below = total = 0
    for first, rows in mel_ref.one_hot_groups(n_fft):
        outs = _run(utts, n_fft, win, mel_ref.one_hot(n_fft, range(first, first + rows)), power, gpu)
        for i, got in enumerate(outs):
            ref = mags[i][first:first + rows] ** power
            ratio = _hold(got, ref, l1[i], torch.ones(rows), power, f"n_fft {n_fft} win {win} power {power} bins {first}..{first + rows - 1} N = {utts[i].numel()}")
            worst[first:first + rows] = torch.maximum(worst[first:first + rows], ratio.max(1).values)
            below += int((ref < CLIP).sum())
            total += ref.numel()
    print(f"per bin, n_fft {n_fft} win {win} power {power}: worst error / bound {float(worst.max()):.3f} (bin {int(worst.argmax())}), "
          f"bin 0 {float(worst[0]):.3f}, bin {n_fft // 2} {float(worst[-1]):.3f}; {below} of {total} references below the clip")
    assert below <= 0.001 * total
    assert float(worst.min()) > 0                                   # no bin compared against nothing


SPECTRUM_ROWS = [0, 1, 2, 511, 512] + list(range(384, 512))


def _read_rows(x, power, gpu):
    """The rows SPECTRUM_ROWS of |STFT|^power at n_fft 1024 through one-hot launches (5 + 128 rows), held to float64 -> exp(out)."""
    mag = mel_ref.magnitudes(x, 1024, 256, 1024)
    l1 = mel_ref.frame_l1(x, 1024, 256, 1024)
    parts = []
    for rows in (SPECTRUM_ROWS[:5], SPECTRUM_ROWS[5:]):
        got = _run([x], 1024, 1024, mel_ref.one_hot(1024, rows), power, gpu)[0]
        _hold(got, mag[rows] ** power, l1, torch.ones(len(rows)), power, f"known spectrum, rows {rows[0]}..{rows[-1]}, power {power}")
        parts.append(got)
    return torch.exp(torch.cat(parts).double()), l1


@pytest.mark.parametrize("power", [1, 2])
def test_known_spectra(gpu, power):
    c = 2.0 ** -20 if power == 1 else 2.0 ** -19
    sum_w = 512.0                                                   # of the periodic Hann of 1024
    # (a) a constant: reflection repeats it, every frame has |X_0| = 0.25 sum(w), |X_1| = half of that, nothing at bins >= 2
    lin, l1 = _read_rows(torch.full((6000,), 0.25), power, gpu)
    absolute = c * l1 ** power
    assert l1.numel() == 24 and bool(((lin[0] - (0.25 * sum_w) ** power).abs() <= absolute + 2.0 ** -18 * lin[0]).all())
    assert bool((lin[2:] <= absolute + CLIP * (1 + 2.0 ** -18)).all())
    # (b) 0.25 (-1)^n, which reflection continues: all of it in bin 512, nothing in bin 0
    n = torch.arange(6000)
    lin, l1 = _read_rows(0.25 * (1 - 2 * (n % 2)).float(), power, gpu)
    absolute = c * l1 ** power
    assert bool(((lin[4] - (0.25 * sum_w) ** power).abs() <= absolute + 2.0 ** -18 * lin[4]).all())
    assert bool((lin[[0, 1, 2]] <= absolute + CLIP * (1 + 2.0 ** -18)).all())
    assert bool((lin[5:5 + 127] <= absolute + CLIP * (1 + 2.0 ** -18)).all())        # 384..510; bin 511 holds the window's side lobe
    # (c) a sine exactly on bin 450: the peak of the rows 384..511 in every frame without reflected samples
    x = (0.5 * torch.sin(2 * math.pi * 450 * torch.arange(4096, dtype=torch.float64) / 1024)).float()
    lin, l1 = _read_rows(x, power, gpu)
    assert l1.numel() == 17
    assert lin[5:, 2:15].argmax(0).tolist() == [450 - 384] * 13


@pytest.mark.parametrize("n_fft,n_mels,power", mel_ref.DENSE_CASES)
def test_dense_matrix_every_width(gpu, n_fft, n_mels, power):
    utts, mags, l1 = _batch(n_fft, n_fft)
    m = mel_ref.dense_matrix(n_mels, n_fft)
    outs = _run(utts, n_fft, n_fft, m, power, gpu)
    worst = 0.0
    for i, got in enumerate(outs):
        ratio = _hold(got, m.double() @ mags[i] ** power, l1[i], m.double().sum(1), power, f"dense {n_mels} x {n_fft // 2 + 1} power {power} N = {utts[i].numel()}")
        worst = max(worst, float(ratio.max()))
    print(f"dense {n_mels} x {n_fft // 2 + 1} power {power}: worst error / bound {worst:.3f}")
    assert worst > 0


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
@pytest.mark.parametrize("which", ["first", "last"])
def test_single_column_matrices(gpu, n_fft, which):
    utts, mags, l1 = _batch(n_fft, n_fft)
    m = mel_ref.single_column_matrix(33, n_fft, 0 if which == "first" else n_fft // 2)
    worst = 0.0
    for power in (1, 2):
        for i, got in enumerate(_run(utts, n_fft, n_fft, m, power, gpu)):
            ratio = _hold(got, m.double() @ mags[i] ** power, l1[i], m.double().sum(1), power, f"{which} column alone, n_fft {n_fft} power {power} N = {utts[i].numel()}")
            worst = max(worst, float(ratio.max()))
    print(f"{which} column alone, n_fft {n_fft}: worst error / bound {worst:.3f}")
    assert worst > 0


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_tile_paths_bitwise(gpu, n_fft):
    hop, ft = n_fft // 4, mel_ref.frames_per_tile(n_fft)
    utts, mags, l1 = _batch(n_fft, n_fft)
    m = mel_ref.dense_matrix(33, n_fft)
    batch = _run(utts, n_fft, n_fft, m, 1, gpu)
    for i, x in enumerate(utts):
        alone = _run([x], n_fft, n_fft, m, 1, gpu)[0]
        assert torch.equal(alone, batch[i]), f"utterance {i} (N = {x.numel()}) alone differs from its slice of the batch"
    rev = _run(utts[::-1], n_fft, n_fft, m, 1, gpu)[::-1]
    again = _run(utts, n_fft, n_fft, m, 1, gpu)
    for i in range(len(utts)):
        assert torch.equal(rev[i], batch[i]), f"utterance {i}, reversed order"
        assert torch.equal(again[i], batch[i]), f"utterance {i}, second run"
    # position in the tile: frame t of x and frame t - 1 of x[hop:] are the same samples, one column apart (FT - 1 | 0 and
    # 2 FT - 1 | 0 across the tile boundaries), wherever no sample is reflected
    n = (3 * ft + 2) * hop - 1
    x = mel_ref.noise(n)
    assert x.numel() == utts[-3].numel() and torch.equal(x, utts[-3])
    whole, late = batch[len(utts) - 3], _run([x[hop:]], n_fft, n_fft, m, 1, gpu)[0]
    # frame t covers x[t hop - n_fft/2, t hop + n_fft/2): inside [hop, n), so that x[hop:] does not reflect at its left edge either
    inside = [t for t in range(whole.shape[1]) if t * hop - n_fft // 2 >= hop and t * hop + n_fft // 2 <= n]
    assert inside == list(range(3, 3 * ft)) and late.shape[1] == whole.shape[1] - 1
    differ = [t for t in inside if not torch.equal(whole[:, t], late[:, t - 1])]
    assert not differ, f"n_fft {n_fft}: frames {differ} depend on their place in the tile"


GUARD, LEAD, SLACK, FRONT, BEHIND = 4, 5, 3, 7, 9


@functools.lru_cache(maxsize=None)
def _guarded(n_fft, win):
    """Five noise utterances around FT and 2 FT frames, the middle one NaN throughout, NaN samples in front of the first and
    behind the last; the output a window of a wider sentinel-filled buffer with guard rows, a lead and slack in every slot
    -> (utterances, the whole buffer on the host, the column of the window, frame offsets, n_mels)."""
    hop, ft = n_fft // 4, mel_ref.frames_per_tile(n_fft)
    lengths = [ft * hop - 1, ft * hop, 2 * ft * hop - 1, 2 * ft * hop, (ft - 1) * hop - 1]      # FT, FT + 1, 2 FT, 2 FT + 1, FT - 1 frames
    utts = [mel_ref.noise(n) for n in lengths]
    utts[2] = torch.full((lengths[2],), float("nan"))
    audio = torch.cat([torch.full((FRONT,), float("nan"))] + utts + [torch.full((BEHIND,), float("nan"))]).to(DEVICE)
    soff = _offsets(lengths, FRONT)
    frames = [n // hop + 1 for n in lengths]
    foff = _offsets([f + SLACK for f in frames], LEAD)
    m = mel_ref.dense_matrix(33, n_fft)
    col0, width = 6, foff[-1] + 11                                  # ld_out = the buffer's row: wider than the window, wider than the frames
    buf = torch.full((GUARD + 33 + GUARD, col0 + width + 8), SENTINEL, device=DEVICE)
    _launch(audio, soff, foff, n_fft, win, m, 1, buf[GUARD:GUARD + 33, col0:col0 + width])
    torch.cuda.synchronize()
    return utts, buf.cpu(), col0, foff, frames, m


@pytest.mark.parametrize("n_fft,win", [(1024, 1024), (2048, 2048), (1024, 800)])
def test_audio_outside_the_utterance_is_not_read(gpu, n_fft, win):
    utts, buf, col0, foff, frames, m = _guarded(n_fft, win)
    for i, x in enumerate(utts):
        got = buf[GUARD:GUARD + 33, col0 + foff[i]:col0 + foff[i] + frames[i]]
        if i == 2:
            continue
        # fmaxf(NaN, clip) = clip: a frame that read a NaN comes out as log(clip), finite, so it is the comparison that decides
        assert bool(torch.isfinite(got).all()), f"utterance {i}"
        assert torch.equal(got, _run([x], n_fft, win, m, 1, gpu)[0]), f"utterance {i} differs from the same utterance alone"


@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_output_outside_the_frames_is_not_written(gpu, n_fft):
    utts, buf, col0, foff, frames, m = _guarded(n_fft, n_fft)
    valid = torch.zeros_like(buf, dtype=torch.bool)
    for i, f in enumerate(frames):
        valid[GUARD:GUARD + 33, col0 + foff[i]:col0 + foff[i] + f] = True
    assert int(valid.sum()) == 33 * sum(frames)
    assert bool((buf[~valid] == SENTINEL).all()), f"{int((buf[~valid] != SENTINEL).sum())} elements outside the frames were written"
    assert not bool((buf[valid] == SENTINEL).any())
