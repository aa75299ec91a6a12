"""Why tests/test_mel_bins_hip.py exists, and that its inputs are read the right way, without a GPU.

The product's own filter banks (22,050 Hz, 0 - 8000 Hz) give bin 0 and every bin above 8 kHz a zero weight: of the n_fft/2 + 1 bins
of rtts_mel_spectrogram, the tests that go through those banks observe 1..371 (n_fft 1024), 1..185 (512) and 1..743 (2048) and
nothing else.  ``test_product_banks_leave_bins_unobserved`` pins that down, so a change of ``f_max`` shows up here; the rest checks
the inputs test_mel_bins_hip.py builds instead (one-hot groups that cover every bin once, dense matrices without a zero column),
and holds a float32 restatement of the kernel (``mel_ref.log_mel_f32``: frames @ dft_basis, column n_fft/2 read as the Nyquist
bin) to the float64 oracle on those inputs under the criterion of tests/test_mel_hip.py, so that a wrong reading of the basis
layout in the tests fails here.  Worst error / bound of that twin, as printed: 0.05 - 0.14 per bin at power 1 (it moves with the
host's matrix product: its summation order is not the kernel's), 0.01 - 0.03 at power 2, 0.03 - 0.05 through the dense matrices;
``0 < ratio < 0.5`` is asserted, which a vacuous bound fails as well."""
import functools

import pytest
import torch

import mel_ref


@functools.lru_cache(maxsize=None)
def _basis(n_fft, win):
    from reformer_tts_amd.dataset.audio import dft_basis
    return dft_basis(n_fft, win)


@functools.lru_cache(maxsize=None)
def _batch(n_fft, win):
    """The 14 utterances of tile_lengths with their float64 magnitudes and frame scales."""
    hop = n_fft // 4
    utts = [mel_ref.noise(n) for n in mel_ref.tile_lengths(n_fft)]
    return utts, [mel_ref.magnitudes(x, n_fft, hop, win) for x in utts], [mel_ref.frame_l1(x, n_fft, hop, win) for x in utts]


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_one_hot_groups_cover_every_bin_once(n_fft):
    groups = mel_ref.one_hot_groups(n_fft)
    assert all(1 <= rows <= 128 for _, rows in groups) and groups[-1] == (n_fft // 2, 1)
    total = torch.zeros(n_fft // 2 + 1)
    for first, rows in groups:
        m = mel_ref.one_hot(n_fft, range(first, first + rows))
        assert tuple(m.shape) == (rows, n_fft // 2 + 1) and bool((m.sum(1) == 1).all())
        total += m.sum(0)
    assert bool((total == 1).all())


def test_tile_lengths_hit_both_ends_of_every_frame_count():
    for n_fft in (512, 1024, 2048):
        hop, ft = n_fft // 4, mel_ref.frames_per_tile(n_fft)
        lengths = mel_ref.tile_lengths(n_fft)
        frames = [n // hop + 1 for n in lengths]
        assert len(lengths) == 14 and min(lengths) > n_fft // 2
        assert sorted(set(frames)) == [3, ft - 1, ft, ft + 1, 2 * ft, 2 * ft + 1, 3 * ft + 2]
        assert frames[-4:] == [3 * ft + 2, 3 * ft + 2, 3, 3]          # the short ones follow the longest
        for f in set(frames) - {3}:
            assert sorted(n for n in lengths if n // hop + 1 == f) == [(f - 1) * hop, f * hop - 1]


def test_dense_matrices_have_no_zero_column():
    for n_fft, n_mels, _ in mel_ref.DENSE_CASES:
        m = mel_ref.dense_matrix(n_mels, n_fft)
        assert m.dtype == torch.float32 and tuple(m.shape) == (n_mels, n_fft // 2 + 1)
        assert bool((m > 0).any(0).all()), (n_fft, n_mels)
    last = mel_ref.single_column_matrix(33, 1024, 512)
    assert bool((last[:, 512] > 0).all()) and float(last[:, :512].abs().max()) == 0.0


@pytest.mark.parametrize("kind,n_fft,n_mels,last", [("mel", 1024, 80, 371), ("taco", 512, 40, 185), ("taco", 2048, 128, 743),
                                                    ("taco", 1024, 80, 371)])
def test_product_banks_leave_bins_unobserved(kind, n_fft, n_mels, last):
    """The reason this file and test_mel_bins_hip.py exist: through the product's banks no test sees bin 0 or a bin above ``last``."""
    from reformer_tts_amd.dataset.audio import mel_filterbank
    scale, norm = ("slaney", "slaney") if kind == "taco" else ("htk", None)
    fb = mel_filterbank(22050, n_fft, n_mels, 0.0, 8000.0, scale, norm).float()
    seen = (fb != 0).any(0)
    assert not bool(seen[0]) and bool(seen[1:last + 1].all()) and not bool(seen[last + 1:].any())
    assert last < n_fft // 2 - n_fft // 8                           # the last wave's bins (and more) are among the unobserved


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("n_fft,win", mel_ref.SIZES)
def test_f32_twin_meets_the_criterion_per_bin(n_fft, win, power):
    hop = n_fft // 4
    utts, mags, l1 = _batch(n_fft, win)
    basis = _basis(n_fft, win)
    worst, below, total = 0.0, 0, 0
    for x, mag, scale in zip(utts, mags, l1):
        tw = mel_ref.twin_magnitudes(x, basis, n_fft, hop, power)
        for first, rows in mel_ref.one_hot_groups(n_fft):
            got = mel_ref.twin_log_mel(tw, mel_ref.one_hot(n_fft, range(first, first + rows)))
            ref = mag[first:first + rows] ** power
            assert float(got.abs().max()) < 16
            worst = max(worst, float(mel_ref.error_over_bound(got, ref, scale, torch.ones(rows), power).max()))
            below += int((ref < mel_ref.CLIP).sum())
            total += ref.numel()
    print(f"f32 twin per bin, n_fft {n_fft} win {win} power {power}: worst error / bound {worst:.3f}; {below} of {total} references below the clip")
    assert 0 < worst < 0.5
    assert below <= 0.001 * total


@pytest.mark.parametrize("n_fft,n_mels,power", mel_ref.DENSE_CASES)
def test_f32_twin_meets_the_criterion_through_dense_matrices(n_fft, n_mels, power):
    hop = n_fft // 4
    utts, mags, l1 = _batch(n_fft, n_fft)
    m = mel_ref.dense_matrix(n_mels, n_fft)
    worst = 0.0
    for x, mag, scale in zip(utts, mags, l1):
        got = mel_ref.log_mel_f32(x, _basis(n_fft, n_fft), m, n_fft, hop, power)
        assert float(got.abs().max()) < 16
        worst = max(worst, float(mel_ref.error_over_bound(got, m.double() @ mag ** power, scale, m.double().sum(1), power).max()))
    print(f"f32 twin, dense {n_mels} x {n_fft // 2 + 1} power {power}: worst error / bound {worst:.3f}")
    assert 0 < worst < 0.5
