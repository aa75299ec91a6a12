"""Host-side checks of the vocoder denoiser: the float64 restatement of tests/denoise_ref.py against torch.stft / torch.istft, the
inverse basis against the forward one, the plan of a ragged call (short utterances pass through), and the argument checks of
rtts_denoise and of the Python layers that need no GPU (no launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import denoise_ref

N_FFT, HOP = 1024, 256
ALL_CLAMP = 1e9                  # strength * bias above every |X| (at most sum(w) * peak = 512 * peak) for a bias >= 1e-3
LENGTHS = (513, 600, 1792, 1793, 7424, 7425, 8449)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    return _lib.load()


def _inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    x = (torch.rand(n, generator=g, dtype=torch.float64) - 0.5) * 0.8
    bias = torch.rand(N_FFT // 2 + 1, generator=g, dtype=torch.float64) * 0.5 + 1e-3
    return x, bias


def _torch_denoise(x, bias, strength):
    w = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    X = torch.stft(x, N_FFT, HOP, N_FFT, w, center=True, pad_mode="reflect", return_complex=True)
    mag = X.abs()
    g = torch.where(mag > 0, torch.clamp(mag - strength * bias[:, None], min=0) / torch.where(mag > 0, mag, torch.ones_like(mag)),
                    torch.zeros_like(mag))
    return torch.istft(X * g, N_FFT, HOP, N_FFT, w, center=True, length=x.numel())


@pytest.mark.parametrize("n", LENGTHS)
def test_restatement_matches_torch_stft_istft_in_float64(n):
    """1e-12: float64 sums of 1024 terms of size <= 1 carry about 1e-13."""
    x, bias = _inputs(n)
    for strength in (0.0, 0.1):
        got = denoise_ref.denoise_f64(x.numpy(), bias.numpy(), strength)
        want = _torch_denoise(x, bias, strength).numpy()
        err = float(np.abs(got - want).max())
        print(f"n {n} strength {strength}: restatement vs torch {err:.3e}; change of the signal {float(np.abs(want - x.numpy()).max()):.3e}")
        assert got.shape == (n,) and err <= 1e-12
        if strength == 0.0:
            assert float(np.abs(got - x.numpy()).max()) <= 1e-12
    got = denoise_ref.denoise_f64(x.numpy(), bias.numpy(), ALL_CLAMP)
    assert np.array_equal(got, np.zeros(n)), "every bin clamps: the output is exactly zero"
    assert bool((_torch_denoise(x, bias, ALL_CLAMP) == 0).all())


def test_f32_twin_is_close_to_the_restatement():
    """The float32 twin differs from float64 by f32 rounding only (the torch pair differs by 5e-8 .. 9e-8 at a peak of 0.4)."""
    from reformer_tts_amd.dataset.audio import dft_basis, idft_basis
    dft32, idft32 = dft_basis(N_FFT, N_FFT).numpy(), idft_basis(N_FFT, N_FFT).numpy()
    x, bias = _inputs(7425)
    for strength in (0.0, 0.1):
        want = denoise_ref.denoise_f64(x.numpy(), bias.numpy(), strength)
        got = denoise_ref.denoise_f32_twin(x.numpy(), bias.numpy(), strength, dft32, idft32)
        err = float(np.abs(got - want).max() / np.abs(x.numpy()).max())
        print(f"strength {strength}: f32 twin vs float64, relative to the peak: {err:.3e}")
        assert got.dtype == np.float32 and err <= 2e-6
    got = denoise_ref.denoise_f32_twin(x.numpy(), bias.numpy(), ALL_CLAMP, dft32, idft32)
    assert np.array_equal(got, np.zeros(7425, dtype=np.float32))


def test_inverse_basis_inverts_the_forward_basis():
    """dft_basis @ idft_basis = diag(w^2) in float64: analysis and synthesis window, and nothing else, to 1e-12."""
    from reformer_tts_amd.dataset.audio import dft_basis, hann_window, idft_basis
    d64, i64 = dft_basis(N_FFT, N_FFT, dtype=torch.float64), idft_basis(N_FFT, N_FFT, dtype=torch.float64)
    assert d64.dtype == torch.float64 and i64.dtype == torch.float64 and tuple(i64.shape) == (N_FFT, N_FFT)
    w = torch.from_numpy(hann_window(N_FFT, N_FFT))
    err = float((d64 @ i64 - torch.diag(w * w)).abs().max())
    print(f"dft_basis @ idft_basis - diag(w^2): {err:.3e}")
    assert err <= 1e-12
    # with the windows divided out where they are not zero: the identity
    nz = w > 0
    prod = (d64 @ i64)[nz][:, nz] / (w[nz, None] * w[None, nz])
    assert float((prod - torch.eye(int(nz.sum()), dtype=torch.float64)).abs().max()) <= 1e-9      # 1 / w^2 reaches 1e5 at the edges
    # the f32 matrices are the float64 ones rounded once, and the forward one is what the log-mel launch has always used
    d32, i32 = dft_basis(N_FFT, N_FFT), idft_basis(N_FFT, N_FFT)
    assert d32.dtype == torch.float32 and torch.equal(d32, d64.to(torch.float32)) and torch.equal(i32, i64.to(torch.float32))


def test_bias_magnitudes_of_frame_zero():
    from reformer_tts_amd.squeeze_wave.denoiser import first_frame_magnitudes
    x, _ = _inputs(88 * 256)
    got = first_frame_magnitudes(x).numpy()
    want = denoise_ref.first_frame_magnitudes_f64(x.numpy())
    w = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    ref = torch.stft(x, N_FFT, HOP, N_FFT, w, center=True, pad_mode="reflect", return_complex=True).abs()[:, 0].numpy()
    assert got.shape == (N_FFT // 2 + 1,)
    assert float(np.abs(got - want).max()) <= 1e-12 and float(np.abs(want - ref).max()) <= 1e-12


def test_plan_of_a_ragged_call():
    """Short utterances (<= n_fft / 2 samples) pass through as copies; the long ones between them are launched run by run."""
    from reformer_tts_amd.squeeze_wave.denoiser import DenoiseTables
    t = DenoiseTables([600, 1, 256, 7000, 513, 0, 512, 900], N_FFT, "cpu")
    assert t.sample_offsets == [0, 600, 601, 857, 7857, 8370, 8370, 8882, 9782]
    assert t.runs == [(0, 1), (3, 2), (7, 1)]
    assert t.copies == [(600, 857), (8370, 8882)]
    assert [list(h) for h in t.soff_host] == [[0, 600], [857, 7857, 8370], [8882, 9782]]
    only_short = DenoiseTables([0, 512, 3], N_FFT, "cpu")
    assert only_short.runs == [] and only_short.copies == [(0, 515)]
    assert DenoiseTables([0, 0], N_FFT, "cpu").copies == []
    with pytest.raises(ValueError):
        DenoiseTables([], N_FFT, "cpu")
    with pytest.raises(ValueError):
        DenoiseTables([600, -1], N_FFT, "cpu")


def _call(lib, *, n_fft=1024, hop=256, strength=0.1, lengths=(4096,), nseg=None, null=None, out=None):
    """rtts_denoise with dummy (never dereferenced) device pointers: every case here must be rejected before a launch."""
    soff = [0]
    for n in lengths:
        soff.append(soff[-1] + n)
    audio = 1 << 20
    args = dict(audio=audio, soff_h=(ctypes.c_int64 * len(soff))(*soff), soff=64, nseg=len(lengths) if nseg is None else nseg, dft=64,
                idft=64, bias=64, strength=strength, n_fft=n_fft, hop=hop, out=audio + 4 * soff[-1] if out is None else audio + 4 * out,
                stream=None)
    if null is not None:
        args[null] = None
    rc = lib.rtts_denoise(*args.values())
    return rc, lib.rtts_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(n_fft=512, hop=128), "n_fft"),
    (dict(n_fft=2048, hop=512), "n_fft"),
    (dict(hop=128), "hop"),
    (dict(hop=512), "hop"),
    (dict(strength=-0.1), "strength"),
    (dict(strength=float("nan")), "strength"),
    (dict(strength=float("inf")), "strength"),
    (dict(lengths=(4096, 512)), "reflect"),
    (dict(lengths=(0,)), "reflect"),
    (dict(nseg=0), "nseg"),
    (dict(nseg=65536), "nseg"),
    (dict(out=0), "overlap"),
    (dict(out=4095), "overlap"),
    (dict(out=-4095), "overlap"),
    (dict(null="audio"), "null"),
    (dict(null="soff_h"), "null"),
    (dict(null="soff"), "null"),
    (dict(null="dft"), "null"),
    (dict(null="idft"), "null"),
    (dict(null="bias"), "null"),
    (dict(null="out"), "null"),
])
def test_bad_arguments_are_rejected_without_a_launch(lib, kw, word):
    rc, msg = _call(lib, **kw)
    assert rc != 0
    assert "rtts_denoise" in msg and word in msg, msg


def test_header_declares_the_new_export(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rtts.h")).read()
    assert "rtts_denoise(" in text and hasattr(lib, "rtts_denoise")


def test_python_layers_refuse_by_name_off_the_gpu():
    from reformer_tts_amd import _lib, ops
    from reformer_tts_amd.squeeze_wave.denoiser import Denoiser
    bias = torch.rand(N_FFT // 2 + 1)
    d = Denoiser(bias_spec=bias)
    assert list(d.state_dict()) == ["bias_spec"] and torch.equal(d.bias_spec, bias)              # the bases are non-persistent
    with pytest.raises(_lib.RttsError, match="GPU only"):
        d([torch.zeros(4096)])
    with pytest.raises(_lib.RttsError, match="GPU only"):
        d.forward_packed(torch.zeros(4096), [4096])
    with pytest.raises(_lib.RttsError, match="GPU only"):
        ops.denoise(torch.zeros(4096), (ctypes.c_int64 * 2)(0, 4096), torch.zeros(2, dtype=torch.int64), 1, d.dft_basis, d.idft_basis,
                    d.bias_spec, 0.1, N_FFT, HOP, torch.zeros(4096))
    for kw in (dict(n_fft=512, win_length=512, hop_length=128), dict(n_fft=2048, win_length=2048, hop_length=512), dict(hop_length=128),
               dict(win_length=800)):
        with pytest.raises(ValueError, match="n_fft"):
            Denoiser(bias_spec=bias, **kw)
    with pytest.raises(ValueError, match="n_fft / 2 \\+ 1"):
        Denoiser(bias_spec=torch.rand(512))
    with pytest.raises(ValueError, match="vocoder or a bias_spec"):
        Denoiser()
