"""Host-side checks of Griffin-Lim vocoding: the float64 restatement of tests/griffin_lim_ref.py against torch.stft / torch.istft,
the momentum carried through the signal against the momentum carried through the spectrogram, the convergence condition of the GPU
suite asserted for the float32 twin, the offset tables, and the argument checks of the entry points and of the Python layers that
need no GPU (no launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import griffin_lim_ref as ref

N_FFT, HOP, BINS = 1024, 256, 513


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def creator():
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram
    return Tacotron2Spectrogram(22050, N_FFT, N_FFT, HOP, 80)


@pytest.fixture(scope="module")
def pinv(creator):
    from reformer_tts_amd.griffin_lim import mel_pseudo_inverse
    return mel_pseudo_inverse(creator.mel_basis).numpy()


def _magnitudes(creator, pinv, frames, seed):
    """M (bins, L + 1) float64 of the voiced test signal's own log-mel, through step 1 with the f32 pseudo-inverse."""
    x = ref.voiced_signal(HOP * max(frames, 3), seed)
    mel = ref.log_mel_f64(x, creator.mel_basis.numpy(), creator.power)[:, :frames].astype(np.float32)
    return ref.magnitudes_f64(mel, pinv, creator.power)[1]


def _torch_griffin_lim(mag, n_iter, momentum, phase, seed):
    """torchaudio's loop (functional.griffinlim) in float64 with the start phases of the definition: the previous rebuilt
    spectrogram is kept, angles = rebuilt - momentum / (1 + momentum) * previous, normalised (1 where it is zero)."""
    m = torch.from_numpy(np.asarray(mag, dtype=np.float64))                           # (bins, T)
    n = HOP * (m.shape[1] - 1)
    w = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    phi = torch.from_numpy(ref.phases(phase, seed, m.shape[1]).T)
    beta = momentum / (1.0 + momentum)
    xs = [torch.istft(torch.polar(m, phi), N_FFT, HOP, N_FFT, w, center=True, length=n)]
    prev = None
    for _ in range(n_iter):
        c = torch.stft(xs[-1], N_FFT, HOP, N_FFT, w, center=True, pad_mode="reflect", return_complex=True)
        r = c if prev is None else c - beta * prev
        prev = c
        a = r.abs()
        unit = torch.where(a > 0, r / torch.where(a > 0, a, torch.ones_like(a)), torch.ones_like(r))
        xs.append(torch.istft(m * unit, N_FFT, HOP, N_FFT, w, center=True, length=n))
    return [x.numpy() for x in xs]


@pytest.mark.parametrize("frames", [3, 4, 30, 61])
def test_restatement_matches_torch_stft_istft_in_float64(creator, pinv, frames):
    """1e-10 (the issue's bound): float64 sums of 1024 terms carry about 1e-13; four iterations amplify it a little."""
    mag = _magnitudes(creator, pinv, frames, 100 + frames)
    for phase, momentum in (("hash", 0.99), ("hash", 0.0), ("zero", 0.99)):
        got = ref.griffin_lim_f64(mag, 4, momentum, phase, seed=7)
        want = _torch_griffin_lim(mag, 4, momentum, phase, seed=7)
        peak = max(float(np.abs(w).max()) for w in want)
        err = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
        print(f"L {frames} {phase} momentum {momentum}: restatement vs torch over x_0..x_4 {err:.3e} (peak {peak:.3e})")
        assert all(g.shape == (HOP * frames,) for g in got) and peak > 1e-3
        assert err <= 1e-10


def test_hash_phases_follow_the_counter_hash():
    from edges_ref import drop_hash
    phi = ref.phases("hash", 5, 4)
    assert phi.shape == (4, BINS) and float(phi.min()) >= 0.0 and float(phi.max()) < 2 * np.pi
    for t, k in ((0, 0), (0, 512), (1, 0), (3, 17)):
        h = int(drop_hash(5, np.array([t * BINS + k], dtype=np.uint64))[0])
        assert phi[t, k] == 2.0 * np.pi * (h >> 8) / 2.0 ** 24
    assert not np.array_equal(phi, ref.phases("hash", 6, 4))
    assert np.array_equal(ref.phases("hash", 5, 3), phi[:3]), "the phases of a frame depend on its own index only"
    assert not ref.phases("zero", 5, 4).any()


@pytest.mark.parametrize("frames", [4, 30, 61])
def test_momentum_through_the_signal_equals_the_spectrogram_form(creator, pinv, frames):
    """STFT(x_k) - beta STFT(x_{k-1}) = STFT(x_k - beta x_{k-1}): 1e-12 over eight iterations."""
    mag = _magnitudes(creator, pinv, frames, 200 + frames)
    a = ref.griffin_lim_f64(mag, 8, 0.99)
    b = ref.griffin_lim_spectrogram_form_f64(mag, 8, 0.99)
    err = max(float(np.abs(x - y).max()) for x, y in zip(a, b))
    print(f"L {frames}: signal form vs spectrogram form {err:.3e}")
    assert err <= 1e-12
    assert float(np.abs(a[8] - ref.griffin_lim_f64(mag, 8, 0.0)[8]).max()) > 1e-4, "the momentum term is seen"


def test_short_utterances_are_zeros_and_zero_input_returns_istft_of_m(creator, pinv):
    for frames in (0, 1, 2):
        mag = np.ones((BINS, frames + 1))
        assert np.array_equal(ref.init_f64(mag), np.zeros(HOP * frames))
        assert np.array_equal(ref.step_f64(mag, np.ones(HOP * frames)), np.zeros(HOP * frames))
    mag = _magnitudes(creator, pinv, 5, 1)
    assert np.array_equal(ref.step_f64(mag, np.zeros(HOP * 5)), ref.init_f64(mag, "zero"))


@pytest.mark.parametrize("frames", [30, 61])
def test_convergence_condition_holds_for_the_f32_twin(creator, pinv, frames):
    """The condition of the GPU suite: 32 iterations in f32 lose to 16 in float64 only if a step is wrong."""
    from reformer_tts_amd.dataset.audio import dft_basis, idft_basis
    dft32, idft32 = dft_basis(N_FFT, N_FFT).numpy(), idft_basis(N_FFT, N_FFT).numpy()
    mag = _magnitudes(creator, pinv, frames, frames).astype(np.float32)
    for momentum in (0.0, 0.99):
        truth = ref.griffin_lim_f64(mag, 16, momentum, "hash", 3)
        twin = ref.griffin_lim_f32_twin(mag, 32, momentum, dft32, idft32, "hash", 3)
        d0, d16, d32 = ref.spectral_error(truth[0], mag), ref.spectral_error(truth[16], mag), ref.spectral_error(twin[32], mag)
        print(f"L {frames} momentum {momentum}: d_0 {d0:.4f}, float64 d_16 {d16:.4f}, twin d_32 {d32:.4f}")
        assert twin[32].dtype == np.float32 and d32 <= d16 < d0
        # the twin starts where the truth starts, and stays close for the first iterations
        for k, tol in ((0, 5e-6), (1, 1e-5), (4, 5e-5)):
            assert float(np.abs(twin[k] - truth[k]).max() / np.abs(truth[k]).max()) <= tol, k


def test_magnitudes_clamp_and_repeat_the_last_column(creator, pinv):
    g = torch.Generator().manual_seed(3)
    mel = (torch.randn(80, 6, generator=g) * 2 - 5).numpy()
    for power in (1, 2):
        a, m = ref.magnitudes_f64(mel, pinv, power)
        assert a.shape == m.shape == (BINS, 7) and np.array_equal(m[:, 6], m[:, 5]) and float(m.min()) == 0.0
        assert np.allclose(m ** power, a, rtol=1e-12, atol=0)
        assert (pinv.astype(np.float64) @ np.exp(mel)).min() < 0, "a random mel makes the pseudo-inverse overshoot: the clamp is seen"
        twin = ref.magnitudes_f32_twin(mel.astype(np.float32), pinv, power)
        a32, _ = ref.magnitudes_f64(mel.astype(np.float32), pinv, power)
        assert bool((np.abs(twin.astype(np.float64) ** power - a32) <= ref.magnitude_bound(mel.astype(np.float32), pinv) + 4 * 2.0 ** -24 * a32).all())


def test_tables_follow_the_mel_tables():
    """Column offsets = the frame offsets a MelTables gives for lengths 256 L (n // hop + 1 frames each: rtts_mel_frames)."""
    from reformer_tts_amd.dataset.audio import _offsets, mel_frames
    from reformer_tts_amd.griffin_lim import GriffinLimTables
    frames = [1, 2, 3, 4, 27, 28, 29, 30, 31, 59, 60, 61, 0]
    t = GriffinLimTables(frames, "cpu")
    assert t.lengths == [HOP * n for n in frames]
    assert t.sample_offsets == _offsets(t.lengths)
    assert t.col_offsets == _offsets([mel_frames(n, HOP) if n else 1 for n in t.lengths])      # an empty utterance: one (zero) column
    assert t.mel_offsets == _offsets(frames)
    assert list(t.soff_host) == t.sample_offsets and list(t.coff_host) == t.col_offsets
    assert t.device_table.dtype == torch.int64 and t.device_table.tolist() == [t.sample_offsets, t.col_offsets, t.mel_offsets, [0] * 14]
    for bad in ([], [3, -1]):
        with pytest.raises(ValueError):
            GriffinLimTables(bad, "cpu")


def _tables(frames):
    soff, coff = [0], [0]
    for n in frames:
        soff.append(soff[-1] + HOP * n)
        coff.append(coff[-1] + n + 1)
    return soff, coff


def _arr(values):
    return (ctypes.c_int64 * len(values))(*values)


def _call_step(lib, *, entry="rtts_gl_step", n_fft=N_FFT, hop=HOP, beta=0.5, frames=(16,), nseg=None, null=None, out=None, prev=None,
               soff=None, coff=None, ld_mag=None, phase=1):
    """rtts_gl_step / rtts_gl_init with dummy (never dereferenced) device pointers: every case here must be rejected before a launch."""
    s, c = _tables(frames)
    soff, coff = soff or s, coff or c
    cur = 1 << 20
    far = cur + 64 * soff[-1]
    args = dict(cur=cur, prev=None if prev is None else cur + 4 * prev, beta=beta, mag=64, ld_mag=coff[-1] if ld_mag is None else ld_mag,
                coff_h=_arr(coff), coff=64, soff_h=_arr(soff), soff=64, nseg=len(frames) if nseg is None else nseg, dft=64, idft=64,
                n_fft=n_fft, hop=hop, out=far if out is None else cur + 4 * out, stream=None)
    if entry == "rtts_gl_init":
        args = dict(mag=64, ld_mag=args["ld_mag"], coff_h=args["coff_h"], coff=64, soff_h=args["soff_h"], soff=64, nseg=args["nseg"], dft=64,
                    idft=64, phase=phase, seed=0, n_fft=n_fft, hop=hop, out=far, stream=None)
    if null is not None:
        args[null] = None
    rc = getattr(lib, entry)(*args.values())
    return rc, lib.rtts_last_error().decode()


@pytest.mark.parametrize("entry", ["rtts_gl_step", "rtts_gl_init"])
@pytest.mark.parametrize("kw,word", [
    (dict(n_fft=512, hop=128), "n_fft"),
    (dict(n_fft=2048, hop=512), "n_fft"),
    (dict(hop=128), "hop"),
    (dict(hop=512), "hop"),
    (dict(nseg=0), "nseg"),
    (dict(nseg=65536), "nseg"),
    (dict(soff=[0, 4097]), "sample_offsets"),
    (dict(soff=[0, -256]), "sample_offsets"),
    (dict(coff=[0, 16]), "col_offsets"),
    (dict(soff=[-256, 3840]), "negative"),
    (dict(ld_mag=16), "ld_mag"),
    (dict(null="mag"), "null"),
    (dict(null="coff_h"), "null"),
    (dict(null="coff"), "null"),
    (dict(null="soff_h"), "null"),
    (dict(null="soff"), "null"),
    (dict(null="dft"), "null"),
    (dict(null="idft"), "null"),
    (dict(null="out"), "null"),
])
def test_bad_arguments_are_rejected_without_a_launch(lib, entry, kw, word):
    rc, msg = _call_step(lib, entry=entry, **kw)
    assert rc != 0
    assert entry in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(out=0), "overlap cur"),
    (dict(out=4095), "overlap cur"),
    (dict(out=-4095), "overlap cur"),
    (dict(prev=8192, out=8192 + 100), "overlap prev"),
    (dict(prev=8192, out=8192 - 4095), "overlap prev"),
    (dict(beta=-0.1), "beta"),
    (dict(beta=1.0), "beta"),
    (dict(beta=float("nan")), "beta"),
    (dict(null="cur"), "null"),
])
def test_step_refuses_overlap_and_bad_beta(lib, kw, word):
    rc, msg = _call_step(lib, **kw)
    assert rc != 0
    assert "rtts_gl_step" in msg and word in msg, msg


def test_init_refuses_an_unknown_phase(lib):
    rc, msg = _call_step(lib, entry="rtts_gl_init", phase=2)
    assert rc != 0 and "rtts_gl_init" in msg and "phase" in msg


@pytest.mark.parametrize("kw,word", [
    (dict(n_fft=512), "n_fft"),
    (dict(nseg=0), "nseg"),
    (dict(n_mels=0), "n_mels"),
    (dict(n_mels=129), "n_mels"),
    (dict(power=3), "power"),
    (dict(power=0), "power"),
    (dict(coff=[0, 0]), "col_offsets"),
    (dict(coff=[-1, 16]), "col_offsets"),
    (dict(ld_mag=16), "ld_mag"),
    (dict(null="mel"), "null"),
    (dict(null="mel_start"), "null"),
    (dict(null="coff_h"), "null"),
    (dict(null="coff"), "null"),
    (dict(null="pinv"), "null"),
    (dict(null="mag"), "null"),
])
def test_magnitudes_rejects_bad_arguments_without_a_launch(lib, kw, word):
    kw = dict(kw)
    coff = kw.pop("coff", [0, 17])
    null = kw.pop("null", None)
    args = dict(mel=64, sb=0, sc=16, st=1, mel_start=64, coff_h=_arr(coff), coff=64, nseg=kw.pop("nseg", 1), pinv=64, n_mels=kw.pop("n_mels", 80),
                power=kw.pop("power", 1), n_fft=kw.pop("n_fft", N_FFT), mag=64, ld_mag=kw.pop("ld_mag", 17), stream=None)
    assert not kw
    if null is not None:
        args[null] = None
    rc = lib.rtts_gl_magnitudes(*args.values())
    msg = lib.rtts_last_error().decode()
    assert rc != 0 and "rtts_gl_magnitudes" in msg and word in msg, msg


def test_header_declares_the_new_exports(lib):
    from reformer_tts_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rtts.h")).read()
    for name in ("rtts_gl_magnitudes", "rtts_gl_init", "rtts_gl_step"):
        assert name + "(" in text and hasattr(lib, name) and name in _lib.SIGNATURES


def test_python_layers_refuse_by_name_off_the_gpu(creator):
    from reformer_tts_amd import _lib, ops, synthesis
    from reformer_tts_amd.dataset.audio import MelSpectrogram, Tacotron2Spectrogram
    from reformer_tts_amd.griffin_lim import GriffinLim, GriffinLimTables
    assert synthesis.GriffinLim is GriffinLim and synthesis.GriffinLimTables is GriffinLimTables
    gl = GriffinLim(creator)
    assert (gl.n_iter, gl.momentum, gl.phase, gl.seed, gl.power) == (32, 0.99, "hash", 0, 1) and list(gl.state_dict()) == []
    assert GriffinLim(MelSpectrogram(22050, N_FFT, N_FFT, HOP, 80)).power == 2
    assert tuple(gl.pinv.shape) == (BINS, 80) and gl.pinv.dtype == torch.float32
    want = torch.linalg.pinv(creator.mel_basis.double())
    assert torch.equal(gl.pinv, want.to(torch.float32)), "float64 on the host, rounded once"
    assert float((creator.mel_basis.double() @ want - torch.eye(80, dtype=torch.float64)).abs().max()) <= 1e-9
    mel = torch.zeros(1, 80, 8)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        gl(mel, [8])
    with pytest.raises(_lib.RttsError, match="GPU only"):
        gl.forward_packed(mel, [8])
    with pytest.raises(_lib.RttsError, match="GPU only"):
        gl.infer_ragged(mel, [8])
    with pytest.raises(ValueError, match="noise"):
        gl.infer_ragged(mel, [8], noise=[[torch.zeros(1)]])
    t = GriffinLimTables([8], "cpu")
    mag, audio = torch.zeros(BINS, 9), torch.zeros(2048)
    with pytest.raises(_lib.RttsError, match="GPU only: mel"):
        ops.gl_magnitudes(mel, [0], t.device_table[3], t.coff_host, t.device_table[:2], 1, gl.pinv, 1, N_FFT, mag)
    with pytest.raises(_lib.RttsError, match="GPU only: mag"):
        ops.gl_init(mag, t.coff_host, t.soff_host, t.device_table[:2], 1, gl.dft_basis, gl.idft_basis, "hash", 0, N_FFT, HOP, audio)
    with pytest.raises(_lib.RttsError, match="GPU only: cur"):
        ops.gl_step(audio, None, 0.0, mag, t.coff_host, t.soff_host, t.device_table[:2], 1, gl.dft_basis, gl.idft_basis, N_FFT, HOP, audio)
    with pytest.raises(ValueError, match="phase"):
        ops.gl_init(mag, t.coff_host, t.soff_host, t.device_table[:2], 1, gl.dft_basis, gl.idft_basis, "random", 0, N_FFT, HOP, audio)
    for bad in (Tacotron2Spectrogram(22050, 512, 512, 128, 80), Tacotron2Spectrogram(22050, 2048, 2048, 512, 80),
                Tacotron2Spectrogram(22050, N_FFT, 800, HOP, 80)):
        with pytest.raises(ValueError, match="creator: supported are n_fft"):
            GriffinLim(bad)
    for kw, word in ((dict(n_iter=-1), "n_iter"), (dict(momentum=1.0), "momentum"), (dict(momentum=-0.1), "momentum"), (dict(phase="random"), "phase")):
        with pytest.raises(ValueError, match=word):
            GriffinLim(creator, **kw)
