"""Host-side checks of the audio -> log-mel path: the mel filter bank against the float64 restatement of tests/mel_ref.py,
the frame count and the argument checks of the C ABI (no launch, no GPU), and the WAV reader."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

import mel_ref

CONFIG = (22050, 1024, 80, 0.0, 8000.0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("scale,norm", [("slaney", "slaney"), ("htk", None)])
@pytest.mark.parametrize("n_fft,n_mels", [(1024, 80), (512, 40), (2048, 128)])
def test_filterbank_matches_the_restatement(scale, norm, n_fft, n_mels):
    from reformer_tts_amd.dataset.audio import mel_filterbank
    got = mel_filterbank(22050, n_fft, n_mels, 0.0, 8000.0, scale, norm)
    want = mel_ref.filterbank(22050, n_fft, n_mels, 0.0, 8000.0, scale, norm)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n_mels, n_fft // 2 + 1)
    err = float((got - want).abs().max())
    print(f"filterbank {scale}/{norm} n_fft {n_fft}: max abs difference {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("scale,norm", [("slaney", "slaney"), ("htk", None)])
def test_filterbank_shape_properties_at_the_config(scale, norm):
    from reformer_tts_amd.dataset.audio import mel_filterbank
    sr, n_fft, n_mels, f_min, f_max = CONFIG
    fb = mel_filterbank(sr, n_fft, n_mels, f_min, f_max, scale, norm)
    assert int((fb.sum(1) == 0).sum()) == 0, "empty filters"
    assert float(fb.min()) >= 0.0
    freqs = torch.linspace(0, sr / 2, n_fft // 2 + 1, dtype=torch.float64)
    assert float(fb[:, freqs > f_max].abs().max()) == 0.0
    for m in range(n_mels):                                        # unimodal: non-decreasing up to the peak, non-increasing after it
        row = fb[m]
        peak = int(row.argmax())
        assert bool((row[1:peak + 1] >= row[:peak]).all()) and bool((row[peak + 1:] <= row[peak:-1]).all()), m


def test_filterbank_rejects_unknown_options():
    from reformer_tts_amd.dataset.audio import mel_filterbank
    with pytest.raises(ValueError):
        mel_filterbank(22050, 1024, 80, 0.0, 8000.0, "bark", None)
    with pytest.raises(ValueError):
        mel_filterbank(22050, 1024, 80, 0.0, 8000.0, "htk", "area")


@pytest.mark.parametrize("n", [513, 1000, 8192, 8465])
def test_frame_count(lib, n):
    from reformer_tts_amd.dataset.audio import mel_frames
    assert lib.rtts_mel_frames(n, 256) == n // 256 + 1
    assert mel_frames(n, 256) == n // 256 + 1


def _call(lib, *, n_fft=1024, hop=256, n_mels=80, power=1, clip=1e-5, lengths=(4096,), nseg=None, null=None):
    """rtts_mel_spectrogram with dummy (never dereferenced) device pointers: every case here must be rejected before a launch."""
    hop_f = max(hop, 1)
    soff, foff = [0], [0]
    for n in lengths:
        soff.append(soff[-1] + n)
        foff.append(foff[-1] + n // hop_f + 1)
    n1 = len(lengths) + 1
    args = dict(audio=64, soff_h=(ctypes.c_int64 * n1)(*soff), foff_h=(ctypes.c_int64 * n1)(*foff), soff=64, foff=64,
                nseg=len(lengths) if nseg is None else nseg, dft=64, mel=64, n_fft=n_fft, hop=hop, n_mels=n_mels, power=power, clip=clip,
                out=64, ld_out=foff[-1], stream=None)
    if null is not None:
        args[null] = None
    rc = lib.rtts_mel_spectrogram(*args.values())
    return rc, lib.rtts_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(n_fft=768, hop=192), "n_fft"),
    (dict(hop=128), "hop"),
    (dict(hop=512), "hop"),
    (dict(n_mels=129), "n_mels"),
    (dict(n_mels=0), "n_mels"),
    (dict(power=3), "power"),
    (dict(clip=0.0), "clip"),
    (dict(lengths=(4096, 512)), "reflect"),
    (dict(n_fft=512, hop=128, lengths=(256,)), "reflect"),
    (dict(nseg=0), "nseg"),
    (dict(null="audio"), "null"),
    (dict(null="soff_h"), "null"),
    (dict(null="foff"), "null"),
    (dict(null="dft"), "null"),
    (dict(null="mel"), "null"),
    (dict(null="out"), "null"),
])
def test_bad_arguments_are_rejected_without_a_launch(lib, kw, word):
    rc, msg = _call(lib, **kw)
    assert rc != 0
    assert "rtts_mel_spectrogram" in msg and word in msg, msg


def test_frame_count_rejects_nonsense(lib):
    assert lib.rtts_mel_frames(0, 256) < 0 and "rtts_mel_frames" in lib.rtts_last_error().decode()
    assert lib.rtts_mel_frames(1000, 0) < 0


def test_header_declares_the_new_exports(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rtts.h")).read()
    for name in ("rtts_mel_frames", "rtts_mel_spectrogram"):
        assert f"{name}(" in text and hasattr(lib, name)


def _write_wav(path, pcm: np.ndarray, width: int, channels: int, rate: int = 22050):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())


def test_wav_reader_scales_pcm16_exactly(tmp_path):
    from reformer_tts_amd.dataset.audio import read_wav
    pcm = np.concatenate([np.array([-32768, -1, 0, 1, 32767], dtype="<i2"),
                          np.random.RandomState(0).randint(-32768, 32768, 1000).astype("<i2")])
    _write_wav(tmp_path / "a.wav", pcm, 2, 1)
    x, rate = read_wav(tmp_path / "a.wav")
    assert rate == 22050 and x.dtype == torch.float32
    assert np.array_equal(x.numpy(), pcm.astype(np.float32) / np.float32(32768.0))


def test_wav_reader_refuses_other_encodings(tmp_path):
    from reformer_tts_amd.dataset.audio import read_wav
    _write_wav(tmp_path / "u8.wav", np.arange(100, dtype=np.uint8), 1, 1)
    _write_wav(tmp_path / "stereo.wav", np.zeros(200, dtype="<i2"), 2, 2)
    for name in ("u8.wav", "stereo.wav"):
        with pytest.raises(ValueError, match="16-bit PCM mono"):
            read_wav(tmp_path / name)


def test_creators_refuse_to_run_off_the_gpu():
    from reformer_tts_amd import _lib
    from reformer_tts_amd.dataset.audio import MelSpectrogram, Tacotron2Spectrogram
    for cls in (Tacotron2Spectrogram, MelSpectrogram):
        creator = cls(22050, 1024, 1024, 256, 80)
        assert not any(k in creator.state_dict() for k in ("dft_basis", "mel_basis"))     # non-persistent buffers
        with pytest.raises(_lib.RttsError, match="GPU only"):
            creator([torch.zeros(4096)])
    with pytest.raises(ValueError, match="n_fft"):
        Tacotron2Spectrogram(22050, 768, 768, 192, 80)


def test_wav_info_reads_the_header_and_the_rate_is_checked(tmp_path):
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram, wav_info
    _write_wav(tmp_path / "a.wav", np.zeros(1234, dtype="<i2"), 2, 1, rate=16000)
    assert wav_info(tmp_path / "a.wav") == (1234, 16000)
    _write_wav(tmp_path / "u8.wav", np.arange(100, dtype=np.uint8), 1, 1)
    with pytest.raises(ValueError, match="16-bit PCM mono"):
        wav_info(tmp_path / "u8.wav")
    creator = Tacotron2Spectrogram(22050, 1024, 1024, 256, 80)
    with pytest.raises(ValueError, match="sample rate 16000"):
        creator._check_rate(16000, "a.wav")
    creator._check_rate(22050, "a.wav")
