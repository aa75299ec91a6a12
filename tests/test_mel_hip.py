"""rtts_mel_spectrogram (csrc/mel.hip) and the modules of reformer_tts_amd/dataset/audio.py on the GPU, against the float64
restatement of tests/mel_ref.py (torch.stft, an FFT, and a filter bank of its own).

Criterion, per output element, with L1_t = sum_n |x_n w_n| of frame t and S_m = sum_k M[m, k]:
    |exp(out) - ref| <= 2^-20 * L1_t^power * S_m * power + 2^-18 * ref,        ref clamped at clip
(power 1: 2^-20 L1 S; power 2: 2^-19 L1^2 S).  A float32 k-ordered DFT chain errs by a few 1e-8 of L1 per bin (measured on the
CPU against the same oracle: 1.4e-8 for an FFT, 3.6e-8 for a blocked DFT-GEMM), so 2^-20 ~ 9.5e-7 leaves about 25x, four orders
of magnitude below the median signal (0.037 of L1 S): a wrong bin, window, reflection or offset cannot hide.  The relative term
is the spacing of the stored f32 log (2^-20 near -11.5).
The banks used here weigh bin 0 and the bins above 8 kHz with zero: tests/test_mel_bins_hip.py reads every bin, tile path and mel width."""
import math
import os

import numpy as np
import pytest
import torch

import mel_ref

pytestmark = pytest.mark.gpu

SR = 22050
LOG_CLIP = float(np.float32(math.log(float(np.float32(1e-5)))))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _noise(n, seed):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) - 0.5


def _chirp(n, f0=50.0, f1=10000.0):
    t = torch.arange(n, dtype=torch.float64) / SR
    dur = n / SR
    return (0.5 * torch.sin(2 * math.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t))).float()


def _case1_utterances():
    return [_noise(513, 1), _noise(1000, 2), _noise(8192, 3), _noise(8465, 4), _chirp(16384), torch.zeros(4096)]


def _creator(kind, n_fft, win, n_mels, gpu):
    from reformer_tts_amd.dataset.audio import MelSpectrogram, Tacotron2Spectrogram
    cls = Tacotron2Spectrogram if kind == "taco" else MelSpectrogram
    return cls(SR, n_fft, win, n_fft // 4, n_mels).to(gpu)


def _ref_fb(kind, n_fft, n_mels):
    scale, norm = ("slaney", "slaney") if kind == "taco" else ("htk", None)
    return mel_ref.filterbank(SR, n_fft, n_mels, 0.0, 8000.0, scale, norm)


def _check_parity(got_log, x, fb, n_fft, win, power, tag):
    """got_log (n_mels, T) f32 from the device against the oracle under the module docstring's criterion -> worst error as a
    multiple of the absolute scale L1^power * S (the whole error, the part the relative term covers included)."""
    hop = n_fft // 4
    ref = mel_ref.mel_linear(x, fb, n_fft, hop, win, power)
    assert tuple(got_log.shape) == tuple(ref.shape), (tag, got_log.shape, ref.shape)
    l1 = mel_ref.frame_l1(x, n_fft, hop, win)
    scale = fb.sum(1)[:, None] * (l1 ** power)[None, :]
    absolute = (2.0 ** -20 if power == 1 else 2.0 ** -19) * scale
    err = (torch.exp(got_log.double().cpu()) - ref).abs()
    bound = absolute + 2.0 ** -18 * ref
    raw = float((err / scale.clamp_min(1e-300)).max()) if float(scale.max()) > 0 else 0.0
    print(f"{tag}: max |exp(out) - ref| {float(err.max()):.3e} = at most {raw:.3e} of L1^p S, relative term included "
          f"(the absolute term alone allows {2.0 ** -20 if power == 1 else 2.0 ** -19:.3e})")
    bad = err > bound
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} elements over the bound, worst {float((err - bound).max()):.3e}"
    return raw


@pytest.fixture(scope="module")
def case1(gpu):
    """The six utterances, the config-shape creator, its ragged output (computed once, read by several tests)."""
    creator = _creator("taco", 1024, 1024, 80, gpu)
    utts = _case1_utterances()
    mel, frames = creator([u.to(gpu) for u in utts])
    torch.cuda.synchronize()
    return creator, utts, mel, frames


def test_ragged_parity_config_shape(case1):
    creator, utts, mel, frames = case1
    fb = _ref_fb("taco", 1024, 80)
    assert frames.tolist() == [u.numel() // 256 + 1 for u in utts] == [3, 4, 33, 34, 65, 17]
    worst = 0.0
    for i, u in enumerate(utts):
        t = int(frames[i])
        worst = max(worst, _check_parity(mel[i, :, :t], u, fb, 1024, 1024, 1, f"utterance {i} (N = {u.numel()})"))
    print(f"config shape: worst error {worst:.3e} of L1 S")
    silence = mel[5, :, :int(frames[5])].cpu()
    assert float((silence - math.log(1e-5)).abs().max()) <= 1e-6


def test_batch_independence(case1, gpu):
    creator, utts, mel, frames = case1
    for i, u in enumerate(utts):
        alone, f = creator([u.to(gpu)])
        assert int(f[0]) == int(frames[i])
        assert torch.equal(alone[0], mel[i, :, :int(frames[i])]), f"utterance {i} alone differs from its slice of the batch"
    rev, frev = creator([u.to(gpu) for u in reversed(utts)])
    n = len(utts)
    for i in range(n):
        t = int(frames[i])
        assert int(frev[n - 1 - i]) == t and torch.equal(rev[n - 1 - i, :, :t], mel[i, :, :t]), f"utterance {i}, reversed order"
    again, _ = creator([u.to(gpu) for u in utts])
    assert torch.equal(again, mel)


def test_padded_form(case1, gpu):
    creator, utts, mel, frames = case1
    lengths = [u.numel() for u in utts]
    padded = torch.full((len(utts), max(lengths)), 0.25)             # padding samples that would show if they were read
    for i, u in enumerate(utts):
        padded[i, :u.numel()] = u
    got, f = creator(padded.to(gpu), lengths)
    assert f.tolist() == [n // 256 + 1 for n in lengths] and torch.equal(f, frames)
    assert torch.equal(got, mel)
    got2, _ = creator(padded.to(gpu), torch.tensor(lengths))
    assert torch.equal(got2, mel)
    for i, t in enumerate(f.tolist()):
        tail = got[i, :, t:].cpu()
        assert tail.numel() == 0 or bool((tail == LOG_CLIP).all()), i
    assert abs(creator.log_clip - math.log(1e-5)) < 1e-6 and creator.log_clip == LOG_CLIP


@pytest.mark.parametrize("kind,n_fft,win,n_mels", [("mel", 1024, 1024, 80), ("taco", 512, 512, 40), ("taco", 2048, 2048, 128),
                                                   ("taco", 1024, 800, 80)])
def test_other_variants(gpu, kind, n_fft, win, n_mels):
    hop = n_fft // 4
    creator = _creator(kind, n_fft, win, n_mels, gpu)
    fb = _ref_fb(kind, n_fft, n_mels)
    utts = [_noise(n_fft // 2 + 1, 10 + n_fft // 512), _noise(5 * hop + 3, 20 + n_fft // 512)]
    mel, frames = creator([u.to(gpu) for u in utts])
    assert frames.tolist() == [3, 6]
    for i, u in enumerate(utts):
        _check_parity(mel[i, :, :int(frames[i])], u, fb, n_fft, win, creator.power, f"{kind} {n_fft}/{win}/{n_mels} N = {u.numel()}")


def test_pure_tone(gpu):
    creator = _creator("taco", 1024, 1024, 80, gpu)
    freq = 100 * SR / 1024
    x = (0.5 * torch.sin(2 * math.pi * freq * torch.arange(4096, dtype=torch.float64) / SR)).float()
    mel, frames = creator([x.to(gpu)])
    t = int(frames[0])
    assert t == 17
    _check_parity(mel[0, :, :t], x, _ref_fb("taco", 1024, 80), 1024, 1024, 1, "pure tone")
    lo, hi = mel_ref.hz_to_mel(0.0, "slaney"), mel_ref.hz_to_mel(8000.0, "slaney")
    peaks = torch.tensor([mel_ref.mel_to_hz(lo + (hi - lo) * (m + 1) / 81, "slaney") for m in range(80)], dtype=torch.float64)
    want = int((peaks - freq).abs().argmin())                        # the filter whose peak is nearest the tone
    interior = mel[0, :, 2:t - 2].cpu()                              # frames that see no reflected samples
    assert interior.argmax(0).tolist() == [want] * interior.shape[1]


def test_graph_capture_replays_on_new_audio(case1, gpu):
    from reformer_tts_amd import _graphs
    creator, utts, _, _ = case1
    lengths = [u.numel() for u in utts]
    tables = creator.tables(lengths)
    flat = torch.cat(utts).to(gpu)
    out = torch.empty(80, tables.frame_offsets[-1], device=gpu)
    creator.forward_packed(flat, tables=tables, out=out)             # warm-up: the LDS attribute is set outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _graphs.capturing(graph):
        creator.forward_packed(flat, tables=tables, out=out)
    for seed in (100, 200):
        new = torch.cat([_noise(n, seed + i) for i, n in enumerate(lengths)]).to(gpu)
        flat.copy_(new)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager, _ = creator.forward_packed(new, lengths)
        assert torch.equal(out, eager), f"replay on audio of seed {seed} differs from the eager call"


def test_round_trip_wiring(gpu, golden_dir):
    from oracle import squeezewave_ref as sw_ref
    from reformer_tts_amd import synthesis
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    z = np.load(os.path.join(golden_dir, "squeezewave_small.npz"))
    cfg = sw_ref.small_cfg()
    vocoder = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                          cfg["early_return_size"], WNConfig(**cfg["wn_config"]))
    vocoder.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, strict=False)
    vocoder = vocoder.to(gpu).eval()
    creator = _creator("taco", 1024, 1024, 80, gpu)
    frames = [7, 12]
    g = torch.Generator().manual_seed(5)
    spec = ((torch.randn(2, 80, 12, generator=g) * 2 - 5).clamp(-11.5, 2.0)).to(gpu)
    _, waves = vocoder.infer_ragged(spec, frames)
    assert [w.numel() for w in waves] == [256 * f for f in frames]
    both = synthesis.mel_round_trip_error(waves, spec, frames, creator)
    assert tuple(both.shape) == (2,) and bool(torch.isfinite(both).all())
    for i in range(2):
        one = synthesis.mel_round_trip_error([waves[i]], spec[i:i + 1], [frames[i]], creator)
        assert torch.equal(one[0], both[i]), i


def test_preprocess_directory_equals_per_file_calls(gpu, tmp_path):
    """Three PCM16 files through preprocess_directory with a max_batch_samples that splits them into two launches (the two
    shortest together, the longest alone, although it exceeds the limit by itself): every ``.pt`` is a (1, n_mels, T) CPU tensor,
    bitwise what audio_to_mel_spectrogram writes for that file alone, and the paths come back in the order of the sorted names."""
    import wave
    from reformer_tts_amd.dataset.audio import preprocess_directory
    creator = _creator("taco", 1024, 1024, 80, gpu)
    audio_dir, mel_dir, one_dir = tmp_path / "wav", tmp_path / "mel", tmp_path / "one"
    audio_dir.mkdir()
    one_dir.mkdir()
    lengths = {"b_long.wav": 9000, "a_short.wav": 700, "c_mid.wav": 3000}
    for k, (name, n) in enumerate(lengths.items()):
        pcm = np.random.RandomState(k).randint(-20000, 20000, n).astype("<i2")
        with wave.open(str(audio_dir / name), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(SR)
            f.writeframes(pcm.tobytes())
    (audio_dir / "notes.txt").write_text("not audio")
    calls = []
    packed_call = creator.forward_packed
    creator.forward_packed = lambda flat, lens: (calls.append(list(lens)), packed_call(flat, lens))[1]
    paths = preprocess_directory(audio_dir, mel_dir, creator, max_batch_samples=4000)
    del creator.forward_packed
    assert calls == [[700, 3000], [9000]]
    assert [os.path.basename(p) for p in paths] == ["a_short.pt", "b_long.pt", "c_mid.pt"]
    for name, n in lengths.items():
        got = torch.load(mel_dir / (name[:-4] + ".pt"))
        creator.audio_to_mel_spectrogram(audio_dir / name, one_dir / (name[:-4] + ".pt"))
        want = torch.load(one_dir / (name[:-4] + ".pt"))
        assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == (1, 80, n // 256 + 1)
        assert torch.equal(got, want), name
    with wave.open(str(audio_dir / "d_rate.wav"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.zeros(2000, dtype="<i2").tobytes())
    with pytest.raises(ValueError, match="sample rate 16000"):
        preprocess_directory(audio_dir, mel_dir, creator)
