"""rtts_resample (csrc/resample.hip) and the resampling half of reformer_tts_amd/dataset/audio.py on the GPU, against the float64
oracle of tests/resample_ref.py (the dense definition: no phases, no tables).

Criterion, per output sample, with A_k = sum_i |x_i| |h(i / orig - k / new)|:
    |out_k - ref_k| <= (taps + 2) * 2^-24 * A_k
the standard bound of an f32 chain of ``taps`` fused multiply-adds (each rounds once: at most taps * 2^-24 of the running sum of
magnitudes, to first order) over coefficients rounded once to f32 (2^-24 each) and the oracle's own float64 error (far below one
more 2^-24).  The same chain run in f32 on a CPU stays below 0.33 of it.  The noise input has no structure a wrong phase or
offset could hide behind: such a fault is an error of order A_k itself, 10^5 times the bound."""
import ctypes
import math
import os
import wave

import numpy as np
import pytest
import torch

import resample_ref

pytestmark = pytest.mark.gpu

RATIOS = [(44100, 22050), (11025, 22050), (48000, 22050), (16000, 22050), (22050, 16000), (96000, 22050), (11025, 32000), (48000, 8000),
          (7, 5),
          (32000, 11025)]        # 441 phases of 36 taps: the one pair of the common rates whose coefficients stay in global memory


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _noise(n, seed):
    return 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _chirp(n, orig):
    t = torch.arange(n, dtype=torch.float64) / orig
    dur = max(n / orig, 1e-9)
    return (0.5 * torch.sin(2 * math.pi * (0.001 * orig * t + 0.25 * orig / dur * t * t))).float()     # 0.001 orig -> 0.5 orig Hz


def _resampler(orig, new, gpu):
    from reformer_tts_amd.dataset.audio import Resample
    return Resample(orig, new).to(gpu)


def _n_for(m, o, w):
    """The shortest utterance with at least ``m`` output samples."""
    return max(((m - 1) * o) // w + 1, 1)


def _lengths(orig, new, taps):
    from reformer_tts_amd.dataset.audio import RESAMPLE_TILE as tile
    g = math.gcd(orig, new)
    o, w = orig // g, new // g
    lens = [1, 2, max(taps - 1, 1), o, o + 1, 3 * o, _n_for(tile - 1, o, w), _n_for(tile, o, w), _n_for(tile + 1, o, w),
            _n_for(2 * tile + 17, o, w), 20011]
    return lens


@pytest.mark.parametrize("orig,new", RATIOS)
def test_ragged_parity(gpu, orig, new):
    from reformer_tts_amd.dataset.audio import RESAMPLE_TILE as tile
    r = _resampler(orig, new, gpu)
    lens = _lengths(orig, new, r.taps)
    utts = [_noise(n, 100 + i) for i, n in enumerate(lens)] + [_chirp(6007, orig)]
    out, m = r([u.to(gpu) for u in utts])
    torch.cuda.synchronize()
    want_m = [resample_ref.out_len(u.numel(), orig, new) for u in utts]
    assert m.tolist() == want_m
    assert want_m[5] == 3 * r.new_red                                # M = N new / orig exactly
    assert {tile, tile + 1} <= set(want_m[6:10]) or new > orig       # upsampling cannot reach every length
    assert max(want_m) > 2 * tile
    got = out.cpu().double().numpy()
    worst = 0.0
    for i, u in enumerate(utts):
        ref, scale = resample_ref.resample(u.numpy(), orig, new)
        bound = (r.taps + 2) * 2.0 ** -24 * scale
        err = np.abs(got[i, :want_m[i]] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        bad = err > bound
        assert not bad.any(), f"{orig} -> {new}, utterance {i} (N = {u.numel()}): {int(bad.sum())} samples over the bound, first at {int(bad.argmax())}"
        assert not got[i, want_m[i]:].any(), f"utterance {i}: the padding behind its samples is not zero"
    print(f"{orig} -> {new} ({r.new_red} phases, {r.taps} taps): worst error {worst:.3f} of the bound (taps + 2) 2^-24 A_k")


@pytest.mark.parametrize("orig,new", [(48000, 22050), (16000, 22050), (44100, 22050), (7, 5)])
def test_impulse_reads_the_table_back(gpu, orig, new):
    """A unit sample at position i: output k = j new' + p is coefficient t = i - j orig' - first[p] of phase p where that is a tap,
    and exactly zero elsewhere."""
    from reformer_tts_amd.dataset.audio import resample_tables
    first, coef, o, w, taps = resample_tables(orig, new)
    n = 6 * o + 5
    positions = sorted({0, 1, o - 1, n // 2, n - 1})
    x = torch.zeros(len(positions), n)
    for row, i in enumerate(positions):
        x[row, i] = 1.0
    out, m = _resampler(orig, new, gpu)(x.to(gpu), [n] * len(positions))
    got = out.cpu()
    k = torch.arange(int(m[0]))
    j, p = k // w, k % w
    for row, i in enumerate(positions):
        t = i - j * o - first[p].long()
        inside = (t >= 0) & (t < taps)
        want = torch.where(inside, coef[t.clamp(0, taps - 1), p], torch.zeros(()))
        assert bool(inside.any())
        assert torch.equal(got[row], want), f"{orig} -> {new}: impulse at {i}"


@pytest.fixture(scope="module")
def batch48(gpu):
    """48000 -> 22050: four utterances, the resampler and its ragged output (computed once, read by several tests)."""
    r = _resampler(48000, 22050, gpu)
    utts = [_noise(n, 7 + i) for i, n in enumerate((5000, 333, 2300, 9001))]
    out, m = r([u.to(gpu) for u in utts])
    torch.cuda.synchronize()
    return r, utts, out, m


def test_int16_stereo_equals_f32_of_channel0(batch48, gpu):
    r, _, _, _ = batch48
    g = torch.Generator().manual_seed(3)
    lens = [4000, 17, 2500]
    for channels in (1, 2, 8):
        pcm = torch.randint(-32768, 32768, (sum(lens), channels), generator=g, dtype=torch.int32).to(torch.int16)
        got, off = r.forward_packed(pcm.reshape(-1).to(gpu), lens, channels=channels)
        want, off2 = r.forward_packed((pcm[:, 0].float() / 32768.0).to(gpu), lens)
        assert off == off2 and torch.equal(got, want), channels
    assert float(got.abs().max()) > 0.1


def test_batch_independence(batch48, gpu):
    r, utts, out, m = batch48
    for i, u in enumerate(utts):
        alone, mi = r([u.to(gpu)])
        assert int(mi[0]) == int(m[i]) and torch.equal(alone[0], out[i, :int(m[i])]), f"utterance {i} alone"
    rev, mrev = r([u.to(gpu) for u in reversed(utts)])
    n = len(utts)
    for i in range(n):
        assert torch.equal(rev[n - 1 - i, :int(m[i])], out[i, :int(m[i])]), f"utterance {i}, reversed order"
    rot, _ = r([u.to(gpu) for u in utts[1:] + utts[:1]])
    assert torch.equal(rot[n - 1, :int(m[0])], out[0, :int(m[0])]) and torch.equal(rot[0, :int(m[1])], out[1, :int(m[1])])
    again, _ = r([u.to(gpu) for u in utts])
    assert torch.equal(again, out)
    lens = [u.numel() for u in utts]
    padded = torch.full((n, max(lens)), 0.25)                         # padding samples that would show if they were read
    for i, u in enumerate(utts):
        padded[i, :u.numel()] = u
    form2, m2 = r(padded.to(gpu), torch.tensor(lens))
    assert torch.equal(m2, m) and torch.equal(form2, out)


def test_nothing_outside_the_output_slots_is_written(batch48, gpu):
    from reformer_tts_amd import ops
    from reformer_tts_amd.dataset.audio import ResampleTables
    r, utts, out, m = batch48
    lens = [u.numel() for u in utts]
    tables = ResampleTables(lens, r.orig_red, r.new_red, gpu)
    slack = [3, 1030, 0, 64]
    ooff = [0]
    for mi, s in zip(tables.out_lengths, slack):
        ooff.append(ooff[-1] + mi + s)
    ooff_host = (ctypes.c_int64 * len(ooff))(*ooff)
    table = torch.tensor([tables.in_offsets, ooff], dtype=torch.int64).to(gpu)
    lead, sentinel = 17, -7.5
    buf = torch.full((lead + ooff[-1] + 2000,), sentinel, device=gpu)
    ops.resample(torch.cat(utts).to(gpu), tables.ioff_host, ooff_host, table, len(lens), r.first, r.coefficients, r.orig_red, r.new_red,
                 buf[lead:])
    host, untouched = buf.cpu(), torch.ones(buf.numel(), dtype=torch.bool)
    for i, mi in enumerate(tables.out_lengths):
        a = lead + ooff[i]
        assert torch.equal(host[a:a + mi], out[i, :mi].cpu()), i
        untouched[a:a + mi] = False
    assert bool((host[untouched] == sentinel).all()) and int(untouched.sum()) == lead + sum(slack) + 2000


def test_graph_capture_replays_on_new_audio(batch48, gpu):
    from reformer_tts_amd import _graphs
    r, utts, _, _ = batch48
    lens = [u.numel() for u in utts]
    tables = r.tables(lens)
    flat = torch.cat(utts).to(gpu)
    out = torch.empty(tables.out_offsets[-1], device=gpu)
    r.forward_packed(flat, tables=tables, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _graphs.capturing(graph):
        r.forward_packed(flat, tables=tables, out=out)
    for seed in (100, 200):
        new = torch.cat([_noise(n, seed + i) for i, n in enumerate(lens)]).to(gpu)
        flat.copy_(new)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager, _ = r.forward_packed(new, lens)
        assert torch.equal(out, eager), f"replay on audio of seed {seed} differs from the eager call"


def _write_pcm(path, pcm, channels, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


def test_preprocess_directory_resamples(gpu, tmp_path):
    """A 48 kHz stereo file, a 16 kHz mono file and a 22,050 Hz mono file: with resample=True every ``.pt`` is bitwise the creator's
    output on the module's resampling of channel 0; the file already at the rate is what resample=False writes; without the option
    the directory is refused as before."""
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram, preprocess_directory
    creator = Tacotron2Spectrogram(22050, 1024, 1024, 256, 80).to(gpu)
    audio_dir, mel_dir, plain_dir, only_dir = (tmp_path / d for d in ("wav", "mel", "plain", "only"))
    audio_dir.mkdir()
    only_dir.mkdir()
    rs = np.random.RandomState(0)
    files = {"a48.wav": (48000, 2, 24000), "b16.wav": (16000, 1, 5000), "c22.wav": (22050, 1, 9000)}
    pcm = {}
    for name, (rate, channels, n) in files.items():
        pcm[name] = rs.randint(-20000, 20000, (n, channels)).astype(np.int16)
        _write_pcm(audio_dir / name, pcm[name], channels, rate)
    _write_pcm(only_dir / "c22.wav", pcm["c22.wav"], 1, 22050)
    paths = preprocess_directory(audio_dir, mel_dir, creator, resample=True)
    assert [os.path.basename(p) for p in paths] == ["a48.pt", "b16.pt", "c22.pt"]
    for name, (rate, channels, n) in files.items():
        got = torch.load(mel_dir / (name[:-4] + ".pt"))
        x = (torch.from_numpy(pcm[name][:, 0].astype(np.float32)) / 32768.0).to(gpu)
        if rate != 22050:
            x, m = _resampler(rate, 22050, gpu)([x])
            x = x[0, :int(m[0])]
            assert int(m[0]) == math.ceil(n * 22050 / rate)
        want, _ = creator([x])
        assert got.device.type == "cpu" and tuple(got.shape) == (1, 80, x.numel() // 256 + 1)
        assert torch.equal(got, want.cpu()), name
    preprocess_directory(only_dir, plain_dir, creator)
    assert torch.equal(torch.load(plain_dir / "c22.pt"), torch.load(mel_dir / "c22.pt"))
    with pytest.raises(ValueError):
        preprocess_directory(audio_dir, plain_dir, creator)
    _write_pcm(audio_dir / "d_short.wav", np.zeros((1000, 1), dtype=np.int16), 1, 48000)       # 460 samples at 22,050 Hz
    with pytest.raises(ValueError, match=r"d_short\.wav.*reflect padding needs more than n_fft / 2"):
        preprocess_directory(audio_dir, mel_dir, creator, resample=True)


def test_resample_wav(gpu, tmp_path):
    from reformer_tts_amd.dataset.audio import read_wav, resample_wav, write_wav
    pcm = np.random.RandomState(5).randint(-30000, 30000, (7000, 2)).astype(np.int16)
    _write_pcm(tmp_path / "in.wav", pcm, 2, 44100)
    resample_wav(tmp_path / "in.wav", tmp_path / "out.wav", 22050, device=gpu)
    x = (torch.from_numpy(pcm[:, 0].astype(np.float32)) / 32768.0).to(gpu)
    out, m = _resampler(44100, 22050, gpu)([x])
    write_wav(tmp_path / "want.wav", out[0, :int(m[0])], 22050)
    got, rate = read_wav(tmp_path / "out.wav")
    want, _ = read_wav(tmp_path / "want.wav")
    assert rate == 22050 and got.numel() == 3500 and torch.equal(got, want)
    assert (tmp_path / "out.wav").read_bytes() == (tmp_path / "want.wav").read_bytes()
    resample_wav(tmp_path / "in.wav", tmp_path / "same.wav", 44100, device=gpu)             # at the rate already: channel 0 as it is
    same, rate = read_wav(tmp_path / "same.wav")
    assert rate == 44100 and torch.equal(same, x.cpu())
