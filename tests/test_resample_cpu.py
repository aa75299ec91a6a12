"""Host-side checks of the sample-rate conversion: the float64 oracle of tests/resample_ref.py against what a resampler must do,
``resample_tables`` against the oracle's filter, the output length and the argument checks of the C ABI (no launch, no GPU), and
the PCM reader / writer."""
import ctypes
import math
import os
import wave

import numpy as np
import pytest
import torch

import resample_ref

# (orig, new) -> (phases, taps): the sizes the filter definition gives
TABLE_SIZES = {(44100, 22050): (1, 25), (48000, 22050): (147, 27), (16000, 22050): (441, 13), (96000, 22050): (147, 53),
               (11025, 32000): (1280, 13), (48000, 8000): (1, 73)}
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("orig,new", [(44100, 22050), (11025, 22050), (48000, 22050), (16000, 22050), (22050, 16000), (96000, 22050),
                                      (11025, 32000), (48000, 8000), (8000, 44100), (24000, 16000)])
def test_oracle_keeps_a_tone_in_the_passband(orig, new):
    """A sine at 0.2 min(orig, new) comes out as the same sine sampled at ``new``, to 1e-3 away from the edges (the filter's
    passband ripple; 3.7e-4 is the worst of these ten pairs)."""
    f = 0.2 * min(orig, new)
    n = int(0.05 * orig)
    x = np.sin(2 * np.pi * f * np.arange(n) / orig)
    got, _ = resample_ref.resample(x, orig, new)
    assert got.size == math.ceil(n * new / orig)
    want = np.sin(2 * np.pi * f * np.arange(got.size) / new)
    edge = int(math.ceil(resample_ref.LOWPASS_FILTER_WIDTH / (2 * resample_ref.cutoff(orig, new)) * new)) + 1
    err = float(np.abs(got - want)[edge:-edge].max())
    print(f"{orig} -> {new}: tone at {f:.0f} Hz, max error {err:.2e} away from the edges")
    assert err <= 1e-3


def test_oracle_removes_a_tone_above_the_new_nyquist():
    """15 kHz does not exist at 22,050 Hz: it must not fold back to 7,050 Hz."""
    x = np.sin(2 * np.pi * 15000.0 * np.arange(4800) / 48000)
    got, _ = resample_ref.resample(x, 48000, 22050)
    rms = float(np.sqrt(np.mean(got[40:-40] ** 2)))
    print(f"15 kHz through 48000 -> 22050: rms {rms:.4f} (input 0.707)")
    assert rms < 0.01


@pytest.mark.parametrize("orig,new,n", [(48000, 22050, 700), (16000, 22050, 300), (7, 5, 40), (44100, 22050, 5)])
def test_oracle_band_equals_the_dense_sum(orig, new, n):
    x = np.random.RandomState(n).randn(n)
    a, sa = resample_ref.resample(x, orig, new)
    b, sb = resample_ref.resample(x, orig, new, dense=True)
    # the same non-zero terms, summed in another order: float64 rounding of a sum of at most 60 terms
    assert a.shape == b.shape and bool(np.all(np.abs(sa - sb) <= 1e-14 * sb)) and bool(np.all(np.abs(a - b) <= 1e-14 * sb))


def _support(orig, new, p):
    """Inputs i (relative to the block of output p < new') whose filter value can be non-zero, found by scanning."""
    width = resample_ref.LOWPASS_FILTER_WIDTH / (2.0 * resample_ref.cutoff(orig, new))
    reach = int(width * orig) + 3
    centre = int(p * orig / new)
    i = np.arange(centre - reach, centre + reach + 1)
    return i[np.abs(i / orig - p / new) < width]


@pytest.mark.parametrize("orig,new", [(44100, 22050), (11025, 22050), (48000, 22050), (16000, 22050), (7, 5)])
def test_tables_match_the_filter(orig, new):
    """2:1, 1:2, 320:147, 320:441 and 7:5: first[p] is the first input inside the window, every coefficient is the oracle's h
    rounded to f32 to one ulp, and what pads a short phase is exactly zero."""
    from reformer_tts_amd.dataset.audio import resample_tables
    first, coef, o, w, taps = resample_tables(orig, new)
    g = math.gcd(orig, new)
    assert (o, w) == (orig // g, new // g)
    assert first.dtype == torch.int32 and tuple(first.shape) == (w,)
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (taps, w) and coef.is_contiguous()
    longest, worst = 0, 0.0
    for p in range(w):
        sup = _support(orig, new, p)
        assert int(first[p]) == int(sup[0]), (p, int(first[p]), int(sup[0]))
        longest = max(longest, sup.size)
        i = int(first[p]) + np.arange(taps)
        want = resample_ref.h(i / orig - p / new, orig, new)
        got = coef[:, p].numpy().astype(np.float64)
        assert np.all(got[sup.size:] == 0.0), p
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        worst = max(worst, float((np.abs(got - want) / ulp).max()))
    print(f"{orig} -> {new}: {w} phases, {taps} taps, worst coefficient error {worst:.3f} f32 ulp")
    assert longest == taps
    assert worst <= 1.0


@pytest.mark.parametrize("pair", sorted(TABLE_SIZES))
def test_table_sizes(pair):
    from reformer_tts_amd.dataset.audio import resample_tables
    _, coef, _, w, taps = resample_tables(*pair)
    assert (w, taps) == TABLE_SIZES[pair] and tuple(coef.shape) == (taps, w)


def test_largest_table_and_most_taps_of_the_common_rates():
    from reformer_tts_amd.dataset.audio import RESAMPLE_MAX_TABLE, RESAMPLE_MAX_TAPS, resample_tables
    sizes = {(a, b): resample_tables(a, b)[3:] for a in RATES for b in RATES if a != b}
    assert max(sizes, key=lambda k: sizes[k][0] * sizes[k][1]) == (11025, 32000) and sizes[(11025, 32000)] == (1280, 13)
    assert max(sizes, key=lambda k: sizes[k][1]) == (48000, 8000) and sizes[(48000, 8000)] == (1, 73)
    assert all(t <= RESAMPLE_MAX_TAPS and w * t <= RESAMPLE_MAX_TABLE for w, t in sizes.values())
    with pytest.raises(ValueError):
        resample_tables(22050, 22050)
    with pytest.raises(ValueError, match="taps"):
        resample_tables(48000, 1000)


@pytest.mark.parametrize("orig,new", [(44100, 22050), (48000, 22050), (16000, 22050), (7, 5), (22050, 48000)])
def test_output_length(lib, orig, new):
    from reformer_tts_amd.dataset.audio import resample_len
    o = orig // math.gcd(orig, new)
    for n in sorted({1, max(o - 1, 1), o, o + 1, 12345}):
        want = -((-n * new) // orig)
        assert lib.rtts_resample_len(n, orig, new) == want == resample_len(n, orig, new) == resample_ref.out_len(n, orig, new)


def test_output_length_rejects_nonsense(lib):
    assert lib.rtts_resample_len(0, 48000, 22050) < 0 and "rtts_resample_len" in lib.rtts_last_error().decode()
    assert lib.rtts_resample_len(100, 0, 22050) < 0
    assert lib.rtts_resample_len(100, 48000, -1) < 0
    assert lib.rtts_resample_len(1 << 62, 7, 5) < 0 and "overflow" in lib.rtts_last_error().decode()


def _call(lib, *, in_format=0, channels=1, lengths=(4096,), in_off=None, out_off=None, nseg=None, orig_red=320, new_red=147, taps=27,
          null=None):
    """rtts_resample with dummy (never dereferenced) device pointers: every case here must be rejected before a launch."""
    ioff, ooff = [0], [0]
    for n in lengths:
        ioff.append(ioff[-1] + n)
        ooff.append(ooff[-1] + -((-n * max(new_red, 1)) // max(orig_red, 1)))
    ioff, ooff = in_off or ioff, out_off or ooff
    n1 = len(ioff)
    args = dict(audio=64, in_format=in_format, channels=channels, ioff_h=(ctypes.c_int64 * n1)(*ioff), ooff_h=(ctypes.c_int64 * n1)(*ooff),
                ioff=64, ooff=64, nseg=n1 - 1 if nseg is None else nseg, first=64, coef=64, orig_red=orig_red, new_red=new_red, taps=taps,
                out=64, stream=None)
    if null is not None:
        args[null] = None
    rc = lib.rtts_resample(*args.values())
    return rc, lib.rtts_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(taps=257), "taps"),
    (dict(taps=0), "taps"),
    (dict(orig_red=3, new_red=1 << 20, taps=13), "new_red * taps"),
    (dict(orig_red=100, new_red=1, taps=250), "LDS"),
    (dict(null="audio"), "null"),
    (dict(null="ioff_h"), "null"),
    (dict(null="ooff_h"), "null"),
    (dict(null="ioff"), "null"),
    (dict(null="ooff"), "null"),
    (dict(null="first"), "null"),
    (dict(null="coef"), "null"),
    (dict(null="out"), "null"),
    (dict(orig_red=147, new_red=147), "orig_red"),
    (dict(orig_red=0), "orig_red"),
    (dict(new_red=-3), "new_red"),
    (dict(in_format=2), "in_format"),
    (dict(in_format=-1), "in_format"),
    (dict(in_format=0, channels=2), "channels"),
    (dict(in_format=1, channels=0), "channels"),
    (dict(in_format=1, channels=9), "channels"),
    (dict(in_off=[0, 4096, 4000]), "in_offsets"),
    (dict(in_off=[0, 4096, 4096]), "in_offsets"),
    (dict(in_off=[-1, 4096]), "in_offsets"),
    (dict(lengths=(4096, 1000), out_off=[0, 1882, 1882 + 459]), "out_offsets"),
    (dict(lengths=(4096,), out_off=[0, 1881]), "out_offsets"),
    (dict(nseg=0), "nseg"),
    (dict(nseg=65536), "nseg"),
])
def test_bad_arguments_are_rejected_without_a_launch(lib, kw, word):
    rc, msg = _call(lib, **kw)
    assert rc != 0
    assert "rtts_resample" in msg and word in msg, msg


def test_header_declares_the_new_exports(lib):
    from reformer_tts_amd import _lib
    from reformer_tts_amd.dataset import audio
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rtts.h")).read()
    for name in ("rtts_resample_len", "rtts_resample"):
        assert f"{name}(" in text and hasattr(lib, name) and name in _lib.SIGNATURES
    assert "convert.py:131-146" in text
    for macro, value in (("RTTS_RESAMPLE_TILE", audio.RESAMPLE_TILE), ("RTTS_RESAMPLE_MAX_TAPS", audio.RESAMPLE_MAX_TAPS)):
        assert f"#define {macro} {value}\n" in text
    assert "#define RTTS_RESAMPLE_MAX_TABLE (1 << 22)\n" in text and audio.RESAMPLE_MAX_TABLE == 1 << 22


def _write_pcm(path, pcm: np.ndarray, channels: int, rate: int, width: int = 2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())


def test_read_pcm_keeps_the_channels(tmp_path):
    from reformer_tts_amd.dataset.audio import pcm_info, read_pcm
    pcm = np.random.RandomState(0).randint(-32768, 32768, (500, 2)).astype("<i2")
    _write_pcm(tmp_path / "stereo.wav", pcm, 2, 48000)
    got, rate = read_pcm(tmp_path / "stereo.wav")
    assert rate == 48000 and got.dtype == torch.int16 and tuple(got.shape) == (500, 2)
    assert np.array_equal(got.numpy(), pcm)
    assert pcm_info(tmp_path / "stereo.wav") == (500, 48000, 2)
    _write_pcm(tmp_path / "u8.wav", np.arange(100, dtype=np.uint8), 1, 8000, width=1)
    for fn in (read_pcm, pcm_info):
        with pytest.raises(ValueError, match="16-bit PCM"):
            fn(tmp_path / "u8.wav")


def test_write_wav_round_trips_and_clips(tmp_path):
    from reformer_tts_amd.dataset.audio import read_wav, wav_info, write_wav
    pcm = np.concatenate([np.array([-32768, -1, 0, 1, 32767], dtype=np.int16),
                          np.random.RandomState(1).randint(-32768, 32768, 1000).astype(np.int16)])
    x = torch.from_numpy(pcm.astype(np.float32) / np.float32(32768.0))
    write_wav(tmp_path / "a.wav", x, 16000)
    assert wav_info(tmp_path / "a.wav") == (pcm.size, 16000)
    back, rate = read_wav(tmp_path / "a.wav")
    assert rate == 16000 and torch.equal(back, x)
    write_wav(tmp_path / "clip.wav", torch.tensor([1.0, 1.5, -1.0, -1.5, 0.99999, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.4 / 32768]), 8000)
    with wave.open(str(tmp_path / "clip.wav"), "rb") as f:
        got = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    assert got.tolist() == [32767, 32767, -32768, -32768, 32767, 0, 2, 2, 0]       # clipped at both ends; ties to even


def test_resample_refuses_to_run_off_the_gpu():
    from reformer_tts_amd import _lib
    from reformer_tts_amd.dataset.audio import Resample
    r = Resample(48000, 22050)
    assert (r.orig_red, r.new_red, r.taps) == (320, 147, 27)
    assert not r.state_dict()                                       # the tables are non-persistent buffers
    with pytest.raises(_lib.RttsError, match="GPU only"):
        r([torch.zeros(4096)])
    with pytest.raises(_lib.RttsError, match="GPU only"):
        r.forward_packed(torch.zeros(4096), [4096])
    with pytest.raises(ValueError):
        Resample(0, 22050)
    same = Resample(22050, 22050)
    x = [torch.zeros(10)]
    assert same(x)[0] is x


def test_files_are_grouped_by_rate_and_channels():
    from reformer_tts_amd.dataset.audio import group_by_format
    info = {"a.wav": (900, 48000, 2), "b.wav": (500, 16000, 1), "c.wav": (300, 48000, 2), "d.wav": (300, 48000, 1),
            "e.wav": (100, 22050, 1), "f.wav": (300, 48000, 2)}
    groups = group_by_format(info)
    assert list(groups) == [(16000, 1), (22050, 1), (48000, 1), (48000, 2)]
    assert groups[(48000, 2)] == ["c.wav", "f.wav", "a.wav"] and groups[(16000, 1)] == ["b.wav"]
    assert sorted(n for v in groups.values() for n in v) == sorted(info)
