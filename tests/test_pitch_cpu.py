"""Host-side checks of the pitch path: the float64 restatement of tests/pitch_ref.py on signals whose F0 is known, the contour
comparison worked by hand, ``PitchTracker``'s argument checks and tables, the arithmetic of ``f0_errors_from_counts``, and the
argument checks of the two entry points (dummy pointers, no launch, no GPU)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import pitch_ref as ref

TAU_MIN, TAU_MAX, THR = 45, 490, 0.1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def picks():
    return {name: ref.yin_pick(ref.yin_cmnd(x, 256)[0], TAU_MIN, TAU_MAX, THR, ref.SR) for name, x in ref.signals().items()}


def test_the_batch_is_181_frames():
    sig = ref.signals()
    assert len(sig) == 12 and sum(ref.frames_of(len(x), 256) for x in sig.values()) == 181
    assert [len(sig[k]) for k in ("one", "short255", "short256", "short300", "short1279")] == [1, 255, 256, 300, 1279]


@pytest.mark.parametrize("name", sorted(ref.STEADY))
def test_oracle_recovers_a_steady_tone(picks, name):
    """Within 0.5 % at EVERY voiced frame, and every frame whose whole reach lies inside the tone is voiced."""
    p, want = picks[name], ref.STEADY[name]
    inside = [t for t in range(len(p["tau"])) if t * 256 - ref.REACH // 2 >= 0 and t * 256 + ref.REACH // 2 <= 6000]
    assert len(inside) >= 15 and p["voiced"][inside].all()
    err = np.abs(p["f0"][p["voiced"]] / want - 1.0)
    print(f"{name}: {int(p['voiced'].sum())} voiced frames, worst relative F0 error {err.max():.2e}")
    assert err.max() <= 5e-3
    assert (p["aperiodicity"][inside] < THR).all()


def test_oracle_calls_noise_and_silence_unvoiced(picks):
    assert not picks["noise"]["voiced"].any() and (picks["noise"]["aperiodicity"] > THR).all()
    p = picks["pause_tone_pause"]
    silent = [t for t in range(len(p["tau"])) if t * 256 + ref.REACH // 2 <= 2000 or t * 256 - ref.REACH // 2 >= 5000]
    assert len(silent) >= 3 and not p["voiced"][silent].any() and (p["aperiodicity"][silent] == 1.0).all()
    assert p["voiced"][10:19].all() and np.abs(p["f0"][10:19] / 200.0 - 1.0).max() <= 5e-3
    assert not picks["one"]["voiced"].any()


def test_pick_follows_the_definition_on_a_hand_made_row():
    row = np.ones(513)
    row[100:104] = [0.3, 0.08, 0.05, 0.07]            # below the threshold at 101, descends to 102
    row[200] = 0.01                                    # a deeper dip further on is not looked at
    p = ref.yin_pick(row[None, :], 45, 490, 0.1, 22050.0)
    off = 0.5 * (0.08 - 0.07) / (0.08 - 0.1 + 0.07)
    assert p["tau"][0] == 102 and p["voiced"][0] and p["aperiodicity"][0] == 0.05
    assert p["f0"][0] == 22050.0 / (102 + off) and not p["fragile"][0]
    row[101] = 0.1 * (1 + 1e-4)                        # a comparison with the threshold that another rounding could turn
    assert ref.yin_pick(row[None, :], 45, 490, 0.1, 22050.0)["fragile"][0]
    flat = ref.yin_pick(np.full((1, 513), 0.5), 45, 490, 0.1, 22050.0)
    assert flat["tau"][0] == 0 and flat["f0"][0] == 0.0 and flat["aperiodicity"][0] == 0.5


def test_compare_ref_by_hand():
    fa = np.array([100.0, 0.0, 200.0, 130.0, 30.0, 50.0, 7.0], dtype=np.float32)      # utterances of 4 and 3 frames
    fb = np.array([100.0, 100.0, 100.0, 0.0, 0.0, 0.0, 50.0, 60.0], dtype=np.float32)     # 5 and 3
    t = ref.f0_compare_ref(fa, [0, 4, 7], fb, [0, 5, 8], 0.2)
    assert t[0].tolist() == [4.0, 2.0, 1200.0 ** 2, 1.0, 2.0]
    assert t[1, 0] == 3 and t[1, 1] == 2 and t[1, 3] == 1 and t[1, 4] == 1
    assert math.isclose(t[1, 2], (1200.0 * math.log2(7.0 / 60.0)) ** 2, rel_tol=1e-14)
    assert np.array_equal(t[2], t[0] + t[1])
    fa[5] = np.nan
    t = ref.f0_compare_ref(fa, [0, 4, 7], fb, [0, 5, 8], 0.2)
    assert np.isnan(t[1]).all() and np.isnan(t[2]).all() and not np.isnan(t[0]).any()


@pytest.mark.parametrize("kw,word", [
    (dict(sample_rate=0), "sample_rate"),
    (dict(hop_length=200), "hop_length"),
    (dict(f_min=40.0), "tau_max"),                     # 22050 / 40 = 551 samples
    (dict(sample_rate=48000), "tau_max"),
    (dict(f_max=30000.0), "tau_min"),                  # less than one sample
    (dict(f_min=300.0, f_max=200.0), "f_min"),
    (dict(f_min=444.0, f_max=448.0), "whole period"),  # 49.2 .. 49.7 samples
    (dict(threshold=0.0), "threshold"),
    (dict(threshold=1.0), "threshold"),
])
def test_tracker_refuses_by_name(kw, word):
    from reformer_tts_amd.evaluation import PitchTracker
    with pytest.raises(ValueError, match=word):
        PitchTracker(**kw)


def test_tracker_lags_tables_and_gpu_only():
    from reformer_tts_amd import _lib
    from reformer_tts_amd.dataset.audio import MelTables
    from reformer_tts_amd.evaluation import PitchTracker, audio_f0_errors
    tr = PitchTracker()
    assert (tr.tau_min, tr.tau_max) == (45, 441)
    assert (PitchTracker(f_min=45.0, f_max=490.0).tau_min, PitchTracker(f_min=45.0, f_max=490.0).tau_max) == (TAU_MIN, TAU_MAX)
    lengths = [1, 255, 256, 6000]
    got, want = tr.tables(lengths, "cpu"), MelTables(lengths, 256, "cpu")
    assert isinstance(got, MelTables) and got.frame_offsets == want.frame_offsets == [0, 1, 2, 4, 28]
    assert got.sample_offsets == want.sample_offsets and torch.equal(got.device_table, want.device_table)
    assert list(got.soff_host) == want.sample_offsets and list(got.foff_host) == want.frame_offsets
    with pytest.raises(_lib.RttsError, match="GPU only"):
        tr.forward_packed(torch.zeros(4096), [4096])
    with pytest.raises(_lib.RttsError, match="GPU only"):
        tr([torch.zeros(4096)])
    with pytest.raises(ValueError, match="waveforms"):
        audio_f0_errors([torch.zeros(10)], [], tr)


def test_error_figures_from_hand_made_counts():
    from reformer_tts_amd.evaluation import f0_errors_from_counts
    nan = float("nan")
    rows = [[10.0, 8.0, 8.0 * 2500.0, 2.0, 1.0],       # rmse 50 cents, gpe 1/4, vde 1/10, ffe 3/10
            [5.0, 0.0, 0.0, 0.0, 5.0],                 # nothing voiced in both: rmse and gpe NaN, vde = ffe = 1
            [0.0, 0.0, 0.0, 0.0, 0.0],                 # no frame: all NaN
            [nan] * 5]
    rows.append([15.0, 8.0, 20000.0, 2.0, 6.0])
    out = f0_errors_from_counts(torch.tensor(rows, dtype=torch.float64))
    want = {"rmse_cents": [50.0, nan, nan, nan], "gpe": [0.25, nan, nan, nan], "vde": [0.1, 1.0, nan, nan], "ffe": [0.3, 1.0, nan, nan]}
    for key, w in want.items():
        assert out[key].dtype == torch.float64 and np.array_equal(out[key].numpy(), np.array(w), equal_nan=True), key
    assert np.array_equal(out["totals"].numpy(), np.array([50.0, 0.25, 6.0 / 15.0, 8.0 / 15.0]))
    assert not torch.isinf(torch.cat([out[k] for k in want])).any()
    with pytest.raises(ValueError, match="table"):
        f0_errors_from_counts(torch.zeros(3, 4, dtype=torch.float64))


def test_header_and_signatures_hold_the_new_symbols(lib):
    from reformer_tts_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rtts.h")).read()
    for name in ("rtts_pitch_yin", "rtts_f0_compare"):
        assert f"{name}(" in text and hasattr(lib, name) and name in _lib.SIGNATURES
    assert "#define RTTS_PITCH_MAX_LAG 512" in text and "#define RTTS_PITCH_TILE_FRAMES" in text
    assert ops.PITCH_MAX_LAG == ref.MAX_LAG and ops.PITCH_WINDOW == ref.W


def _yin(lib, *, hop=256, tau_min=45, tau_max=490, thr=0.1, sr=22050.0, lengths=(6000, 300), nseg=None, null=None, soff=None, slack=0):
    """rtts_pitch_yin with dummy (never dereferenced) device pointers: every case here must be rejected before a launch."""
    so, fo = [0], [0]
    for n in lengths:
        so.append(so[-1] + n)
        fo.append(fo[-1] + n // (hop if hop > 0 else 1) + 1 + slack)
    so = list(soff) if soff is not None else so
    n1 = len(so)
    args = dict(audio=64, soff_h=(ctypes.c_int64 * n1)(*so), foff_h=(ctypes.c_int64 * n1)(*fo), soff=64, foff=64,
                nseg=len(lengths) if nseg is None else nseg, hop=hop, tau_min=tau_min, tau_max=tau_max, thr=thr, sr=sr, f0=64, ap=64,
                cmnd=None, stream=None)
    if null is not None:
        args[null] = None
    rc = lib.rtts_pitch_yin(*args.values())
    return rc, lib.rtts_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(hop=64), "hop"),
    (dict(hop=192), "hop"),
    (dict(hop=1024), "hop"),
    (dict(tau_min=1), "tau_min"),
    (dict(tau_max=512), "tau_max"),
    (dict(tau_min=300, tau_max=299), "tau_min"),
    (dict(thr=0.0), "threshold"),
    (dict(thr=1.0), "threshold"),
    (dict(thr=float("nan")), "threshold"),
    (dict(sr=0.0), "sample_rate"),
    (dict(sr=float("inf")), "sample_rate"),
    (dict(nseg=0), "nseg"),
    (dict(nseg=65536, lengths=(10,)), "nseg"),
    (dict(soff=[0, 6000, 5000]), "sample_offsets"),    # a decreasing offset
    (dict(soff=[0, 6000, 6000]), "sample_offsets"),    # an empty utterance
    (dict(soff=[-1, 6000, 6300]), "sample_offsets"),
    (dict(slack=-1), "frame_offsets"),                 # a slot one frame short
    (dict(null="audio"), "null"),
    (dict(null="soff_h"), "null"),
    (dict(null="foff_h"), "null"),
    (dict(null="soff"), "null"),
    (dict(null="foff"), "null"),
    (dict(null="f0"), "null"),
    (dict(null="ap"), "null"),
])
def test_yin_rejects_bad_arguments_without_a_launch(lib, kw, word):
    rc, msg = _yin(lib, **kw)
    assert rc != 0
    assert "rtts_pitch_yin" in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(nseg=0), "nseg"),
    (dict(nseg=65536), "nseg"),
    (dict(gross=0.0), "gross"),
    (dict(gross=1.0), "gross"),
    (dict(gross=float("nan")), "gross"),
    (dict(null=0), "null"),
    (dict(null=1), "null"),
    (dict(null=2), "null"),
    (dict(null=3), "null"),
    (dict(null=6), "null"),
])
def test_compare_rejects_bad_arguments_without_a_launch(lib, kw, word):
    args = [64, 64, 64, 64, kw.get("nseg", 2), kw.get("gross", 0.2), 64, None]
    if "null" in kw:
        args[kw["null"]] = None
    rc = lib.rtts_f0_compare(*args)
    msg = lib.rtts_last_error().decode()
    assert rc != 0 and "rtts_f0_compare" in msg and word in msg, msg
