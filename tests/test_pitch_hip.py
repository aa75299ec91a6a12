"""``rtts_pitch_yin`` and ``rtts_f0_compare`` (csrc/pitch.hip) on the GPU against their float64 restatement (tests/pitch_ref.py).

The batch: the twelve signals of ``pitch_ref.signals()`` (181 frames at hop 256) and one more tone of 2 * RTTS_PITCH_TILE_FRAMES + 1
hops, whose frames cross two tile seams; lags 45..490 (45 to 490 Hz at 22,050 Hz), threshold 0.1.  Every utterance's frame slot
has two frames of slack that hold a sentinel.

The bounds, none of them measured:

  d'     |kernel - oracle| <= 2e-4 * d' at every frame and every lag 1..512, and equality where the oracle's d is 0.  d is a sum of
         1024 non-negative terms: at most 1026 roundings go into it (the fmaf chains over the hop blocks and the sums of the
         blocks; the rounded difference of a term counts twice, it is squared), at most 512 into the running sum, 3 into the
         ratio: (1026 + 512 + 3) * 2^-24 = 9.2e-5 on each side of the ratio, about 1.6e-4 in all.
  pick   ``yin_pick`` applied to the kernel's OWN d': f32 comparisons of f32 values are exact, so voicing and lag must agree at
         EVERY frame: the aperiodicity is bit for bit the d' at the restatement's lag (its minimum over the range in an unvoiced
         frame), and f0 is within 2^-24 * (8 + 8 max(a, b, c) / |a - 2 b + c|) relative, the rounding of the three-point
         interpolation (a - c and a - 2 b + c each carry up to 2^-24 max(a, b, c) of absolute error, their quotient is at most
         1/2 of a lag, the lag at least 2; the additions and the two divisions carry the rest).
  end to end, against the float64 d': the lag and the voicing agree on every frame that is not FRAGILE (a comparison of the pick
         within 4e-4 relative, twice the d' bound); fragile frames may be at most 5 % of all, so that the exemption cannot
         hide a failure.  The kernel's lag is the one ``yin_pick`` finds on the kernel's d', which the test before it has
         established."""
import os
import re

import numpy as np
import pytest
import torch

import pitch_ref as ref

pytestmark = pytest.mark.gpu

TAU_MIN, TAU_MAX, THR, GROSS = 45, 490, 0.1, 0.2
SLACK, SENTINEL = 2, -7.5
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_FRAMES = int(re.search(r"#define RTTS_PITCH_TILE_FRAMES (\d+)", open(os.path.join(ROOT, "include", "rtts.h")).read()).group(1))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _offsets(counts):
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    return off


def _launch(gpu, utts, hop=256, slack=SLACK, cmnd=True, tau=(TAU_MIN, TAU_MAX), thr=THR, sr=float(ref.SR)):
    """One rtts_pitch_yin launch over ``utts`` with frame slots ``slack`` wider than the utterances need, outputs pre-filled with
    the sentinel -> (f0, aperiodicity, cmnd or None as numpy arrays over the slots, frame offsets)."""
    from reformer_tts_amd import ops
    from reformer_tts_amd.dataset.audio import _host_array
    lens = [len(u) for u in utts]
    soff, foff = _offsets(lens), _offsets([n // hop + 1 + slack for n in lens])
    table = torch.tensor([soff, foff], dtype=torch.int64).to(gpu)
    audio = torch.from_numpy(np.concatenate(utts).astype(np.float32)).to(gpu)
    f0 = torch.full((foff[-1],), SENTINEL, dtype=torch.float32, device=gpu)
    ap = torch.full((foff[-1],), SENTINEL, dtype=torch.float32, device=gpu)
    cm = torch.full((foff[-1], ref.MAX_LAG + 1), SENTINEL, dtype=torch.float32, device=gpu) if cmnd else None
    ops.pitch_yin(audio, _host_array(soff), _host_array(foff), table, len(utts), hop, tau[0], tau[1], thr, sr, f0, ap, cm)
    torch.cuda.synchronize()
    return f0.cpu().numpy(), ap.cpu().numpy(), None if cm is None else cm.cpu().numpy(), foff


def _real(values, foff, utts, hop=256):
    """The frames the utterances own, slot by slot (the slack left out)."""
    return [values[foff[i]: foff[i] + len(u) // hop + 1] for i, u in enumerate(utts)]


@pytest.fixture(scope="module")
def batch():
    utts = list(ref.signals().values()) + [ref.seam_tone(TILE_FRAMES)]
    assert sum(len(u) // 256 + 1 for u in utts[:12]) == 181 and len(utts[12]) == (2 * TILE_FRAMES + 1) * 256
    return utts


@pytest.fixture(scope="module")
def oracle(batch):
    """Per utterance (d', d) in float64, computed once and left unchanged."""
    return [ref.yin_cmnd(u, 256) for u in batch]


@pytest.fixture(scope="module")
def run(gpu, batch):
    return _launch(gpu, batch)


def _check_cmnd(got, want, d, what):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    g, w, dd = got[:, 1:].astype(np.float64), want[:, 1:], d[:, 1:]
    assert (got[:, 0] == 1.0).all(), what
    zero = dd == 0.0
    assert np.array_equal(g[zero], w[zero]), f"{what}: d' where the oracle's d is 0"
    rel = np.abs(g - w)[~zero] / w[~zero]
    if rel.size:
        print(f"{what}: largest relative d' difference {rel.max():.3e} (bound 2e-4)")
        assert rel.max() <= 2e-4, what


def _check_pick(f0, ap, cm, tau=(TAU_MIN, TAU_MAX), thr=THR, sr=float(ref.SR)):
    """The kernel's f0 / aperiodicity against ``yin_pick`` on the kernel's own d' -> that pick."""
    p = ref.yin_pick(cm, tau[0], tau[1], np.float32(thr), sr)
    assert np.array_equal(f0 > 0, p["voiced"])
    want_ap = np.where(p["voiced"], cm[np.arange(len(f0)), p["tau"]], cm[:, tau[0]: tau[1] + 1].min(axis=1)).astype(np.float32)
    assert np.array_equal(ap.view(np.uint32), want_ap.view(np.uint32))
    for f in np.flatnonzero(p["voiced"]):
        a, b, c = (float(v) for v in cm[f, p["tau"][f] - 1: p["tau"][f] + 2])
        bound = U * (8.0 + 8.0 * max(a, b, c) / abs(a - 2.0 * b + c)) if (a > b and c >= b) else 8.0 * U
        assert abs(float(f0[f]) / p["f0"][f] - 1.0) <= bound, (f, float(f0[f]), p["f0"][f], bound)
    assert (f0[~p["voiced"]] == 0.0).all()
    return p


def test_cmnd_against_the_oracle(run, batch, oracle):
    _, _, cm, foff = run
    for i, (got, (want, d)) in enumerate(zip(_real(cm, foff, batch), oracle)):
        _check_cmnd(got, want, d, f"utterance {i}")


def test_pick_on_the_kernels_own_cmnd(run, batch):
    f0, ap, cm, foff = run
    voiced = 0
    for f, a, c in zip(_real(f0, foff, batch), _real(ap, foff, batch), _real(cm, foff, batch)):
        voiced += int(_check_pick(f, a, c)["voiced"].sum())
    assert voiced >= 100                                           # the tones are there


def test_end_to_end_against_the_float64_oracle(run, batch, oracle):
    f0, _, cm, foff = run
    frames = fragile = 0
    for i, (got_f0, got_cm, (want_cm, _)) in enumerate(zip(_real(f0, foff, batch), _real(cm, foff, batch), oracle)):
        want = ref.yin_pick(want_cm, TAU_MIN, TAU_MAX, THR, float(ref.SR))
        got = ref.yin_pick(got_cm, TAU_MIN, TAU_MAX, np.float32(THR), float(ref.SR))
        firm = ~want["fragile"]
        assert np.array_equal(got["tau"][firm], want["tau"][firm]) and np.array_equal((got_f0 > 0)[firm], want["voiced"][firm]), i
        for f in np.flatnonzero(firm & want["voiced"]):
            # same lag, same branch of the interpolation (a frame where that could differ is fragile): what is left is the offset
            # 0.5 (a - c) / (a - 2 b + c) computed from values 2e-4 apart.  With m = max(a, b, c) and q = a - 2 b + c the numerator
            # moves by at most 4e-4 m and q by 8e-4 m, |a - c| <= q, so to first order the offset moves by 6e-4 m / q lags;
            # 1e-3 m / q leaves room for the second order while 8e-4 m / q <= 0.1 (beyond that the offset is ill-conditioned and
            # only the lag is compared), and 1e-6 covers the f32 roundings of the pick itself
            tau = want["tau"][f]
            a, b, c = want_cm[f, tau - 1: tau + 2]
            tol = 1e-6
            if a > b and c >= b:
                r = max(a, b, c) / (a - 2.0 * b + c)
                if 8e-4 * r > 0.1:
                    continue
                tol += 1e-3 * r / (tau - 0.5)
            assert abs(float(got_f0[f]) / want["f0"][f] - 1.0) <= tol, (i, f, float(got_f0[f]), want["f0"][f], tol)
        frames += len(firm)
        fragile += int((~firm).sum())
    print(f"{fragile} fragile frames of {frames}")
    assert frames == 181 + 2 * TILE_FRAMES + 2 and fragile <= 0.05 * frames


def test_slack_keeps_the_sentinel(run, batch):
    f0, ap, cm, foff = run
    for i, u in enumerate(batch):
        lo, hi = foff[i] + len(u) // 256 + 1, foff[i + 1]
        assert hi - lo == SLACK
        assert (f0[lo:hi] == SENTINEL).all() and (ap[lo:hi] == SENTINEL).all() and (cm[lo:hi] == SENTINEL).all()


def test_each_utterance_alone_equals_its_place_in_the_batch(gpu, run, batch):
    f0, ap, cm, foff = run
    for i, u in enumerate(batch):
        f1, a1, c1, o1 = _launch(gpu, [u], slack=0)
        t = o1[1]
        assert np.array_equal(f1.view(np.uint32), f0[foff[i]: foff[i] + t].view(np.uint32)), i
        assert np.array_equal(a1.view(np.uint32), ap[foff[i]: foff[i] + t].view(np.uint32)), i
        assert np.array_equal(c1.view(np.uint32), cm[foff[i]: foff[i] + t].view(np.uint32)), i


def test_two_calls_agree_and_cmnd_is_optional(gpu, run, batch):
    f0, ap, cm, _ = run
    f2, a2, c2, _ = _launch(gpu, batch)
    assert np.array_equal(f2.view(np.uint32), f0.view(np.uint32)) and np.array_equal(a2.view(np.uint32), ap.view(np.uint32))
    assert np.array_equal(c2.view(np.uint32), cm.view(np.uint32))
    f3, a3, c3, _ = _launch(gpu, batch, cmnd=False)
    assert c3 is None and np.array_equal(f3.view(np.uint32), f0.view(np.uint32)) and np.array_equal(a3.view(np.uint32), ap.view(np.uint32))


@pytest.mark.parametrize("hop", [128, 512])
def test_the_other_hops(gpu, hop):
    """The glide and pause-tone-pause (its silence gives d = 0 rows), then a one-sample and a 300-sample utterance."""
    sig = ref.signals()
    utts = [sig["glide"], sig["pause_tone_pause"], sig["one"], sig["short300"]]
    f0, ap, cm, foff = _launch(gpu, utts, hop=hop)
    voiced = 0
    for i, u in enumerate(utts):
        t = len(u) // hop + 1
        want, d = ref.yin_cmnd(u, hop)
        _check_cmnd(cm[foff[i]: foff[i] + t], want, d, f"hop {hop}, utterance {i}")
        voiced += int(_check_pick(f0[foff[i]: foff[i] + t], ap[foff[i]: foff[i] + t], cm[foff[i]: foff[i] + t])["voiced"].sum())
        assert (f0[foff[i] + t: foff[i + 1]] == SENTINEL).all() and (cm[foff[i] + t: foff[i + 1]] == SENTINEL).all()
        f1, a1, c1, _ = _launch(gpu, [u], hop=hop, slack=0)
        assert np.array_equal(f1.view(np.uint32), f0[foff[i]: foff[i] + t].view(np.uint32))
        assert np.array_equal(c1.view(np.uint32), cm[foff[i]: foff[i] + t].view(np.uint32))
    assert voiced >= 6


@pytest.mark.parametrize("hop,where,value", [(256, 2501, np.nan), (256, 0, np.inf), (128, 5999, -np.inf), (512, 3000, np.nan)])
def test_a_non_finite_sample_reaches_exactly_the_frames_that_touch_it(gpu, hop, where, value):
    sig = ref.signals()
    clean = [sig["tone110"], sig["tone_noise"], sig["short300"]]
    dirty = [u.copy() for u in clean]
    dirty[1][where] = value
    f0, ap, _, foff = _launch(gpu, clean, hop=hop, cmnd=False)
    g0, gp, _, _ = _launch(gpu, dirty, hop=hop, cmnd=False)
    hit = np.zeros(len(f0), dtype=bool)
    t = len(dirty[1]) // hop + 1
    hit[foff[1]: foff[1] + t] = ref.touched(dirty[1], hop)
    want = [f for f in range(t) if f * hop - ref.REACH // 2 <= where < f * hop + ref.REACH // 2]
    assert np.flatnonzero(hit).tolist() == [foff[1] + f for f in want] and 3 <= len(want) <= ref.REACH // hop
    assert np.isnan(g0[hit]).all() and np.isnan(gp[hit]).all()
    assert np.array_equal(g0[~hit].view(np.uint32), f0[~hit].view(np.uint32))
    assert np.array_equal(gp[~hit].view(np.uint32), ap[~hit].view(np.uint32))


def test_a_captured_launch_replays_to_the_eager_bits(gpu, batch):
    from reformer_tts_amd import _graphs
    from reformer_tts_amd.evaluation import PitchTracker
    tracker = PitchTracker(f_min=45.0, f_max=490.0)
    assert (tracker.tau_min, tracker.tau_max, tracker.threshold) == (TAU_MIN, TAU_MAX, THR)
    tables = tracker.tables([len(u) for u in batch], gpu)
    audio = torch.from_numpy(np.concatenate(batch)).to(gpu)
    f0, ap, foff, cm = tracker.forward_packed(audio, tables=tables, return_cmnd=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _graphs.capturing(graph):
        g0, gp, _, gcm = tracker.forward_packed(audio, tables=tables, return_cmnd=True)
    for t in (g0, gp, gcm):
        t.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for eager, replayed in ((f0, g0), (ap, gp), (cm, gcm)):
        assert torch.equal(eager.view(torch.int32), replayed.view(torch.int32))
    assert foff == _offsets([len(u) // 256 + 1 for u in batch])


def test_tracker_forward_pads_with_zeros(gpu, run, batch):
    from reformer_tts_amd.evaluation import PitchTracker
    tracker = PitchTracker(f_min=45.0, f_max=490.0).to(gpu)
    picked = [batch[0], batch[7], batch[11]]
    padded, frames = tracker([torch.from_numpy(u).to(gpu) for u in picked])
    f0, _, _, foff = run
    assert frames.tolist() == [len(u) // 256 + 1 for u in picked] and tuple(padded.shape) == (3, 24)
    got = padded.cpu().numpy()
    for row, i in zip(got, (0, 7, 11)):
        t = len(batch[i]) // 256 + 1
        assert np.array_equal(row[:t].view(np.uint32), f0[foff[i]: foff[i] + t].view(np.uint32)) and (row[t:] == 0.0).all()
    lens = torch.tensor([len(u) for u in picked])
    stacked = torch.zeros(3, 6100)
    for k, u in enumerate(picked):
        stacked[k, :len(u)] = torch.from_numpy(u)
    again, _ = tracker(stacked.to(gpu), lens)
    assert torch.equal(again, padded)


def _perturbed(run, batch):
    """The batch's contours as b, and a perturbed copy as a: octave errors, a detune, voicing flipped both ways, T_a = T_b - 1 and
    T_a = T_b + 1.  -> (fa, offsets_a, fb, offsets_b) on the host."""
    f0, _, _, foff = run
    rng = np.random.default_rng(5)
    fb_parts = [p.copy() for p in _real(f0, foff, batch)]
    fa_parts = []
    for i, b in enumerate(fb_parts):
        a = b.copy()
        v = np.flatnonzero(a > 0)
        if len(v) >= 8:
            a[v[0:2]] *= 2.0                                       # octave up
            a[v[2]] *= 0.5                                         # octave down
            a[v[3]] *= np.float32(1.19)                            # inside the gross bound
            a[v[4]] *= np.float32(1.21)                            # outside
            a[v[5]] = 0.0                                          # voiced -> unvoiced
            a[v[6:]] *= (1.0 + 0.01 * rng.standard_normal(len(v) - 6)).astype(np.float32)
        u = np.flatnonzero(b == 0)
        if len(u) >= 2 and i != 4:
            a[u[0]] = 123.0                                        # unvoiced -> voiced
        if i == 0:
            a = a[:-1]
        if i == 1:
            a = np.concatenate([a, np.float32([77.0])])
        fa_parts.append(a.astype(np.float32))
    assert not (fb_parts[4] > 0).any()                             # the noise: nothing voiced in both contours
    return (np.concatenate(fa_parts), _offsets([len(p) for p in fa_parts]), np.concatenate(fb_parts), _offsets([len(p) for p in fb_parts]))


def test_compare_against_the_restatement(gpu, run, batch):
    from reformer_tts_amd import evaluation, ops
    fa, oa, fb, ob = _perturbed(run, batch)
    want = ref.f0_compare_ref(fa, oa, fb, ob, GROSS)
    assert want[0, 0] == 23 and want[1, 0] == 24 and want[4, 1] == 0 and (want[:, 3].sum() > 0) and (want[:, 4].sum() > 0)
    dev = [torch.from_numpy(np.asarray(x)).to(gpu) for x in (fa, oa, fb, ob)]
    got = ops.f0_compare(*dev, GROSS).cpu().numpy()
    again = ops.f0_compare(*dev, GROSS).cpu().numpy()
    assert got.shape == (len(batch) + 1, 5) and np.array_equal(got, again)
    assert np.array_equal(got[:, [0, 1, 3, 4]], want[:, [0, 1, 3, 4]])
    assert (np.abs(got[:, 2] - want[:, 2]) <= 1e-12 * want[:, 2]).all()
    res = evaluation.f0_errors(dev[0], oa, dev[2], ob, GROSS)
    assert np.array_equal(res["counts"].cpu().numpy(), got)
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = np.where(got[:, 1] == 0, np.nan, np.sqrt(got[:, 2] / got[:, 1]))
        ffe = np.where(got[:, 0] == 0, np.nan, (got[:, 3] + got[:, 4]) / got[:, 0])
    assert res["rmse_cents"].dtype == torch.float64 and res["rmse_cents"].is_cuda
    assert np.allclose(res["rmse_cents"].cpu().numpy(), rmse[:-1], rtol=1e-14, atol=0.0, equal_nan=True) and np.isnan(rmse[4])
    assert np.allclose(res["ffe"].cpu().numpy(), ffe[:-1], rtol=1e-14, atol=0.0, equal_nan=True)
    assert np.allclose(res["totals"].cpu().numpy()[[0, 3]], [rmse[-1], ffe[-1]], rtol=1e-14, atol=0.0)


def test_compare_a_nan_contour_makes_its_row_and_the_totals_nan(gpu, run, batch):
    from reformer_tts_amd import ops
    fa, oa, fb, ob = _perturbed(run, batch)
    want_clean = ref.f0_compare_ref(fa, oa, fb, ob, GROSS)
    fb = fb.copy()
    fb[ob[3] + 5] = np.nan
    fa[oa[1 + 1] - 1] = np.nan                                     # the frame of utterance 1 past T_b: not compared, reaches nothing
    got = ops.f0_compare(*[torch.from_numpy(np.asarray(x)).to(gpu) for x in (fa, oa, fb, ob)], GROSS).cpu().numpy()
    assert np.isnan(got[3]).all() and np.isnan(got[-1]).all()
    keep = [s for s in range(len(batch)) if s != 3]
    assert np.array_equal(got[keep][:, [0, 1, 3, 4]], want_clean[keep][:, [0, 1, 3, 4]])


def test_audio_f0_errors_of_a_batch_against_itself_and_a_detuned_copy(gpu, batch):
    from reformer_tts_amd.evaluation import PitchTracker, audio_f0_errors
    tracker = PitchTracker(f_min=45.0, f_max=490.0)
    waves = [torch.from_numpy(u).to(gpu) for u in (batch[0], batch[4], batch[2])]
    same = audio_f0_errors(waves, waves, tracker)
    rmse = same["rmse_cents"].cpu().numpy()
    assert rmse[0] == 0.0 and np.isnan(rmse[1]) and rmse[2] == 0.0 and (same["ffe"].cpu().numpy() == 0.0).all()
    rng = np.random.default_rng(3)
    other = [torch.from_numpy(ref.tone(113.0, 6000, rng).astype(np.float32)).to(gpu), waves[1], waves[2][:5000]]
    res = audio_f0_errors(other, waves, tracker)
    # each side is within 0.5 % of its tone at every voiced frame (tests/test_pitch_cpu.py holds the oracle to that): 8.6 cents a side
    cents = 1200.0 * np.log2(113.0 / 110.0)
    assert abs(res["rmse_cents"][0].item() - cents) <= 2.0 * 1200.0 * np.log2(1.005) and res["gpe"][0].item() == 0.0
    assert res["counts"][2, 0].item() == 5000 // 256 + 1


def test_validations_reject_without_launching(gpu):
    from reformer_tts_amd import _lib, ops
    from reformer_tts_amd.dataset.audio import _host_array
    audio = torch.zeros(6000, device=gpu)
    soff, foff = [0, 6000], [0, 24]
    table = torch.tensor([soff, foff], dtype=torch.int64).to(gpu)
    f0 = torch.full((24,), SENTINEL, device=gpu)
    ap = torch.full((24,), SENTINEL, device=gpu)
    good = dict(hop=256, tau_min=TAU_MIN, tau_max=TAU_MAX, threshold=THR, sample_rate=22050.0)
    for change, word in ((dict(hop=192), "hop"), (dict(tau_min=1), "tau_min"), (dict(tau_max=512), "tau_max"), (dict(threshold=1.5), "threshold"),
                         (dict(sample_rate=-1.0), "sample_rate")):
        kw = dict(good, **change)
        with pytest.raises(_lib.RttsError, match=word):
            ops.pitch_yin(audio, _host_array(soff), _host_array(foff), table, 1, kw["hop"], kw["tau_min"], kw["tau_max"], kw["threshold"],
                          kw["sample_rate"], f0, ap)
    with pytest.raises(_lib.RttsError, match="frame_offsets"):
        ops.pitch_yin(audio, _host_array(soff), _host_array([0, 23]), table, 1, 256, TAU_MIN, TAU_MAX, THR, 22050.0, f0, ap)
    with pytest.raises(_lib.RttsError, match="sample_offsets"):
        ops.pitch_yin(audio, _host_array([0, 0]), _host_array(foff), table, 1, 256, TAU_MIN, TAU_MAX, THR, 22050.0, f0, ap)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        ops.pitch_yin(audio.cpu(), _host_array(soff), _host_array(foff), table, 1, 256, TAU_MIN, TAU_MAX, THR, 22050.0, f0, ap)
    offs = torch.tensor(foff, dtype=torch.int64).to(gpu)
    with pytest.raises(_lib.RttsError, match="gross"):
        ops.f0_compare(f0, offs, ap, offs, 1.0)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        ops.f0_compare(f0.cpu(), offs, ap, offs)
    torch.cuda.synchronize()
    assert (f0 == SENTINEL).all() and (ap == SENTINEL).all()
