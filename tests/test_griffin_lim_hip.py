"""rtts_gl_magnitudes / rtts_gl_init / rtts_gl_step (csrc/griffin_lim.hip) and griffin_lim.GriffinLim on the GPU, against the float64
restatement of tests/griffin_lim_ref.py.

The bounds are set in the tests themselves.  Magnitudes: the elementwise a-priori bound of an f32 fmaf chain over the mel channels
(griffin_lim_ref.magnitude_bound).  init, one step and the chain of four: the float32 twin of griffin_lim_ref.py (the package's own
f32 bases as f32 matmuls) is measured against float64 on the test's own inputs, relative to each utterance's peak, and the kernels
-- the same arithmetic as k-ordered f32 chains -- get 4 x the twin's worst value over the batch.  Convergence is a condition, not a
tolerance: 32 iterations of the kernels must reach a spectral error no larger than 16 iterations of the float64 reference from the
same start.  Every test prints its figures.
Measured on an MI355X (worst over the batch, relative to the utterance's peak; twin -> bound; kernel):
    init, hash phases     7.94e-07 -> 3.18e-06; 1.33e-06          init, zero phases     9.23e-07 -> 3.69e-06; 1.58e-06
    step, momentum 0      9.77e-06 -> 3.91e-05; 9.28e-06          step, momentum 0.99   3.74e-06 -> 1.49e-05; 2.89e-06
    step from silence     9.23e-07 -> 3.69e-06; 1.58e-06          chain of 4            4.16e-05 -> 1.67e-04; 2.16e-05
    convergence, momentum 0:    L 30: d_0 0.654, float64 d_16 0.237, kernel d_32 0.198;  L 61: 0.656, 0.239, 0.203
    convergence, momentum 0.99: L 30: d_0 0.654, float64 d_16 0.202, kernel d_32 0.159;  L 61: 0.656, 0.174, 0.135
    mel_round_trip_error of 4 iterations on 7 / 20 / 3 / 13 frames: 0.237, 0.244, 0.206, 0.176"""
import ctypes

import numpy as np
import pytest
import torch

import griffin_lim_ref as ref

pytestmark = pytest.mark.gpu

N_FFT, HOP, BINS, N_MELS = 1024, 256, 513, 80
# one ragged batch: 1 and 2 frames give zeros, 3 is the shortest that runs; 30 / 31 are the last frame count of one tile and the
# first of two, 59 / 60 the last of two tiles and the first of three (a tile completes 29 hops)
FRAMES = [1, 2, 3, 4, 27, 28, 29, 30, 31, 59, 60, 61]
SEED = 7


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def creator(gpu):
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram
    return Tacotron2Spectrogram(22050, N_FFT, N_FFT, HOP, N_MELS).to(gpu)


def _gl(creator, **kw):
    from reformer_tts_amd.griffin_lim import GriffinLim
    return GriffinLim(creator, **kw)


def _mel_of(creator, frames, seed):
    """(n_mels, frames) f32: the first frames of the voiced test signal's own log-mel (float64 on the host, rounded once)."""
    x = ref.voiced_signal(HOP * max(frames, 3), seed)
    return ref.log_mel_f64(x, creator.mel_basis.cpu().numpy(), creator.power)[:, :frames].astype(np.float32)


def _padded(mels, gpu, fill=float("nan")):
    """(B, n_mels, Lmax) on the device; the frames behind each utterance are NaN: whoever reads them is seen."""
    out = torch.full((len(mels), N_MELS, max(m.shape[1] for m in mels)), fill)
    for i, m in enumerate(mels):
        out[i, :, :m.shape[1]] = torch.from_numpy(m)
    return out.to(gpu)


@pytest.fixture(scope="module")
def case(gpu, creator):
    """The ragged batch and what every test shares, computed once and left unchanged: the mels, the f32 pseudo-inverse and bases, the
    float64 magnitudes and their f32 rounding (the kernels' input in the init / step tests), the fixed signals of the step tests."""
    from reformer_tts_amd.dataset.audio import dft_basis, idft_basis
    gl = _gl(creator)
    mels = [_mel_of(creator, n, 10 + i) for i, n in enumerate(FRAMES)]
    pinv = gl.pinv.cpu().numpy()
    mags = [ref.magnitudes_f64(m, pinv, 1)[1] for m in mels]
    mags32 = [m.astype(np.float32) for m in mags]
    cur = [ref.voiced_signal(HOP * n, 500 + i).astype(np.float32) for i, n in enumerate(FRAMES)]
    prev = [ref.voiced_signal(HOP * n, 600 + i).astype(np.float32) for i, n in enumerate(FRAMES)]
    return dict(gl=gl, mels=mels, pinv=pinv, mags=mags, mags32=mags32, cur=cur, prev=prev, tables=gl.tables(FRAMES),
                dft32=dft_basis(N_FFT, N_FFT).numpy(), idft32=idft_basis(N_FFT, N_FFT).numpy(),
                mag_dev=torch.from_numpy(np.concatenate(mags32, axis=1)).to(gpu))


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def _split(packed, off):
    host = packed.cpu().numpy()
    return [host[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _check_against(name, got, truth, twin):
    """Every utterance of ``got`` within 4 x the twin's worst error over the batch, relative to the utterance's peak; utterances of
    fewer than three frames are exactly zero.  -> (twin's worst, the kernel's worst)."""
    long = [i for i, n in enumerate(FRAMES) if n >= 3]
    for i, n in enumerate(FRAMES):
        assert got[i].shape == (HOP * n,)
        if n < 3:
            assert not truth[i].any() and not twin[i].any() and not got[i].any(), f"{name}: L = {n} gives zeros"
    t_err = [_rel(twin[i], truth[i]) for i in long]
    k_err = [_rel(got[i], truth[i]) for i in long]
    bound = 4.0 * max(t_err)
    print(f"{name}: f32 twin vs float64, worst over the batch, relative to the peak {max(t_err):.3e} -> bound {bound:.3e}; "
          f"kernel per utterance {['%.2e' % e for e in k_err]}, worst {max(k_err):.3e}")
    assert 0.0 < max(t_err) < 1e-3
    assert max(k_err) <= bound, (name, k_err, bound)
    return max(t_err), max(k_err)


# ------------------------------------------------------------------ 1. magnitudes
def test_magnitudes_against_float64(gpu, case):
    from reformer_tts_amd import ops
    gl, t, mels, pinv = case["gl"], case["tables"], case["mels"], case["pinv"]
    padded = _padded(mels, gpu)
    packed = torch.from_numpy(np.concatenate(mels, axis=1)).to(gpu)
    strided = padded.permute(0, 2, 1).contiguous().permute(0, 2, 1)                 # the same values, frames no longer fastest
    assert strided.stride() != padded.stride()
    for power in (1, 2):
        outs = []
        for mel, start_host, row in ((padded, [0] * len(FRAMES), 3), (packed, t.mel_offsets, 2), (strided, [0] * len(FRAMES), 3)):
            mag = torch.full((BINS, t.col_offsets[-1] + 3), -7.0, device=gpu)
            ops.gl_magnitudes(mel, start_host, t.device_table[row], t.coff_host, t.device_table[:2], len(FRAMES), gl.pinv, power, N_FFT, mag)
            assert bool((mag[:, t.col_offsets[-1]:] == -7.0).all()), "columns past the offsets are not written"
            outs.append(mag[:, :t.col_offsets[-1]].cpu().numpy())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), "padded, packed and strided layouts give the same bits"
        worst = 0.0
        for i, n in enumerate(FRAMES):
            got = outs[0][:, t.col_offsets[i]:t.col_offsets[i + 1]].astype(np.float64)
            a, m = ref.magnitudes_f64(mels[i], pinv, power)
            assert got.shape == (BINS, n + 1) and np.array_equal(got[:, n], got[:, n - 1]) and float(got.min()) >= 0.0
            # power 2: the square root is not Lipschitz at 0, so the comparison is made on A = M^2 (sqrt and the square: 4 u more)
            bound = ref.magnitude_bound(mels[i], pinv) + (4 * 2.0 ** -24 * a if power == 2 else 0.0)
            err = np.abs(got ** power - a)
            live = bound > 0                                          # bins above the last mel filter have a zero row of P: exactly 0
            worst = max(worst, float((err[live] / bound[live]).max()))
            assert bool((err <= bound).all()), (power, n, float((err[live] / bound[live]).max()))
            assert float(m.max()) > 1e-3 and float((a == 0).mean()) > 0.0, "the clamp is seen on this input"
        print(f"power {power}: |A_kernel - A_f64| / bound, worst over the batch {worst:.3f}")


# ------------------------------------------------------------------ 2. init
def _init(case, gpu, phase, seed=SEED, out=None):
    from reformer_tts_amd import ops
    gl, t = case["gl"], case["tables"]
    out = torch.full((t.sample_offsets[-1],), float("nan"), device=gpu) if out is None else out
    ops.gl_init(case["mag_dev"], t.coff_host, t.soff_host, t.device_table[:2], len(FRAMES), gl.dft_basis, gl.idft_basis, phase, seed, N_FFT,
                HOP, out)
    return out


@pytest.mark.parametrize("phase", ["hash", "zero"])
def test_init_against_float64(gpu, case, phase):
    got = _split(_init(case, gpu, phase), case["tables"].sample_offsets)
    truth = [ref.init_f64(m, phase, SEED) for m in case["mags32"]]
    twin = [ref.init_f32_twin(m, case["dft32"], case["idft32"], phase, SEED) for m in case["mags32"]]
    _check_against(f"init {phase}", got, truth, twin)
    if phase == "hash":
        other = _split(_init(case, gpu, "hash", SEED + 1), case["tables"].sample_offsets)
        assert not np.array_equal(other[5], got[5]), "the seed is seen"


# ------------------------------------------------------------------ 3. one step
def _step(case, gpu, cur, prev, beta):
    from reformer_tts_amd import ops
    gl, t = case["gl"], case["tables"]
    dev = lambda parts: torch.from_numpy(np.concatenate(parts)).to(gpu)    # noqa: E731
    out = torch.full((t.sample_offsets[-1],), float("nan"), device=gpu)
    ops.gl_step(dev(cur), None if prev is None else dev(prev), beta, case["mag_dev"], t.coff_host, t.soff_host, t.device_table[:2],
                len(FRAMES), gl.dft_basis, gl.idft_basis, N_FFT, HOP, out)
    return out


@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_one_step_against_float64(gpu, case, momentum):
    beta = momentum / (1.0 + momentum)
    prev = case["prev"] if momentum > 0 else None
    got = _split(_step(case, gpu, case["cur"], prev, beta), case["tables"].sample_offsets)
    pv = prev or [None] * len(FRAMES)
    truth = [ref.step_f64(m, c, p, beta) for m, c, p in zip(case["mags32"], case["cur"], pv)]
    twin = [ref.step_f32_twin(m, c, p, beta, case["dft32"], case["idft32"]) for m, c, p in zip(case["mags32"], case["cur"], pv)]
    _check_against(f"step momentum {momentum}", got, truth, twin)
    if momentum > 0:
        plain = _split(_step(case, gpu, case["cur"], None, 0.0), case["tables"].sample_offsets)
        assert not np.array_equal(plain[5], got[5]), "prev is seen"
        ignored = _step(case, gpu, case["cur"], prev, 0.0)
        assert torch.equal(ignored, _step(case, gpu, case["cur"], None, 0.0)), "beta = 0 does not read prev"


def test_step_from_silence_returns_istft_of_m(gpu, case):
    """|R| = 0 everywhere: R / |R| = 1, the step returns iSTFT(M) -- the zero-phase start, bit for bit."""
    zeros = [np.zeros(HOP * n, dtype=np.float32) for n in FRAMES]
    out = _step(case, gpu, zeros, zeros, 0.5)
    got = _split(out, case["tables"].sample_offsets)
    truth = [ref.init_f64(m, "zero") for m in case["mags32"]]
    twin = [ref.step_f32_twin(m, z, None, 0.0, case["dft32"], case["idft32"]) for m, z in zip(case["mags32"], zeros)]
    _check_against("step from silence", got, truth, twin)
    assert torch.equal(out, _init(case, gpu, "zero"))


# ------------------------------------------------------------------ 4. a chain of four iterations
def test_chain_of_four_against_float64(gpu, creator, case):
    gl = _gl(creator, n_iter=4, momentum=0.99, seed=SEED)
    waves = gl(_padded(case["mels"], gpu), FRAMES)
    got = [w.cpu().numpy() for w in waves]
    truth = [ref.griffin_lim_f64(m, 4, 0.99, "hash", SEED)[4] for m in case["mags"]]
    twin = [ref.griffin_lim_f32_twin(ref.magnitudes_f32_twin(mel, case["pinv"], 1), 4, 0.99, case["dft32"], case["idft32"], "hash", SEED)[4]
            for mel in case["mels"]]
    _check_against("chain of 4", got, truth, twin)
    # the packed layout a creator's forward_packed returns gives the same bits
    packed, off = gl.forward_packed(torch.from_numpy(np.concatenate(case["mels"], axis=1)).to(gpu), FRAMES)
    assert off == case["tables"].sample_offsets and torch.equal(packed, torch.cat(waves))
    # n_iter = 0 is the start, and the rotation of the three buffers returns the right one for every n_iter mod 3
    start = _gl(creator, n_iter=0, seed=SEED)(_padded(case["mels"], gpu), FRAMES)
    for k in (1, 2, 3):
        step_by_step = _gl(creator, n_iter=k, momentum=0.99, seed=SEED)(_padded(case["mels"], gpu), FRAMES)
        assert not torch.equal(step_by_step[9], start[9])
        want = ref.griffin_lim_f64(case["mags"][9], k, 0.99, "hash", SEED)[k]
        assert _rel(step_by_step[9].cpu().numpy(), want) <= 1e-4, k


# ------------------------------------------------------------------ 5. convergence
@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_32_iterations_beat_16_in_float64(gpu, creator, case, momentum):
    """d_k = || |STFT(x_k)| - M || / || M ||, measured on the host in float64 from the audio."""
    frames = [30, 61]
    idx = [FRAMES.index(n) for n in frames]
    mels = [case["mels"][i] for i in idx]
    waves = _gl(creator, n_iter=32, momentum=momentum, seed=SEED)(_padded(mels, gpu), frames)
    for i, w, n in zip(idx, waves, frames):
        mag = case["mags"][i]
        truth = ref.griffin_lim_f64(mag, 16, momentum, "hash", SEED)
        d0, d16, d32 = ref.spectral_error(truth[0], mag), ref.spectral_error(truth[16], mag), ref.spectral_error(w.cpu().numpy(), mag)
        print(f"L {n} momentum {momentum}: d_0 {d0:.4f}, float64 d_16 {d16:.4f}, kernel d_32 {d32:.4f}")
        assert d32 <= d16 < d0, (n, momentum, d0, d16, d32)


# ------------------------------------------------------------------ 6. independence
def test_batch_independence_and_untouched_memory(gpu, creator, case):
    from reformer_tts_amd import ops
    gl = _gl(creator, n_iter=3, momentum=0.99, seed=SEED)
    mels = case["mels"]
    batch = gl(_padded(mels, gpu), FRAMES)
    again = gl(_padded(mels, gpu), FRAMES)
    rev = gl(_padded(mels[::-1], gpu), FRAMES[::-1])[::-1]
    for i, n in enumerate(FRAMES):
        alone = gl(_padded([mels[i]], gpu), [n])[0]
        assert alone.numel() == HOP * n
        assert torch.equal(alone, batch[i]) and torch.equal(rev[i], batch[i]) and torch.equal(again[i], batch[i]), n
        assert (n >= 3) == bool(batch[i].abs().max() > 0), f"L = {n}: zeros exactly when fewer than three frames"
    # sentinels: samples in front of the first offset and behind the last are neither read (NaN) nor written (-7 stays)
    t = case["tables"]
    lead, tail, total = 5, 9, t.sample_offsets[-1]
    soff = [lead + o for o in t.sample_offsets]
    host = (ctypes.c_int64 * len(soff))(*soff)
    table = torch.tensor([soff, t.col_offsets], dtype=torch.int64, device=gpu)
    base = case["gl"]
    cur = torch.full((lead + total + tail,), float("nan"), device=gpu)
    cur[lead:lead + total] = torch.from_numpy(np.concatenate(case["cur"])).to(gpu)
    prv = torch.full_like(cur, float("nan"))
    prv[lead:lead + total] = torch.from_numpy(np.concatenate(case["prev"])).to(gpu)
    out = torch.full_like(cur, -7.0)
    ops.gl_step(cur, prv, 0.25, case["mag_dev"], t.coff_host, host, table, len(FRAMES), base.dft_basis, base.idft_basis, N_FFT, HOP, out)
    assert bool((out[:lead] == -7.0).all()) and bool((out[lead + total:] == -7.0).all())
    assert torch.equal(out[lead:lead + total], _step(case, gpu, case["cur"], case["prev"], 0.25))
    out.fill_(-7.0)
    ops.gl_init(case["mag_dev"], t.coff_host, host, table, len(FRAMES), base.dft_basis, base.idft_basis, "hash", SEED, N_FFT, HOP, out)
    assert bool((out[:lead] == -7.0).all()) and bool((out[lead + total:] == -7.0).all())
    assert torch.equal(out[lead:lead + total], _init(case, gpu, "hash"))
    # two calls into one buffer with a gap between their slots (utterances of 4 and of 31 frames): the gap keeps the sentinel
    whole = _split(_step(case, gpu, case["cur"], None, 0.0), t.sample_offsets)
    buf = torch.full((HOP * 4 + 300 + HOP * 31,), float("nan"), device=gpu)
    out = torch.full_like(buf, -7.0)
    slots = ((3, 0), (8, HOP * 4 + 300))
    for i, lo in slots:
        buf[lo:lo + HOP * FRAMES[i]] = torch.from_numpy(case["cur"][i]).to(gpu)
    for i, lo in slots:
        so, co = [lo, lo + HOP * FRAMES[i]], [t.col_offsets[i], t.col_offsets[i + 1]]
        ops.gl_step(buf, None, 0.0, case["mag_dev"], (ctypes.c_int64 * 2)(*co), (ctypes.c_int64 * 2)(*so),
                    torch.tensor([so, co], dtype=torch.int64, device=gpu), 1, base.dft_basis, base.idft_basis, N_FFT, HOP, out)
    assert bool((out[HOP * 4:HOP * 4 + 300] == -7.0).all())
    for i, lo in slots:
        assert np.array_equal(out[lo:lo + HOP * FRAMES[i]].cpu().numpy(), whole[i])


def test_tables_are_the_mel_tables_of_the_audio(gpu, case):
    from reformer_tts_amd.dataset.audio import MelTables
    t = case["tables"]
    m = MelTables([HOP * n for n in FRAMES], HOP, gpu)
    assert t.col_offsets == m.frame_offsets and t.sample_offsets == m.sample_offsets
    assert torch.equal(t.device_table[:2], m.device_table)


# ------------------------------------------------------------------ 7. graph replay
def test_graph_capture_replays_on_a_new_mel(gpu, creator):
    from reformer_tts_amd import _graphs
    frames = [31, 2, 4, 60]
    gl = _gl(creator, n_iter=5, momentum=0.99, seed=SEED)
    tables = gl.tables(frames)
    mel_buf = _padded([_mel_of(creator, n, 300 + i) for i, n in enumerate(frames)], gpu, fill=0.0)
    gl.forward_packed(mel_buf, tables=tables)                      # warm-up: the LDS attributes are set outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _graphs.capturing(graph):
        out, off = gl.forward_packed(mel_buf, tables=tables)
    assert off == [0, HOP * 31, HOP * 33, HOP * 37, HOP * 97]
    for seed in (400, 500):
        new = _padded([_mel_of(creator, n, seed + i) for i, n in enumerate(frames)], gpu, fill=0.0)
        mel_buf.copy_(new)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager, _ = gl.forward_packed(new, frames)
        assert torch.equal(out, eager), f"replay on the mel of seed {seed} differs from the eager call"
        assert bool((out[HOP * 31:HOP * 33] == 0).all()) and bool(out[:HOP * 31].abs().max() > 0)


# ------------------------------------------------------------------ 8. wiring
def test_synthesis_wiring(gpu, creator, case):
    from reformer_tts_amd import synthesis
    from reformer_tts_amd.squeeze_wave import Denoiser
    gl = synthesis.GriffinLim(creator, n_iter=4, seed=SEED)
    frames = [7, 20, 3, 13]
    spec = _padded([_mel_of(creator, 20, 700 + i) for i in range(4)], gpu)           # every utterance generated to 20 frames
    stop = torch.tensor(frames)
    waves = synthesis.vocode_trimmed(gl, spec, stop)
    assert [w.numel() for w in waves] == [HOP * n for n in frames]
    for i, n in enumerate(frames):
        assert torch.equal(waves[i], gl(spec[i:i + 1, :, :n], [n])[0]), "each utterance as its own trimmed call"
    graphed = synthesis.vocode_trimmed(gl, spec, stop, use_graph=True)               # no capture_ragged: the stage runs eagerly
    assert all(torch.equal(a, b) for a, b in zip(graphed, waves))
    g = torch.Generator().manual_seed(77)
    d = Denoiser(bias_spec=torch.rand(BINS, generator=g) * 0.05).to(gpu)
    clean = synthesis.vocode_trimmed(gl, spec, stop, denoiser=d, denoiser_strength=0.5)
    want = d(waves, strength=0.5)
    assert all(torch.equal(a, b) for a, b in zip(clean, want)) and not torch.equal(clean[1], waves[1])
    err = synthesis.mel_round_trip_error(waves, spec, frames, creator)
    print(f"mel_round_trip_error of 4 iterations: {[round(float(e), 4) for e in err]}")
    assert tuple(err.shape) == (4,) and bool(torch.isfinite(err).all()) and bool((err > 0).all())
    packed, views = gl.infer_ragged(spec, frames, sigma=0.6)
    assert packed.numel() == HOP * sum(frames) and all(torch.equal(a, b) for a, b in zip(views, waves))
    assert all(torch.equal(a, b) for a, b in zip(gl.split_packed(packed, [0, 7, 27, 30, 43]), waves))


# ------------------------------------------------------------------ 9. refusals
def test_refusals_name_the_argument(gpu, creator, case):
    from reformer_tts_amd import _lib, ops
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram, dft_basis, idft_basis
    from reformer_tts_amd.griffin_lim import GriffinLim
    gl = case["gl"]
    n = HOP * 16
    t = gl.tables([16])
    mag = torch.ones(BINS, 17, device=gpu)
    cur, out = torch.zeros(n, device=gpu), torch.full((n,), -7.0, device=gpu)

    def step(cur=cur, prev=None, out=out, n_fft=N_FFT, hop=HOP, mag=mag, bases=None, beta=0.5):
        dft, idft = bases or (gl.dft_basis, gl.idft_basis)
        ops.gl_step(cur, prev, beta, mag, t.coff_host, t.soff_host, t.device_table[:2], 1, dft, idft, n_fft, hop, out)

    def init(out=out, n_fft=N_FFT, hop=HOP, mag=mag, bases=None):
        dft, idft = bases or (gl.dft_basis, gl.idft_basis)
        ops.gl_init(mag, t.coff_host, t.soff_host, t.device_table[:2], 1, dft, idft, "hash", 0, n_fft, hop, out)

    for n_fft in (512, 2048):                                            # other n_fft / hop
        with pytest.raises(ValueError, match="creator: supported are n_fft"):
            GriffinLim(Tacotron2Spectrogram(22050, n_fft, n_fft, n_fft // 4, N_MELS))
        bases = (dft_basis(n_fft, n_fft).to(gpu), idft_basis(n_fft, n_fft).to(gpu))
        small = torch.ones(n_fft // 2 + 1, 17, device=gpu)
        with pytest.raises(_lib.RttsError, match="rtts_gl_step: n_fft must be 1024"):
            step(n_fft=n_fft, hop=n_fft // 4, mag=small, bases=bases)
        with pytest.raises(_lib.RttsError, match="rtts_gl_init: n_fft must be 1024"):
            init(n_fft=n_fft, hop=n_fft // 4, mag=small, bases=bases)
    for hop in (128, 512):
        with pytest.raises(_lib.RttsError, match="rtts_gl_step: hop must be 256"):
            step(hop=hop)
        with pytest.raises(_lib.RttsError, match="rtts_gl_init: hop must be 256"):
            init(hop=hop)
    buf = torch.zeros(3 * n, device=gpu)                                 # out overlapping an input
    for c, o in ((buf[:n], buf[:n]), (buf[:n], buf[100:n + 100]), (buf[100:n + 100], buf[:n])):
        with pytest.raises(_lib.RttsError, match="rtts_gl_step: out must not overlap cur"):
            step(cur=c, out=o)
        with pytest.raises(_lib.RttsError, match="rtts_gl_step: out must not overlap prev"):
            step(cur=buf[2 * n:], prev=c, out=o)
    step(cur=buf[:n], prev=buf[n:2 * n], out=buf[2 * n:])                # adjacent is not overlapping
    for kw, word in ((dict(out=torch.zeros(n - 1, device=gpu)), "out has"), (dict(cur=torch.zeros(n - 1, device=gpu)), "cur has"),
                     (dict(prev=torch.zeros(n - 1, device=gpu)), "prev has"), (dict(mag=torch.ones(BINS, 16, device=gpu)), "mag has"),
                     (dict(mag=torch.ones(BINS - 1, 17, device=gpu)), "mag must be")):       # offsets past a buffer
        with pytest.raises(ValueError, match=word):
            step(**kw)
    with pytest.raises(ValueError, match="out has"):
        init(out=torch.zeros(n - 1, device=gpu))
    with pytest.raises(ValueError, match="mag has"):
        init(mag=torch.ones(BINS, 16, device=gpu))
    mel = torch.zeros(1, N_MELS, 16, device=gpu)
    with pytest.raises(ValueError, match="mel_start / col_offsets"):     # 16 frames wanted, 15 there
        ops.gl_magnitudes(mel[:, :, :15], [0], t.device_table[3], t.coff_host, t.device_table[:2], 1, gl.pinv, 1, N_FFT, mag)
    with pytest.raises(ValueError, match="mel_start / col_offsets"):
        ops.gl_magnitudes(mel[0], [1], t.device_table[3], t.coff_host, t.device_table[:2], 1, gl.pinv, 1, N_FFT, mag)
    with pytest.raises(ValueError, match="mel must be"):
        ops.gl_magnitudes(mel[:, :79], [0], t.device_table[3], t.coff_host, t.device_table[:2], 1, gl.pinv, 1, N_FFT, mag)
    with pytest.raises(_lib.RttsError, match="rtts_gl_magnitudes: power"):
        ops.gl_magnitudes(mel, [0], t.device_table[3], t.coff_host, t.device_table[:2], 1, gl.pinv, 3, N_FFT, mag)
    for kw in (dict(cur=cur.cpu()), dict(out=out.cpu()), dict(prev=cur.cpu()), dict(mag=mag.cpu()),
               dict(bases=(gl.dft_basis.cpu(), gl.idft_basis))):         # a CPU tensor
        with pytest.raises(_lib.RttsError, match="GPU only"):
            step(**kw)
    with pytest.raises(_lib.RttsError, match="GPU only: out"):
        init(out=out.cpu())
    with pytest.raises(_lib.RttsError, match="GPU only: mel"):
        ops.gl_magnitudes(mel.cpu(), [0], t.device_table[3], t.coff_host, t.device_table[:2], 1, gl.pinv, 1, N_FFT, mag)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        gl(mel.cpu(), [16])
    with pytest.raises(ValueError, match="noise"):                       # noise given to infer_ragged
        gl.infer_ragged(mel, [16], noise=[[torch.zeros(1, device=gpu)]])
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((mag == 1.0).all()), "a refused call wrote nothing"
