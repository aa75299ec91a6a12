"""The SqueezeWave likelihood on the GPU: the three kernels of the analysis direction against float64, ``forward`` / ``nll``
against the reference's fixture, the flow's invertibility, and the ragged and captured paths against per-utterance calls.

Tolerances of the model-level tests: ``tests/sw_likelihood_ref.py`` holds a bf16 rounding model of the executor; its error
against the float64 forward on the fixture inputs (``MODEL_ERR``, re-measured by tests/test_sw_likelihood_cpu.py) is

    tag     z max err   z mean err   loss diff
    small   5.852e-3    7.983e-4     6.671e-5
    full    5.212e-3    8.648e-4     1.672e-5

and the bound is 4x that: the model rounds at operand boundaries only, the kernels also differ in accumulation order and in
exp / tanh.  4x stays under the inference golden's 3e-2 / 4e-3 (small: 2.34e-2 / 3.19e-3, full: 2.08e-2 / 3.46e-3)."""
import math
import os

import numpy as np
import pytest
import torch

import sw_likelihood_ref as ref64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "squeezewave_likelihood.npz"))


def _s():
    return torch.cuda.current_stream().cuda_stream


def _build(golden_dir, tag, gpu):
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    cfg, sd, mel, audio = ref64.load_case(golden_dir, tag)
    model = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                        cfg["early_return_size"], WNConfig(**cfg["wn_config"]))
    model.load_state_dict(sd, strict=False)
    return model.to(gpu).eval(), mel.to(gpu), audio.to(gpu)


@pytest.fixture(scope="module")
def cases(golden_dir, gpu):
    """tag -> (model on the GPU in eval mode, golden mel, golden audio): built once, never modified by a test."""
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = _build(golden_dir, tag, gpu)
        return cache[tag]
    return get


def _bounds(tag):
    return tuple(4 * v for v in ref64.MODEL_ERR[tag])


# ------------------------------------------------------------------ 1. the boundary kernel
BOUNDARY_CASES = [  # (n_in, n_early, rows, ld_wn, coupling, convolution)
    (128, 0, 70, 128, True, True),
    (128, 16, 33, 128, True, True),
    (64, 16, 31, 64, True, True),             # n = 48
    (16, 4, 1, 16, True, True),               # n = 12: the toy width, a partial column group
    (16, 0, 40, 16, False, True),             # first flow: no coupling, ls_row untouched
    (48, 48, 77, 64, True, False),            # after the last flow: everything goes to z
]


@pytest.mark.parametrize("n_in,n_early,rows,ld_wn,coupled,conv", BOUNDARY_CASES)
def test_boundary_kernel_vs_float64(gpu, n_in, n_early, rows, ld_wn, coupled, conv):
    """rtts_sw_coupling_fwd1x1 against torch in float64 with the inputs of test_coupling_and_inverse_1x1_kernel_vs_torch
    (unit normal rows, 0.3 x normal WN output, orthonormal W): max |err| < 2e-5 on out and z, ls_row to rel 1e-5 + abs 1e-5
    and accumulated over two calls; z outside the written block keeps its NaN."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(100 + n_in + n_early + rows)
    n, half, z_col = n_in - n_early, n_in // 2, 6
    x = torch.randn(rows, n_in, generator=g)
    wn = 0.3 * torch.randn(rows, ld_wn, generator=g)
    w = torch.linalg.qr(torch.randn(max(n, 1), max(n, 1), generator=g))[0].contiguous()
    ls0 = torch.randn(rows, generator=g)
    xd, wnd, wd = x.to(gpu), wn.to(gpu), w.to(gpu)
    out = torch.full((rows, max(n, 1)), float("nan"), device=gpu)
    z = torch.full((rows, z_col + n_early + 5), float("nan"), device=gpu)
    ls = ls0.to(gpu)
    for _ in range(2):
        _lib.call("rtts_sw_coupling_fwd1x1", xd.data_ptr(), n_in, wnd.data_ptr() if coupled else None, ld_wn, wd.data_ptr() if conv else None,
                  n_in, n_early, rows, out.data_ptr() if conv else None, out.stride(0), z.data_ptr(), z.stride(0), z_col, ls.data_ptr(), _s())
    x64, wn64 = x.double(), wn.double()
    c = torch.cat([x64[:, :half], torch.exp(wn64[:, :half]) * x64[:, half:] + wn64[:, half:n_in]], 1) if coupled else x64
    got_z = z.cpu()
    if n_early:
        err = float((got_z[:, z_col:z_col + n_early].double() - c[:, :n_early]).abs().max())
        print("z err", err)
        assert err < 2e-5, err
    assert torch.isnan(got_z[:, :z_col]).all() and torch.isnan(got_z[:, z_col + n_early:]).all()
    if conv:
        err = float((out.cpu().double() - c[:, n_early:] @ w.double().t()).abs().max())
        print("out err", err)
        assert err < 2e-5, err
    else:
        assert torch.isnan(out).all()
    want_ls = ls0.double() + (2 * wn64[:, :half].sum(1) if coupled else 0)
    if coupled:
        torch.testing.assert_close(ls.cpu().double(), want_ls, rtol=1e-5, atol=1e-5)
    else:
        assert torch.equal(ls.cpu(), ls0)


def test_boundary_kernel_does_not_depend_on_the_row_tiling(gpu):
    """A row's out, z and ls_row are the same bits wherever the row falls in a workgroup: rows [5, 70) of a call, called alone."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(9)
    n_in, n_early, rows, off = 64, 16, 70, 5
    n = n_in - n_early
    x, wn = torch.randn(rows, n_in, generator=g).to(gpu), (0.3 * torch.randn(rows, n_in, generator=g)).to(gpu)
    w = torch.linalg.qr(torch.randn(n, n, generator=g))[0].contiguous().to(gpu)
    res = []
    for a in (0, off):
        out, z, ls = torch.empty(rows - a, n, device=gpu), torch.empty(rows - a, n_early, device=gpu), torch.zeros(rows - a, device=gpu)
        _lib.call("rtts_sw_coupling_fwd1x1", x[a:].data_ptr(), n_in, wn[a:].data_ptr(), n_in, w.data_ptr(), n_in, n_early, rows - a,
                  out.data_ptr(), n, z.data_ptr(), n_early, 0, ls.data_ptr(), _s())
        res.append((out, z, ls))
    for whole, part in zip(*res):
        assert torch.equal(whole[off:], part)


# ------------------------------------------------------------------ 2. the reduce kernel
def _check_sums(got, z64, ls64, brackets):
    """got (nseg, 2) float64 against float64 sums over the row brackets: rel 1e-10 of the sum of magnitudes (double
    accumulation of N < 1e6 terms: N * 2^-53 ~ 1e-10)."""
    assert got.dtype == torch.float64
    for s, (a, e) in enumerate(brackets):
        sq, ls = (z64[a:e] ** 2).sum(), ls64[a:e].sum()
        assert math.isfinite(float(got[s, 0])) and math.isfinite(float(got[s, 1])), (s, got[s])
        assert abs(float(got[s, 0] - sq)) <= 1e-10 * float(sq), (s, float(got[s, 0]), float(sq))
        assert abs(float(got[s, 1] - ls)) <= 1e-10 * float(ls64[a:e].abs().sum()), (s, float(got[s, 1]), float(ls))
        if a == e:
            assert float(got[s, 0]) == 0.0 and float(got[s, 1]) == 0.0


@pytest.mark.parametrize("c,ld_z", [(128, 128), (48, 56)])
def test_reduce_kernel_vs_float64(gpu, c, ld_z):
    """rtts_sw_nll_reduce, uniform and with an offset table whose boundaries fall on (32, 96) and off (6, 166, 200) 32-row
    tiles, one empty segment; the rows before moff[0] and the capacity rows hold NaN in z and ls_row and reach no sum."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(c)
    b, length = 3, 70
    z = torch.randn(b * length, ld_z, generator=g)
    ls = torch.randn(b * length, generator=g)
    zd, lsd = z.to(gpu), ls.to(gpu)
    out = torch.full((b, 2), float("nan"), dtype=torch.float64, device=gpu)
    _lib.call("rtts_sw_nll_reduce", zd.data_ptr(), ld_z, c, lsd.data_ptr(), None, b, 1, length, b * length, out.data_ptr(), _s())
    _check_sums(out.cpu(), z[:, :c].double(), ls.double(), [(i * length, (i + 1) * length) for i in range(b)])

    up, cap = 2, 110
    moff = [3, 16, 16, 48, 83, 100]
    rows = up * cap
    z = torch.randn(rows, ld_z, generator=g)
    ls = torch.randn(rows, generator=g)
    for t in (z, ls):
        t[:up * moff[0]] = float("nan")
        t[up * moff[-1]:] = float("nan")
    z[:, c:] = float("nan")                                              # the columns between C and the row stride are not read
    zd, lsd, moff_d = z.to(gpu), ls.to(gpu), torch.tensor(moff, dtype=torch.int32, device=gpu)
    out = torch.full((len(moff) - 1, 2), float("nan"), dtype=torch.float64, device=gpu)
    _lib.call("rtts_sw_nll_reduce", zd.data_ptr(), ld_z, c, lsd.data_ptr(), moff_d.data_ptr(), len(moff) - 1, up, 0, rows, out.data_ptr(), _s())
    _check_sums(out.cpu(), z[:, :c].double(), ls.double(), [(up * moff[i], up * moff[i + 1]) for i in range(len(moff) - 1)])

    # a table that runs past the capacity is clamped to the rows there are
    z, ls = torch.randn(rows, ld_z, generator=g), torch.randn(rows, generator=g)
    zd, lsd, moff_d = z.to(gpu), ls.to(gpu), torch.tensor([-2, 50, 115, 400], dtype=torch.int32, device=gpu)
    out = torch.full((3, 2), float("nan"), dtype=torch.float64, device=gpu)
    _lib.call("rtts_sw_nll_reduce", zd.data_ptr(), ld_z, c, lsd.data_ptr(), moff_d.data_ptr(), 3, up, 0, rows, out.data_ptr(), _s())
    _check_sums(out.cpu(), z[:, :c].double(), ls.double(), [(0, 100), (100, rows), (rows, rows)])


# ------------------------------------------------------------------ 3. the pack-audio kernel
@pytest.mark.parametrize("up,c", [(16, 16), (2, 128)])
def test_pack_audio_gathers_segments_and_zeroes_the_rest(gpu, up, c):
    """rtts_sw_pack_audio: utterance s contributes exactly 256 * frames_s samples from its start in a NaN-separated source;
    rows past the total are zero; nothing outside dst is written (NaN guards around it)."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(up)
    spf, frames, cap = up * c, [2, 0, 3, 1], 8
    moff = [0, 2, 2, 5, 6]
    src = torch.full((spf * 10,), float("nan"))
    starts, pieces, pos = [], [], 7
    for f in frames:
        starts.append(pos)
        pieces.append(torch.randn(spf * f, generator=g))
        src[pos:pos + spf * f] = pieces[-1]
        pos += spf * f + 13                                              # a NaN gap after every utterance
    guard = 64
    buf = torch.full((guard + cap * spf + guard,), float("nan"), device=gpu)
    dst = buf[guard:guard + cap * spf]
    src_d = src.to(gpu)
    start_d = torch.tensor(starts, dtype=torch.int64, device=gpu)
    moff_d = torch.tensor(moff, dtype=torch.int32, device=gpu)
    _lib.call("rtts_sw_pack_audio", src_d.data_ptr(), src_d.numel(), start_d.data_ptr(), moff_d.data_ptr(), len(frames), up, c, up * cap,
              dst.data_ptr(), _s())
    got = buf.cpu()
    assert torch.isnan(got[:guard]).all() and torch.isnan(got[-guard:]).all()
    body, total = got[guard:-guard], spf * moff[-1]
    assert torch.equal(body[:total], torch.cat(pieces))
    assert torch.equal(body[total:], torch.zeros(cap * spf - total))
    # a start that would read past the source gives zeros, not a read outside it
    start_d = torch.tensor([0, 0, 0, src.numel() - 5], dtype=torch.int64, device=gpu)
    _lib.call("rtts_sw_pack_audio", src_d.data_ptr(), src_d.numel(), start_d.data_ptr(), moff_d.data_ptr(), len(frames), up, c, up * cap,
              dst.data_ptr(), _s())
    tail = buf.cpu()[guard + spf * moff[3]:guard + spf * moff[4]]
    assert torch.isnan(tail[:5]).all() and torch.equal(tail[5:], torch.zeros(spf - 5))


# ------------------------------------------------------------------ 4. forward and nll against the reference's fixture
@pytest.mark.parametrize("tag", ["small", "full"])
def test_forward_and_nll_match_the_reference_fixture(cases, fixture, tag):
    """z (max, mean) and the loss against the reference's fp32 CPU forward: within 4x the bf16 rounding model's error
    (module docstring: small 2.34e-2 / 3.19e-3 / 2.67e-4, full 2.08e-2 / 3.46e-3 / 6.69e-5)."""
    from reformer_tts_amd.squeeze_wave import SqueezeWaveLoss
    model, mel, audio = cases(tag)
    zmax, zmean, dloss = _bounds(tag)
    assert zmax <= 3e-2 and zmean <= 4e-3
    z, log_s_list, log_det_list = model((mel, audio))
    ref = torch.from_numpy(fixture[f"{tag}/z"])
    assert z.shape == ref.shape and z.is_cuda and z.dtype == torch.float32
    err = (z.cpu() - ref).abs()
    loss = float(model.nll(mel, audio))
    loss_fwd = float(SqueezeWaveLoss(1.0)((z, log_s_list, log_det_list)))
    print(tag, "z max", float(err.max()), "mean", float(err.mean()), "loss diff", abs(loss - float(fixture[f"{tag}/loss"])))
    assert float(err.max()) < zmax and float(err.mean()) < zmean, (float(err.max()), float(err.mean()))
    assert abs(loss - float(fixture[f"{tag}/loss"])) < dloss, (loss, float(fixture[f"{tag}/loss"]))
    assert abs(loss_fwd - float(fixture[f"{tag}/loss"])) < dloss
    ld = np.array([float(d) for d in log_det_list])
    assert np.abs(ld - fixture[f"{tag}/log_det_W"]).max() < 1e-3               # the reference's fp32 logdet of ~orthonormal W: noise of 1e-4


# ------------------------------------------------------------------ 5. SqueezeWaveLoss(forward) == nll
@pytest.mark.parametrize("tag", ["small", "full"])
def test_loss_of_forward_equals_nll(cases, tag):
    from reformer_tts_amd.squeeze_wave import SqueezeWaveLoss
    model, mel, audio = cases(tag)
    cfg = ref64.cfg_of(tag)
    out = model((mel, audio))
    b, length = mel.shape[0], audio.shape[1] // cfg["n_audio_channels"]
    halves, n_half = [], cfg["n_audio_channels"] // 2
    for k in range(cfg["n_flows"]):
        if k % cfg["early_return_interval"] == 0 and k > 0:
            n_half -= cfg["early_return_size"] // 2
        halves.append(n_half)
    assert out[0].shape == (b, cfg["n_audio_channels"], length)
    assert [tuple(s.shape) for s in out[1]] == [(b, n, length) for n in halves]
    assert len(out[2]) == cfg["n_flows"] and all(d.dim() == 0 and d.dtype == torch.float32 and d.is_cuda for d in out[2])
    for sigma in (1.0, 0.6):
        a, c = float(SqueezeWaveLoss(sigma)(out)), float(model.nll(mel, audio, sigma=sigma))
        print(tag, sigma, a, c)
        assert abs(a - c) <= 1e-6 * abs(a), (sigma, a, c)


# ------------------------------------------------------------------ 6. the flow inverts
@pytest.mark.parametrize("tag", ["small", "full"])
def test_forward_inverts_infer(cases, tag):
    """audio = infer(mel, noise = 0.1 x draws) with no sample clamped; forward((mel, audio)) returns the draws -- the final
    block as drawn, the early blocks times sigma, in z's column order -- within the bound measured for the fixture test."""
    model, mel, _ = cases(tag)
    sigma = 0.6
    g = torch.Generator().manual_seed(21)
    noise = [0.1 * torch.randn(s, generator=g) for s in model.noise_shapes(mel.shape[0], mel.shape[2])]
    audio = model.infer(mel, sigma=sigma, noise=noise)
    assert float(audio.abs().max()) < 1.0                                # no sample clamped: the clamp is not invertible
    z = model((mel, audio))[0]
    want = torch.cat([sigma * t for t in reversed(noise[1:])] + [noise[0]], dim=1)
    assert z.shape == want.shape
    err = (z.cpu() - want).abs()
    print(tag, "max |audio|", float(audio.abs().max()), "z max err", float(err.max()), "mean", float(err.mean()))
    zmax, zmean, _ = _bounds(tag)
    assert float(err.max()) < zmax and float(err.mean()) < zmean, (float(err.max()), float(err.mean()))


# ------------------------------------------------------------------ 7. ragged against per-utterance
def _ragged_inputs(mel, audio, gpu):
    """Frames [7, 0, 17, 1]: the fixture's pieces of utterance 0 and one more frame -> (frames, padded mel (4, n_mel, 19) and
    padded audio (4, 256 * 17 + 9), NaN behind every utterance, and the per-utterance (mel, audio) pairs)."""
    pieces = ref64.ragged_pieces(mel, audio)
    pieces.append((mel[1:2, :, :1], audio[1:2, :256]) if mel.shape[0] > 1 else (mel[:1, :, 24:25], audio[:1, 256 * 24:256 * 25]))
    frames = [p[0].shape[2] for p in pieces]
    assert frames == [7, 0, 17, 1]
    pmel = torch.full((4, mel.shape[1], 19), float("nan"), device=gpu)
    paudio = torch.full((4, 256 * 17 + 9), float("nan"), device=gpu)
    for i, (m, a) in enumerate(pieces):
        pmel[i, :, :m.shape[2]] = m[0]
        paudio[i, :a.shape[1]] = a[0]
    return frames, pmel, paudio, pieces


@pytest.mark.parametrize("tag", ["small", "full"])
def test_nll_ragged_is_per_utterance_nll(cases, fixture, tag):
    """Frames [7, 0, 17, 1] packed in a capacity of 64: the z rows of every utterance are the bits of its own ``forward``;
    its NLL is ``nll`` of it alone (rel 1e-9; NaN for the empty one); ``batch`` is the element-weighted recombination; the
    reference's per-piece losses hold within the fixture test's loss bound."""
    from reformer_tts_amd.squeeze_wave.modules import _Segments, segment_offsets
    model, mel, audio = cases(tag)
    gpu = mel.device
    frames, pmel, paudio, pieces = _ragged_inputs(mel, audio, gpu)
    up, cap, moff_h = model._up(), 64, segment_offsets(frames)
    moff = model._offsets_to(moff_h, gpu)
    mel_rows = model._pack_mel(pmel, frames, moff, cap)
    flat, starts = model._audio_starts(paudio, frames, None, gpu, "test")
    audio_rows = model._pack_audio(flat, starts, moff, len(frames), cap)
    z_rows, _, _ = model._flows_fwd(model._fold(), mel_rows, _Segments.packed(moff, cap, up), audio_rows, False)
    per, batch = model.nll_ragged(pmel, frames, paudio)
    assert per.shape == (4,) and per.dtype == torch.float32 and batch.dim() == 0 and per.is_cuda
    alone = []
    for i, (m, a) in enumerate(pieces):
        if frames[i] == 0:
            assert math.isnan(float(per[i]))
            alone.append(float("nan"))
            continue
        z_i = model((m, a))[0]                                           # (1, C, L)
        assert torch.equal(z_rows[up * moff_h[i]:up * moff_h[i + 1]], z_i[0].t()), (tag, i)
        alone.append(float(model.nll(m, a)))
        assert abs(float(per[i]) - alone[-1]) <= 1e-9 * abs(alone[-1]), (i, float(per[i]), alone[-1])
    want = sum(v * f for v, f in zip(alone, frames) if f) / sum(frames)
    assert abs(float(batch) - want) <= 1e-6 * abs(want), (float(batch), want)          # fp32 per-utterance values recombined
    dloss = _bounds(tag)[2]
    for i, ref in enumerate(fixture[f"{tag}/ragged"]):
        if frames[i]:
            print(tag, "piece", frames[i], abs(float(per[i]) - float(ref)))
            assert abs(float(per[i]) - float(ref)) < dloss, (i, float(per[i]), float(ref))
    # a flat buffer with explicit sample offsets is the same call
    soff = [i * paudio.shape[1] for i in range(4)]
    per2, batch2 = model.nll_ragged(pmel, frames, paudio.reshape(-1), sample_offsets=soff)
    assert torch.allclose(per, per2, rtol=0, atol=0, equal_nan=True) and torch.equal(batch, batch2)


def test_nll_ragged_equal_lengths_is_nll(cases):
    model, _, _ = cases("full")
    gpu = next(model.parameters()).device
    g = torch.Generator().manual_seed(8)
    mel = (torch.randn(3, 80, 9, generator=g) * 2 - 5).clamp(-11.5, 2.0).to(gpu)
    audio = (0.3 * torch.randn(3, 256 * 9, generator=g)).to(gpu)
    want = model.nll(mel, audio)
    per, batch = model.nll_ragged(mel, [9, 9, 9], audio)
    assert torch.equal(batch, want), (float(batch), float(want))
    assert all(torch.equal(per[i], model.nll(mel[i:i + 1], audio[i:i + 1])) for i in range(3))
    nan_per, nan_batch = model.nll_ragged(mel, [0, 0, 0], audio)
    assert torch.isnan(nan_per).all() and torch.isnan(nan_batch)


# ------------------------------------------------------------------ 8. the captured graph
def test_capture_nll_ragged_replays_new_lengths(cases):
    """One graph at one capacity, two replays with different lengths: each equals the eager nll_ragged on the same inputs.
    An over-capacity call raises before anything runs, and the graph stays usable."""
    model, _, _ = cases("full")
    gpu = next(model.parameters()).device
    g = torch.Generator().manual_seed(12)
    batch, cap = 4, 64
    run = model.capture_nll_ragged(batch, cap)
    assert model.capture_nll_ragged(batch, cap) is run                   # kept per (batch, capacity, sigma)
    mel = (torch.randn(batch, 80, 40, generator=g) * 2 - 5).clamp(-11.5, 2.0).to(gpu)
    audio = (0.3 * torch.randn(batch, 256 * 40, generator=g)).to(gpu)
    got = {}
    for frames in ([7, 0, 17, 1], [20, 3, 11, 30]):
        per, total = run(mel, frames, audio)
        got[tuple(frames)] = (per.clone(), total.clone())
        with pytest.raises(ValueError, match="capture_nll_ragged graph for 4 utterances of 64 frames"):
            run(mel, [40, 20, 4, 1], audio)
        with pytest.raises(ValueError, match="capture_nll_ragged"):
            run(mel[:2], [1, 1], audio[:2])
        torch.cuda.synchronize()
        assert torch.allclose(per, got[tuple(frames)][0], rtol=0, atol=0, equal_nan=True)      # nothing replayed by the refused calls
    for frames, (per, total) in got.items():
        eper, etotal = model.nll_ragged(mel, list(frames), audio)
        assert torch.allclose(per, eper, rtol=0, atol=0, equal_nan=True), (frames, per, eper)
        assert torch.equal(total, etotal), (frames, float(total), float(etotal))
        assert torch.isfinite(total)


# ------------------------------------------------------------------ 9. no library GEMM
def test_nll_runs_no_library_gemm(gpu):
    """As test_default_configuration_runs_no_library_gemm for infer: with the reference's default configuration ``nll`` and
    ``nll_ragged`` dispatch no ATen matrix product or convolution and report no general path."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from reformer_tts_amd import _lib
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    sw = SqueezeWave(12, 128, 80, 2, 16, WNConfig(8, 256, 3, 2)).to(gpu).eval()
    mel = torch.randn(2, 80, 37, device=gpu)
    audio = 0.3 * torch.randn(2, 256 * 37, device=gpu)
    sw.nll(mel, audio)                                # folding happens once, outside the census
    seen = []

    class Census(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    before = len(_lib.PATHS_LEFT)
    with Census():
        loss = sw.nll(mel, audio)
        per, batch = sw.nll_ragged(mel, [37, 5], audio)
    assert torch.isfinite(loss) and torch.isfinite(per).all() and torch.isfinite(batch)
    bad = [f for f in seen if any(k in f for k in ("aten.mm", "aten.addmm", "aten.bmm", "aten.matmul", "aten.convolution", "aten.linear"))]
    assert not bad, bad
    assert len(_lib.PATHS_LEFT) == before, _lib.PATHS_LEFT[before:]
    assert all(f.in_tree for f in sw._fold())


# ------------------------------------------------------------------ 10. score_audio
def test_score_audio_is_nll_ragged_on_the_creators_mels(cases):
    """Two waveforms of 2,000 and 5,300 samples: score_audio == nll_ragged on creator.forward's mels cut to n // 256 frames."""
    from reformer_tts_amd import synthesis
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram
    model, _, _ = cases("full")
    gpu = next(model.parameters()).device
    creator = Tacotron2Spectrogram(22050, 1024, 1024, 256, 80).to(gpu)
    g = torch.Generator().manual_seed(13)
    waves = [(0.3 * torch.randn(n, generator=g)).to(gpu) for n in (2000, 5300)]
    per, batch = synthesis.score_audio(model, creator, waves)
    mel, frames = creator(waves)
    assert frames.tolist() == [2000 // 256 + 1, 5300 // 256 + 1]
    cut = [2000 // 256, 5300 // 256]
    padded = torch.zeros(2, 5300, device=gpu)
    for i, w in enumerate(waves):
        padded[i, :w.numel()] = w
    want_per, want_batch = model.nll_ragged(mel, cut, padded)
    assert torch.equal(per, want_per) and torch.equal(batch, want_batch), (per, want_per)
    assert per.shape == (2,) and torch.isfinite(per).all()
    per2, _ = synthesis.score_audio(model, creator, padded, [2000, 5300])         # the padded form of the same batch
    assert torch.equal(per2, per)


# ------------------------------------------------------------------ 11. refusals
def test_likelihood_refuses_bad_calls(golden_dir, gpu):
    from reformer_tts_amd import _lib
    model, mel, audio = _build(golden_dir, "small", gpu)                 # its own model: this test changes it
    model.train()
    for call in (lambda: model((mel, audio)), lambda: model.nll(mel, audio), lambda: model.nll_ragged(mel, [24, 24], audio),
                 lambda: model.capture_nll_ragged(2, 64)):
        with pytest.raises(_lib.RttsError, match="batch-statistics .* BatchNorm is not on the HIP path"):
            call()
    model.eval()
    with pytest.raises(ValueError, match=r"audio \(2, 6143\) is not \(B, 256 \* Lm\) = \(2, 6144\)"):
        model.nll(mel, audio[:, :-1])
    with pytest.raises(ValueError, match=r"is not \(B, 256 \* Lm\)"):
        model((mel[:, :, :-1], audio))
    with pytest.raises(_lib.RttsError, match="GPU only: audio is on cpu"):
        model.nll(mel, audio.cpu())
    with pytest.raises(_lib.RttsError, match="GPU only: mel is on cpu"):
        model((mel.cpu(), audio))
    with pytest.raises(_lib.RttsError, match="GPU only: audio is on cpu"):
        model.nll_ragged(mel, [24, 24], audio.cpu())
    with pytest.raises(ValueError, match=r"1\.\.1024 utterances \(got 1025\)"):
        model.nll_ragged(mel, [1] * 1025, audio)
    with pytest.raises(ValueError, match=r"utterance 1 has 25 frames = 6400 samples, its audio holds 6144"):
        model.nll_ragged(torch.zeros(2, 80, 25, device=gpu), [24, 25], audio)
    # the entry point itself: out == x, odd n, n_in > 128 (real buffers, refused before a launch)
    x = torch.zeros(40, 130, device=gpu)
    out, z, ls = torch.zeros(40, 130, device=gpu), torch.zeros(40, 130, device=gpu), torch.zeros(40, device=gpu)
    w = torch.eye(128, device=gpu)

    def boundary(n_in, n_early, o=out):
        _lib.call("rtts_sw_coupling_fwd1x1", x.data_ptr(), 130, x.data_ptr(), 130, w.data_ptr(), n_in, n_early, 40, o.data_ptr(), 130,
                  z.data_ptr(), 130, 0, ls.data_ptr(), _s())
    with pytest.raises(_lib.RttsError, match="not in place"):
        boundary(128, 0, x)
    with pytest.raises(_lib.RttsError, match="n_early must be even"):
        boundary(128, 15)
    with pytest.raises(_lib.RttsError, match="n_in must be even"):
        boundary(127, 0)
    with pytest.raises(_lib.RttsError, match=r"n_in must be even and <= 128 \(got n_in=130\)"):
        boundary(130, 0)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(z.abs().max()) == 0.0            # nothing ran
    assert math.isfinite(float(model.nll(mel, audio)))                                # the model still scores
    with torch.no_grad():
        model.inv_conv_layers[1].conv.weight[:, 0] *= -1
    with pytest.raises(ValueError, match=r"inv_conv_layers\.1: det W is negative"):
        model.nll(mel, audio)
    assert model.infer(mel).shape == audio.shape                                      # inference does not need log det W
