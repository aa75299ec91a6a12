"""Ragged (packed-row) SqueezeWave inference on the GPU: the segment kernels against float64 per segment, and
``infer_ragged`` / ``capture_ragged`` against per-utterance ``infer`` bit for bit.

Why bit identity is expected: every 1x1 convolution of the default configuration is ``rtts_gemm_nt``, which has one MFMA
shape and no split-K, so a row's result does not depend on the row count or the tile picked; every other step is row-wise
or stops at the segment edges."""
import os

import numpy as np
import pytest
import torch

from oracle import squeezewave_ref as sw_ref
from oracle import synth

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 5, 127, 128, 129, 300]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _moff(lengths, gpu):
    from reformer_tts_amd.squeeze_wave.modules import segment_offsets
    moff = segment_offsets(lengths)
    return moff, torch.tensor(moff, dtype=torch.int32, device=gpu)


def _model(golden_dir, tag, gpu):
    """The models of the vocoder goldens: the small configuration's own weights, or the default configuration with its
    recorded tensors over a seeded synthetic state dict (as tests/test_squeezewave_hip.py loads them)."""
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    z = np.load(os.path.join(golden_dir, f"squeezewave_{tag}.npz"))
    cfg = sw_ref.small_cfg() if tag == "small" else sw_ref.default_cfg()
    model = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                        cfg["early_return_size"], WNConfig(**cfg["wn_config"]))
    if tag == "small":
        sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    else:
        shapes = {k[len("shape/"):]: tuple(z[k]) for k in z.files if k.startswith("shape/")}
        sd = {k: v * (0.05 if "end_conv" in k else 1.0) for k, v in synth.synth_state_dict(shapes, seed=11).items()}
        for k in z.files:
            if k.startswith("sd/"):
                sd[k[3:]] = torch.from_numpy(z[k])
    model.load_state_dict(sd, strict=False)
    return z, model.to(gpu).eval()


# ------------------------------------------------------------------ segment kernels
@pytest.mark.parametrize("up", [1, 2])
def test_depthwise_segments_vs_float64(gpu, up):
    """rtts_sw_depthwise_k3_seg: every segment is its own zero-padded k = 3 convolution with the edge corrections at its
    first and last row; boundaries on and off 128-row tiles; the capacity rows past the total are NaN and no real row may
    read them."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(0)
    c = 256
    moff, moff_d = _moff(LENGTHS, gpu)
    total, cap = moff[-1], moff[-1] + 37
    x = torch.randn(up * cap, c, generator=g)
    x[up * total:] = float("nan")
    w, bias = torch.randn(c, 3, generator=g), torch.randn(c, generator=g)
    lo, hi = torch.randn(c, generator=g), torch.randn(c, generator=g)
    y = torch.full((up * cap, c), float("nan"), dtype=torch.bfloat16, device=gpu)
    dev_args = [t.to(gpu) for t in (x, w, bias, lo, hi)]                        # held: the launch is asynchronous
    xd, wd, bd, lod, hid = (t.data_ptr() for t in dev_args)
    _lib.call("rtts_sw_depthwise_k3_seg", xd, wd, bd, moff_d.data_ptr(), len(LENGTHS), up, up * cap, c, y.data_ptr(), lod, hid, _s())
    got = y.float().cpu().double()
    x64, w64, b64 = x.double(), w.double(), bias.double()
    for s, n in enumerate(LENGTHS):
        a, e = up * moff[s], up * moff[s + 1]
        seg = x64[a:e].t().unsqueeze(0)                                             # (1, C, rows)
        want = torch.nn.functional.conv1d(seg, w64.unsqueeze(1), b64, padding=1, groups=c)[0].t().clone()
        want[0] -= lo.double()
        want[-1] -= hi.double()
        scale = torch.nn.functional.conv1d(seg.abs(), w64.abs().unsqueeze(1), b64.abs(), padding=1, groups=c)[0].t() + lo.double().abs() + hi.double().abs()
        err = (got[a:e] - want).abs()
        assert torch.isfinite(got[a:e]).all(), (s, n)
        # bf16 output: round to nearest (2^-9 relative) on top of fp32 FMA error
        assert bool((err <= 2.0 ** -8 * want.abs() + 1e-6 * scale + 1e-30).all()), (s, n, float((err - 2.0 ** -8 * want.abs()).max()))


def test_depthwise_uniform_equals_equal_segments(gpu):
    """The uniform entry point is the segment kernel with moff[s] = s * L / up: bit for bit, with and without edges."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(1)
    for b, l, c, up in ((3, 258, 256, 2), (5, 17, 64, 1), (1, 300, 128, 2)):
        x = torch.randn(b * l, c, generator=g).to(gpu)
        w, bias = torch.randn(c, 3, generator=g).to(gpu), torch.randn(c, generator=g).to(gpu)
        lo, hi = torch.randn(c, generator=g).to(gpu), torch.randn(c, generator=g).to(gpu)
        _, moff_d = _moff([l // up] * b, gpu)
        for edges in ((None, None), (lo.data_ptr(), hi.data_ptr())):
            y0 = torch.empty(b * l, c, dtype=torch.bfloat16, device=gpu)
            y1 = torch.empty_like(y0)
            _lib.call("rtts_sw_depthwise_k3", x.data_ptr(), w.data_ptr(), bias.data_ptr(), b, l, c, y0.data_ptr(), *edges, _s())
            _lib.call("rtts_sw_depthwise_k3_seg", x.data_ptr(), w.data_ptr(), bias.data_ptr(), moff_d.data_ptr(), b, up, b * l, c, y1.data_ptr(),
                      *edges, _s())
            assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)), (b, l, c, up)


@pytest.mark.parametrize("up", [2, 16])
def test_gate_over_packed_rows_vs_float64(gpu, up):
    """The gate over packed rows (the uniform entry with B = 1 over the capacity): audio row r of segment s reads
    conditioning row moff[s] + (r - up * moff[s]) // up; NaN in the padding rows of pw and of the conditioning stays there."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(2)
    c, nl = 64, 3
    moff, _ = _moff(LENGTHS, gpu)
    total, cap = moff[-1], moff[-1] + 11
    pw = torch.randn(up * cap, 2 * c, generator=g).bfloat16()
    cond = torch.randn(cap, nl * 2 * c, generator=g).bfloat16()
    pw[up * total:] = float("nan")
    cond[total:] = float("nan")
    acts = torch.full((up * cap, c), float("nan"), dtype=torch.bfloat16, device=gpu)
    off = 1 * 2 * c
    pw_d, cond_d = pw.to(gpu), cond.to(gpu)
    _lib.call("rtts_sw_gate", pw_d.data_ptr(), cond_d.data_ptr(), cond_d.stride(0), off, up, 1, up * cap, cap, c, acts.data_ptr(), _s())
    got = acts.float().cpu().double()
    for s, n in enumerate(LENGTHS):
        rows = torch.arange(up * moff[s], up * moff[s + 1])
        crow = moff[s] + (rows - up * moff[s]) // up
        sm = pw[rows].double() + cond[crow][:, off:off + 2 * c].double()
        want = torch.tanh(sm[:, :c]) * torch.sigmoid(sm[:, c:])
        err = (got[rows] - want).abs()
        assert torch.isfinite(got[rows]).all(), s
        assert bool((err <= 2.0 ** -8 * want.abs() + 2e-6).all()), (s, float(err.max()))


def test_pack_mel_gathers_segments_and_zeroes_the_rest(gpu):
    """rtts_sw_pack_mel: row moff[s] + t = frame t of utterance s for any strides of (B, n_mel, L); frames past an
    utterance's length (NaN here) are never read; rows past the total are zero."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(4)
    lengths = [5, 0, 300, 128, 1]
    b, n_mel, lmax = len(lengths), 80, 310
    base = torch.randn(b, lmax, n_mel, generator=g)
    for i, n in enumerate(lengths):
        base[i, n:] = float("nan")
    moff, moff_d = _moff(lengths, gpu)
    cap = moff[-1] + 21
    for mel in (base.transpose(1, 2).to(gpu), base.transpose(1, 2).contiguous().to(gpu), base.permute(2, 0, 1).contiguous().to(gpu).permute(1, 0, 2)):
        dst = torch.full((cap, 88), float("nan"), device=gpu)
        _lib.call("rtts_sw_pack_mel", mel.data_ptr(), *mel.stride(), lmax, n_mel, moff_d.data_ptr(), b, cap, dst.data_ptr(), dst.stride(0), _s())
        got = dst.cpu()
        for i, n in enumerate(lengths):
            assert torch.equal(got[moff[i]:moff[i + 1], :n_mel], base[i, :n])
        assert torch.equal(got[moff[-1]:, :n_mel], torch.zeros(cap - moff[-1], n_mel))
        assert torch.isnan(got[:, n_mel:]).all()                                  # columns past n_mel untouched


def test_segment_entry_points_refuse_bad_arguments(gpu):
    from reformer_tts_amd import _lib
    x = torch.zeros(8, 64, device=gpu)
    w, y = torch.zeros(64, 3, device=gpu), torch.zeros(8, 64, dtype=torch.bfloat16, device=gpu)
    moff = torch.zeros(2000, dtype=torch.int32, device=gpu)
    dw = lambda nseg, up, rows, m=moff.data_ptr(): _lib.call("rtts_sw_depthwise_k3_seg", x.data_ptr(), w.data_ptr(), w.data_ptr(), m, nseg, up,  # noqa: E731
                                                              rows, 64, y.data_ptr(), None, None, _s())
    for args in ((0, 2, 8), (1025, 2, 8), (1, 0, 8), (1, 3, 8), (1, 2, 0)):
        with pytest.raises(_lib.RttsError):
            dw(*args)
    with pytest.raises(_lib.RttsError):
        dw(1, 2, 8, None)
    with pytest.raises(_lib.RttsError, match="segments"):
        _lib.call("rtts_sw_pack_mel", x.data_ptr(), 64, 1, 64, 8, 64, moff.data_ptr(), 1025, 8, x.data_ptr(), 64, _s())
    with pytest.raises(_lib.RttsError):
        _lib.call("rtts_sw_pack_mel", x.data_ptr(), 64, 1, 64, 8, 64, moff.data_ptr(), 1, 8, x.data_ptr(), 32, _s())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ infer_ragged vs per-utterance infer
def _first_divergence(model, mel, lengths, noise):
    """Where the ragged and per-utterance paths part: (utterance, flow) of the first WN output that differs, for the
    failure message of the bit-identity tests."""
    from reformer_tts_amd.squeeze_wave import modules
    rec = []
    orig = modules._FoldedWN.forward

    def spy(self, audio, mel_rows, seg):
        out = orig(self, audio, mel_rows, seg)
        rec.append(out.clone())
        return out
    modules._FoldedWN.forward = spy
    try:
        model.infer_ragged(mel, lengths, noise=noise)
        ragged, rec[:] = list(rec), []
        per = []
        for i, n in enumerate(lengths):
            model.infer(mel[i:i + 1, :, :n], noise=noise[i])
            per.append(list(rec))
            rec[:] = []
    finally:
        modules._FoldedWN.forward = orig
    moff = np.cumsum([0] + list(lengths))
    up = model.wn_layers[0].upsample_scale
    for f in range(len(ragged)):
        for i, n in enumerate(lengths):
            a = ragged[f][up * moff[i]:up * moff[i + 1]]
            if not torch.equal(a, per[i][f][:up * n]):
                return f"utterance {i} ({n} frames) parts at WN block {f} of the flows (in execution order), max |diff| {float((a - per[i][f][:up * n]).abs().max()):.3e}"
    return "every WN output agrees: the paths part in the coupling, the early-return concatenation or the clamp"


@pytest.mark.parametrize("tag", ["small", "full"])
def test_infer_ragged_is_per_utterance_infer(golden_dir, gpu, tag):
    """infer_ragged over mixed lengths == infer(mel[i:i+1, :, :len_i], noise=noise_i) for every utterance, bit for bit.  One
    utterance is the golden mel with the golden's draws: the ragged path also stays within the reference golden's
    3e-2 max / 4e-3 mean."""
    z, model = _model(golden_dir, tag, gpu)
    gmel = torch.from_numpy(z["mel"])[:1]
    torch.manual_seed(int(z["seed"]))
    gnoise = [torch.empty(*s).normal_() for s in model.noise_shapes(z["mel"].shape[0], z["mel"].shape[2])]
    glen = gmel.shape[2]
    lengths = [3, glen, 1, 77, 64, 5] if tag == "small" else [3, glen, 1, 129, 64, 200]
    g = torch.Generator().manual_seed(5)
    lmax = max(lengths) + 4
    mel = ((torch.randn(len(lengths), 80, lmax, generator=g) * 2 - 5).clamp(-11.5, 2.0))
    mel[1, :, :glen] = gmel[0]
    noise = [[torch.randn(s, generator=g) for s in model.noise_shapes(1, n)] for n in lengths]
    noise[1] = [t[:1] for t in gnoise]
    mel_d = mel.to(gpu)
    audio, views = model.infer_ragged(mel_d, lengths, noise=noise)
    assert audio.shape == (256 * sum(lengths),)
    for i, n in enumerate(lengths):
        want = model.infer(mel_d[i:i + 1, :, :n], noise=noise[i])
        assert views[i].shape == (256 * n,)
        if not torch.equal(views[i], want[0]):
            pytest.fail(f"{tag}: " + _first_divergence(model, mel_d, lengths, noise))
    ref = torch.from_numpy(z["audio"][0])
    err = (views[1].cpu() - ref).abs()
    assert float(err.max()) < 3e-2 and float(err.mean()) < 4e-3, (float(err.max()), float(err.mean()))


def test_infer_ragged_equal_lengths_is_infer(golden_dir, gpu):
    """Equal lengths: the packed batch is the uniform one, and infer_ragged returns infer's audio bit for bit."""
    z, model = _model(golden_dir, "full", gpu)
    g = torch.Generator().manual_seed(6)
    b, n = 3, 70
    mel = torch.randn(b, 80, n, generator=g).to(gpu)
    noise = [torch.randn(s, generator=g) for s in model.noise_shapes(b, n)]
    want = model.infer(mel, noise=noise)
    per = [[t[i:i + 1] for t in noise] for i in range(b)]
    audio, views = model.infer_ragged(mel, [n] * b, noise=per)
    assert torch.equal(audio.view(b, -1), want)
    assert all(torch.equal(v, w) for v, w in zip(views, want))


def test_capture_ragged_replays_new_lengths(golden_dir, gpu):
    """One capture_ragged graph at one capacity replays two different length sets; fed the draws the graph made, the eager
    infer_ragged matches each replay bit for bit.  An over-capacity total is refused before anything runs."""
    z, model = _model(golden_dir, "full", gpu)
    g = torch.Generator().manual_seed(7)
    batch, cap = 3, 400
    run = model.capture_ragged(batch, cap)
    assert model.capture_ragged(batch, cap) is run                    # kept per (batch, capacity)
    for lengths in ([100, 3, 250], [1, 129, 64]):
        mel = torch.randn(batch, 80, 260, generator=g).to(gpu)
        out, views = run(mel, lengths)
        got = [v.clone() for v in views]
        draws = [d.clone() for d in run.noise]
        torch.cuda.synchronize()
        assert out.shape == (256 * cap,) and [v.numel() for v in got] == [256 * n for n in lengths]
        _, eager = model.infer_ragged(mel, lengths, noise=model.unpack_noise(draws, lengths))
        for i, (a, b) in enumerate(zip(got, eager)):
            assert torch.equal(a, b), (lengths, i, float((a - b).abs().max()))
    before = run.noise[0].clone()
    with pytest.raises(ValueError, match="capture_ragged"):
        run(torch.zeros(batch, 80, 300, device=gpu), [200, 200, 1])
    with pytest.raises(ValueError):
        run(torch.zeros(2, 80, 300, device=gpu), [1, 1])
    torch.cuda.synchronize()
    assert torch.equal(run.noise[0], before)                           # nothing replayed


def test_infer_ragged_runs_no_library_gemm(gpu):
    """As test_default_configuration_runs_no_library_gemm for infer: with the default configuration the ragged path
    dispatches no ATen matrix product or convolution, and reports no general path."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from reformer_tts_amd import _lib
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    sw = SqueezeWave(12, 128, 80, 2, 16, WNConfig(8, 256, 3, 2)).to(gpu).eval()
    mel = torch.randn(3, 80, 41, device=gpu)
    sw.infer_ragged(mel, [37, 2, 41])
    seen = []

    class Census(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    before = len(_lib.PATHS_LEFT)
    with Census():
        audio, views = sw.infer_ragged(mel, [37, 2, 41])
    assert audio.shape == (256 * 80,) and torch.isfinite(audio).all()
    bad = [f for f in seen if any(k in f for k in ("aten.mm", "aten.addmm", "aten.bmm", "aten.matmul", "aten.convolution", "aten.linear"))]
    assert not bad, bad
    assert len(_lib.PATHS_LEFT) == before, _lib.PATHS_LEFT[before:]
