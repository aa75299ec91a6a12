"""rtts_denoise (csrc/denoise.hip) and squeeze_wave.denoiser.Denoiser on the GPU, against the float64 restatement of
tests/denoise_ref.py.

The error bound of the parity test is set in the test itself: the float32 twin of denoise_ref.py (the same two f32 bases, the
transforms as blocked float32 matmuls) is measured against float64 on the test's own inputs, relative to each utterance's peak,
and the kernel -- the same arithmetic as k-ordered f32 chains -- gets 4 x the worst value.
Measured on an MI355X (test_ragged_parity_with_float64 prints the figures): twin 1.416e-06, so the bound is 5.665e-06; the kernel's
worst utterance is 1.639e-06 at strength 0 (against float64 and against its own input alike), 1.539e-06 at strength 0.1 and
7.6e-08 at the all-clamping strength, where only the bins with a zero bias pass."""
import ctypes
import os

import numpy as np
import pytest
import torch

import denoise_ref

pytestmark = pytest.mark.gpu

N_FFT, HOP = 1024, 256
ALL_CLAMP = 1e9
# the issue's lengths; then frame counts one below / at / one above the tile stride of 29 (28, 29, 30 frames), the lengths around the
# first tile boundary (hop 31 is the last of tile 0: 7680 samples end in it, 7681 need a second tile), and the ones around the second
# (15104 / 15105: two / three tiles, 60 frames = one above twice the stride)
LENGTHS = [513, 600, 1792, 1793, 7424, 7425, 6917, 7268, 7680, 7681, 15104, 15105]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _audio(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) * 2 - 1) * 0.1


def _bias(zeros=True):
    g = torch.Generator().manual_seed(77)
    b = torch.rand(N_FFT // 2 + 1, generator=g) * 0.5
    b[[0, 3, 200, 512]] = 0.0 if zeros else 0.25
    return b if zeros else b.clamp(min=1e-3)


@pytest.fixture(scope="module")
def denoiser(gpu):
    from reformer_tts_amd.squeeze_wave import Denoiser
    return Denoiser(bias_spec=_bias()).to(gpu)


@pytest.fixture(scope="module")
def case(gpu):
    """The ragged batch and its float64 references, computed once and left unchanged."""
    utts = [_audio(n, 10 + i) for i, n in enumerate(LENGTHS)]
    bias = _bias().numpy()
    ref = {s: [denoise_ref.denoise_f64(u.numpy(), bias, s) for u in utts] for s in (0.0, 0.1, ALL_CLAMP)}
    return utts, ref


def _rel(got, want, x):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(x).max())


def test_ragged_parity_with_float64(gpu, denoiser, case):
    from reformer_tts_amd.dataset.audio import dft_basis, idft_basis
    utts, ref = case
    bias = _bias().numpy()
    dft32, idft32 = dft_basis(N_FFT, N_FFT).numpy(), idft_basis(N_FFT, N_FFT).numpy()
    twin = max(_rel(denoise_ref.denoise_f32_twin(u.numpy(), bias, s, dft32, idft32), ref[s][i], u.numpy())
               for s in (0.0, 0.1, ALL_CLAMP) for i, u in enumerate(utts))
    bound = 4.0 * twin
    print(f"f32 twin vs float64, worst over the batch, relative to the peak: {twin:.3e} -> bound {bound:.3e}")
    assert 0.0 < twin < 1e-5
    worst = {}
    for s in (0.0, 0.1, ALL_CLAMP):
        got = denoiser([u.to(gpu) for u in utts], strength=s)
        assert [g.numel() for g in got] == LENGTHS
        errs = [_rel(g.cpu().numpy(), ref[s][i], utts[i].numpy()) for i, g in enumerate(got)]
        worst[s] = max(errs)
        print(f"strength {s}: kernel vs float64 per utterance {['%.2e' % e for e in errs]}")
        if s == 0.0:                                                    # nothing is subtracted: the input comes back
            back = max(_rel(g.cpu().numpy(), utts[i].numpy().astype(np.float64), utts[i].numpy()) for i, g in enumerate(got))
            print(f"strength 0: kernel vs its input {back:.3e}")
            assert back <= bound
    print(f"kernel vs float64, worst per strength: {worst}")
    assert all(e <= bound for e in worst.values()), (worst, bound)
    # every bin clamps (a bias without zeros): exactly zero
    from reformer_tts_amd.squeeze_wave import Denoiser
    clamp = Denoiser(bias_spec=_bias(zeros=False)).to(gpu)
    for g in clamp([u.to(gpu) for u in utts], strength=ALL_CLAMP):
        assert bool((g == 0).all())
    # where the bias is zero the bin passes whatever the strength: the zeros of _bias() are seen
    assert max(float(np.abs(r).max()) for r in ref[ALL_CLAMP]) > 1e-4


def _packed_call(d, utts, gpu, strength=0.1, lead=0, tail=0, sentinel=-7.0):
    """ops.denoise on a buffer with ``lead`` samples in front of the first utterance and ``tail`` behind the last."""
    from reformer_tts_amd import ops
    lens = [u.numel() for u in utts]
    off = [lead]
    for n in lens:
        off.append(off[-1] + n)
    audio = torch.full((off[-1] + tail,), float("nan"))
    for i, u in enumerate(utts):
        audio[off[i]:off[i + 1]] = u
    out = torch.full((off[-1] + tail,), sentinel, device=gpu)
    host = (ctypes.c_int64 * len(off))(*off)
    ops.denoise(audio.to(gpu), host, torch.tensor(off, dtype=torch.int64, device=gpu), len(lens), d.dft_basis, d.idft_basis, d.bias_spec,
                strength, N_FFT, HOP, out)
    return out, off


def test_batch_independence_and_untouched_memory(gpu, denoiser, case):
    utts, _ = case
    dev = [u.to(gpu) for u in utts]
    batch = denoiser(dev, strength=0.1)
    again = denoiser(dev, strength=0.1)
    rev = denoiser(dev[::-1], strength=0.1)[::-1]
    for i, u in enumerate(dev):
        alone = denoiser([u], strength=0.1)[0]
        assert torch.equal(alone, batch[i]) and torch.equal(rev[i], batch[i]) and torch.equal(again[i], batch[i]), LENGTHS[i]
    # samples in front of the first offset and behind the last are neither read (they are NaN) nor written (the sentinel stays)
    out, off = _packed_call(denoiser, utts, gpu, lead=5, tail=9)
    assert bool((out[:5] == -7.0).all()) and bool((out[off[-1]:] == -7.0).all())
    assert torch.equal(out[5:off[-1]], torch.cat(batch))
    # two calls into one buffer with a gap between their slots: the gap keeps the sentinel
    from reformer_tts_amd import ops
    a, b = utts[1], utts[3]
    gap0, gap1 = a.numel(), a.numel() + 300
    audio = torch.full((gap1 + b.numel(),), float("nan"))
    audio[:gap0], audio[gap1:] = a, b
    audio, out = audio.to(gpu), torch.full((gap1 + b.numel(),), -7.0, device=gpu)
    for lo, hi in ((0, gap0), (gap1, gap1 + b.numel())):
        ops.denoise(audio, (ctypes.c_int64 * 2)(lo, hi), torch.tensor([lo, hi], dtype=torch.int64, device=gpu), 1, denoiser.dft_basis,
                    denoiser.idft_basis, denoiser.bias_spec, 0.1, N_FFT, HOP, out)
    assert bool((out[gap0:gap1] == -7.0).all())
    assert torch.equal(out[:gap0], batch[1]) and torch.equal(out[gap1:], batch[3])


def test_short_utterances_pass_through(gpu, denoiser, case):
    utts, _ = case
    long = [utts[1], utts[3], utts[6]]
    short = [_audio(1, 90), _audio(256, 91), _audio(512, 92), _audio(0, 93)]
    mixed = [long[0], short[0], short[1], long[1], short[2], short[3], long[2]]
    got = denoiser([u.to(gpu) for u in mixed], strength=0.1)
    want = denoiser([u.to(gpu) for u in long], strength=0.1)
    assert [g.numel() for g in got] == [u.numel() for u in mixed]
    for i, j in ((1, 0), (2, 1), (4, 2), (5, 3)):
        assert torch.equal(got[i].cpu(), short[j]), i
    for i, j in ((0, 0), (3, 1), (6, 2)):
        assert torch.equal(got[i], want[j]), i
    # a batch of short utterances only launches nothing and returns them as they are
    only = denoiser([u.to(gpu) for u in short], strength=0.1)
    assert all(torch.equal(o.cpu(), s) for o, s in zip(only, short))
    assert denoiser.tables([u.numel() for u in short]).runs == []
    # the padded form: (B, N) with lengths -> (B, N), zero behind each utterance
    n_max = max(u.numel() for u in mixed)
    padded = torch.zeros(len(mixed), n_max)
    for i, u in enumerate(mixed):
        padded[i, :u.numel()] = u
    res = denoiser(padded.to(gpu), [u.numel() for u in mixed], strength=0.1)
    assert tuple(res.shape) == (len(mixed), n_max)
    for i, u in enumerate(mixed):
        assert torch.equal(res[i, :u.numel()], got[i]) and bool((res[i, u.numel():] == 0).all())


def test_graph_capture_replays_on_new_audio(gpu, denoiser):
    from reformer_tts_amd import _graphs
    lengths = [7681, 100, 600, 15105]
    tables = denoiser.tables(lengths)
    flat = torch.cat([_audio(n, 300 + i) for i, n in enumerate(lengths)]).to(gpu)
    out = torch.empty_like(flat)
    denoiser.forward_packed(flat, tables=tables, strength=0.1, out=out)  # warm-up: the LDS attribute is set outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _graphs.capturing(graph):
        denoiser.forward_packed(flat, tables=tables, strength=0.1, out=out)
    for seed in (400, 500):
        new = torch.cat([_audio(n, seed + i) for i, n in enumerate(lengths)]).to(gpu)
        flat.copy_(new)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager, off = denoiser.forward_packed(new, lengths, strength=0.1)
        assert off == [0, 7681, 7781, 8381, 23486]
        assert torch.equal(out, eager), f"replay on audio of seed {seed} differs from the eager call"
        assert torch.equal(out[7681:7781], new[7681:7781])


@pytest.fixture(scope="module")
def vocoder(gpu, golden_dir):
    from oracle import squeezewave_ref as sw_ref
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    z = np.load(os.path.join(golden_dir, "squeezewave_small.npz"))
    cfg = sw_ref.small_cfg()
    sw = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                     cfg["early_return_size"], WNConfig(**cfg["wn_config"]))
    sw.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, strict=False)
    return sw.to(gpu).eval()


def test_module_bias_and_synthesis_wiring(gpu, vocoder):
    from reformer_tts_amd import synthesis
    from reformer_tts_amd.squeeze_wave import Denoiser
    d = Denoiser(vocoder)
    bias_audio = Denoiser.bias_audio(vocoder, 88)
    assert bias_audio.numel() == 88 * 256 and torch.equal(bias_audio, Denoiser.bias_audio(vocoder, 88))    # zero latent: deterministic
    want = denoise_ref.first_frame_magnitudes_f64(bias_audio.cpu().numpy())
    assert d.bias_spec.dtype == torch.float32 and d.bias_spec.device.type == "cuda" and tuple(d.bias_spec.shape) == (N_FFT // 2 + 1,)
    assert float(want.max()) > 0.0
    # f32 rounding: half an ulp of each value, and the float64 paths themselves differ by about 1e-15 of the largest
    assert bool((np.abs(d.bias_spec.cpu().numpy().astype(np.float64) - want) <= 2.0 ** -24 * want + 1e-12 * want.max()).all())
    assert "bias_spec" in d.state_dict()

    g = torch.Generator().manual_seed(1)
    spec = ((torch.randn(4, 80, 20, generator=g) * 2 - 5).clamp(-11.5, 2.0)).to(gpu)
    stop = torch.tensor([7, 20, 2, 13])
    frames = [7, 20, 2, 13]
    noise = [[torch.randn(s, generator=g) for s in vocoder.noise_shapes(1, n)] for n in frames]
    plain = synthesis.vocode_trimmed(vocoder, spec, stop, noise=noise)
    for i, n in enumerate(frames):                                       # denoiser=None: today's waves
        assert torch.equal(plain[i], vocoder.infer(spec[i:i + 1, :, :n], noise=noise[i])[0])
    for s in (0.01, 0.5):
        got = synthesis.vocode_trimmed(vocoder, spec, stop, noise=noise, denoiser=d, denoiser_strength=s)
        want = d(plain, strength=s)
        assert [w.numel() for w in got] == [256 * n for n in frames]
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert torch.equal(got[2], plain[2])                             # two frames = 512 samples: passed through
    assert not torch.equal(got[1], plain[1])
    # the graphed path: the denoiser reads the graph's buffer; the replay's own draws reproduce it eagerly
    waves = synthesis.vocode_trimmed(vocoder, spec, stop, use_graph=True, denoiser=d, denoiser_strength=0.5)
    run = vocoder.capture_ragged(len(frames), synthesis.capacity_frames(sum(frames)))
    eager = synthesis.vocode_trimmed(vocoder, spec, stop, noise=vocoder.unpack_noise([z.clone() for z in run.noise], frames), denoiser=d,
                                     denoiser_strength=0.5)
    for a, b in zip(waves, eager):
        assert torch.equal(a, b)


def test_refusals_name_the_argument(gpu, denoiser):
    from reformer_tts_amd import _lib, ops
    from reformer_tts_amd.dataset.audio import dft_basis, idft_basis
    from reformer_tts_amd.squeeze_wave import Denoiser
    n = 4096
    audio, out = torch.zeros(n, device=gpu), torch.full((n,), -7.0, device=gpu)
    host, table = (ctypes.c_int64 * 2)(0, n), torch.tensor([0, n], dtype=torch.int64, device=gpu)

    def call(audio=audio, out=out, n_fft=N_FFT, hop=HOP, strength=0.1, bias=denoiser.bias_spec, bases=None):
        dft, idft = bases or (denoiser.dft_basis, denoiser.idft_basis)
        ops.denoise(audio, host, table, 1, dft, idft, bias, strength, n_fft, hop, out)

    for n_fft in (512, 2048):
        bases = (dft_basis(n_fft, n_fft).to(gpu), idft_basis(n_fft, n_fft).to(gpu))
        with pytest.raises(_lib.RttsError, match="rtts_denoise: n_fft must be 1024"):
            call(n_fft=n_fft, hop=n_fft // 4, bias=torch.zeros(n_fft // 2 + 1, device=gpu), bases=bases)
    for hop in (128, 512):
        with pytest.raises(_lib.RttsError, match="rtts_denoise: hop must be 256"):
            call(hop=hop)
    for s in (-0.1, float("nan"), float("inf")):
        with pytest.raises(_lib.RttsError, match="rtts_denoise: strength"):
            call(strength=s)
    buf = torch.zeros(2 * n, device=gpu)
    for a, o in ((buf[:n], buf[:n]), (buf[:n], buf[100:n + 100]), (buf[100:n + 100], buf[:n])):
        with pytest.raises(_lib.RttsError, match="rtts_denoise: out must not overlap audio"):
            call(audio=a, out=o)
    call(audio=buf[:n], out=buf[n:])                                     # adjacent is not overlapping
    for m in (512, 514):
        with pytest.raises(ValueError, match="bias must hold"):
            call(bias=torch.zeros(m, device=gpu))
    for kw in (dict(audio=audio.cpu()), dict(out=out.cpu()), dict(bias=denoiser.bias_spec.cpu()),
               dict(bases=(denoiser.dft_basis.cpu(), denoiser.idft_basis))):
        with pytest.raises(_lib.RttsError, match="GPU only"):
            call(**kw)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        denoiser([torch.zeros(n)])
    with pytest.raises(_lib.RttsError, match="GPU only"):
        denoiser.forward_packed(torch.zeros(n), [n])
    with pytest.raises(ValueError, match="n_fft"):
        Denoiser(bias_spec=_bias(), n_fft=512, win_length=512, hop_length=128)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote nothing"
