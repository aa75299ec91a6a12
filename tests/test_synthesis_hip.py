"""Batched text -> waveform (reformer_tts_amd.synthesis) on the GPU: the trim-and-vocode step against per-utterance
``SqueezeWave.infer`` bit for bit, generation from text with the recorded rotations of the reference golden, and the
graphed path's reuse of its vocoder graph."""
import os

import numpy as np
import pytest
import torch

from oracle import model_ref, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def vocoder(gpu):
    """The reference's default SqueezeWave configuration (every 1x1 convolution in-tree), seeded weights with a live
    end_conv so that every flow changes the audio."""
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    torch.manual_seed(0)
    sw = SqueezeWave(12, 128, 80, 2, 16, WNConfig(8, 256, 3, 2))
    for wn in sw.wn_layers:
        wn.end_conv.weight.data.normal_(0, 0.01)
    return sw.to(gpu).eval()


def _lsh_layers(model):
    from reformer_tts_amd.model.lsh_attention import LSHSelfAttention
    return [m for m in model.modules() if isinstance(m, LSHSelfAttention)]


def _tts(golden_dir, gpu, case="concat_stop"):
    """The small ReformerTTS of model_small.npz with the running statistics of infer_small.npz and the rotations recorded for
    ``case``, in call order (as tests/test_model_hip.py loads them for test_infer_matches_reference_golden)."""
    from reformer_tts_amd.model.config import model_config_from_dict
    from reformer_tts_amd.training import build_model
    cfg = model_ref.small_cfg()
    cfg["enc_reformer_kwargs"]["attn_kwargs"]["implementation"] = "hip"
    cfg["dec_reformer_kwargs"]["self_attn_kwargs"]["implementation"] = "hip"
    z = np.load(os.path.join(golden_dir, "model_small.npz"))
    model = build_model(model_config_from_dict(cfg), gpu)
    shapes = {k[len("shape/"):]: tuple(z[k]) for k in z.files if k.startswith("shape/")}
    model.load_state_dict(synth.synth_state_dict(shapes, seed=3), strict=False)
    zi = np.load(os.path.join(golden_dir, "infer_small.npz"))
    model.load_state_dict({k[4:]: torch.from_numpy(zi[k]) for k in zi.files if k.startswith("buf/")}, strict=False)
    rots = [torch.from_numpy(zi[f"{case}/rot/{i}"]) for i in range(int(zi[f"{case}/n_rot"]))]
    enc_l, dec_l = _lsh_layers(model)
    enc_l.forced_rotations, dec_l.forced_rotations = iter(rots[0::2]), iter(rots[1::2])
    return zi, model


def test_trim_and_vocode_is_per_utterance_infer(gpu, vocoder):
    """vocode_trimmed (what synthesize runs after infer): utterance i keeps spectrogram[:, :, :stop_i] (cli.py:241) -- a stop
    past the generated frames and a never-stopped one (stop == max_len) keep all 50 -- and its waveform equals
    vocoder.infer(spec[i:i+1, :, :stop_i]) with the same draws, bit for bit."""
    from reformer_tts_amd import synthesis
    g = torch.Generator().manual_seed(1)
    spec = ((torch.randn(5, 80, 50, generator=g) * 2 - 5).clamp(-11.5, 2.0)).to(gpu)
    stop = torch.tensor([7, 23, 55, 60, 1], device=gpu)
    frames = [7, 23, 50, 50, 1]
    noise = [[torch.randn(s, generator=g) for s in vocoder.noise_shapes(1, n)] for n in frames]
    waves = synthesis.vocode_trimmed(vocoder, spec, stop, noise=noise, max_len=60)
    assert [w.numel() for w in waves] == [256 * n for n in frames]
    for i, n in enumerate(frames):
        want = vocoder.infer(spec[i:i + 1, :, :int(min(int(stop[i]), 50))], noise=noise[i])[0]
        assert torch.equal(waves[i], want), (i, n, float((waves[i] - want).abs().max()))


def test_synthesize_from_text_matches_the_golden_stops(golden_dir, gpu, vocoder):
    """End to end from phoneme ids: the concat_stop case of infer_small.npz with check_every=1 (one recorded rotation set per
    forward, as test_infer_matches_reference_golden runs it).  The stop indices are the reference's; every waveform is
    finite, in [-1, 1], and 256 samples per kept frame."""
    from reformer_tts_amd import synthesis
    zi, tts = _tts(golden_dir, gpu)
    max_len, thr, use_stop = zi["concat_stop/kw"]
    phonemes = [torch.from_numpy(p) for p in zi["phonemes"]]
    waves, spec, stop = synthesis.synthesize(tts, vocoder, phonemes, max_len=int(max_len), stop_threshold=float(thr),
                                             stop_at_stop_token=bool(use_stop), check_every=1)
    assert torch.equal(stop.cpu(), torch.from_numpy(zi["concat_stop/stop"]))
    assert spec.shape == zi["concat_stop/spectrogram"].shape
    frames = synthesis.frame_counts(stop.cpu(), spec.shape[2], int(max_len))
    assert len(waves) == len(phonemes) and [w.numel() for w in waves] == [256 * n for n in frames]
    for w in waves:
        assert torch.isfinite(w).all() and float(w.abs().max()) <= 1.0


def test_synthesize_graphed_reuses_its_vocoder_graph(golden_dir, gpu, vocoder):
    """use_graph=True: graphed generation and one capture_ragged graph per capacity bucket.  A second call with other
    lengths in the same bucket replays the same graph; fed that replay's draws, the eager trim-and-vocode step gives the
    same waveforms bit for bit."""
    from reformer_tts_amd import synthesis
    zi, tts = _tts(golden_dir, gpu)
    enc_l, dec_l = _lsh_layers(tts)
    enc_l.forced_rotations = torch.from_numpy(zi["concat_stop/rot/0"])           # one tensor: reused by every call
    dec_l.forced_rotations = torch.from_numpy(zi["concat_stop/rot/1"])
    phonemes = [torch.from_numpy(p) for p in zi["phonemes"]]
    cache = vocoder.__dict__.setdefault("_ragged_graphs", {})
    cache.clear()
    runs = []
    for max_len in (90, 94):                   # generation runs while max(B, frames, n_mels = 80) <= max_len (reformer_tts.py:145-221)
        waves, spec, stop = synthesis.synthesize(tts, vocoder, phonemes, max_len=max_len, stop_at_stop_token=False, use_graph=True)
        frames = synthesis.frame_counts(stop.cpu(), spec.shape[2], max_len)
        assert synthesis.capacity_frames(sum(frames)) == 192 and len(set(frames)) == 1
        assert len(cache) == 1
        run = next(iter(cache.values()))
        runs.append(run)
        draws = [d.clone() for d in run.noise]
        eager = synthesis.vocode_trimmed(vocoder, spec, stop, noise=vocoder.unpack_noise(draws, frames))
        assert [w.numel() for w in waves] == [256 * n for n in frames]
        for a, b in zip(waves, eager):
            assert torch.equal(a, b), float((a - b).abs().max())
    assert runs[0] is runs[1] and runs[0].capacity == 192
