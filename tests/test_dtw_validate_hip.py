"""MCD-DTW where the package reports it: ``Trainer.validate_inference(dtw=True)`` / ``validate_inference_corpus`` /
``validation_epoch(dtw=True)`` and ``evaluation.audio_mcd``.  The small model and corpus of tests/test_validate_inference_hip.py
(90 generated frames, truths of 50 and 120 frames on either side); the kernel itself is held to float64 in tests/test_dtw_hip.py,
so here the extra entries only have to BE one ``evaluation.mel_cepstral_distortion`` call on the outputs the call returned, and
everything else has to be the bits it was without the keyword."""
import numpy as np
import pytest
import torch

import dtw_ref as ref
from test_model_hip import _load_infer, _lsh_layers

pytestmark = pytest.mark.gpu

KEYS = ("concat_inference_pred_mse", "concat_inference_stop_mae", "concat_inference_time")
LENGTHS = (50, 120, 70, 130, 60)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def env(golden_dir, gpu):
    from reformer_tts_amd import _seeds
    from reformer_tts_amd.dataset import TTSCorpus
    from reformer_tts_amd.model.config import TTSTrainingConfig
    from reformer_tts_amd.training import Trainer
    _seeds.reset()
    zi, model = _load_infer(golden_dir, gpu, "concat_stop")
    for layer in _lsh_layers(model):
        layer.forced_rotations = {nb: torch.randn(1, 64, 4, nb // 2, generator=torch.Generator().manual_seed(nb)) for nb in (2, 4, 6)}
    tr = Trainer(model, TTSTrainingConfig(batch_size=2, learning_rate=1e-3, warmup_steps=None, stop_loss_weight=0.0), gpu)
    model.train()
    g = torch.Generator().manual_seed(7)
    texts = [torch.from_numpy(p[p != 0]).long() for p in zi["phonemes"]] + [torch.randint(1, 77, (n,), generator=g) for n in (30, 44, 25)]
    items = [dict(phonemes=t, spectrogram=(torch.randn(n, 80, generator=g) * 2 - 5).clamp(-11.5, 2.0)) for t, n in zip(texts, LENGTHS)]
    corpus = TTSCorpus.from_items(items, gpu)
    return dict(tr=tr, model=model, items=items, corpus=corpus, batch=corpus.collate([0, 1]))


def test_validate_inference_adds_one_mcd_call_and_changes_nothing_else(env):
    from reformer_tts_amd import evaluation
    tr, batch = env["tr"], env["batch"]
    plain = tr.validate_inference(batch, max_len=90, return_outputs=True)
    with_dtw = tr.validate_inference(batch, max_len=90, return_outputs=True, dtw=True)
    assert set(with_dtw) == set(plain) | {"concat_inference_mcd", "mcd", "dtw_steps"}
    for k in plain:
        if k != KEYS[2]:
            assert torch.equal(plain[k], with_dtw[k]), k
    # the same call, made by hand on the returned outputs against the collate batch's own rows
    spec = batch["spectrogram"]
    b, rows, n_mel = spec.shape
    lengths = (batch["stop_tokens"].argmax(dim=1) + 1).to(torch.int32)
    mcd, steps, totals = evaluation.mel_cepstral_distortion(
        with_dtw["spectrogram"], with_dtw["stop"], spec.contiguous().view(b * rows, n_mel), rows - 1, truth_frames_last=False,
        starts=torch.arange(b, dtype=torch.int64, device=spec.device) * rows + 1, lengths=lengths)
    assert torch.equal(with_dtw["mcd"], mcd) and torch.equal(with_dtw["dtw_steps"], steps) and torch.equal(with_dtw["concat_inference_mcd"], totals[0])
    assert with_dtw["mcd"].dtype == torch.float64 and with_dtw["dtw_steps"].dtype == torch.int32 and with_dtw["concat_inference_mcd"].dim() == 0
    # and that call is the restatement's, on min(stop_b, L) generated frames and the utterance's own truth
    gen, stop = with_dtw["spectrogram"].cpu().numpy(), with_dtw["stop"].cpu().tolist()
    gens = [gen[i, :, :min(int(stop[i]), gen.shape[2])] for i in range(2)]
    truths = [env["items"][i]["spectrogram"].t().numpy() for i in (0, 1)]
    cost, want_steps, _, slots = ref.align(gens, truths, ref.cepstral_basis(80, 13).astype(np.float32))
    print(f"\n[validate dtw] mcd {mcd.tolist()} dB over {steps.tolist()} steps; restatement cost / steps {(cost / want_steps).tolist()} over "
          f"{want_steps.tolist()}, margins {[s['margin'] for s in slots]}, E {[s['E'] for s in slots]}")
    # the path cost to the kernel test's bound; the path LENGTH only where the restatement's path is not a near-tie (the small
    # model's 90 frames are far from any truth and almost alike, so two paths of different lengths can cost the same to 1e-8)
    np.testing.assert_allclose((mcd * steps).cpu().numpy(), cost, rtol=17 * 2.0 ** -23)
    for i, s in enumerate(slots):
        if s["margin"] > 8 * s["E"]:
            assert int(steps[i]) == want_steps[i]
    assert [max(g.shape[1], t.shape[1]) <= s < g.shape[1] + t.shape[1] for g, t, s in zip(gens, truths, steps.tolist())] == [True, True]
    np.testing.assert_allclose(float(with_dtw["concat_inference_mcd"]), np.mean(mcd.cpu().numpy()), rtol=1e-14)
    assert np.all(mcd.cpu().numpy() > 0)


def test_corpus_form_gives_the_same_bits(env):
    tr = env["tr"]
    a = tr.validate_inference(env["batch"], max_len=90, dtw=True)
    b = tr.validate_inference_corpus(env["corpus"], [0, 1], max_len=90, dtw=True)
    assert set(a) == set(b) == set(KEYS) | {"sse", "stop_err", "mcd", "dtw_steps", "concat_inference_mcd"}
    for k in a:
        if k != KEYS[2]:
            assert torch.equal(a[k], b[k]), k
    assert set(tr.validate_inference_corpus(env["corpus"], [0, 1], max_len=90)) == set(KEYS) | {"sse", "stop_err"}


def test_validation_epoch_has_nine_entries(env):
    tr, corpus = env["tr"], env["corpus"]
    ids = [3, 1, 4, 0, 2]
    logs = tr.validation_epoch(corpus, ids, batch_size=2, max_len=90, dtw=True)
    eight = {"val_loss", "val_stop_loss", "val_raw_pred_loss", "val_post_pred_loss", "val_stop_mae"} | set(KEYS)
    assert set(logs) == eight | {"concat_inference_mcd"} and len(logs) == 9
    assert all(isinstance(v, float) for v in logs.values())
    inf = tr.validate_inference_corpus(corpus, ids[:2], max_len=90, dtw=True)
    assert logs["concat_inference_mcd"] == float(inf["concat_inference_mcd"]) and logs[KEYS[0]] == float(inf[KEYS[0]])
    plain = tr.validation_epoch(corpus, ids, batch_size=2, max_len=90)
    assert set(plain) == eight and all(plain[k] == logs[k] for k in eight - {KEYS[2]})
    assert set(tr.validation_epoch(corpus, ids, batch_size=2, inference=False, dtw=True)) == eight - set(KEYS)


def test_audio_mcd_of_a_waveform_against_its_own_log_mel_is_zero(gpu):
    from reformer_tts_amd import evaluation
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram
    creator = Tacotron2Spectrogram(22050, 1024, 1024, 256, 80).to(gpu)
    g = torch.Generator().manual_seed(3)
    waves = [(0.3 * torch.randn(n, generator=g)).to(gpu) for n in (256 * 20, 256 * 33 + 100)]
    mel, frames = creator(waves)
    frames = frames.cpu().tolist()
    assert frames == [21, 34]
    own = evaluation.audio_mcd(waves, mel, frames, creator)
    assert own.dtype == torch.float64 and own.tolist() == [0.0, 0.0]
    # another waveform is not at distance zero, and fewer spectrogram frames than the audio has still align
    other = evaluation.audio_mcd([waves[0].flip(0), waves[1]], mel, [21, 30], creator)
    assert float(other[0]) > 0 and np.isfinite(other.cpu().numpy()).all()
    with pytest.raises(ValueError, match="audio_mcd"):
        evaluation.audio_mcd(waves[:1], mel, frames, creator)
