"""Alignment scores and durations where the trainer reports them: ``validate`` / ``validate_corpus(alignment=True)``,
``validation_epoch(alignment=True)`` and ``extract_durations``.  The small model and corpus of tests/test_dtw_validate_hip.py; the
kernels are held to float64 in tests/test_align_hip.py, so here the extra entries only have to BE the ``evaluation`` calls on the
matrices the forward collected, and everything else has to be the bits it was without the keyword."""
import numpy as np
import pytest
import torch

from test_model_hip import _load_infer, _lsh_layers

pytestmark = pytest.mark.gpu

LENGTHS = (50, 120, 70, 130, 60)
NEW = ("val_alignment_focus", "val_alignment_guided", "val_alignment_monotonic", "val_alignment_path_mass", "val_alignment_layer")


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


def _equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def test_validate_appends_the_two_dictionaries_and_moves_nothing_else(env):
    from reformer_tts_amd import evaluation
    tr, batch, model = env["tr"], env["batch"], env["model"]
    plain = tr.validate(batch)
    got = tr.validate(batch, alignment=True)
    both = tr.validate(batch, return_attention=True, alignment=True)
    assert len(plain) == 5 and len(got) == 7 and len(both) == 8 and isinstance(both[5], list)
    for x, y, z in zip(plain, got[:5], both[:5]):
        assert torch.equal(x, y) and torch.equal(x, z)
    scores, durs = got[5], got[6]
    # the same two calls, made by hand on the matrices of return_attention's forward, with its stop indices
    full = list(model.dec.reformer.attention_matrices_)
    n_frames = batch["stop_tokens"].argmax(dim=1)
    n_keys = (batch["phonemes"] != 0).sum(dim=1)
    want_scores = evaluation.alignment_scores(full, n_frames.to(torch.int32), n_keys.to(torch.int32))
    want_durs = evaluation.alignment_durations(full, n_frames.to(torch.int32), n_keys.to(torch.int32))
    depth, b = model.dec.reformer.depth, batch["phonemes"].shape[0]
    assert set(scores) == set(want_scores) and set(durs) == set(want_durs)
    for k in scores:
        assert scores[k].is_cuda and _equal(scores[k], want_scores[k]) and _equal(scores[k], both[6][k]), k
    for k in durs:
        assert durs[k].is_cuda and _equal(durs[k], want_durs[k]) and _equal(durs[k], both[7][k]), k
    assert scores["focus"].shape == (depth, b) and durs["durations"].shape[:2] == (depth, b)
    # the trimmed matrices of return_attention are the rows the statistics read
    stops = n_frames.tolist()
    assert [m[0].shape[0] for m in both[5]] == stops and scores["table"][0, :-1, 0].tolist() == [float(s) for s in stops]
    assert scores["table"][0, :-1, 1].tolist() == [float(k) for k in n_keys.tolist()]
    focus = torch.stack([torch.stack([both[5][i][l][:, :int(n_keys[i])].max(dim=1).values.double().mean() for i in range(b)]) for l in range(depth)])
    np.testing.assert_allclose(scores["focus"].cpu().numpy(), focus.cpu().numpy(), rtol=1e-12)
    assert bool((durs["durations"].sum(-1) == n_frames.to(torch.int32)).all())
    assert model.training and model.dec.reformer.collect_attention
    # the corpus form is the batch form
    via_corpus = tr.validate_corpus(env["corpus"], [0, 1], alignment=True)
    assert len(via_corpus) == 7 and all(torch.equal(x, y) for x, y in zip(plain, via_corpus[:5]))
    assert _equal(via_corpus[5]["table"], scores["table"]) and _equal(via_corpus[6]["scores"], durs["scores"])


def test_validation_epoch_adds_five_entries(env):
    from reformer_tts_amd import evaluation
    tr, corpus = env["tr"], env["corpus"]
    ids = [3, 1, 4, 0, 2]
    plain = tr.validation_epoch(corpus, ids, batch_size=2, inference=False)
    logs = tr.validation_epoch(corpus, ids, batch_size=2, inference=False, alignment=True)
    assert set(logs) == set(plain) | set(NEW) and len(logs) == len(plain) + 5
    assert all(logs[k] == plain[k] for k in plain)
    assert isinstance(logs["val_alignment_layer"], int) and all(isinstance(logs[k], float) for k in NEW[:4])
    rows, layer = [], None
    for pair in ([3, 1], [4, 0]):
        out = tr.validate_corpus(corpus, pair, alignment=True)
        layer = int(evaluation.most_focused_layer(out[5]))
        rows.append([float(out[5][k][layer].mean()) for k in ("focus", "guided", "monotonic")] + [float(out[6]["path_mass"][layer].mean())])
    np.testing.assert_allclose([logs[k] for k in NEW[:4]], np.mean(rows, axis=0), rtol=1e-12)
    assert logs["val_alignment_layer"] == layer
    assert 0.0 < logs["val_alignment_focus"] <= 1.0 and 0.0 <= logs["val_alignment_guided"] <= 1.0
    assert 0.0 <= logs["val_alignment_monotonic"] <= 1.0 and 0.0 < logs["val_alignment_path_mass"] <= 1.0
    with_inference = tr.validation_epoch(corpus, ids, batch_size=2, max_len=90, alignment=True)
    assert set(with_inference) == set(logs) | {"concat_inference_pred_mse", "concat_inference_stop_mae", "concat_inference_time"}
    assert all(with_inference[k] == logs[k] for k in logs)


def test_extract_durations(env):
    tr, corpus, model = env["tr"], env["corpus"], env["model"]
    ids = [1, 3, 0]
    snap = tr.flat_p.clone()
    out = tr.extract_durations(corpus, ids)
    assert set(out) == {"durations", "layer", "log_prob", "path_mass", "n_frames", "n_keys"} and all(v.is_cuda for v in out.values())
    batch = corpus.collate(ids)
    n_frames, n_keys = batch["stop_tokens"].argmax(dim=1), (batch["phonemes"] != 0).sum(dim=1)
    assert out["n_frames"].dtype == torch.int32 and out["n_frames"].tolist() == n_frames.tolist() and out["n_keys"].tolist() == n_keys.tolist()
    assert n_keys.tolist() == [len(env["items"][i]["phonemes"]) for i in ids]
    dur = out["durations"]
    assert dur.dtype == torch.int32 and dur.dim() == 2 and dur.shape[0] == 3
    assert dur.sum(dim=1).tolist() == n_frames.tolist()
    for i, k in enumerate(n_keys.tolist()):
        assert int(dur[i, :k].min()) >= 1 and not bool(dur[i, k:].any())
    assert out["layer"].dtype == torch.int64 and 0 <= int(out["layer"]) < model.dec.reformer.depth
    assert out["log_prob"].shape == out["path_mass"].shape == (3,) and bool((out["log_prob"] < 0).all()) and bool((out["path_mass"] > 0).all())
    # the same figures as validate_corpus(alignment=True) reports for that layer
    scores, durs = tr.validate_corpus(corpus, ids, alignment=True)[5:]
    layer = int(out["layer"])
    assert _equal(dur, durs["durations"][layer]) and _equal(out["path_mass"], durs["path_mass"][layer])
    assert torch.equal(tr.flat_p, snap) and model.training
