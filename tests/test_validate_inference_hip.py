"""The generating half of validation on the GPU: ``Trainer.validate_inference`` / ``validate_inference_corpus`` (reference
``training/wrappers.py:165-211``), ``validation_epoch`` (``:130-163``, ``:224-232``) and ``predict_corpus`` (``cli.py:93-166``).

The small model of ``infer_small.npz``, loaded as tests/test_model_hip.py loads it, with one fixed rotation tensor per layer and
bucket count so that two generations are comparable.  ``stop_loss_weight = 0`` in the training configuration, so that generation
does not stop at a stop token (``wrappers.py:180``) and runs its 90 frames: the two truths, 50 and 120 frames, lie on either side.
Metrics are held to the float64 restatement (tests/infer_metrics_ref.py) on the very outputs they were computed from, 1e-10
relative (tests/test_infer_metrics_hip.py derives the bound)."""
import numpy as np
import pytest
import torch

import infer_metrics_ref as ref
from test_model_hip import _load_infer, _lsh_layers

pytestmark = pytest.mark.gpu

LENGTHS = (50, 120, 70, 130, 60)
KEYS = ("concat_inference_pred_mse", "concat_inference_stop_mae", "concat_inference_time")


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
    return dict(tr=tr, model=model, items=items, corpus=corpus, batch=corpus.collate([0, 1]), out={})


def _truths(env, ids):
    return [env["items"][i]["spectrogram"].t().numpy() for i in ids]


def _first(env):
    """The one graphed batch-form call most tests look at, made once."""
    if "first" not in env["out"]:
        env["out"]["first"] = env["tr"].validate_inference(env["batch"], max_len=90, return_outputs=True)
    return env["out"]["first"]


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    rel = float(np.max(np.abs(got - want) / np.abs(want)))
    print(f"[validate_inference] {what}: rel err {rel:.2e} (tol 1e-10)")
    assert rel <= 1e-10, what


def test_batch_form_is_infer_plus_the_restatement(env):
    out = _first(env)
    assert set(out) == set(KEYS) | {"sse", "stop_err", "spectrogram", "stop"}
    spec, stop = env["model"].infer(env["batch"]["phonemes"], combine_strategy="concat", max_len=90, stop_threshold=0.25,
                                    stop_at_stop_token=False, cache_encoder=False, use_graph=True)
    assert out["spectrogram"].shape == (2, 80, 90)
    assert torch.equal(out["spectrogram"], spec) and torch.equal(out["stop"], stop)
    sse, stop_err, totals = ref.infer_metrics(spec.cpu().numpy(), stop.cpu().numpy(), _truths(env, [0, 1]), 120)
    for k in KEYS[:2] + ("sse", "stop_err"):
        assert out[k].is_cuda and out[k].dtype == torch.float64
    _close(out["sse"].cpu(), sse, "sse")
    _close(out[KEYS[0]].cpu(), totals[0], "pred_mse")
    assert np.array_equal(out["stop_err"].cpu().numpy(), stop_err) and float(out[KEYS[1]]) == totals[1]
    assert isinstance(out[KEYS[2]], float) and out[KEYS[2]] > 0
    assert set(env["tr"].validate_inference(env["batch"], max_len=90)) == set(KEYS) | {"sse", "stop_err"}


def test_stop_at_stop_token_follows_the_stop_loss_weight(env, monkeypatch):
    """wrappers.py:180: generation stops at stop tokens unless the stop loss is switched off."""
    tr, seen = env["tr"], []
    real = env["model"].infer

    def infer(*a, **kw):
        seen.append(kw["stop_at_stop_token"])
        return real(*a, **kw)
    monkeypatch.setattr(env["model"], "infer", infer)
    for weight in (0.0, 1.0):
        monkeypatch.setattr(tr.cfg, "stop_loss_weight", weight)
        tr.validate_inference(env["batch"], max_len=90)
    assert seen == [False, True]


def test_graphed_and_eager_generation_agree(env):
    """Same stops; frames within the tolerance tests/test_model_hip.py::test_infer_graphed_crosses_a_padding_window holds the
    two loops to (0.2 of the value range over the first frames), and the metrics within the same fraction."""
    a = _first(env)
    b = env["tr"].validate_inference(env["batch"], max_len=90, use_graph=False, return_outputs=True)
    assert torch.equal(a["stop"], b["stop"]) and torch.equal(a["stop_err"], b["stop_err"]) and torch.equal(a[KEYS[1]], b[KEYS[1]])
    scale = float(b["spectrogram"].abs().max())
    frames = float((a["spectrogram"][:, :, :4] - b["spectrogram"][:, :, :4]).abs().max())
    mse = abs(float(a[KEYS[0]]) - float(b[KEYS[0]])) / float(b[KEYS[0]])
    print(f"[validate_inference] graphed vs eager: first frames differ by {frames:.3e} (range {scale:.3e}), pred_mse by {mse:.3e} relative")
    assert frames < 0.2 * scale and mse < 0.2
    sse, _, totals = ref.infer_metrics(b["spectrogram"].cpu().numpy(), b["stop"].cpu().numpy(), _truths(env, [0, 1]), 120)
    _close(b["sse"].cpu(), sse, "eager sse")
    _close(b[KEYS[0]].cpu(), totals[0], "eager pred_mse")


def test_replace_strategy_runs_the_eager_loop_under_its_own_keys(env):
    out = env["tr"].validate_inference(env["batch"], "replace", max_len=60, return_outputs=True)     # max_len < n_mel: one forward
    assert out["spectrogram"].shape[2] >= 1
    assert {"replace_inference_pred_mse", "replace_inference_stop_mae", "replace_inference_time"} <= set(out)
    sse, stop_err, totals = ref.infer_metrics(out["spectrogram"].cpu().numpy(), out["stop"].cpu().numpy(), _truths(env, [0, 1]), 120)
    _close(out["replace_inference_pred_mse"].cpu(), totals[0], "replace pred_mse")
    assert np.array_equal(out["stop_err"].cpu().numpy(), stop_err)


def test_corpus_form_gives_the_same_bits(env, monkeypatch):
    a = _first(env)
    monkeypatch.setattr(env["corpus"], "collate", None)                         # no padded truth batch is built
    b = env["tr"].validate_inference_corpus(env["corpus"], [0, 1], max_len=90, return_outputs=True)
    assert set(a) == set(b)
    for k in a:
        if k != KEYS[2]:
            assert torch.equal(a[k], b[k]), k


def test_each_slot_is_scored_against_its_own_truth(env, monkeypatch):
    """The small model's 90 generated frames dwarf the truths, so the checks above say little about WHICH truth frames were
    read.  Here ``infer`` is replaced by a log-mel-like spectrogram of 90 frames: both forms must still equal the restatement,
    for a batch whose slots are out of corpus order."""
    gen, stop, _ = ref.make_case(80, [130, 50], 90, seed=3)
    fake = (torch.from_numpy(gen).to(env["batch"]["phonemes"].device), torch.from_numpy(stop).to(env["batch"]["phonemes"].device))
    monkeypatch.setattr(env["model"], "infer", lambda *a, **kw: fake)
    ids = [3, 0]
    sse, stop_err, totals = ref.infer_metrics(gen, stop, _truths(env, ids), 130)
    outs = [env["tr"].validate_inference_corpus(env["corpus"], ids, max_len=90), env["tr"].validate_inference(env["corpus"].collate(ids), max_len=90)]
    for out in outs:
        _close(out["sse"].cpu(), sse, "sse of a tame spectrogram")
        _close(out[KEYS[0]].cpu(), totals[0], "pred_mse of a tame spectrogram")
        assert np.array_equal(out["stop_err"].cpu().numpy(), stop_err) and float(out[KEYS[1]]) == totals[1]
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in ("sse", "stop_err") + KEYS[:2])


def _snapshot(tr):
    m = tr.model
    stacks = (m.enc.reformer.layers, m.dec.reformer.layers)
    return dict(p=tr.flat_p.clone(), m=tr.flat_m.clone(), v=tr.flat_v.clone(), buffers=[t.clone() for t in m.buffers()], step=tr.global_step,
                training=m.training, collect=m.dec.reformer.collect_attention, fused=[st.fused_in_eval for st in stacks])


def _same_state(tr, was):
    now = _snapshot(tr)
    for k in ("p", "m", "v"):
        assert torch.equal(now[k], was[k]), k
    assert all(torch.equal(a, b) for a, b in zip(now["buffers"], was["buffers"]))
    assert [now[k] for k in ("step", "training", "collect", "fused")] == [was[k] for k in ("step", "training", "collect", "fused")]


def test_the_trainer_is_left_as_it_was(env, monkeypatch):
    """After a real optimizer step (non-zero moments, a cached shape graph): parameters, moments, BatchNorm statistics,
    global_step, mode and flags survive every form, in train and in eval mode, and the next fit_corpus step replays the cached
    graph -- a new capture would call ``_shape_graph``."""
    tr, corpus, model = env["tr"], env["corpus"], env["model"]
    tr.fit_corpus(corpus, [[0, 1]], graphs=True)
    graphs = dict(tr._shape_graphs)
    assert len(graphs) == 1 and all(e is not None for e in graphs.values())
    dec = model.dec.reformer
    for training, collect in ((True, True), (False, False)):
        model.train(training)
        dec.collect_attention = collect
        was = _snapshot(tr)
        batch = corpus.collate([0, 1])
        tr.validate_inference(batch, max_len=90)
        _same_state(tr, was)
        tr.validate_inference(batch, max_len=60, use_graph=False)                # max_len < n_mel: one eager forward
        _same_state(tr, was)
        tr.validate_inference_corpus(corpus, [1, 0], max_len=90)
        _same_state(tr, was)
        tr.predict_corpus(corpus, [0, 1])
        _same_state(tr, was)
    model.train()
    dec.collect_attention = False
    assert sorted(tr._shape_graphs) == sorted(graphs) and all(tr._shape_graphs[k] is e for k, e in graphs.items())

    def never(*a, **kw):
        raise AssertionError("a new capture after validate_inference")
    monkeypatch.setattr(tr, "_shape_graph", never)
    step = tr.global_step
    losses = tr.fit_corpus(corpus, [[0, 1]], graphs=True)
    assert tr.global_step == step + 1 and np.isfinite(float(losses[0]))
    env["out"].pop("first", None)                                               # the parameters moved: earlier outputs are stale


def test_validation_epoch_is_the_reference_epoch(env):
    """Five utterances in batches of two: two batches, the fifth dropped; the mean over batches of validate_corpus's five values
    and validate_inference_corpus of the first batch, under exactly the reference's eight names."""
    tr, corpus = env["tr"], env["corpus"]
    ids = [3, 1, 4, 0, 2]
    logs = tr.validation_epoch(corpus, ids, batch_size=2, max_len=90)
    assert set(logs) == {"val_loss", "val_stop_loss", "val_raw_pred_loss", "val_post_pred_loss", "val_stop_mae"} | set(KEYS)
    assert all(isinstance(v, float) for v in logs.values())
    rows = [tr.validate_corpus(corpus, ids[:2]), tr.validate_corpus(corpus, ids[2:4])]          # total, raw, post, stop, stop_mae
    for k, name in enumerate(("val_loss", "val_raw_pred_loss", "val_post_pred_loss", "val_stop_loss", "val_stop_mae")):
        assert logs[name] == float((rows[0][k] + rows[1][k]) / 2), name
    inf = tr.validate_inference_corpus(corpus, ids[:2], max_len=90)
    assert logs[KEYS[0]] == float(inf[KEYS[0]]) and logs[KEYS[1]] == float(inf[KEYS[1]]) and logs[KEYS[2]] > 0
    assert set(tr.validation_epoch(corpus, ids, batch_size=2, inference=False)) == set(logs) - set(KEYS)
    with pytest.raises(ValueError, match="no batch"):
        tr.validation_epoch(corpus, ids[:1], batch_size=2)


def test_predict_corpus_scores_and_trims_per_utterance(env, gpu):
    from reformer_tts_amd import synthesis
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    tr, corpus = env["tr"], env["corpus"]
    ids = [1, 0, 4]
    out = tr.predict_corpus(corpus, ids)
    assert set(out) == {"spectrogram", "mse", "cutoff"} and out["spectrogram"].shape == (3, 80, 120)
    lens = [LENGTHS[i] for i in ids]
    sse, _, _ = ref.infer_metrics(out["spectrogram"].cpu().numpy(), None, _truths(env, ids), 120)
    _close(out["mse"].cpu(), sse / (np.array(lens) * 80.0), "predict mse")
    # the stop logits of the same eval forward (validate's), argmax over each utterance's own frames on the host
    batch = corpus.collate(ids)
    model = env["model"]
    flags = tr._eval_flags()
    model.eval()
    for st, _ in flags[2]:
        st.fused_in_eval = True
    with torch.no_grad():
        _, post, stop, _ = model(batch["phonemes"], batch["spectrogram"][:, :-1], spectrogram_mask=batch["loss_mask"].mean(dim=-1))
    tr._restore_flags(flags)
    assert torch.equal(post.transpose(1, 2), out["spectrogram"])
    stop = stop.reshape(3, -1).float().cpu().numpy()
    assert out["cutoff"].tolist() == [int(np.argmax(stop[b, :n])) for b, n in enumerate(lens)]
    torch.manual_seed(0)
    vocoder = SqueezeWave(12, 128, 80, 2, 16, WNConfig(8, 256, 3, 2)).to(gpu).eval()
    waves = synthesis.vocode_trimmed(vocoder, out["spectrogram"], out["cutoff"])
    assert [w.numel() for w in waves] == [256 * int(c) for c in out["cutoff"].tolist()]
