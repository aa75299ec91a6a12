"""``Trainer.fit_corpus`` against ``Trainer.fit`` on the GPU.

The small model, the batches and the forced rotations of ``test_fit_graph_cache_follows_the_eager_trajectory``
(tests/test_model_hip.py): ragged batches of three (text, mel) lengths in two padded shapes, accumulate 2, a trailing partial
group.  The same six items once as pinned host batches through ``fit(graphs=True)`` and once as a ``TTSCorpus`` with the same plan
through ``fit_corpus``: after every fill the graph entry's buffers hold the same bits, so the replayed graphs read the same
batch."""
import numpy as np
import pytest
import torch

from oracle import synth
from test_model_hip import _hip_cfg, _lsh_layers

pytestmark = pytest.mark.gpu

PLAN = [[0, 1], [2, 3], [4, 5], [0, 1], [2, 3], [4, 5], [0, 1]]                # groups (a,b) (c,a) (b,c) (a)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _items():
    g = torch.Generator().manual_seed(0)

    def items(n, lp, lm):
        return [dict(phonemes=torch.randint(1, 77, (int(lp * (0.6 + 0.4 * k / n)),), generator=g),
                     spectrogram=(torch.randn(int(lm * (0.5 + 0.5 * k / n)), 80, generator=g) * 2 - 5).clamp(-11.5, 2.0)) for k in range(1, n + 1)]
    return items(2, 60, 200) + items(2, 90, 150) + items(2, 150, 300)          # (128, 256), the same graph, (256, 384)


def _trainer(gpu, noise_std=None):
    from reformer_tts_amd import _seeds
    from reformer_tts_amd.model.config import TTSTrainingConfig
    from reformer_tts_amd.training import Trainer, build_model
    _seeds.reset()
    model = build_model(_hip_cfg(), gpu)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.synth_state_dict(shapes, seed=11), strict=False)
    for layer in _lsh_layers(model):
        layer.forced_rotations = {nb: torch.randn(1, 64, 4, nb // 2, generator=torch.Generator().manual_seed(nb)) for nb in (2, 4, 6)}
    tr = Trainer(model, TTSTrainingConfig(batch_size=2, learning_rate=1e-3, warmup_steps=None, accumulate_grad_batches=2, noise_std=noise_std), gpu)
    model.train()
    return tr


def _record(fills, tr, corpus=None):
    """Every fill of a graph entry's buffers, by either way, leaves a copy of the buffers in ``fills``."""
    host_fill = tr._fill_shape_buffers

    def filled(entry, batch):
        host_fill(entry, batch)
        fills.append(("host", {k: v.clone() for k, v in entry["bufs"].items()}))
    tr._fill_shape_buffers = filled
    if corpus is not None:
        device_fill = corpus.fill

        def launched(bufs, *a, **kw):
            device_fill(bufs, *a, **kw)
            fills.append(("device", {k: v.clone() for k, v in bufs.items()}))
        corpus.fill = launched


@pytest.fixture(scope="module")
def runs(gpu):
    from reformer_tts_amd.dataset import TTSCorpus, custom_sequence_padder
    items = _items()
    batches = [custom_sequence_padder([items[i] for i in ids], pin_memory=True) for ids in PLAN]
    out = dict(items=items)
    tr = _trainer(gpu)
    fills = []
    _record(fills, tr)
    out["host"] = dict(losses=[float(x) for x in tr.fit(batches, graphs=True)], fills=fills, keys=sorted(tr._shape_graphs), step=tr.global_step)
    corpus = TTSCorpus.from_items(items, gpu)
    tr = _trainer(gpu)
    fills = []
    _record(fills, tr, corpus)
    losses = [float(x) for x in tr.fit_corpus(corpus, PLAN, graphs=True)]
    torch.cuda.synchronize()
    out["corpus"] = dict(losses=losses, fills=fills, keys=sorted(tr._shape_graphs), step=tr.global_step, trainer=tr, corpus=corpus)
    return out


def test_fit_corpus_feeds_the_graphs_what_fit_feeds_them(runs):
    host, dev = runs["host"], runs["corpus"]
    assert host["step"] == 4 and dev["step"] == 4 and len(dev["losses"]) == 4
    assert dev["keys"] == host["keys"] == [(2, 1, 2), (2, 2, 3)]
    assert all(e is not None for e in dev["trainer"]._shape_graphs.values())
    assert len(dev["fills"]) == len(host["fills"]) == 2 + len(PLAN)             # two captures, seven micro-batches
    # a shape's first sight fills its buffers on the host path in both runs (the capture); every replay's fill is one launch
    assert [how for how, _ in host["fills"]] == ["host"] * 9
    assert [how for how, _ in dev["fills"]] == ["host", "device", "device", "host"] + ["device"] * 5
    for k, ((_, a), (_, b)) in enumerate(zip(host["fills"], dev["fills"])):
        for name in a:
            assert a[name].dtype == b[name].dtype and torch.equal(a[name], b[name]), (k, name)
    print(f"\n[fit vs fit_corpus] losses {host['losses']} vs {dev['losses']}: bit-equal {host['losses'] == dev['losses']}")
    np.testing.assert_allclose(dev["losses"], host["losses"], rtol=2e-3)


def test_second_epoch_runs_without_the_host_path(runs, monkeypatch):
    import reformer_tts_amd.dataset as D
    import reformer_tts_amd.dataset.utils as U
    tr, corpus = runs["corpus"]["trainer"], runs["corpus"]["corpus"]

    def never(*a, **kw):
        raise AssertionError("the host collate path ran inside fit_corpus")
    for mod in (D, U):
        monkeypatch.setattr(mod, "custom_sequence_padder", never)
        monkeypatch.setattr(mod, "BatchPrefetcher", never)
    monkeypatch.setattr(tr, "_fill_shape_buffers", never)
    monkeypatch.setattr(corpus, "collate", never)                              # every shape has its graph: nothing is collated either
    step, epoch = tr.global_step, tr.epoch
    losses = [float(x) for x in tr.fit_corpus(corpus, PLAN)]
    assert tr.global_step == step + 4 and tr.epoch == epoch + 1 and len(losses) == 4 and all(np.isfinite(losses))


def test_input_noise_changes_the_losses_reproducibly(runs, gpu):
    from reformer_tts_amd.dataset import TTSCorpus
    clean = runs["corpus"]["losses"]
    noisy = []
    for _ in range(2):
        tr = _trainer(gpu, noise_std=0.5)
        fills = []
        corpus = TTSCorpus.from_items(runs["items"], gpu)
        _record(fills, tr, corpus)
        noisy.append([float(x) for x in tr.fit_corpus(corpus, PLAN, graphs=True)])
        assert tr.global_step == 4
        # the noise reached the input, and only the input, of every replayed micro-batch; no two micro-batches share a seed
        micro = [bufs for how, bufs in fills if how == "device"]
        assert len(micro) == len(PLAN)
        for got, want in zip(micro, [bufs for how, bufs in runs["corpus"]["fills"] if how == "device"]):
            assert not torch.equal(got["spectrogram_input"], want["spectrogram_input"])
            for name in want:
                assert name == "spectrogram_input" or torch.equal(got[name], want[name]), name
        assert not torch.equal(micro[0]["spectrogram_input"], micro[3]["spectrogram_input"])       # the same batch, another step
    print(f"\n[fit_corpus, noise_std 0.5] losses {noisy[0]} (clean {clean})")
    assert noisy[0] == noisy[1]
    assert all(a != b for a, b in zip(noisy[0], clean))
    # a step without graphs trains on the same pair of arrays, unpadded
    eager = [float(x) for x in tr.fit_corpus(corpus, PLAN[:3], graphs=False)]
    assert tr.global_step == 6 and len(eager) == 2 and all(np.isfinite(eager))


def test_fit_on_host_batches_says_that_it_applies_no_noise(gpu):
    from reformer_tts_amd import _lib
    tr = _trainer(gpu, noise_std=0.5)
    tr.fit([], graphs=True)
    assert any(where == "Trainer.fit" and "fit_corpus" in why for where, why in _lib.PATHS_LEFT)


def test_validate_corpus_is_validate_of_the_collated_batch(runs, gpu):
    from reformer_tts_amd.dataset import custom_sequence_padder
    tr, corpus = runs["corpus"]["trainer"], runs["corpus"]["corpus"]
    for ids in ([4, 5], [1, 2]):
        host = {k: v.to(gpu) for k, v in custom_sequence_padder([runs["items"][i] for i in ids]).items()}
        want = tr.validate(host)
        got = tr.validate_corpus(corpus, ids)
        assert len(got) == len(want) == 5
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    got = tr.validate_corpus(corpus, [4, 5], return_attention=True)
    want = tr.validate({k: v.to(gpu) for k, v in custom_sequence_padder([runs["items"][i] for i in [4, 5]]).items()}, return_attention=True)
    assert len(got) == 6 and all(torch.equal(x, y) for a, b in zip(got[5], want[5]) for x, y in zip(a, b))
