"""The host side of the device-resident TTS corpus: the restatement the GPU tests hold ``rtts_tts_collate`` to
(tests/tts_corpus_ref.py) against ``custom_sequence_padder`` and ``Trainer._fill_shape_buffers``, the noise's hash and statistics,
the two epoch plans, the transcript vocabulary, the configuration key and ``TTSCorpus``'s refusals.  No GPU."""
import csv

import numpy as np
import pytest
import torch

import tts_corpus_ref as ref
from oracle.synth import drop_hash

BATCHES = ([5], [0, 0, 3], [6, 5, 4, 2, 1], [0, 1, 2, 3, 4, 5, 6])


def _bufs(b, LP, LM, n_mel, fill=float("nan")):
    return dict(phonemes=torch.full((b, LP), -1, dtype=torch.int64), spectrogram_input=torch.full((b, LM, n_mel), fill),
                spectrogram_target=torch.full((b, LM, n_mel), fill), stop_tokens=torch.full((b, LM), fill),
                loss_mask=torch.full((b, LM, n_mel), fill), valid_len=torch.full((1,), -1, dtype=torch.int32))


@pytest.mark.parametrize("n_mel", [80, 8])
@pytest.mark.parametrize("ids", BATCHES, ids=str)
def test_restated_collate_is_the_reference_collate_and_the_graph_fill(ids, n_mel):
    from reformer_tts_amd.dataset import custom_sequence_padder
    from reformer_tts_amd.training import Trainer
    items = ref.toy_items(n_mel)
    batch = [items[i] for i in ids]
    pad = custom_sequence_padder(batch)
    got = ref.collate(batch, n_mel)
    assert torch.equal(got["phonemes"], pad["phonemes"]) and got["phonemes"].dtype == pad["phonemes"].dtype
    assert torch.equal(got["spectrogram_input"], pad["spectrogram"])
    assert torch.equal(got["spectrogram_target"], pad["spectrogram"][:, 1:])
    assert torch.equal(got["stop_tokens"], pad["stop_tokens"]) and torch.equal(got["loss_mask"], pad["loss_mask"])
    lp, lm = pad["phonemes"].shape[1], pad["stop_tokens"].shape[1]
    for LM in (lm, -(-lm // 128) * 128):
        LP = -(-lp // 128) * 128
        bufs = _bufs(len(ids), LP, LM, n_mel)
        Trainer._fill_shape_buffers(None, dict(bufs=bufs), pad)
        got = ref.collate(batch, n_mel, LP=LP, R_in=LM, valid_in=lm, R=LM)
        for k, v in got.items():
            assert torch.equal(v, bufs[k]), (k, LM)
        assert int(bufs["valid_len"]) == lm


def test_a_missing_utterance_is_an_all_zero_slot():
    items = ref.toy_items(8)
    got = ref.collate([items[1], None, items[3]], 8)
    want = ref.collate([items[1], items[3]], 8)
    for k in got:
        assert torch.equal(got[k][[0, 2]], want[k]) and not got[k][1].any(), k


def test_hash_twin_stays_in_32_bits():
    rng = np.random.default_rng(0)
    idx = np.concatenate([rng.integers(0, 2 ** 32, 4096, dtype=np.uint64), [0, 1, 2 ** 31, 2 ** 32 - 1]]).astype(np.uint32)
    for seed in (0, 1, 0x9E3779B9, 2 ** 32 - 1):
        got = ref.drop_hash32(seed, idx)
        assert got.dtype == np.uint32
        assert np.array_equal(got.astype(np.uint64), drop_hash(seed, idx.astype(np.uint64)))
    # the doubled element index wraps as the kernel's 2u * e does
    u1, u2 = ref.uniforms(3, 1, np.array([2 ** 31 + 5], dtype=np.uint32))
    w1, w2 = ref.uniforms(3, 1, np.array([5], dtype=np.uint32))
    assert u1 == w1 and u2 == w2 and 0 < u1 <= 1 and 0 <= u2 < 1


def test_noise_is_standard_normal():
    n = 1 << 17
    z = ref.gauss64(1234, 3, np.arange(n, dtype=np.uint32))
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.77
    assert abs(z.mean()) <= 4 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= 0.03, z.var()
    other = ref.gauss64(1234, 4, np.arange(n, dtype=np.uint32))                 # another slot, another stream
    assert abs(np.corrcoef(z, other)[0, 1]) <= 4 / np.sqrt(n)
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) <= 4 / np.sqrt(n)             # neighbours do not follow each other


@pytest.mark.parametrize("drop_last", [True, False])
def test_batch_plan_is_a_permutation_per_epoch(drop_last):
    from reformer_tts_amd.dataset import batch_plan
    idx = list(range(3, 26))                                                     # 23 utterances, batches of 4
    plans = [batch_plan([1] * 40, idx, 4, True, drop_last, seed=7, epoch=e) for e in (0, 1)]
    for e, plan in enumerate(plans):
        flat = [i for b in plan for i in b]
        assert len(set(flat)) == len(flat) and set(flat) <= set(idx)
        assert len(flat) == (20 if drop_last else 23)
        assert all(len(b) == 4 for b in plan[:-1]) and len(plan[-1]) == (4 if drop_last else 3)
        assert plan == ref.batch_plan(idx, 4, True, drop_last, 7, e)
        assert plan == batch_plan([1] * 40, idx, 4, True, drop_last, seed=7, epoch=e)
    assert plans[0] != plans[1]
    assert batch_plan([1] * 6, None, 4, False, drop_last) == ([[0, 1, 2, 3]] if drop_last else [[0, 1, 2, 3], [4, 5]])


def test_variable_batch_plan_is_the_reference_bucketing():
    from reformer_tts_amd.dataset import variable_batch_plan
    # buckets 64.. (batch 4), 128.. (2), 256.. (1); 512 and 700 are >= max_mel_len; one 64-bucket and one 128-bucket stay incomplete
    lengths = [64, 300, 127, 128, 512, 100, 255, 65, 90, 256, 200, 511, 700, 70, 64]
    want, want_dropped = ref.variable_buckets(lengths, 64, 512, 1)
    assert want == [[0, 2, 5, 7], [3, 6], [1], [9], [11]] and want_dropped == [4, 12, 8, 13, 14, 10]
    plan, dropped = variable_batch_plan(lengths, None, 64, 512, 1, seed=1, epoch=0)
    assert [sorted(b) for b in plan] == [sorted(b) for b in want] and dropped == want_dropped
    again, _ = variable_batch_plan(lengths, None, 64, 512, 1, seed=1, epoch=0)
    other, _ = variable_batch_plan(lengths, None, 64, 512, 1, seed=1, epoch=1)
    assert again == plan and other != plan and [sorted(b) for b in other] == [sorted(b) for b in plan]
    # a subset keeps the corpus's ids; batch_size_for_max_len scales every bucket
    sub = [i for i in range(len(lengths)) if i % 2 == 0]
    plan2, dropped2 = variable_batch_plan(lengths, sub, 64, 512, 2)
    w2, d2 = ref.variable_buckets([lengths[i] for i in sub], 64, 512, 2)
    assert [sorted(b) for b in plan2] == [sorted(sub[j] for j in b) for b in w2] and dropped2 == [sub[j] for j in d2]
    with pytest.raises(ValueError, match="min_mel_len"):
        variable_batch_plan([63, 64], None, 64, 512)
    with pytest.raises(ValueError, match="powers of 2"):
        variable_batch_plan([64], None, 64, 500)


def test_transcript_vocabulary_and_items(tmp_path):
    from reformer_tts_amd._lib import RttsError
    from reformer_tts_amd.dataset.corpus import TTSCorpus, transcript_items, transcript_vocabulary
    rows = [("clips/a.wav", "HH AH0 L OW1"), ("clips/b.wav", "W ER1 L D"), ("other/c.wav", "AH0 B")]
    with open(tmp_path / "t.csv", "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["audio_path", "text", "phonemes"])
        for path, ph in rows:
            w.writerow([path, "ignored, with a comma", ph])
    vocab = transcript_vocabulary(ph for _, ph in rows)
    assert vocab == {"AH0": 1, "B": 2, "D": 3, "ER1": 4, "HH": 5, "L": 6, "OW1": 7, "W": 8}
    for k, (path, _) in enumerate(rows):
        torch.save(torch.full((1, 8, 3 + k), float(k)), tmp_path / (path.split("/")[1][0] + ".pt"))
    items, names, got_vocab = transcript_items(tmp_path / "t.csv", tmp_path)
    assert names == ["a", "b", "c"] and got_vocab == vocab
    assert [e["phonemes"].tolist() for e in items] == [[5, 1, 6, 7], [8, 4, 6, 3], [1, 2]]
    for k, e in enumerate(items):
        assert e["phonemes"].dtype == torch.int64 and torch.equal(e["spectrogram"], torch.full((3 + k, 8), float(k)))
    with pytest.raises(RttsError, match="GPU only"):                            # the upload is the last step
        TTSCorpus.from_transcript(tmp_path / "t.csv", tmp_path, "cpu")
    with pytest.raises(FileNotFoundError):
        TTSCorpus.from_transcript(tmp_path / "t.csv", tmp_path / "nowhere", "cpu")


def test_load_yaml_keeps_noise_std(tmp_path):
    from reformer_tts_amd.model.config import TTSTrainingConfig, load_yaml
    (tmp_path / "c.yml").write_text("experiment:\n  tts_training:\n    noise_std: 0.25\n    num_visualizations: 3\n    batch_size: 4\n")
    _, cfg = load_yaml(str(tmp_path / "c.yml"))
    assert cfg.noise_std == 0.25 and cfg.batch_size == 4
    (tmp_path / "d.yml").write_text("experiment:\n  tts_training:\n    batch_size: 4\n")
    assert load_yaml(str(tmp_path / "d.yml"))[1].noise_std is None and TTSTrainingConfig().noise_std is None


def test_corpus_refuses_host_tensors_and_bad_offsets():
    from reformer_tts_amd._lib import RttsError
    from reformer_tts_amd.dataset import TTSCorpus
    mel, ph = torch.zeros(8, 10), torch.ones(6, dtype=torch.int32)
    with pytest.raises(RttsError, match="GPU only"):
        TTSCorpus(mel, [0, 4, 10], ph, [0, 2, 6])
    with pytest.raises(RttsError, match="GPU only"):
        TTSCorpus.from_items(ref.toy_items(8), "cpu")
    for fo, po in (([0, 4, 11], [0, 2, 6]), ([0, 6, 4], [0, 2, 6]), ([-1, 4, 10], [0, 2, 6]), ([0, 4, 10], [0, 2, 7]), ([0, 4, 10], [0, 3, 2]),
                   ([0, 4, 10], [0, 6]), ([0], [0])):
        with pytest.raises(ValueError, match="offsets|utterances"):
            TTSCorpus(mel, fo, ph, po)
    with pytest.raises(ValueError, match="f32"):
        TTSCorpus(mel.double(), [0, 4, 10], ph, [0, 2, 6])
    with pytest.raises(ValueError, match="int32"):
        TTSCorpus(mel, [0, 4, 10], ph.long(), [0, 2, 6])
    with pytest.raises(ValueError, match="n_mel"):
        TTSCorpus(torch.zeros(129, 10), [0, 4, 10], ph, [0, 2, 6])


def test_split_is_get_subset_lengths_over_a_seeded_permutation():
    from reformer_tts_amd.dataset.corpus import get_subset_lengths, split_indices
    assert get_subset_lengths(103, (0.8, 0.1, 0.1)) == (83, 10, 10) and get_subset_lengths(7, (1.0, 0.0, 0.0)) == (7, 0, 0)
    train, val, test = split_indices(103, (0.8, 0.1, 0.1), seed=5)
    assert (len(train), len(val), len(test)) == (83, 10, 10) and sorted(train + val + test) == list(range(103))
    assert split_indices(103, (0.8, 0.1, 0.1), seed=5) == (train, val, test) and split_indices(103, (0.8, 0.1, 0.1), seed=6)[0] != train
    with pytest.raises(AssertionError):
        get_subset_lengths(10, (0.5, 0.1, 0.1))
