"""The restatement of ``rtts_sw_draw_segments`` in tests/sw_corpus_ref.py against the reference's own crop
(``dataset.utils.vocoder_segment`` = ``SpectrogramToSpeechDataset.__getitem__``) and the properties of its hop draw.  No GPU."""
import numpy as np
import pytest
import torch

import sw_corpus_ref as ref


@pytest.mark.parametrize("n_mel", [80, 8])
def test_gather_is_vocoder_segment_for_every_utterance_and_hop(n_mel):
    audio, so, mel, fo = ref.toy_corpus(n_mel)
    picks = ref.all_picks()
    assert [sum(1 for u, _ in picks if u == k) for k in range(len(ref.LENGTHS))] == [1, 1, 4, 1, 1, 5]
    a, m = ref.gather(audio, so, mel, fo, picks)
    assert not (a == ref.SENTINEL).any() and not (m == ref.SENTINEL).any()
    for b, (u, h) in enumerate(picks):
        wa, wm = ref.segment_rows(audio[so[u]:so[u + 1]], mel[:, fo[u]:fo[u + 1]], h)
        assert torch.equal(a[b], wa), (u, h)
        assert torch.equal(m[b * ref.SEG_FRAMES:(b + 1) * ref.SEG_FRAMES], wm), (u, h)
    # the short utterances end in zeros, audio and mel alike (constant padding, not log(clip))
    b = picks.index((4, 0))
    assert (a[b, 513:] == 0).all() and a[b, 512] != 0
    assert (m[b * ref.SEG_FRAMES + 3] == 0).all() and (m[b * ref.SEG_FRAMES + 2, 1:] != 0).all()


def test_an_illegal_hop_is_refused_by_the_reference_crop():
    audio, so, mel, fo = ref.toy_corpus(8)
    with pytest.raises(ValueError, match="random_hop"):
        ref.segment_rows(audio[so[2]:so[3]], mel[:, fo[2]:fo[3]], 4)


def test_hop_draw_covers_its_range_and_stays_in_it():
    hops = [ref.draw_hop(11, 3, i, 3) for i in range(256)]
    assert set(hops) == {0, 1, 2, 3}
    assert all(ref.draw_hop(11, 3, i, 0) == 0 for i in range(256))
    big = [ref.draw_hop(0xFFFFFFFF, 7, i, 1 << 20) for i in range(4096)]
    assert min(big) >= 0 and max(big) <= 1 << 20 and len(set(big)) > 4000
    # the seed and the epoch seed enter as one 32-bit sum
    assert ref.draw_hop(5, 6, 9, 1000) == ref.draw_hop(11, 0, 9, 1000) == ref.draw_hop(0xFFFFFFFF, 12, 9, 1000)


def test_draw_picks_wraps_the_order_and_marks_strangers():
    order = [2, 5, 0, 9, 4, 1]
    picks = ref.draw_picks(4, 1, 3, order, ref.LENGTHS, 4)
    assert [u for u, _ in picks] == [4, 1, 2, 5]                  # i = 4, 5, then 6 and 7 wrap to order[0], order[1]
    assert picks[0][1] == 0 and picks[1][1] == 0                  # shorter than S / max_hop 0
    assert picks[2][1] == ref.draw_hop(3, 1, 6, 3) and picks[3][1] == ref.draw_hop(3, 1, 7, 4)
    assert ref.draw_picks(3, 1, 3, order, ref.LENGTHS, 1) == [(-1, 0)]
    other = ref.draw_picks(4, 2, 3, order, ref.LENGTHS, 4)
    assert [u for u, _ in other] == [u for u, _ in picks]
    # over many counters the epoch seed changes the hops
    a = [ref.draw_hop(3, 1, i, 4) for i in range(64)]
    b = [ref.draw_hop(3, 2, i, 4) for i in range(64)]
    assert a != b


def test_hash_twin_is_32_bit():
    h = ref.drop_hash(123, np.arange(1000, dtype=np.uint64))
    assert int(h.max()) < 1 << 32
