"""Host logic of batched synthesis without a device: the per-utterance trim, the segment offsets, the capacity buckets of
the vocoder graphs and the packing of per-utterance noise into rows."""
import pytest
import torch

from reformer_tts_amd import synthesis
from reformer_tts_amd.dataset.utils import custom_sequence_padder
from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
from reformer_tts_amd.squeeze_wave.modules import segment_offsets


def test_frame_counts_are_the_reference_slice():
    """cli.py:241 keeps spectrogram[:, :, :stop]: a stop past the generated frames and a never-stopped utterance (stop ==
    max_len) keep every generated frame."""
    spec = torch.zeros(4, 2, 50)
    stop = torch.tensor([7, 23, 55, 60])
    want = [spec[i:i + 1, :, :int(s)].shape[2] for i, s in enumerate(stop)]
    assert synthesis.frame_counts(stop, 50, max_len=60) == want == [7, 23, 50, 50]
    assert synthesis.frame_counts([1, 50], 50) == [1, 50]
    with pytest.raises(ValueError):
        synthesis.frame_counts([61], 50, max_len=60)
    with pytest.raises(ValueError):
        synthesis.frame_counts([-1], 50)


def test_segment_offsets_and_capacity_buckets():
    assert segment_offsets([3, 0, 5]) == [0, 3, 3, 8]
    assert segment_offsets(torch.tensor([2, 2])) == [0, 2, 4]
    cap = synthesis.capacity_frames
    assert [cap(t) for t in (0, 1, 64, 65, 512, 513, 1000, 4000, 4096, 4097)] == [64, 64, 64, 128, 512, 576, 1024, 4096, 4096, 4608]
    prev = 0
    for t in range(1, 20000, 7):
        c = cap(t)
        assert t <= c and (c - t) * 8 <= max(c, 512)            # at most 1/8 padding above 512 frames
        assert c >= prev                                         # monotone: nearby totals share a bucket
        prev = c
    assert len({cap(t) for t in range(3841, 4097)}) == 1


@pytest.mark.parametrize("lengths,capacity", [([3, 0, 5], None), ([1, 2, 3], 10), ([7], 7)])
def test_noise_packs_into_rows_and_back(lengths, capacity):
    """Draw k of utterance i lands in rows [up * moff[i], up * moff[i+1]) of packed draw k in the row layout infer makes
    of a (1, C, L) draw; unpacking gives back exactly the noise_shapes(1, n) tensors."""
    sw = SqueezeWave(4, 16, 80, 2, 4, WNConfig(2, 32, 3, 16))
    up = 16
    g = torch.Generator().manual_seed(1)
    noise = [[torch.randn(s, generator=g) for s in sw.noise_shapes(1, n)] for n in lengths]
    packed = sw.pack_noise(noise, lengths, capacity)
    total, cap = sum(lengths), capacity or sum(lengths)
    assert [tuple(d.shape) for d in packed] == [(up * cap, s[1]) for s in sw.noise_shapes(1, 1)]
    moff = segment_offsets(lengths)
    for k, d in enumerate(packed):
        for i, z in enumerate(noise):
            assert torch.equal(d[up * moff[i]:up * moff[i + 1]], z[k][0].t())
        assert not d[up * total:].any()
    back = sw.unpack_noise(packed, lengths)
    for z, b, n in zip(noise, back, lengths):
        assert [tuple(t.shape) for t in b] == sw.noise_shapes(1, n)
        assert all(torch.equal(x, y) for x, y in zip(z, b))
    with pytest.raises(ValueError):
        sw.pack_noise(noise[:1], lengths[:1] and [lengths[0] + 1])
    if capacity:
        with pytest.raises(ValueError):
            sw.pack_noise(noise, lengths, total - 1)


def test_pad_phonemes_matches_the_training_padder():
    ph = [torch.tensor([3, 1, 4]), torch.tensor([1, 5, 9, 2, 6]), torch.tensor([5])]
    want = custom_sequence_padder([{"phonemes": p, "spectrogram": torch.zeros(2, 4)} for p in ph])["phonemes"]
    assert torch.equal(synthesis.pad_phonemes(ph), want)
    with pytest.raises(ValueError):
        synthesis.pad_phonemes([])


def test_ragged_vocoder_refuses_the_cpu():
    from reformer_tts_amd import _lib
    sw = SqueezeWave(4, 16, 80, 2, 4, WNConfig(2, 32, 3, 16))
    with pytest.raises(_lib.RttsError, match="GPU only"):
        sw.infer_ragged(torch.zeros(1, 80, 4), [4])
