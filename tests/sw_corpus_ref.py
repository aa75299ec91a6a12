"""numpy / torch restatement of ``rtts_sw_draw_segments`` (include/rtts.h) -- TEST HELPER, not the product.

The draw (which utterance, which hop) with ``oracle.synth.drop_hash``, the numpy twin of the kernels' counter hash, and the
gather written as the header writes it, element by element from the packed buffers.  tests/test_sw_corpus_cpu.py holds both
against ``dataset.utils.vocoder_segment`` (the reference's ``SpectrogramToSpeechDataset.__getitem__``) on the toy corpus below;
tests/test_sw_corpus_hip.py holds the kernel against them."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from oracle.synth import drop_hash

HOP, SEG_FRAMES, C = 256, 4, 128
S = HOP * SEG_FRAMES
# N = S exactly (max_hop 0); max_hop 0 with an unread tail; max_hop 3; one sample short; the shortest the mel launch takes; max_hop 4
LENGTHS = (1024, 1279, 1792, 1023, 513, 2048)
SENTINEL = -7.0e9          # the spare mel columns: never to be seen in an output


def max_hop(n: int, s: int = S, hop: int = HOP) -> int:
    """The largest legal hop of an utterance of n samples; -1 for one shorter than the segment (it is padded, hop 0)."""
    return (n - s) // hop if n >= s else -1


def draw_hop(seed: int, epoch_seed: int, i: int, mh: int) -> int:
    """Multiply-shift of the counter hash onto [0, mh]."""
    h = int(drop_hash((int(seed) + int(epoch_seed)) & 0xFFFFFFFF, np.uint64(int(i) & 0xFFFFFFFF)))
    return (h * (mh + 1)) >> 32


def draw_picks(cursor: int, epoch_seed: int, seed: int, order: Sequence[int], lengths: Sequence[int], batch: int, s: int = S,
               hop: int = HOP) -> List[Tuple[int, int]]:
    """{utterance, hop} of every slot of the batch drawn at ``cursor``; an utterance outside the corpus gives (-1, 0)."""
    picks = []
    for b in range(batch):
        i = cursor + b
        u = int(order[i % len(order)])
        if not 0 <= u < len(lengths):
            picks.append((-1, 0))
            continue
        mh = max_hop(lengths[u], s, hop)
        picks.append((u, draw_hop(seed, epoch_seed, i, mh) if mh >= 0 else 0))
    return picks


def gather(audio: torch.Tensor, so: Sequence[int], mel: torch.Tensor, fo: Sequence[int], picks, seg_frames: int = SEG_FRAMES,
           hop: int = HOP):
    """audio flat f32, mel (n_mel, ld) -> (audio (B, S), mel_rows (B * seg_frames, n_mel)) by the header's two formulas."""
    s, n_mel = seg_frames * hop, mel.shape[0]
    a = torch.zeros(len(picks), s, dtype=torch.float32)
    m = torch.zeros(len(picks) * seg_frames, n_mel, dtype=torch.float32)
    for b, (u, h) in enumerate(picks):
        if u < 0:
            continue
        n, t_u = so[u + 1] - so[u], fo[u + 1] - fo[u]
        j = torch.arange(s)
        ok = h * hop + j < n
        a[b, ok] = audio[so[u] + h * hop + j[ok]]
        for t in range(seg_frames):
            if h + t < t_u:
                m[b * seg_frames + t] = mel[:, fo[u] + h + t]
    return a, m


def toy_corpus(n_mel: int, spare: int = 5):
    """Audio = arange, mel[m, column] = m * 1e5 + column, T_u = N / hop + 1 frames, ``spare`` sentinel columns behind the frames
    -> (audio f32 flat, sample offsets, mel (n_mel, total + spare), frame offsets); all values are exact in f32."""
    so, fo = [0], [0]
    for n in LENGTHS:
        so.append(so[-1] + n)
        fo.append(fo[-1] + n // HOP + 1)
    audio = torch.arange(so[-1], dtype=torch.float32)
    mel = torch.full((n_mel, fo[-1] + spare), SENTINEL, dtype=torch.float32)
    mel[:, :fo[-1]] = torch.arange(n_mel, dtype=torch.float32)[:, None] * 1e5 + torch.arange(fo[-1], dtype=torch.float32)[None, :]
    return audio, so, mel, fo


def all_picks() -> List[Tuple[int, int]]:
    """Every (utterance, legal hop) of the toy corpus."""
    return [(u, h) for u, n in enumerate(LENGTHS) for h in range(max(max_hop(n), 0) + 1)]


def segment_rows(audio_u: torch.Tensor, mel_u: torch.Tensor, h: int, s: int = S, hop: int = HOP):
    """``vocoder_segment`` of one utterance at hop h -> (audio (S,), mel rows (seg_frames, n_mel)): the reference's crop in the
    kernel's row layout."""
    from reformer_tts_amd.dataset.utils import vocoder_segment
    a, m = vocoder_segment(audio_u, mel_u, s, hop, random_hop=h)
    return a, m.t().contiguous()
