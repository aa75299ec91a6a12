"""Host restatement of ``rtts_tts_collate`` (include/rtts.h) and of the epoch plans of ``dataset/corpus.py`` -- TEST HELPER, not
the product.  Plain torch / numpy / Python:

* the collate rules, built from ``custom_sequence_padder`` (the reference's collate) and generalised to the kernel's row counts;
* a 32-bit twin of ``rtts_drop_hash`` (numpy uint32 arrays: the arithmetic wraps where the kernel's does);
* ``z`` of the input noise in float64 from the same ``u1``, ``u2``;
* the two plans, the variable one as the reference's bucketing loop walks the samples.

tests/test_tts_corpus_cpu.py holds these against ``custom_sequence_padder`` / ``_fill_shape_buffers`` / the product's plans;
tests/test_tts_corpus_hip.py holds the kernel against them."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

MEL_LENGTHS = (1, 2, 63, 64, 65, 130, 64)          # columns start at odd offsets; one tile, its edges, three tiles
PHONEME_LENGTHS = (1, 7, 129, 3, 64, 65, 2)


def toy_items(n_mel: int, seed: int = 0) -> List[Dict[str, torch.Tensor]]:
    """Seven reference-format items: mel values inside [-11.5, 2], phoneme ids in [1, 76]."""
    g = torch.Generator().manual_seed(1000 * n_mel + seed)
    return [dict(phonemes=torch.randint(1, 77, (lp,), generator=g),
                 spectrogram=(torch.randn(lm, n_mel, generator=g) * 2 - 5).clamp(-11.5, 2.0)) for lm, lp in zip(MEL_LENGTHS, PHONEME_LENGTHS)]


def collate(items: Sequence[Optional[dict]], n_mel: int, LP: Optional[int] = None, R_in: Optional[int] = None, valid_in: Optional[int] = None,
            R: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The kernel's outputs for a batch of items (None = an utterance that does not exist: an all-zero slot).  Defaults give the
    reference's layout: LP, R = the batch's own maxima, R_in = valid_in = R + 1, so ``spectrogram_input`` IS the reference's
    ``spectrogram``.  Everything is cut out of ``custom_sequence_padder`` of the items that exist."""
    from reformer_tts_amd.dataset import custom_sequence_padder
    real = [(b, e) for b, e in enumerate(items) if e is not None]
    B = len(items)
    if real:
        pad = custom_sequence_padder([e for _, e in real])
        lp, lm = pad["phonemes"].shape[1], pad["stop_tokens"].shape[1]
    else:
        lp = lm = 0
    LP, R = lp if LP is None else LP, lm if R is None else R
    R_in = R + 1 if R_in is None else R_in
    valid_in = R_in if valid_in is None else valid_in
    out = dict(phonemes=torch.zeros(B, LP, dtype=torch.int64), spectrogram_input=torch.zeros(B, R_in, n_mel),
               spectrogram_target=torch.zeros(B, R, n_mel), stop_tokens=torch.zeros(B, R), loss_mask=torch.zeros(B, R, n_mel))
    for k, (b, _) in enumerate(real):
        spec = pad["spectrogram"][k]                                   # (1 + lm, n_mel): zero start frame, frames, zeros
        n = min(lp, LP)
        out["phonemes"][b, :n] = pad["phonemes"][k, :n]
        n = min(valid_in, lm + 1, R_in)
        out["spectrogram_input"][b, :n] = spec[:n]
        n = min(lm, R)
        out["spectrogram_target"][b, :n] = spec[1:1 + n]
        out["stop_tokens"][b, :n] = pad["stop_tokens"][k, :n]
        out["loss_mask"][b, :n] = pad["loss_mask"][k, :n]
    return out


# ------------------------------------------------------------------ the counter hash, in 32 bits
def drop_hash32(seed, idx) -> np.ndarray:
    """``rtts_drop_hash`` (csrc/rtts_common.h) on numpy uint32 arrays: every intermediate is a uint32, products wrap."""
    u = np.uint32
    s = np.atleast_1d(np.asarray(seed, dtype=np.uint32)).copy()
    with np.errstate(over="ignore"):
        s ^= s >> u(16); s *= u(0x85ebca6b); s ^= s >> u(13); s *= u(0xc2b2ae35); s ^= s >> u(16)
        x = np.atleast_1d(np.asarray(idx, dtype=np.uint32)) * u(0x9E3779B1) + s
        x ^= x >> u(16); x *= u(0x7feb352d); x ^= (s << u(13)) | (s >> u(19)); x ^= x >> u(15); x *= u(0x846ca68b); x ^= x >> u(16)
    assert x.dtype == np.uint32 and s.dtype == np.uint32
    return x


def uniforms(seed: int, b: int, e) -> tuple:
    """(u1, u2) of elements ``e`` (= f * n_mel + c) of slot b, as float64 (both are exact in f32 too)."""
    s_b = drop_hash32(seed, b)
    e = np.asarray(e, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h1, h2 = drop_hash32(s_b, e * np.uint32(2)), drop_hash32(s_b, e * np.uint32(2) + np.uint32(1))
    return ((h1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24, (h2 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def gauss64(seed: int, b: int, e) -> np.ndarray:
    """z of include/rtts.h in float64: Box-Muller from the same u1, u2; the angle's constant is the kernel's f32 one."""
    u1, u2 = uniforms(seed, b, e)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(float(np.float32(6.2831855)) * u2)


def noise64(seed: int, b: int, frames: int, n_mel: int) -> torch.Tensor:
    """z64 (frames, n_mel) of slot b: what the kernel adds, times noise_std, to input row 1 + f."""
    return torch.from_numpy(gauss64(seed, b, np.arange(frames * n_mel, dtype=np.uint32)).reshape(frames, n_mel))


# ------------------------------------------------------------------ plans
def batch_plan(n_or_indices, batch_size: int, shuffle: bool, drop_last: bool, seed: int, epoch: int) -> List[List[int]]:
    idx = list(range(n_or_indices)) if isinstance(n_or_indices, int) else list(n_or_indices)
    if shuffle:
        g = torch.Generator().manual_seed((seed * 1000003 + epoch) & 0x7FFFFFFFFFFFFFFF)
        idx = [idx[j] for j in torch.randperm(len(idx), generator=g).tolist()]
    out = [idx[i:i + batch_size] for i in range(0, len(idx), batch_size)]
    return out[:-1] if drop_last and out and len(out[-1]) < batch_size else out


def variable_buckets(lengths: Sequence[int], min_mel_len: int = 64, max_mel_len: int = 8192, batch_size_for_max_len: int = 1):
    """The bucketing loop of the reference's ``VariableBatchSizeDataset.__init__`` walked over a list of lengths (sample i has
    ``lengths[i]`` frames and idx i) -> (batches in bucket order, before any shuffle inside a batch; dropped ids)."""
    first_key = int(np.log2(min_mel_len))
    n_buckets = int(np.log2(max_mel_len)) - first_key
    done, waiting, size = {}, {}, {}
    floor = min_mel_len
    for i in range(n_buckets):
        done[first_key + i], waiting[first_key + i] = [], []
        size[first_key + i] = batch_size_for_max_len * 2 ** (n_buckets - i - 1)
        floor *= 2
    assert floor == max_mel_len
    dropped = []
    for idx, sample_len in enumerate(lengths):
        if sample_len >= max_mel_len:
            dropped.append(idx)
            continue
        key = int(np.log2(sample_len))
        waiting[key].append(idx)
        if len(waiting[key]) == size[key]:
            done[key].append(waiting[key])
            waiting[key] = []
    for key in waiting:
        dropped.extend(waiting[key])
    return [batch for key in done for batch in done[key]], dropped
