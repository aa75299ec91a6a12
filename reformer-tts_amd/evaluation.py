"""Timing-invariant scores for generated spectrograms and vocoded audio: DTW-aligned mel distance and mel-cepstral distortion.

``Trainer.validate_inference`` reports the reference's ``inference_pred_mse`` (``training/wrappers.py:188-195``), which puts frame
t of the generation against frame t of the truth: a generation that is right but a few frames early, late or at a slightly
different rate scores badly under it.  The scores here first align the two sequences by dynamic time warping and then average
the frame distance along the alignment path (MCD-DTW when the frames are mel cepstra), all in one ``rtts_dtw_align`` call
(``ops.dtw_align``) on the tensors where they lie: nothing is read back.  The metric is not in the reference.

The kernel aligns linearly projected frames and knows nothing about cepstra; ``cepstral_basis`` is the projection that makes its
Euclidean frame distance the usual mel-cepstral distortion in dB."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .squeeze_wave.modules import host_lengths

_BASES: Dict[tuple, torch.Tensor] = {}


def cepstral_basis(n_mel: int, n_coef: int = 13, device=None) -> torch.Tensor:
    """(n_coef, n_mel) f32: rows k = 1..n_coef of the orthonormal DCT-II over the mel channels, sqrt(2 / n_mel) cos(pi k (m + 1/2)
    / n_mel), each scaled by (10 / ln 10) sqrt(2) -- computed in float64 on the host, rounded once.  The k = 0 row (the frame's
    overall level) is left out, as MCD does.  With it, the Euclidean distance of two projected NATURAL-log mel frames (what
    ``spectrogram_to_log_scale`` makes) is (10 / ln 10) sqrt(2 sum_k (c_k - c'_k)^2), the mel-cepstral distortion in dB.
    Cached per (n_mel, n_coef, device)."""
    n_mel, n_coef = int(n_mel), int(n_coef)
    if not 1 <= n_coef < n_mel:
        raise ValueError(f"cepstral_basis: n_coef must be in 1..n_mel - 1 = {n_mel - 1} (got {n_coef})")
    dev = torch.device("cpu" if device is None else device)
    key = (n_mel, n_coef, dev)
    if key not in _BASES:
        k = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
        m = np.arange(n_mel, dtype=np.float64)[None, :]
        rows = math.sqrt(2.0 / n_mel) * np.cos(math.pi * k * (m + 0.5) / n_mel) * (10.0 / math.log(10.0) * math.sqrt(2.0))
        _BASES[key] = torch.from_numpy(rows.astype(np.float32)).to(dev)
    return _BASES[key]


def mel_cepstral_distortion(gen: torch.Tensor, gen_stop: Optional[torch.Tensor], truth: torch.Tensor, lm: int, *, n_coef: int = 13,
                            basis: Optional[torch.Tensor] = None, **where) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """MCD-DTW of B generated log-mel spectrograms against their truths, operands and ``where`` keywords as ``ops.dtw_align``
    takes them (``gen_frames_last``, ``truth_frames_last`` and one truth description).  -> (mcd f64 (B,) = the mean frame
    distortion in dB along utterance b's optimal alignment path (cost / steps), steps int32 (B,) = the path's length, totals f64
    (2,) = [mean_b mcd, sum cost / sum steps]), all on the device.  ``basis``: another projection than
    ``cepstral_basis(n_mel, n_coef)``.  An utterance that cannot be scored (no generated frame, a non-finite value) is NaN, and
    so are the totals."""
    from . import ops
    if basis is None:
        n_mel = gen.shape[1] if where.get("gen_frames_last", True) else gen.shape[2]
        basis = cepstral_basis(n_mel, n_coef, gen.device)
    cost, steps, totals = ops.dtw_align(gen, gen_stop, truth, lm, basis=basis, **where)
    return cost / steps, steps, totals


def dtw_mel_distance(gen: torch.Tensor, gen_stop: Optional[torch.Tensor], truth: torch.Tensor, lm: int,
                     **where) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``mel_cepstral_distortion`` without a projection: the mean Euclidean distance of the log-mel frames themselves along the
    optimal alignment path."""
    from . import ops
    cost, steps, totals = ops.dtw_align(gen, gen_stop, truth, lm, basis=None, **where)
    return cost / steps, steps, totals


@torch.no_grad()
def audio_mcd(vocoder_waves: Sequence[torch.Tensor], spectrogram: torch.Tensor, frames, creator, *, n_coef: int = 13) -> torch.Tensor:
    """How far a vocoded batch is from the spectrograms it was vocoded from, by MCD-DTW: per utterance, the mel-cepstral
    distortion in dB between ``spectrogram[i, :, :frames_i]`` and the log-mel of waveform i, along their optimal alignment path
    -> (B,) f64 on the device.  The DTW sibling of ``synthesis.mel_round_trip_error``, with its arguments: a vocoder that shifts
    or stretches its output by a few frames is not charged for it, which makes the number comparable between Griffin-Lim and
    SqueezeWave.  One ragged mel launch over all the waveforms, one ``rtts_dtw_align`` call on its packed output; an utterance
    needs more than n_fft / 2 samples."""
    lens = host_lengths(frames)
    waves = [w.reshape(-1) for w in vocoder_waves]
    if len(waves) != len(lens) or spectrogram.dim() != 3 or spectrogram.shape[0] != len(lens) or spectrogram.shape[1] != creator.n_mels:
        raise ValueError(f"audio_mcd: {len(waves)} waveforms, {len(lens)} frame counts, spectrogram {tuple(spectrogram.shape)}")
    flat = torch.cat([w.to(torch.float32) for w in waves])
    packed, foff = creator.forward_packed(flat, [int(w.numel()) for w in waves])
    dev = packed.device
    heard = [int(foff[i + 1] - foff[i]) for i in range(len(lens))]
    spec = spectrogram.to(dev, torch.float32)
    mcd, _, _ = mel_cepstral_distortion(spec, torch.tensor(lens, dtype=torch.int64).to(dev), packed, max(heard), n_coef=n_coef,
                                        starts=torch.tensor([int(f) for f in foff[:-1]], dtype=torch.int64).to(dev),
                                        lengths=torch.tensor(heard, dtype=torch.int32).to(dev))
    return mcd
