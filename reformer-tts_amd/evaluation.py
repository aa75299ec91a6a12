"""Timing-invariant scores for generated spectrograms and vocoded audio: DTW-aligned mel distance and mel-cepstral distortion.

``Trainer.validate_inference`` reports the reference's ``inference_pred_mse`` (``training/wrappers.py:188-195``), which puts frame
t of the generation against frame t of the truth: a generation that is right but a few frames early, late or at a slightly
different rate scores badly under it.  The scores here first align the two sequences by dynamic time warping and then average
the frame distance along the alignment path (MCD-DTW when the frames are mel cepstra), all in one ``rtts_dtw_align`` call
(``ops.dtw_align``) on the tensors where they lie: nothing is read back.  The metric is not in the reference.

The kernel aligns linearly projected frames and knows nothing about cepstra; ``cepstral_basis`` is the projection that makes its
Euclidean frame distance the usual mel-cepstral distortion in dB.

A log-mel distance is nearly blind to pitch, so the second half of the module tracks F0 (``PitchTracker``: YIN on the frame grid of
the mel creators, one ragged ``rtts_pitch_yin`` launch) and compares two contours (``f0_errors``, ``audio_f0_errors``: F0 RMSE in
cents, gross pitch error, voicing decision error and F0 frame error from one ``rtts_f0_compare`` launch)."""
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


class PitchTracker(torch.nn.Module):
    """F0 contours on the frame grid of the mel creators (frame t is centred on sample t * hop_length, T = N // hop_length + 1
    frames), by YIN with a 1024-sample integration window: one ragged ``rtts_pitch_yin`` launch (``ops.pitch_yin``, csrc/pitch.hip)
    for any number of utterances.  A frame whose normalised difference function d' never falls below ``threshold`` between the
    periods of ``f_max`` and ``f_min`` is unvoiced and has f0 = 0; ``aperiodicity`` is d' at the chosen period (its minimum over
    the range in an unvoiced frame).  The lags run to 512 samples, so ``sample_rate / f_min`` must stay below 512."""

    def __init__(self, sample_rate: int = 22050, hop_length: int = 256, f_min: float = 50.0, f_max: float = 500.0, threshold: float = 0.1):
        super().__init__()
        if not sample_rate > 0:
            raise ValueError(f"PitchTracker: sample_rate must be positive (got {sample_rate})")
        if hop_length not in (128, 256, 512):
            raise ValueError(f"PitchTracker: hop_length must be 128, 256 or 512, the hops of the mel creators (got {hop_length})")
        if not 0.0 < f_min <= f_max:
            raise ValueError(f"PitchTracker: f_min and f_max must satisfy 0 < f_min <= f_max (got {f_min}, {f_max})")
        if not 0.0 < threshold < 1.0:
            raise ValueError(f"PitchTracker: threshold must lie strictly between 0 and 1 (got {threshold})")
        self.sample_rate, self.hop_length, self.f_min, self.f_max = sample_rate, int(hop_length), float(f_min), float(f_max)
        self.threshold = float(threshold)
        self.tau_min, self.tau_max = math.ceil(sample_rate / f_max), math.floor(sample_rate / f_min)
        if self.tau_min < 2:
            raise ValueError(f"PitchTracker: f_max = {f_max} Hz is a period of tau_min = {self.tau_min} samples at {sample_rate} Hz; "
                             "tau_min must be at least 2 (lower f_max)")
        if self.tau_max > 511:
            raise ValueError(f"PitchTracker: f_min = {f_min} Hz is a period of tau_max = {self.tau_max} samples at {sample_rate} Hz; "
                             "tau_max must be at most 511 (raise f_min or resample)")
        if self.tau_min > self.tau_max:
            raise ValueError(f"PitchTracker: no whole period lies between f_max = {f_max} Hz and f_min = {f_min} Hz at {sample_rate} Hz "
                             f"(tau_min = {self.tau_min} > tau_max = {self.tau_max})")

    def tables(self, lengths: Sequence[int], device=None):
        """The offset tables of one ragged call (``dataset.audio.MelTables``: the same frame grid as the log-mels)."""
        from .dataset.audio import MelTables
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return MelTables(lengths, self.hop_length, device)

    @torch.no_grad()
    def forward_packed(self, audio: torch.Tensor, lengths: Optional[Sequence[int]] = None, *, tables=None, return_cmnd: bool = False):
        """``audio``: the utterances end to end, a flat f32 device tensor; ``lengths``: their sample counts (host ints), or ``tables``
        from an earlier ``self.tables(lengths)`` -> (f0 (total frames,) f32 in Hz, 0 = unvoiced; aperiodicity (total frames,) f32;
        frame offsets: utterance i owns [offsets[i], offsets[i+1])), and with ``return_cmnd`` also d' (total frames, 513).  One
        launch, stream-ordered."""
        from . import _lib, ops
        if not (torch.is_tensor(audio) and audio.is_cuda):
            raise _lib.RttsError("PitchTracker.forward_packed runs on the GPU only (no CPU fallback for the HIP path)")
        if tables is None:
            if lengths is None:
                raise ValueError("forward_packed needs lengths or tables")
            tables = self.tables(lengths, audio.device)
        total = tables.frame_offsets[-1]
        out = torch.empty(2, total, dtype=torch.float32, device=audio.device)
        cmnd = torch.empty(total, ops.PITCH_MAX_LAG + 1, dtype=torch.float32, device=audio.device) if return_cmnd else None
        ops.pitch_yin(audio, tables.soff_host, tables.foff_host, tables.device_table, len(tables.lengths), self.hop_length, self.tau_min,
                      self.tau_max, self.threshold, float(self.sample_rate), out[0], out[1], cmnd)
        res = (out[0], out[1], list(tables.frame_offsets))
        return res + (cmnd,) if return_cmnd else res

    @torch.no_grad()
    def forward(self, audio, lengths=None):
        """``audio``: a list of 1-D device tensors, or a padded (B, N) device tensor with ``lengths`` (host ints or a tensor)
        -> (f0 (B, T_max) f32 with 0 past an utterance's frames, frames (B,) int64 on the device)."""
        from .dataset.audio import _utterances
        parts, lens = _utterances(audio, lengths, type(self).__name__)
        dev = parts[0].device
        f0, _, foff = self.forward_packed(torch.cat([p.to(dev, torch.float32) for p in parts]), lens)
        frames = [foff[i + 1] - foff[i] for i in range(len(lens))]
        padded = torch.zeros(len(lens), max(frames), dtype=torch.float32, device=dev)
        for i, t in enumerate(frames):
            padded[i, :t] = f0[foff[i]:foff[i + 1]]
        return padded, torch.tensor(frames, dtype=torch.int64).to(dev, non_blocking=True)


def f0_errors_from_counts(table: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The pitch-error figures of a (B + 1, 5) f64 count table as ``rtts_f0_compare`` writes it (rows [n, both, sum of squared
    cents, gross, voicing]; the last row the totals) -> ``rmse_cents`` = sqrt(sum / both), ``gpe`` = gross / both, ``vde`` =
    voicing / n, ``ffe`` = (gross + voicing) / n, each (B,) f64 where the table lives, and ``totals`` (4,) = the same four figures
    of the last row.  A division by zero (no frame voiced in both contours, no frame at all) gives NaN, never infinity."""
    if not (torch.is_tensor(table) and table.dtype == torch.float64 and table.dim() == 2 and table.shape[1] == 5 and table.shape[0] >= 2):
        raise ValueError("f0_errors_from_counts: expected a float64 (B + 1, 5) table")
    nan = torch.full_like(table[:, 0], float("nan"))
    n, both, cents2, gross, voicing = table.unbind(1)

    def ratio(num, den):
        return torch.where(den == 0, nan, num / den)

    figures = torch.stack([torch.sqrt(ratio(cents2, both)), ratio(gross, both), ratio(voicing, n), ratio(gross + voicing, n)])
    return {"rmse_cents": figures[0, :-1], "gpe": figures[1, :-1], "vde": figures[2, :-1], "ffe": figures[3, :-1],
            "totals": figures[:, -1], "counts": table}


def f0_errors(f0_a: torch.Tensor, offsets_a, f0_b: torch.Tensor, offsets_b, gross: float = 0.2) -> Dict[str, torch.Tensor]:
    """The usual pitch errors of contour ``f0_a`` against the reference contour ``f0_b``, both packed as
    ``PitchTracker.forward_packed`` returns them, each with its frame offsets (a host list, or an int64 tensor on the device):
    F0 RMSE in cents and gross pitch error (more than ``gross`` off, relative) over the frames voiced in both, voicing decision
    error and F0 frame error over all compared frames -- utterance by utterance over the first min(T_a, T_b) frames, frame t
    against frame t.  One ``rtts_f0_compare`` launch; see ``f0_errors_from_counts`` for what comes back (device f64 tensors)."""
    from . import ops
    dev = f0_a.device
    tabs = [o if torch.is_tensor(o) else torch.tensor([int(v) for v in o], dtype=torch.int64).to(dev) for o in (offsets_a, offsets_b)]
    return f0_errors_from_counts(ops.f0_compare(f0_a, tabs[0], f0_b, tabs[1], gross))


@torch.no_grad()
def audio_f0_errors(waves_a: Sequence[torch.Tensor], waves_b: Sequence[torch.Tensor], tracker: PitchTracker,
                    gross: float = 0.2) -> Dict[str, torch.Tensor]:
    """``f0_errors`` of two batches of waveforms, ``waves_a`` against the references ``waves_b``: Griffin-Lim against SqueezeWave
    from the same mel, or vocoded against recorded audio.  The sibling of ``audio_mcd``: one ragged YIN launch per side and one
    compare launch.  It is frame-synchronous by design: frame t of one side is compared with frame t of the other, over the
    shorter of the two.  Scoring a generated utterance against a truth of other timing needs the DTW path, which
    ``rtts_dtw_align`` does not export -- out of scope here."""
    if len(waves_a) != len(waves_b) or not len(waves_a):
        raise ValueError(f"audio_f0_errors: {len(waves_a)} waveforms against {len(waves_b)}")
    sides = []
    for waves in (waves_a, waves_b):
        flat = [w.reshape(-1).to(torch.float32) for w in waves]
        f0, _, foff = tracker.forward_packed(torch.cat(flat), [int(w.numel()) for w in flat])
        sides += [f0, foff]
    return f0_errors(*sides, gross=gross)


# ---------------------------------------------------------------------------------------------------------------------------------
# Alignment scores and phoneme durations from the decoder's encoder-decoder attention (not in the reference, whose only
# instrument is ``plot_attention_matrix``).  ``mats`` is what ``ReformerTTS`` collects in eval mode: one (B, T_q, T_k) f32 matrix
# per decoder layer (a list, or stacked (L, B, T_q, T_k)); ``n_frames`` / ``n_keys`` are int32 (B,) device tensors (other integer
# types are converted on the device).  Everything stays on the device.
def _lengths(n_frames: torch.Tensor, n_keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return tuple(t if t.dtype == torch.int32 else t.to(torch.int32) for t in (n_frames.contiguous(), n_keys.contiguous()))


def alignment_scores(mats, n_frames: torch.Tensor, n_keys: torch.Tensor, sigma: float = 0.2) -> Dict[str, torch.Tensor]:
    """The usual scalar views of an attention alignment, per layer and utterance, from one ``rtts_align_stats`` call
    (``ops.alignment_stats``) -> (L, B) f64 tensors: ``focus`` = mean_t max_k a (FastSpeech's focus rate), ``entropy`` = the
    mean row entropy / ln K (0 at K = 1), ``guided`` = the mean row mass weighted by 1 - exp(-(k/K - t/T)^2 / 2 sigma^2)
    (Tachibana et al.'s guided-attention weight: mass off the diagonal), ``monotonic`` = the share of frames whose arg-max key
    does not fall back (NaN at T = 1), ``coverage`` = the share of keys that are some frame's arg-max, ``mass`` = mean_t sum_k a;
    and ``argmax`` int32 (L, B, T_q), ``durations`` int32 (L, B, T_k) = frames per arg-max key, and the raw ``table``
    (L, B + 1, 8).  A slot that cannot be scored is NaN."""
    from . import ops
    n_frames, n_keys = _lengths(n_frames, n_keys)
    argmax, dur, table = ops.alignment_stats(mats, n_frames, n_keys, sigma)
    t, k, total, peak, ent, guided, mono, cover = table[:, :-1].unbind(2)
    log_k = torch.log(k)
    return {"focus": peak / t, "entropy": torch.where(k == 1, torch.zeros_like(ent), ent / t / log_k), "guided": guided / t,
            "monotonic": mono / (t - 1), "coverage": cover / k, "mass": total / t, "argmax": argmax, "durations": dur, "table": table}


def alignment_durations(mats, n_frames: torch.Tensor, n_keys: torch.Tensor, floor: float = 1e-30) -> Dict[str, torch.Tensor]:
    """Phoneme durations by monotonic alignment search (Glow-TTS) over each matrix, one ``rtts_align_mas`` call
    (``ops.alignment_mas``) -> ``durations`` int32 (L, B, T_k) (>= 1 below K, summing to T exactly, 0 beyond), ``path`` int32
    (L, B, T_q) (-1 beyond T), ``log_prob`` (L, B) f64 = the path's mean log-probability Q / T, ``path_mass`` (L, B) f64 = the mean
    attention mass on the path, and the raw ``scores`` (L, B + 1, 2).  An utterance with fewer frames than keys, or one that
    cannot be read, has durations 0 and NaN scores."""
    from . import ops
    n_frames, n_keys = _lengths(n_frames, n_keys)
    dur, path, scores = ops.alignment_mas(mats, n_frames, n_keys, floor)
    t = n_frames.to(torch.float64).unsqueeze(0)
    return {"durations": dur, "path": path, "log_prob": scores[:, :-1, 0] / t, "path_mass": scores[:, :-1, 1] / t, "scores": scores}


def most_focused_layer(scores: Dict[str, torch.Tensor]) -> torch.Tensor:
    """FastSpeech's rule for picking the teacher's alignment: the layer with the highest batch-mean focus rate -> an int64 device
    scalar, no host read.  A layer whose mean is NaN never wins against one that has a number."""
    focus = scores["focus"].mean(dim=1)
    return torch.where(torch.isnan(focus), torch.full_like(focus, float("-inf")), focus).argmax()
