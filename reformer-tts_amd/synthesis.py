"""Text -> waveform for a batch of utterances: ``ReformerTTS.infer`` then the ragged SqueezeWave vocoder.

The reference synthesises one utterance at a time (``cli.py:185-255``, ``predict_samples`` likewise at ``:150-157``): it
generates a spectrogram, trims it at the stop index (``spectrogram[:, :, :stop.item()]``, ``cli.py:241``) and vocodes
what is left.  ``synthesize`` does that loop for a whole batch with one generation call and one vocoder call: the trimmed
spectrograms are laid end to end as rows (``SqueezeWave.infer_ragged``), so every utterance is vocoded exactly as its own
trimmed ``infer`` call would vocode it, and nothing generated after an utterance's stop reaches its audio.

Batching the texts keeps the reference's batched ``infer`` semantics (``reformer_tts.py:145-221``, what its
``validate_inference`` runs at B = 12): the utterances are zero padded to a common phoneme length and generated together,
and an utterance that stops keeps being generated until the batch ends; the trim discards those frames."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .griffin_lim import GriffinLim, GriffinLimTables  # noqa: F401  (the vocoder that needs no training)
from .squeeze_wave.modules import host_lengths, segment_offsets  # noqa: F401  (re-exported for callers that pack by hand)


def pad_phonemes(phonemes: Sequence[torch.Tensor]) -> torch.Tensor:
    """1-D phoneme id tensors -> (B, max length) int64, zero padded on the right (``dataset/utils.custom_sequence_padder``)."""
    if len(phonemes) == 0:
        raise ValueError("synthesize: no utterances")
    if any(p.dim() != 1 or p.numel() == 0 for p in phonemes):
        raise ValueError("synthesize: every utterance is a non-empty 1-D tensor of phoneme ids")
    out = torch.zeros(len(phonemes), max(int(p.numel()) for p in phonemes), dtype=torch.long)
    for i, p in enumerate(phonemes):
        out[i, :p.numel()] = p.detach().cpu().long()
    return out


def frame_counts(stop, available: int, max_len: Optional[int] = None) -> List[int]:
    """Frames kept per utterance: ``min(stop_i, available)``, the length of ``spectrogram[:, :, :stop_i]`` for a spectrogram
    of ``available`` frames (``cli.py:241``).  ``stop == max_len`` marks an utterance that never stopped: it keeps every
    generated frame.  ``stop``: host ints or a CPU tensor."""
    stops = host_lengths(stop)
    if max_len is not None and any(s > max_len for s in stops):
        raise ValueError(f"stop indices {stops} exceed max_len {max_len}")
    return [min(s, int(available)) for s in stops]


CAPACITY_MIN = 64


def capacity_frames(total: int) -> int:
    """Capacity (mel frames) of the vocoder graph that serves ``total`` frames: ``total`` rounded up to a multiple of
    ``max(64, 2^(floor(log2 total) - 3))``, i.e. eight buckets per octave above 512 frames and multiples of 64 below.
    At most 1/8 of a graph's rows are padding, and totals within a bucket replay one graph."""
    total = int(total)
    if total < 1:
        return CAPACITY_MIN
    q = max(CAPACITY_MIN, 1 << max(0, total.bit_length() - 4))
    return -(-total // q) * q


def vocode_trimmed(vocoder, spectrogram: torch.Tensor, stop, *, sigma: float = 0.6, noise=None, use_graph: bool = False,
                   max_len: Optional[int] = None, denoiser=None, denoiser_strength: float = 0.01) -> List[torch.Tensor]:
    """The step after ``infer``: utterance i of ``spectrogram`` (B, n_mel, L) keeps ``frame_counts(stop, L)[i]`` frames and
    is vocoded as ``vocoder.infer(spectrogram[i:i+1, :, :frames_i])`` would vocode it -> B waveforms of 256 * frames_i
    samples.  ``stop``: (B,) on any device (read back once).  ``noise``: per-utterance draws (``noise_shapes(1, frames_i)``
    each; eager path only).  ``use_graph``: replay the vocoder's ``capture_ragged`` graph for the bucket
    ``capacity_frames(sum frames)`` (captured on first use, then reused).  ``denoiser``: a ``squeeze_wave.denoiser.Denoiser``;
    the packed audio the vocoder wrote goes through its ``forward_packed(strength=denoiser_strength)`` -- one more launch --
    before it is split, so every waveform is what ``denoiser.forward`` makes of the waveform without it (utterances of one or
    two frames are too short to denoise and come back as vocoded)."""
    frames = frame_counts(stop.cpu() if torch.is_tensor(stop) else stop, spectrogram.shape[2], max_len)
    # a vocoder without capture_ragged (griffin_lim.GriffinLim) runs its stage eagerly whatever use_graph says
    if not use_graph or noise is not None or sum(frames) == 0 or not hasattr(vocoder, "capture_ragged"):
        packed, waves = vocoder.infer_ragged(spectrogram, frames, sigma=sigma, noise=noise)
        if denoiser is None or sum(frames) == 0:
            return waves
        packed, _ = denoiser.forward_packed(packed, [256 * n for n in frames], strength=denoiser_strength)
        return vocoder.split_packed(packed, segment_offsets(frames))
    run = vocoder.capture_ragged(len(frames), capacity_frames(sum(frames)), sigma=sigma)
    out, _ = run(spectrogram, frames)
    if denoiser is None:
        out = out.clone()                              # the graph's buffer is overwritten by its next replay
    else:                                              # read from the graph's buffer, written to a tensor of its own
        out, _ = denoiser.forward_packed(out, [256 * n for n in frames], strength=denoiser_strength)
    return vocoder.split_packed(out, segment_offsets(frames))


@torch.no_grad()
def synthesize(tts, vocoder, phonemes: Sequence[torch.Tensor], *, sigma: float = 0.6, use_graph: bool = False,
               denoiser=None, denoiser_strength: float = 0.01, **infer_kwargs) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """Text -> audio for B utterances: ``phonemes`` (list of 1-D id tensors) -> (B waveforms in [-1, 1] of 256 * frames_i
    samples, the spectrogram (B, n_mel, L) of ``tts.infer``, its stop indices (B,)).

    One batched ``tts.infer(padded phonemes, use_graph=use_graph, **infer_kwargs)`` call (its options -- combine_strategy,
    max_len, stop_threshold, ... -- pass through), the per-utterance trim of ``cli.py:241`` (``frame_counts``), and one
    ragged vocoder call.  ``use_graph=True``: the graphed generation loop ("concat") and a ``capture_ragged`` vocoder graph
    per capacity bucket, cached on the vocoder; between the stages the host only reads the B stop indices (they size the
    waveforms), and the offset table goes to the device without waiting for it.  ``denoiser`` / ``denoiser_strength``: see
    ``vocode_trimmed``; the default ``None`` leaves the vocoder's audio as it is."""
    batch = pad_phonemes(phonemes)
    spectrogram, stop = tts.infer(batch, use_graph=use_graph, **infer_kwargs)
    waves = vocode_trimmed(vocoder, spectrogram, stop, sigma=sigma, use_graph=use_graph, max_len=infer_kwargs.get("max_len"),
                           denoiser=denoiser, denoiser_strength=denoiser_strength)
    return waves, spectrogram, stop


@torch.no_grad()
def mel_round_trip_error(vocoder_waves: Sequence[torch.Tensor], spectrogram: torch.Tensor, frames, creator) -> torch.Tensor:
    """How far a vocoded batch is from the spectrograms it was vocoded from: per utterance, the mean of
    |log-mel(audio_i)[:, :frames_i] - spectrogram[i, :, :frames_i]| -> (B,) f32 on the device.

    ``vocoder_waves``: the waveforms ``synthesize`` / ``vocode_trimmed`` returned (256 * frames_i samples each, on the
    device); ``spectrogram`` (B, n_mel, L) and ``frames`` (host ints: ``frame_counts(stop, L)``) what they were vocoded
    from; ``creator``: a ``dataset.audio`` spectrogram module of the format the vocoder was trained on
    (``Tacotron2Spectrogram`` for the reference's configs).  One ragged mel launch over all the waveforms; an utterance needs
    more than n_fft / 2 samples (three frames at the config values)."""
    lens = host_lengths(frames)
    waves = [w.reshape(-1) for w in vocoder_waves]
    if len(waves) != len(lens) or spectrogram.dim() != 3 or spectrogram.shape[0] != len(lens) or spectrogram.shape[1] != creator.n_mels:
        raise ValueError(f"mel_round_trip_error: {len(waves)} waveforms, {len(lens)} frame counts, spectrogram {tuple(spectrogram.shape)}")
    flat = torch.cat([w.to(torch.float32) for w in waves])
    packed, foff = creator.forward_packed(flat, [int(w.numel()) for w in waves])
    errs = []
    for i, n in enumerate(lens):
        if n > foff[i + 1] - foff[i] or n > spectrogram.shape[2]:
            raise ValueError(f"mel_round_trip_error: utterance {i} has {n} frames, its waveform {foff[i + 1] - foff[i]}, the spectrogram "
                             f"{spectrogram.shape[2]}")
        errs.append((packed[:, foff[i]:foff[i] + n] - spectrogram[i, :, :n].to(packed.device, torch.float32)).abs().mean())
    return torch.stack(errs)


@torch.no_grad()
def score_audio(vocoder, creator, audio, lengths=None, sigma: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Waveforms -> how likely each is under the vocoder: per utterance, the negative log-likelihood per sample of its first
    256 * frames_i samples given its own log-mel, frames_i = n_samples_i // 256 -> (per-utterance NLL (B,) f32, the loss of
    the whole batch, 0-dim f32), both on the device (``SqueezeWave.nll_ragged``; the number of the reference's
    ``validation_step``, ``training/wrappers.py:361-368``, per recording).

    ``audio``: a list of 1-D device tensors, or a padded (B, N) device tensor with ``lengths`` (host ints), as
    ``creator.forward`` takes them; ``creator``: a ``dataset.audio`` spectrogram module of the format the vocoder was trained
    on.  One ragged mel launch over all the waveforms (``creator.forward_packed``: n // 256 + 1 frames per utterance, cut to
    n // 256) and one ragged vocoder call; the host reads only the lengths.  An utterance needs more than n_fft / 2 samples."""
    flat, lens = creator._gather(audio, lengths)
    spf = vocoder.samples_per_frame()
    if creator.hop_length != spf or creator.n_mels != vocoder._n_mel():
        raise ValueError(f"score_audio: the spectrogram format (hop {creator.hop_length}, {creator.n_mels} mels) is not the vocoder's "
                         f"({spf} samples per frame, {vocoder._n_mel()} mels)")
    packed, foff = creator.forward_packed(flat, lens)
    frames = [n // spf for n in lens]
    mel = torch.zeros(len(lens), creator.n_mels, max(max(frames), 1), dtype=torch.float32, device=packed.device)
    for i, t in enumerate(frames):
        mel[i, :, :t] = packed[:, foff[i]:foff[i] + t]
    return vocoder.nll_ragged(mel, frames, flat, sample_offsets=segment_offsets(lens)[:-1], sigma=sigma)
