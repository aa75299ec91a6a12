"""A vocoder training corpus that lives on the device, and the sampler that draws training batches from it inside a graph.

The reference trains SqueezeWave from files: ``SpectrogramToSpeechDataset.__getitem__`` (``dataset/interface.py:64-97``) loads
one utterance's audio and spectrogram, crops a random ``audio_segment_length`` window on a hop boundary (or zero-pads a short
utterance), and a ``DataLoader(shuffle=True, drop_last=True)`` stacks ``batch_size`` of them (``training/wrappers.py:395-403``).
Here the whole corpus -- audio laid end to end, f32 or 16-bit PCM, and the packed log-mels ``rtts_mel_spectrogram`` writes --
stays in device memory, and ``rtts_sw_draw_segments`` (csrc/sw_corpus.hip) writes a batch of crops directly in the row layout of
the training step.  Which utterance and which hop is decided by the kernel from a cursor and a seed that live on the device, so a
replayed graph trains on a fresh batch without any host work (``VocoderTrainer.capture_corpus``)."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import torch

from .. import _lib, ops


def _quantize(audio: torch.Tensor) -> torch.Tensor:
    """f32 samples -> the int16 a 16-bit WAV stores (``dataset.audio.write_wav``: round(x * 32768), ties to even, clipped)."""
    return torch.clamp(torch.round(audio.to(torch.float64) * 32768.0), -32768, 32767).to(torch.int16)


class VocoderCorpus:
    """Packed audio (flat f32, or flat int16 read as x / 32768), packed mel f32 (n_mel, total frames) and both offset tables, on
    the device and as host lists.  Utterance u is samples [sample_offsets[u], sample_offsets[u+1]) and mel columns
    [frame_offsets[u], frame_offsets[u+1])."""

    def __init__(self, audio: torch.Tensor, sample_offsets: Sequence[int], mel: torch.Tensor, frame_offsets: Sequence[int], hop: int,
                 names: Optional[List[str]] = None):
        self.sample_offsets, self.frame_offsets = [int(v) for v in sample_offsets], [int(v) for v in frame_offsets]
        n = len(self.sample_offsets) - 1
        if not (audio.is_cuda and mel.is_cuda and audio.device == mel.device):
            raise _lib.RttsError(f"VocoderCorpus lives on the GPU only: audio is on {audio.device}, mel on {mel.device}")
        if audio.dtype not in (torch.float32, torch.int16) or audio.dim() != 1 or mel.dtype != torch.float32 or mel.dim() != 2:
            raise ValueError(f"VocoderCorpus: audio must be flat f32 or int16 and mel f32 (n_mel, frames) (got {audio.dtype} "
                             f"{tuple(audio.shape)}, {mel.dtype} {tuple(mel.shape)})")
        if n < 1 or len(self.frame_offsets) != n + 1 or int(hop) < 1:
            raise ValueError(f"VocoderCorpus: {n} utterances, {len(self.frame_offsets)} frame offsets, hop {hop}")
        for name, off, size in (("sample_offsets", self.sample_offsets, audio.numel()), ("frame_offsets", self.frame_offsets, mel.shape[1])):
            if off[0] < 0 or any(b < a for a, b in zip(off, off[1:])) or off[-1] > size:
                raise ValueError(f"VocoderCorpus: {name} must start at >= 0, not decrease and end within the buffer of {size} (ends at {off[-1]})")
        self.audio, self.mel, self.hop, self.names = audio.contiguous(), mel.contiguous(), int(hop), names
        host = torch.tensor([self.sample_offsets, self.frame_offsets], dtype=torch.int64)
        self.tables = host.to(audio.device)                        # (2, n + 1): what the kernel reads

    def __len__(self) -> int:
        return len(self.sample_offsets) - 1

    @property
    def device(self) -> torch.device:
        return self.audio.device

    @property
    def n_mel(self) -> int:
        return self.mel.shape[0]

    def utterance(self, u: int):
        """-> (audio (N,) f32, mel (n_mel, T)) of utterance u, on the device: what the reference's dataset loads from two files."""
        a = self.audio[self.sample_offsets[u]:self.sample_offsets[u + 1]]
        if a.dtype == torch.int16:
            a = a.to(torch.float32) / 32768.0
        return a, self.mel[:, self.frame_offsets[u]:self.frame_offsets[u + 1]]

    @classmethod
    def from_packed(cls, audio: torch.Tensor, lengths: Sequence[int], mel: torch.Tensor, frame_offsets: Sequence[int], hop: int,
                    names: Optional[List[str]] = None) -> "VocoderCorpus":
        """``audio``: the utterances end to end with their sample counts ``lengths``; ``mel`` and ``frame_offsets``: the output of a
        creator's ``forward_packed`` on that audio (or anything in that layout)."""
        off = [0]
        for n in lengths:
            off.append(off[-1] + int(n))
        return cls(audio, off, mel, frame_offsets, hop, names)

    @classmethod
    def from_waveforms(cls, waveforms: Sequence[torch.Tensor], creator, pcm16: bool = False) -> "VocoderCorpus":
        """1-D waveforms (f32 in [-1, 1), or int16) -> a corpus whose mels are ``creator.forward_packed`` of them, one launch.
        ``pcm16``: keep the audio as 16-bit PCM, half the memory; f32 waveforms are rounded as a WAV file would store them, and
        the mels are computed from the rounded samples, so audio and mel stay a pair."""
        dev = creator._device("VocoderCorpus.from_waveforms")
        parts = list(waveforms)
        if not parts or any(not torch.is_tensor(w) or w.dim() != 1 for w in parts):
            raise ValueError("from_waveforms takes a non-empty list of 1-D tensors")
        flat = torch.cat([w.to(dev) for w in parts])
        if flat.dtype == torch.int16 or pcm16:
            pcm = flat if flat.dtype == torch.int16 else _quantize(flat)
            flat = pcm.to(torch.float32) / 32768.0
        else:
            pcm, flat = None, flat.to(torch.float32)
        lengths = [int(w.numel()) for w in parts]
        mel, foff = creator.forward_packed(flat, lengths)
        return cls.from_packed(pcm if pcm16 else flat, lengths, mel, foff, creator.hop_length)

    @classmethod
    def from_directory(cls, audio_dir, creator, resample: bool = False, pcm16: bool = False, max_batch_samples: int = 1 << 24,
                       suffix: str = ".wav") -> "VocoderCorpus":
        """Every ``*.wav`` of ``audio_dir`` -> a corpus, through the launches of ``dataset.audio.preprocess_directory`` (ragged
        batches of at most ``max_batch_samples`` samples, ``resample`` = the reference's ``resample_wav`` step on the GPU in front)
        but without writing a file: each batch's audio and mels stay on the device.  ``names`` lists the files in corpus order.
        ``pcm16``: as ``from_waveforms``; with ``resample`` the resampled audio is rounded to 16 bits before its mels are made,
        which is what the reference's resampled WAV files hold."""
        from ..dataset import audio as A
        dev = creator._device("VocoderCorpus.from_directory")
        files = sorted(f for f in os.listdir(audio_dir) if f.endswith(suffix))
        if not files:
            raise ValueError(f"{audio_dir}: no *{suffix} files")
        info = {name: A.pcm_info(os.path.join(audio_dir, name)) for name in files}
        frames = {name: info[name][0] for name in files}
        names, lengths, audios, mels = [], [], [], []
        for (rate, channels), order in A.group_by_format(info).items():
            if not resample:                                       # as preprocess_directory(resample=False): mono files at the rate
                if channels != 1:
                    raise ValueError(f"{os.path.join(audio_dir, order[0])}: expected 16-bit PCM mono, got {channels} channels "
                                     "(resample=True takes channel 0 of any file)")
                creator._check_rate(rate, os.path.join(audio_dir, order[0]))
            resampler = None if rate == creator.sample_rate else A.Resample(rate, creator.sample_rate).to(dev)
            for batch in A._batches(order, frames, max_batch_samples):
                pcm = [A.read_pcm(os.path.join(audio_dir, name))[0] for name in batch]
                if resampler is None:
                    raw = torch.cat([p[:, 0] for p in pcm]).to(dev)
                    lens, stored = [p.shape[0] for p in pcm], raw
                    flat = raw.to(torch.float32) / 32768.0
                    if not pcm16:
                        stored = flat
                else:
                    raw = torch.cat([p.reshape(-1) for p in pcm]).to(dev)
                    flat, ooff = resampler.forward_packed(raw, [p.shape[0] for p in pcm], channels=channels)
                    lens, stored = [ooff[j + 1] - ooff[j] for j in range(len(batch))], flat
                    if pcm16:
                        stored = _quantize(flat)
                        flat = stored.to(torch.float32) / 32768.0
                short = [(name, n) for name, n in zip(batch, lens) if n <= creator.n_fft // 2]
                if short:
                    raise ValueError(f"{os.path.join(audio_dir, short[0][0])}: {short[0][1]} samples at {creator.sample_rate} Hz; reflect "
                                     f"padding needs more than n_fft / 2 = {creator.n_fft // 2}")
                mel, _ = creator.forward_packed(flat, lens)
                names += batch
                lengths += lens
                audios.append(stored)
                mels.append(mel)
        foff = [0]
        for n in lengths:
            foff.append(foff[-1] + n // creator.hop_length + 1)
        return cls.from_packed(torch.cat(audios), lengths, torch.cat(mels, dim=1), foff, creator.hop_length, names)


class SegmentSampler:
    """The reference's ``DataLoader(dataset, batch_size, shuffle=True, drop_last=True)`` over a ``VocoderCorpus`` (or the subset
    ``indices`` of it, as ``random_split`` gives a train and a validation part), with everything a draw needs on the device:
    ``order`` (int32, the epoch's permutation of the subset), ``state`` (int64 {cursor, epoch_seed}) and the output buffers.
    ``draw`` is one ``rtts_sw_draw_segments`` launch and one device add on the cursor; both can be captured into a graph, and
    ``start_epoch`` only writes into those buffers, so captured graphs stay valid over epochs."""

    def __init__(self, corpus: VocoderCorpus, batch: int, audio_segment_length: int, indices: Optional[Sequence[int]] = None,
                 seed: int = 0, n_audio_channels: int = 128):
        self.corpus, self.batch, self.seed, self.n_audio_channels = corpus, int(batch), int(seed), int(n_audio_channels)
        self.segment = int(audio_segment_length)
        if self.batch < 1 or self.segment < 1 or self.segment % corpus.hop or self.segment % self.n_audio_channels:
            raise ValueError(f"SegmentSampler: batch {batch}, audio_segment_length {audio_segment_length} must be positive, the latter a "
                             f"multiple of the hop {corpus.hop} and of n_audio_channels {n_audio_channels}")
        self.mel_len = self.segment // corpus.hop
        self.indices = list(range(len(corpus))) if indices is None else [int(i) for i in indices]
        if not self.indices or min(self.indices) < 0 or max(self.indices) >= len(corpus):
            raise ValueError(f"SegmentSampler: indices must be a non-empty subset of the corpus's {len(corpus)} utterances")
        self.steps_per_epoch = len(self.indices) // self.batch                     # drop_last=True
        dev = corpus.device
        self.order = torch.tensor(self.indices, dtype=torch.int32, device=dev)
        self.state = torch.zeros(2, dtype=torch.int64, device=dev)
        self.audio_rows = torch.zeros(self.batch * self.segment // self.n_audio_channels, self.n_audio_channels, device=dev)
        self.mel_rows = torch.zeros(self.batch * self.mel_len, corpus.n_mel, device=dev)
        self.picks = torch.zeros(self.batch, 2, dtype=torch.int32, device=dev)
        self.epoch = None

    def start_epoch(self, epoch: int) -> None:
        """A new shuffle of the subset (``torch.randperm`` from a CPU generator seeded by (seed, epoch)) into ``order``, cursor 0,
        epoch_seed = epoch: stream-ordered copies into the buffers the kernel reads."""
        g = torch.Generator().manual_seed((self.seed * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
        perm = torch.tensor(self.indices, dtype=torch.int32)[torch.randperm(len(self.indices), generator=g)]
        self.order.copy_(perm)
        self.state.copy_(torch.tensor([0, int(epoch)], dtype=torch.int64))
        self.epoch = int(epoch)

    def draw(self, picks: Optional[torch.Tensor] = None):
        """-> (mel_rows (batch * mel_len, n_mel), audio_rows (batch * S / C, C), picks (batch, 2) = {utterance, hop}): the
        sampler's own buffers, overwritten by the next draw.  Without ``picks`` the batch is drawn at the cursor, which then
        advances by ``batch`` (a separate add after the launch: the kernel writes no word that its workgroups read).  With
        ``picks`` (int32 (batch, 2) on the device) exactly those crops are written and the cursor stays."""
        c = self.corpus
        ops.sw_draw_segments(c.audio, c.tables[0], c.mel, c.tables[1], self.order, self.state, self.seed, picks, self.batch, self.mel_len,
                             c.hop, self.n_audio_channels, self.audio_rows, self.mel_rows, self.picks)
        if picks is None:
            self.state[0:1].add_(self.batch)
        return self.mel_rows, self.audio_rows, self.picks

    def batch_dict(self) -> Dict[str, torch.Tensor]:
        """The last draw in the reference's batch format: {'spectrogram': (B, n_mel, Lm), 'audio': (B, S)}, views of the buffers."""
        return {"spectrogram": self.mel_rows.view(self.batch, self.mel_len, -1).permute(0, 2, 1),
                "audio": self.audio_rows.view(self.batch, self.segment)}
