"""A text-to-spectrogram training corpus that lives on the device, the launch that collates batches from it, and the epoch plans.

The reference trains ReformerTTS from files: ``TextToSpectrogramDataset.__getitem__`` (``dataset/interface.py:16-43``) loads one
utterance's phoneme ids and log-mel, ``custom_sequence_padder`` (``dataset/utils.py:5-42``) pads a list of them into four host
tensors, and a ``DataLoader`` (``training/wrappers.py:213-232``) copies those to the GPU.  Here the whole corpus -- the packed
log-mels ``rtts_mel_spectrogram`` writes, (n_mel, total frames), and the phoneme ids laid end to end -- stays in device memory,
and ``rtts_tts_collate`` (csrc/tts_corpus.hip) writes a batch in one launch, either in the reference's collate layout
(``collate``) or into the padded buffers a captured training step reads (``fill``).  Which utterances make a batch is host
integer work on the length tables (``batch_plan``, ``variable_batch_plan``): an epoch's plan is uploaded once
(``Trainer.fit_corpus``).

Input noise (``noise_std``): Gaussian noise on the teacher-forcing input frames, from the counter hash of the dropout sites.
Deliberately NOT the reference as written: its ``noise_std := ... is not None`` (``wrappers.py:45``) binds ``std = True``, and its
in-place write (``wrappers.py:56``) also lands on the target and on the padding.  Here the valid input frames get
``noise_std * z`` and the start frame, the padding and the target stay untouched."""
from __future__ import annotations

import csv
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from .. import _lib, ops


def _offsets(lengths: Sequence[int]) -> List[int]:
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return off


def get_subset_lengths(length: int, split_percentages: Sequence[float]) -> Tuple[int, int, int]:
    """``dataset/utils.py:45-57``: (train, val, test) sizes of a split of ``length`` items."""
    assert sum(split_percentages) == 1, "split_percentages have to sum up to 1"
    assert len(split_percentages) == 3, "expected percentages for exactly 3 subsets"
    test_l = int(length * split_percentages[2]) if split_percentages[2] != 0 else 0
    val_l = int(length * split_percentages[1]) if split_percentages[1] != 0 else 0
    return length - test_l - val_l, val_l, test_l


class TTSCorpus:
    """Packed mel f32 (n_mel, total frames) and packed int32 phoneme ids with both offset tables, on the device and as host lists.
    Utterance u is mel columns [frame_offsets[u], frame_offsets[u+1]) and ids [phoneme_offsets[u], phoneme_offsets[u+1])."""

    def __init__(self, mel: torch.Tensor, frame_offsets: Sequence[int], phoneme_ids: torch.Tensor, phoneme_offsets: Sequence[int],
                 names: Optional[List[str]] = None, phoneme_to_idx: Optional[Dict[str, int]] = None):
        self.frame_offsets, self.phoneme_offsets = [int(v) for v in frame_offsets], [int(v) for v in phoneme_offsets]
        n = len(self.frame_offsets) - 1
        if not (torch.is_tensor(mel) and torch.is_tensor(phoneme_ids)):
            raise ValueError("TTSCorpus: mel and phoneme_ids must be tensors")
        if mel.dtype != torch.float32 or mel.dim() != 2 or phoneme_ids.dtype != torch.int32 or phoneme_ids.dim() != 1:
            raise ValueError(f"TTSCorpus: mel must be f32 (n_mel, frames) and phoneme_ids flat int32 (got {mel.dtype} {tuple(mel.shape)}, "
                             f"{phoneme_ids.dtype} {tuple(phoneme_ids.shape)})")
        if n < 1 or len(self.phoneme_offsets) != n + 1 or not 1 <= mel.shape[0] <= 128:
            raise ValueError(f"TTSCorpus: {n} utterances, {len(self.phoneme_offsets)} phoneme offsets, n_mel {mel.shape[0]} (1..128)")
        for name, off, size in (("frame_offsets", self.frame_offsets, mel.shape[1]), ("phoneme_offsets", self.phoneme_offsets, phoneme_ids.numel())):
            if off[0] < 0 or any(b < a for a, b in zip(off, off[1:])) or off[-1] > size:
                raise ValueError(f"TTSCorpus: {name} must start at >= 0, not decrease and end within the buffer of {size} (ends at {off[-1]})")
        if not (mel.is_cuda and phoneme_ids.is_cuda and mel.device == phoneme_ids.device):
            raise _lib.RttsError(f"TTSCorpus lives on the GPU only: mel is on {mel.device}, phoneme_ids on "
                                 f"{phoneme_ids.device}")
        self.frame_lengths = [b - a for a, b in zip(self.frame_offsets, self.frame_offsets[1:])]
        self.phoneme_lengths = [b - a for a, b in zip(self.phoneme_offsets, self.phoneme_offsets[1:])]
        if min(self.frame_lengths) < 1:
            raise ValueError("TTSCorpus: empty spectrogram")                # custom_sequence_padder's one-hot would index frame -1
        self.mel, self.phoneme_ids, self.names, self.phoneme_to_idx = mel.contiguous(), phoneme_ids.contiguous(), names, phoneme_to_idx
        host = torch.tensor([self.frame_offsets, self.phoneme_offsets], dtype=torch.int64)
        self.tables = host.to(mel.device)                          # (2, n + 1): what the kernel reads

    def __len__(self) -> int:
        return len(self.frame_lengths)

    @property
    def device(self) -> torch.device:
        return self.mel.device

    @property
    def n_mel(self) -> int:
        return self.mel.shape[0]

    def item(self, u: int) -> Dict[str, torch.Tensor]:
        """The reference's dataset item of utterance u, on the device: {"phonemes": int64 (len,), "spectrogram": (len, n_mel)}."""
        return {"phonemes": self.phoneme_ids[self.phoneme_offsets[u]:self.phoneme_offsets[u + 1]].long(),
                "spectrogram": self.mel[:, self.frame_offsets[u]:self.frame_offsets[u + 1]].t()}

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_items(cls, items, device, names: Optional[List[str]] = None, phoneme_to_idx: Optional[Dict[str, int]] = None) -> "TTSCorpus":
        """A list of the reference's dataset items {"phonemes": LongTensor(len), "spectrogram": (len, n_mels)} -> one upload."""
        items = list(items)
        if not items:
            raise ValueError("TTSCorpus.from_items: no items")
        mel = torch.cat([e["spectrogram"].to(torch.float32).t() for e in items], dim=1).contiguous()
        ph = torch.cat([e["phonemes"].reshape(-1) for e in items]).to(torch.int32)
        return cls(mel.to(device), _offsets(e["spectrogram"].shape[0] for e in items), ph.to(device),
                   _offsets(e["phonemes"].numel() for e in items), names, phoneme_to_idx)

    @classmethod
    def from_waveforms(cls, waveforms: Sequence[torch.Tensor], phoneme_ids: Sequence, creator) -> "TTSCorpus":
        """1-D f32 waveforms and their phoneme id lists -> a corpus whose mels are ``creator.forward_packed`` of the waveforms,
        one launch; the mels never leave the device."""
        dev = creator._device("TTSCorpus.from_waveforms")
        parts = list(waveforms)
        if not parts or any(not torch.is_tensor(w) or w.dim() != 1 for w in parts) or len(phoneme_ids) != len(parts):
            raise ValueError("from_waveforms takes a non-empty list of 1-D tensors and as many phoneme id lists")
        flat = torch.cat([w.to(dev) for w in parts]).to(torch.float32)
        mel, foff = creator.forward_packed(flat, [int(w.numel()) for w in parts])
        return cls.from_vocoder_corpus(_Packed(mel, foff), phoneme_ids)

    @classmethod
    def from_vocoder_corpus(cls, vc, phoneme_ids: Sequence, phoneme_to_idx: Optional[Dict[str, int]] = None) -> "TTSCorpus":
        """Shares ``vc.mel`` and ``vc.frame_offsets`` of a ``squeeze_wave.VocoderCorpus``: one upload serves both trainers."""
        ids = [torch.as_tensor(p, dtype=torch.int64).reshape(-1) for p in phoneme_ids]
        if len(ids) != len(vc.frame_offsets) - 1:
            raise ValueError(f"from_vocoder_corpus: {len(ids)} phoneme id lists for {len(vc.frame_offsets) - 1} utterances")
        flat = torch.cat(ids).to(torch.int32).to(vc.mel.device)
        return cls(vc.mel, vc.frame_offsets, flat, _offsets(p.numel() for p in ids), getattr(vc, "names", None), phoneme_to_idx)

    @classmethod
    def from_transcript(cls, csv_path, mel_directory, device) -> "TTSCorpus":
        """``TextToSpectrogramDataset.__init__/__getitem__`` (``dataset/interface.py:16-43``): a CSV with columns ``phonemes``
        (space separated) and ``audio_path``; the vocabulary is sorted(set of phonemes) -> i + 1; the mel of a row is
        ``mel_directory/<audio stem>.pt``, stored (1, n_mels, T)."""
        items, names, phoneme_to_idx = transcript_items(csv_path, mel_directory)
        return cls.from_items(items, device, names, phoneme_to_idx)

    # ------------------------------------------------------------------ batches
    def _shape(self, ids: Sequence[int]) -> Tuple[int, int]:
        """(lp, lm) of a batch of host utterance ids: its own maxima."""
        n = len(self)
        if not ids or min(ids) < 0 or max(ids) >= n:
            raise IndexError(f"TTSCorpus: batch ids must be a non-empty list within the corpus's {n} utterances")
        return max(self.phoneme_lengths[i] for i in ids), max(self.frame_lengths[i] for i in ids)

    def _launch(self, ids: torch.Tensor, lm: int, noise_std, seed, **out) -> None:
        ops.tts_collate(self.mel, self.tables[0], self.phoneme_ids, self.tables[1], ids, lm, noise_std=float(noise_std or 0.0), seed=seed, **out)

    def collate(self, ids: Sequence[int], noise_std: Optional[float] = None, seed: int = 0) -> Dict[str, torch.Tensor]:
        """``custom_sequence_padder`` of the utterances ``ids`` (host ints), on the device, one launch: phonemes (B, Lp) int64,
        spectrogram (B, 1 + Lm, n_mel) behind a zero start frame, stop_tokens (B, Lm), loss_mask (B, Lm, n_mel); Lp, Lm are the
        batch's own maxima.  ``noise_std``: Gaussian noise on the valid frames of ``spectrogram`` (module docstring); a training
        step that slices its target out of this array trains against the noisy frames, as the reference's does -- ``frames`` keeps
        input and target apart."""
        ids = [int(i) for i in ids]
        lp, lm = self._shape(ids)
        dev, b, nm = self.device, len(ids), self.n_mel
        out = dict(phonemes=torch.empty(b, max(lp, 1), dtype=torch.int64, device=dev), spectrogram=torch.empty(b, lm + 1, nm, device=dev),
                   stop_tokens=torch.empty(b, lm, device=dev), loss_mask=torch.empty(b, lm, nm, device=dev))
        self._launch(torch.tensor(ids, dtype=torch.int32).to(dev), lm, noise_std, seed, phonemes=out["phonemes"], spectrogram_input=out["spectrogram"],
                     valid_in=lm + 1, stop_tokens=out["stop_tokens"], loss_mask=out["loss_mask"])
        if lp == 0:
            out["phonemes"] = out["phonemes"][:, :0]
        return out

    def frames(self, ids: Sequence[int], noise_std: Optional[float] = None, seed: int = 0) -> Dict[str, torch.Tensor]:
        """The batch ``ids`` as the training step's own pair of arrays, unpadded: phonemes (B, Lp), spectrogram_input (B, Lm, n_mel)
        = start frame + frames [0, Lm - 1) with the noise, spectrogram_target (B, Lm, n_mel) clean, stop_tokens, loss_mask: what an
        eager step with input noise trains on (``Trainer.forward_loss`` takes either form)."""
        ids = [int(i) for i in ids]
        lp, lm = self._shape(ids)
        dev, b, nm = self.device, len(ids), self.n_mel
        out = dict(phonemes=torch.empty(b, max(lp, 1), dtype=torch.int64, device=dev), spectrogram_input=torch.empty(b, lm, nm, device=dev),
                   spectrogram_target=torch.empty(b, lm, nm, device=dev), stop_tokens=torch.empty(b, lm, device=dev),
                   loss_mask=torch.empty(b, lm, nm, device=dev))
        self._launch(torch.tensor(ids, dtype=torch.int32).to(dev), lm, noise_std, seed, valid_in=lm, **out)
        if lp == 0:
            out["phonemes"] = out["phonemes"][:, :0]
        return out

    def fill(self, bufs: Dict[str, torch.Tensor], ids: Union[Sequence[int], torch.Tensor], noise_std: Optional[float] = None, seed: int = 0,
             lm: Optional[int] = None) -> None:
        """The buffers of a captured step's shape (``Trainer._shape_graph``: phonemes, spectrogram_input, spectrogram_target,
        stop_tokens, loss_mask, valid_len) filled with the batch ``ids`` in one launch, zero padding included: what the host path
        writes with ``custom_sequence_padder`` + a copy + ``_fill_shape_buffers``.  ``ids``: host ints (uploaded here), or an int32
        device tensor -- a slice of an uploaded plan -- with ``lm``, the batch's longest utterance in frames, from the host."""
        if torch.is_tensor(ids):
            if lm is None:
                raise ValueError("TTSCorpus.fill: device ids need lm, the batch's longest utterance, from the host length table")
            dev_ids = ids
        else:
            ids = [int(i) for i in ids]
            lm = self._shape(ids)[1]
            dev_ids = torch.tensor(ids, dtype=torch.int32).to(self.device)
        self._launch(dev_ids, int(lm), noise_std, seed, phonemes=bufs["phonemes"], spectrogram_input=bufs["spectrogram_input"], valid_in=int(lm),
                     spectrogram_target=bufs["spectrogram_target"], stop_tokens=bufs["stop_tokens"], loss_mask=bufs["loss_mask"],
                     valid_len=bufs["valid_len"])

    def split(self, split_percentages: Sequence[float], seed: int = 42) -> Tuple[List[int], List[int], List[int]]:
        """``get_subset_lengths`` (``dataset/utils.py:45-57``) over a seeded permutation of the corpus -> (train, val, test) ids."""
        return split_indices(len(self), split_percentages, seed)


class _Packed:
    """(mel, frame_offsets) in the shape ``from_vocoder_corpus`` reads."""

    def __init__(self, mel, frame_offsets):
        self.mel, self.frame_offsets = mel, list(frame_offsets)


def transcript_vocabulary(phoneme_strings) -> Dict[str, int]:
    """``TextToSpectrogramDataset.__init__`` (``interface.py:19-20``): sorted(set of phonemes) -> i + 1 (0 is the padding)."""
    phonemes = {p for s in phoneme_strings for p in s.split()}
    return {p: i + 1 for i, p in enumerate(sorted(phonemes))}


def transcript_items(csv_path, mel_directory):
    """The host half of ``TTSCorpus.from_transcript`` -> (the reference's dataset items in CSV order, audio stems, vocabulary)."""
    with open(csv_path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    if not rows:
        raise ValueError(f"{csv_path}: no transcript rows")
    phoneme_to_idx = transcript_vocabulary(r["phonemes"] for r in rows)
    items, names = [], []
    for r in rows:
        stem = os.path.splitext(os.path.basename(r["audio_path"]))[0]
        spec = torch.load(os.path.join(str(mel_directory), stem + ".pt"))
        items.append({"phonemes": torch.tensor([phoneme_to_idx[p] for p in r["phonemes"].split()], dtype=torch.int64),
                      "spectrogram": spec.view(spec.shape[1:]).transpose(1, 0)})
        names.append(stem)
    return items, names, phoneme_to_idx


def split_indices(n: int, split_percentages: Sequence[float], seed: int = 42) -> Tuple[List[int], List[int], List[int]]:
    train_l, val_l, _ = get_subset_lengths(n, split_percentages)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed))).tolist()
    return perm[:train_l], perm[train_l:train_l + val_l], perm[train_l + val_l:]


def _epoch_generator(seed: int, epoch: int) -> torch.Generator:
    return torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)


def _lengths(lengths_or_corpus) -> List[int]:
    return list(lengths_or_corpus.frame_lengths) if isinstance(lengths_or_corpus, TTSCorpus) else [int(v) for v in lengths_or_corpus]


def batch_plan(lengths_or_corpus, indices: Optional[Sequence[int]] = None, batch_size: int = 1, shuffle: bool = True, drop_last: bool = True,
               seed: int = 0, epoch: int = 0) -> List[List[int]]:
    """The ``DataLoader(dataset, batch_size, shuffle, drop_last)`` of ``wrappers.py:213-232`` over the subset ``indices`` (default:
    everything) as a list of index lists; the shuffle is ``torch.randperm`` from a CPU generator seeded by (seed, epoch)."""
    idx = list(range(len(_lengths(lengths_or_corpus)))) if indices is None else [int(i) for i in indices]
    if batch_size < 1:
        raise ValueError(f"batch_plan: batch_size must be positive (got {batch_size})")
    if shuffle:
        idx = [idx[j] for j in torch.randperm(len(idx), generator=_epoch_generator(seed, epoch)).tolist()]
    plan = [idx[lo:lo + batch_size] for lo in range(0, len(idx), batch_size)]
    if drop_last and plan and len(plan[-1]) < batch_size:
        plan.pop()
    return plan


def variable_batch_plan(corpus, indices: Optional[Sequence[int]] = None, min_mel_len: int = 64, max_mel_len: int = 8192,
                        batch_size_for_max_len: int = 1, seed: int = 0, epoch: int = 0) -> Tuple[List[List[int]], List[int]]:
    """The bucketing of ``VariableBatchSizeDataset.__init__`` (``dataset/interface.py:133-202``) from the length table alone, no
    sample is loaded: one bucket per power of two of the mel length, key int(log2(len)), batch size
    ``batch_size_for_max_len * 2**(n_buckets - i - 1)`` so that every batch costs about the same memory.  -> (batches in bucket
    order, dropped ids): lengths >= ``max_mel_len`` and the incomplete batch left in each bucket are dropped, as there.  Samples
    are shuffled inside a batch (``__getitem__``, ``interface.py:226``) from a generator seeded by (seed, epoch).
    ``corpus``: a ``TTSCorpus`` -- the sample length is then the reference's ``max(spectrogram.shape)``, i.e. at least n_mel
    (``interface.py:173``) -- or a plain list of lengths."""
    lengths = _lengths(corpus)
    floor = corpus.n_mel if isinstance(corpus, TTSCorpus) else 0
    idx = list(range(len(lengths))) if indices is None else [int(i) for i in indices]
    lo, hi = math.log2(min_mel_len), math.log2(max_mel_len)
    if lo != int(lo) or hi != int(hi):
        raise ValueError("variable_batch_plan: min_mel_len and max_mel_len must be powers of 2")
    min_key, n_buckets = int(lo), int(hi) - int(lo)
    size = {min_key + i: batch_size_for_max_len * 2 ** (n_buckets - i - 1) for i in range(n_buckets)}
    buckets: Dict[int, List[List[int]]] = {k: [] for k in size}
    queue: Dict[int, List[int]] = {k: [] for k in size}
    dropped = []
    for i in idx:
        n = max(lengths[i], floor)
        if n >= max_mel_len:
            dropped.append(i)
            continue
        key = n.bit_length() - 1                                    # int(log2(n)), exactly
        if key not in queue:
            raise ValueError(f"variable_batch_plan: utterance {i} has {n} frames, fewer than min_mel_len = {min_mel_len}")
        queue[key].append(i)
        if len(queue[key]) == size[key]:
            buckets[key].append(queue[key])
            queue[key] = []
    for key in queue:                                               # incomplete buckets are also dropped
        dropped += queue[key]
    g = _epoch_generator(seed, epoch)
    plan = []
    for key in buckets:
        for batch in buckets[key]:
            plan.append([batch[j] for j in torch.randperm(len(batch), generator=g).tolist()])
    if dropped:
        _lib.log_once(f"variable_batch_plan dropped {len(dropped)}", f"variable_batch_plan: {len(dropped)} utterances dropped (longer than "
                      f"max_mel_len = {max_mel_len}, or left in an incomplete bucket); they are the second return value")
    return plan, dropped
