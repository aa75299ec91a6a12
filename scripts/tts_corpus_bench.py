#!/usr/bin/env python3
"""Where a ReformerTTS training epoch gets its batches from, on one MI355X: config/baseline.yml at B = 12 with mel lengths 600-1024
(a few padded shapes), a synthetic corpus of 512 utterances, accumulate_grad_batches 1.  Variants in ONE process, interleaved
epoch by epoch, each on a trainer of its own from the same seed and over the same plan:

    python scripts/tts_corpus_bench.py > profiles/tts_corpus_bench.json

  fit_collating     ``Trainer.fit`` over a generator that runs ``custom_sequence_padder(pin_memory=True)`` per batch inside the
                    epoch (a loader without worker processes): collate, copy, ``_fill_shape_buffers``, replay
  fit_precollated   ``Trainer.fit`` over pinned batches collated before the clock starts (a loader whose workers keep up)
  fit_corpus        ``Trainer.fit_corpus`` over a ``TTSCorpus``: the plan uploaded once, one ``rtts_tts_collate`` launch per batch

The host clock runs around an epoch and a synchronise (what a training loop pays).  ``rtts_tts_collate`` is also timed alone at
the largest shape, with and without the input noise (device events around one launch).  No threshold: medians and ranges are
written down."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd.dataset import TTSCorpus, batch_plan, custom_sequence_padder  # noqa: E402
from reformer_tts_amd.model.config import baseline_model_config, baseline_training_config  # noqa: E402
from reformer_tts_amd.training import Trainer, build_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    items = []
    for _ in range(args.utterances):
        lm, lp = int(torch.randint(600, 1025, (1,), generator=g)), int(torch.randint(50, 201, (1,), generator=g))
        items.append(dict(phonemes=torch.randint(1, 77, (lp,), generator=g), spectrogram=(torch.randn(lm, 80, generator=g) * 2 - 5).clamp(-11.5, 2.0)))
    corpus = TTSCorpus.from_items(items, dev)

    def trainer():
        tcfg = baseline_training_config()
        tcfg.batch_size, tcfg.accumulate_grad_batches, tcfg.lr_scheduler = args.batch, 1, None
        return Trainer(build_model(baseline_model_config(), dev, seed=42), tcfg, dev)

    def plan(epoch):
        return batch_plan(corpus, None, args.batch, shuffle=True, drop_last=True, seed=0, epoch=epoch)

    def collating(p):
        for ids in p:
            yield custom_sequence_padder([items[i] for i in ids], pin_memory=True)

    trainers = {k: trainer() for k in ("fit_collating", "fit_precollated", "fit_corpus")}

    def run(kind, epoch):
        p = plan(epoch)
        tr = trainers[kind]
        batches = list(collating(p)) if kind == "fit_precollated" else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "fit_corpus":
            losses = tr.fit_corpus(corpus, p)
        else:
            losses = tr.fit(collating(p) if batches is None else batches)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(p), len(p), float(losses[-1])

    first = {k: run(k, 0) for k in trainers}                        # the captures of every padded shape happen here
    per_step = {k: [] for k in trainers}
    last = {}
    for epoch in range(1, args.epochs + 1):
        for k in trainers:
            ms, steps, loss = run(k, epoch)
            per_step[k].append(ms)
            last[k] = loss

    # the launch alone, at the largest padded shape of the baseline
    lp_pad, lm_pad, nm = 256, 1024, corpus.n_mel
    bufs = dict(phonemes=torch.zeros(args.batch, lp_pad, dtype=torch.int64, device=dev), spectrogram_input=torch.zeros(args.batch, lm_pad, nm, device=dev),
                spectrogram_target=torch.zeros(args.batch, lm_pad, nm, device=dev), stop_tokens=torch.zeros(args.batch, lm_pad, device=dev),
                loss_mask=torch.zeros(args.batch, lm_pad, nm, device=dev), valid_len=torch.ones(1, dtype=torch.int32, device=dev))
    order = sorted(range(len(corpus)), key=lambda i: -corpus.frame_lengths[i])[:args.batch]
    ids = torch.tensor(order, dtype=torch.int32, device=dev)
    lm = max(corpus.frame_lengths[i] for i in order)
    moved = sum(t.numel() * t.element_size() for t in bufs.values()) + sum(corpus.frame_lengths[i] for i in order) * nm * 4
    alone = {}
    for name, std in (("no_noise", None), ("noise_std_0.5", 0.5)):
        for _ in range(5):
            corpus.fill(bufs, ids, std, 1, lm=lm)
        us = []
        for _ in range(50):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            corpus.fill(bufs, ids, std, 1, lm=lm)
            z.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(z) * 1e3)
        med = statistics.median(us)
        alone[name] = {"median_us": round(med, 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "gb_per_s": round(moved / med * 1e-3, 1)}

    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}     # noqa: E731
    med = {k: statistics.median(v) for k, v in per_step.items()}
    print(json.dumps({
        "what": "ms per optimizer step of one ReformerTTS training epoch by where its batches come from (see the script's docstring); "
                "host clock around an epoch and a synchronise, divided by its steps; epochs interleaved in one process",
        "device": torch.cuda.get_device_name(0), "batch": args.batch, "utterances": len(corpus), "mel_lengths": [600, 1024],
        "steps_per_epoch": first["fit_corpus"][1], "epochs_timed": args.epochs, "padded_shapes": sorted(k for k in trainers["fit_corpus"]._shape_graphs),
        "corpus_mel_mb": round(corpus.mel.numel() * 4 / 2 ** 20, 1),
        **{k: stat(v) for k, v in per_step.items()},
        "first_epoch_with_captures_ms_per_step": {k: round(v[0], 3) for k, v in first.items()},
        "fit_corpus_over_fit_collating": round(med["fit_corpus"] / med["fit_collating"], 4),
        "fit_corpus_over_fit_precollated": round(med["fit_corpus"] / med["fit_precollated"], 4),
        "fit_corpus_minus_fit_precollated_ms": round(med["fit_corpus"] - med["fit_precollated"], 3),
        "rtts_tts_collate_alone": alone, "collate_bytes_moved": moved,
        "loss_last": last}))


if __name__ == "__main__":
    main()
