#!/usr/bin/env python3
"""Where a vocoder training step gets its batch from, on one MI355X at the README's training shape (default SqueezeWave
configuration, B = 96 segments of 16384 samples): three variants in ONE process, interleaved round by round as
``vocoder_train_bench.py --graph`` does, each on a model of its own from the same seed, all drawing from one synthetic corpus.

    python scripts/vocoder_corpus_bench.py > profiles/vocoder_corpus_bench.json

  host_batches     the ``VocoderTrainer.capture`` graph fed batches the host assembles: ``vocoder_segment`` per utterance from
                   host copies of the corpus with a hop from ``random``, stacked into pinned memory, copied to the device by
                   ``run`` (the training loop before the device-resident corpus)
  device_batches   the same graph fed a batch that already lies on the device (two device copies and the permute remain)
  corpus_replay    the ``VocoderTrainer.capture_corpus`` replay: the draw is inside the graph

Per step the host clock around the call and a synchronise (what a training loop pays) and device events around the call are
recorded; ``rtts_sw_draw_segments`` is also timed alone (device events around one launch, and around the launch with the cursor
add).  No threshold: medians and ranges are written down, and whether corpus_replay was slower than device_batches by more than
the spread of the rounds."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import ops  # noqa: E402
from reformer_tts_amd.dataset.utils import vocoder_segment  # noqa: E402
from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig  # noqa: E402
from reformer_tts_amd.squeeze_wave.corpus import SegmentSampler, VocoderCorpus  # noqa: E402
from reformer_tts_amd.squeeze_wave.training import VocoderTrainer  # noqa: E402


def _model(dev):
    torch.manual_seed(0)
    model = SqueezeWave(12, 128, 80, 2, 16, WNConfig(8, 256, 3, 2)).to(dev)
    for wn in model.wn_layers:                      # the reference starts end_conv at zero; a trained one is not
        wn.end_conv.weight.data.normal_(0, 0.01)
    return model.train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--mel-len", type=int, default=64)
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b, lm, hop = args.batch, args.mel_len, 256
    s = hop * lm

    # a synthetic corpus: lengths from half a segment to eight segments (LJSpeech clips are 1 - 10 s = 1.3 - 13 segments)
    g = torch.Generator().manual_seed(1)
    lengths = [int(n) for n in torch.randint(s // 2, 8 * s, (args.utterances,), generator=g)]
    audios = [0.1 * torch.randn(n, generator=g) for n in lengths]
    mels = [torch.randn(80, n // hop + 1, generator=g) for n in lengths]
    foff = [0]
    for m in mels:
        foff.append(foff[-1] + m.shape[1])
    corpus = VocoderCorpus.from_packed(torch.cat(audios).to(dev), lengths, torch.cat(mels, dim=1).to(dev), foff, hop)

    models = {k: _model(dev) for k in ("host_batches", "device_batches", "corpus_replay")}
    trainers = {k: VocoderTrainer(m, logdet="device") for k, m in models.items()}
    run_host = trainers["host_batches"].capture(b, lm)
    run_dev = trainers["device_batches"].capture(b, lm)
    sampler = SegmentSampler(corpus, b, s, seed=1)
    sampler.start_epoch(0)
    run_corpus = trainers["corpus_replay"].capture_corpus(sampler)

    pinned = {"spectrogram": torch.empty(b, 80, lm).pin_memory(), "audio": torch.empty(b, s).pin_memory()}
    staged = {k: torch.empty(v.shape, device=dev) for k, v in pinned.items()}
    rnd = random.Random(2)

    def host_step():
        for i, u in enumerate(rnd.sample(range(len(lengths)), b)):
            mh = (lengths[u] - s) // hop if lengths[u] >= s else 0
            a, m = vocoder_segment(audios[u], mels[u], s, hop, random_hop=rnd.randint(0, mh))
            pinned["audio"][i].copy_(a)
            pinned["spectrogram"][i].copy_(m)
        for k in pinned:
            staged[k].copy_(pinned[k], non_blocking=True)
        return run_host(staged)

    sampler.draw()                                   # a real batch for the device-resident variant
    dev_batch = {k: v.contiguous().clone() for k, v in sampler.batch_dict().items()}
    sampler.start_epoch(0)
    steps = {"host_batches": host_step, "device_batches": lambda: run_dev(dev_batch), "corpus_replay": run_corpus}
    ev = lambda: torch.cuda.Event(enable_timing=True)     # noqa: E731

    def timed(fn):
        a, z = ev(), ev()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        loss = fn()
        z.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, a.elapsed_time(z), float(loss)

    losses = {k: [] for k in steps}
    for _ in range(args.warmup):
        for k, fn in steps.items():
            losses[k].append(timed(fn)[2])
    wall, device = {k: [] for k in steps}, {k: [] for k in steps}
    t_end = time.perf_counter() + 3 * args.seconds
    while time.perf_counter() < t_end or len(wall["corpus_replay"]) < 5:
        for k, fn in steps.items():
            w, d, loss = timed(fn)
            wall[k].append(w)
            device[k].append(d)
            losses[k].append(loss)
    for t in trainers.values():
        t.check_determinants()

    def launch_only():
        c = sampler.corpus
        ops.sw_draw_segments(c.audio, c.tables[0], c.mel, c.tables[1], sampler.order, sampler.state, sampler.seed, None, b, lm, hop, 128,
                             sampler.audio_rows, sampler.mel_rows, sampler.picks)

    alone = {}
    for name, fn in (("launch", launch_only), ("launch_and_cursor_add", sampler.draw)):
        for _ in range(5):
            fn()
        alone[name] = []
        for _ in range(50):
            a, z = ev(), ev()
            a.record()
            fn()
            z.record()
            torch.cuda.synchronize()
            alone[name].append(a.elapsed_time(z))

    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}     # noqa: E731
    med = {k: statistics.median(v) for k, v in wall.items()}
    q = statistics.quantiles(wall["device_batches"], n=4)
    spread = q[2] - q[0]
    print(json.dumps({
        "what": "one vocoder training step by where its batch comes from: the capture graph fed host-assembled batches, the same graph "
                "fed a device-resident batch, and the capture_corpus replay (the draw inside the graph); interleaved in one process; "
                "host clock around each step and a synchronise, device_* = device events around the call",
        "device": torch.cuda.get_device_name(0), "batch": b, "mel_len": lm, "samples_per_segment": s, "utterances": len(lengths),
        "corpus_audio_mb": round(corpus.audio.numel() * 4 / 2 ** 20, 1), "rounds_timed": len(wall["corpus_replay"]),
        **{k: stat(v) for k, v in wall.items()},
        **{"device_" + k: stat(v) for k, v in device.items()},
        "rtts_sw_draw_segments_alone": stat(alone["launch"]), "draw_and_cursor_add_alone": stat(alone["launch_and_cursor_add"]),
        "draw_bytes_written": b * s * 4 + b * lm * 80 * 4,
        "device_batches_interquartile_ms": round(spread, 3),
        "corpus_minus_device_batches_ms": round(med["corpus_replay"] - med["device_batches"], 3),
        "corpus_slower_than_device_batches_beyond_spread": bool(med["corpus_replay"] - med["device_batches"] > spread),
        "corpus_over_host_batches": round(med["corpus_replay"] / med["host_batches"], 4),
        "segments_per_second": {k: round(b / (v * 1e-3), 1) for k, v in med.items()},
        "loss_first": {k: v[0] for k, v in losses.items()}, "loss_last": {k: v[-1] for k, v in losses.items()}}))


if __name__ == "__main__":
    main()
