#!/usr/bin/env python3
"""The SqueezeWave likelihood on one MI355X: how long it takes to score the 16 utterances of 100-870 mel frames that
``vocoder_bench.py --ragged-only`` vocodes (two batches of 8; random-init weights of the default configuration), four ways:

  eager_nll_ragged   ``SqueezeWave.nll_ragged`` per batch
  graph_nll_ragged   ``SqueezeWave.capture_nll_ragged`` replays (one graph per capacity bucket), packing included
  score_audio        ``synthesis.score_audio`` from the waveforms: one ragged mel launch + eager ``nll_ragged`` per batch
  capture_ragged     the OTHER direction over the same utterances: ``capture_ragged`` replays (mel -> audio), the figure
                     the analysis direction is held against -- the same WN work, so about the same time is expected

Method: every leg is warmed up (captures and folding happen there), then the legs are timed in turn, interleaved, ``--reps``
times, each timing a host clock around work that ends in a device synchronise; the record holds the median and the
min / max of every leg.

    python scripts/vocoder_likelihood_bench.py > profiles/vocoder_likelihood_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import synthesis  # noqa: E402
from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram  # noqa: E402
from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig  # noqa: E402

SR = 22050


def ragged_lengths(n=16, seed=0):
    """The utterance lengths of vocoder_bench.py's ragged legs (mel frames, seeded)."""
    g = torch.Generator().manual_seed(seed)
    return [int(x) for x in torch.randint(100, 871, (n,), generator=g)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vocoder_likelihood_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sw = SqueezeWave(12, 128, 80, 2, 16, WNConfig()).to(dev).eval()
    for wn in sw.wn_layers:                                   # end_conv is zero-initialised: give the flow something to do
        wn.end_conv.weight.data.normal_(0, 0.01)
    creator = Tacotron2Spectrogram(SR, 1024, 1024, 256, 80).to(dev)
    lens = ragged_lengths()
    g = torch.Generator().manual_seed(1)
    batches = []
    for i in range(0, len(lens), 8):
        ls = lens[i:i + 8]
        mel = torch.zeros(8, 80, max(ls))
        audio = torch.zeros(8, 256 * max(ls))
        for j, n in enumerate(ls):
            mel[j, :, :n] = (torch.randn(80, n, generator=g) * 2 - 5).clamp(-11.5, 2.0)
            audio[j, :256 * n] = 0.2 * torch.randn(256 * n, generator=g)
        batches.append((mel.to(dev), ls, audio.to(dev), [256 * n for n in ls]))
    caps = [synthesis.capacity_frames(sum(ls)) for _, ls, _, _ in batches]
    nll_runs = [sw.capture_nll_ragged(8, c) for c in caps]
    inf_runs = [sw.capture_ragged(8, c) for c in caps]

    legs = {
        "eager_nll_ragged": lambda: [sw.nll_ragged(mel, ls, audio)[0] for mel, ls, audio, _ in batches],
        "graph_nll_ragged": lambda: [r(mel, ls, audio)[0].clone() for r, (mel, ls, audio, _) in zip(nll_runs, batches)],
        "score_audio": lambda: [synthesis.score_audio(sw, creator, audio, ns)[0] for _, _, audio, ns in batches],
        "capture_ragged": lambda: [r(mel, ls)[0].clone() for r, (mel, ls, _, _) in zip(inf_runs, batches)],
    }
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():                            # interleaved: a slow moment of the host hits every leg alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    audio_s = 256 * sum(lens) / SR
    out = {"lengths": lens, "audio_s": round(audio_s, 2), "batches": 2, "capacities": caps, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "unit": "ms for all 16 utterances (two batches of 8)"}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"median_ms": round(1e3 * med, 3), "min_ms": round(1e3 * min(ts), 3), "max_ms": round(1e3 * max(ts), 3),
                  "audio_s_per_s": round(audio_s / med, 1)}
    out["graph_nll_over_capture_ragged"] = round(out["graph_nll_ragged"]["median_ms"] / out["capture_ragged"]["median_ms"], 3)
    per, batch = sw.nll_ragged(*batches[0][:3])
    gper, gbatch = nll_runs[0](*batches[0][:3])
    out["check"] = {"batch_nll": round(float(batch), 6), "graph_equals_eager": bool(torch.equal(per, gper) and torch.equal(batch, gbatch))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
