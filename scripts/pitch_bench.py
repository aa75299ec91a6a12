#!/usr/bin/env python3
"""F0 tracking on one MI355X: 16 utterances of 1-10 s at 22.05 kHz (the shape of scripts/mel_bench.py) through one ragged
rtts_pitch_yin launch (hop 256, lags 45..441, threshold 0.1), alternated with a float32 torch restatement of its d' on the same
device (``unfold``, differences, ``cumsum``; frames in chunks, its (frames, 513, 1024) differences do not fit at once), and the
one rtts_f0_compare launch on the contours.

    python scripts/pitch_bench.py > profiles/pitch_bench.json

Kernel time: device events around ``--replays`` replays of a hipGraph that holds the one launch; the restatement: device events
around one pass; the two alternate ``--repeats`` times after a warm-up, and the median, minimum and maximum are reported.  Work:
what the algorithm needs when the frames share their hop blocks, one subtraction and one fused multiply-add per (sample of a hop
block, lag) = 3 FLOP in two vector issue slots, against the 157 TFLOP/s f32 vector peak (an fma in every slot: this mix tops out at
3/4 of it).  The restatement computes every frame's whole window, W / hop = 4 times the differences."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import _graphs, ops  # noqa: E402
from reformer_tts_amd.evaluation import PitchTracker  # noqa: E402

SR, HOP, W, LAGS = 22050, 256, 1024, 512
F32_VALU_PEAK = 157.3e12


def utterances(n=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = [int(x) for x in torch.randint(SR, 10 * SR + 1, (n,), generator=g)]
    out = []
    for m in lens:                                                 # a voiced-looking signal: a slow glide with three harmonics, and noise
        t = torch.arange(m, dtype=torch.float64) / SR
        f = 100.0 + 100.0 * torch.rand(1, generator=g, dtype=torch.float64) + 20.0 * torch.sin(2.0 * torch.pi * 0.7 * t)
        phase = 2.0 * torch.pi * torch.cumsum(f, 0) / SR
        x = sum(torch.sin(h * phase) / h for h in (1, 2, 3)) * 0.2 + 0.02 * (torch.rand(m, generator=g, dtype=torch.float64) - 0.5)
        out.append(x.float())
    return out


def torch_cmnd(flat, tables, chunk=128):
    """d' of every frame, (total frames, 513) f32, on the device of ``flat``: the restatement the launch is timed against."""
    rows = []
    lag = torch.arange(1, LAGS + 1, device=flat.device, dtype=torch.float32)
    for i, n in enumerate(tables.lengths):
        x = flat[tables.sample_offsets[i]: tables.sample_offsets[i] + n]
        t = n // HOP + 1
        xp = torch.nn.functional.pad(x, ((W + LAGS) // 2, (t - 1) * HOP + (W + LAGS) // 2 - n + HOP))
        frames = xp.unfold(0, W + LAGS, HOP)[:t]                   # (t, 1536) view
        for f0 in range(0, t, chunk):
            fr = frames[f0: f0 + chunk]
            diff = fr[:, None, :W] - fr.unfold(1, W, 1)            # (chunk, 513, 1024)
            d = (diff * diff).sum(-1)
            run = torch.cumsum(d[:, 1:], 1)
            cm = torch.ones_like(d)
            cm[:, 1:] = torch.where(run == 0, torch.ones_like(run), d[:, 1:] * lag / run)
            rows.append(cm)
    return torch.cat(rows)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pitch_bench measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    utts = utterances()
    lens = [u.numel() for u in utts]
    tracker = PitchTracker(SR, HOP)
    tables = tracker.tables(lens, dev)
    flat = torch.cat(utts).to(dev)
    frames = tables.frame_offsets[-1]
    out = torch.empty(2, frames, device=dev)
    foff = tables.device_table[1]

    def launch():
        ops.pitch_yin(flat, tables.soff_host, tables.foff_host, tables.device_table, len(lens), HOP, tracker.tau_min, tracker.tau_max,
                      tracker.threshold, float(SR), out[0], out[1])

    for _ in range(3):
        launch()
        torch_cmnd(flat, tables)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _graphs.capturing(graph):
        launch()
    table = torch.empty(len(lens) + 1, 5, dtype=torch.float64, device=dev)
    other = (out[0] * 1.01).contiguous()
    cgraph = torch.cuda.CUDAGraph()
    ops.f0_compare(other, foff, out[0], foff, 0.2, out=table)
    torch.cuda.synchronize()
    with _graphs.capturing(cgraph):
        ops.f0_compare(other, foff, out[0], foff, 0.2, out=table)
    for _ in range(10):
        graph.replay()
        cgraph.replay()
    torch.cuda.synchronize()

    def replays(g):
        def run():
            for _ in range(args.replays):
                g.replay()
        return run

    kernel_ms, torch_ms, compare_ms = [], [], []
    for _ in range(args.repeats):
        kernel_ms.append(timed(replays(graph)) / args.replays)
        torch_ms.append(timed(lambda: torch_cmnd(flat, tables)))
        compare_ms.append(timed(replays(cgraph)) / args.replays)

    # same inputs, both paths: the launch's d' (a call with the cmnd output) against the restatement's
    _, _, _, cm = tracker.forward_packed(flat, tables=tables, return_cmnd=True)
    want = torch_cmnd(flat, tables)
    rel = ((cm - want).abs() / want.clamp_min(1e-30))[:, 1:].max().item()
    voiced = int((out[0] > 0).sum())
    blocks = sum(n // HOP + W // HOP for n in lens)                # hop blocks whose partial sums the frames need
    flop = 3.0 * blocks * HOP * LAGS
    ms = statistics.median(kernel_ms)
    print(json.dumps({
        "shape": {"sample_rate": SR, "hop": HOP, "window": W, "lags": LAGS, "tau_min": tracker.tau_min, "tau_max": tracker.tau_max,
                  "threshold": tracker.threshold},
        "utterances": len(lens), "audio_s": round(sum(lens) / SR, 2), "frames": frames, "voiced_frames": voiced,
        "kernel_ms": dict(stats(kernel_ms), replays_per_repeat=args.replays, repeats=args.repeats,
                          timing="device events around hipGraph replays, alternated with the restatement"),
        "frames_per_s": round(frames / (ms * 1e-3), 0), "x_realtime": round(sum(lens) / SR / (ms * 1e-3), 0),
        "algorithm_gflop_shared_hop_blocks": round(flop / 1e9, 3), "tflops": round(flop / (ms * 1e-3) / 1e12, 2),
        "share_of_f32_vector_peak_157TF": round(flop / (ms * 1e-3) / F32_VALU_PEAK, 4),
        "torch_restatement_ms": dict(stats(torch_ms), what="d' only: unfold, differences, cumsum, in chunks of 128 frames, same device"),
        "restatement_over_kernel": round(statistics.median(torch_ms) / ms, 1),
        "f0_compare_ms": stats(compare_ms),
        "max_relative_cmnd_difference_vs_restatement": rel,
    }))


if __name__ == "__main__":
    main()
