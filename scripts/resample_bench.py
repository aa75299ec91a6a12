#!/usr/bin/env python3
"""Sample-rate conversion on one MI355X: 16 utterances of 1-10 s, 48 kHz stereo 16-bit PCM as a WAV file holds it, to 22,050 Hz
mono f32 through one ragged rtts_resample launch, alone and chained with the log-mel launch that takes its output (config shape:
n_fft 1024, hop 256, 80 mels), next to a float32 polyphase conv1d of the same filter on 16 host cores (the stated baseline, not a
target).

    python scripts/resample_bench.py > profiles/resample_bench.json

Kernel time: device events around ``--replays`` replays of a hipGraph that holds the launch (or the two), ``--repeats`` times after
a warm-up; the median, minimum and maximum per-replay time are reported.  Bytes: what the algorithm must move -- every byte of the
interleaved payload (the skipped channel shares its cache lines with channel 0) and 4 bytes per output sample; the coefficient
table (15.5 KB) stays on chip.  The rate is set against the stream-copy rate measured in the same process (rtts_peak_copy, 1 GiB,
as bench.py measures it).  The 16 utterances move about 31 MB, which a replay finds in the 256 MB Infinity Cache: their rate is
a cache rate and is named so; the 256-utterance leg (about 0.5 GB per launch) is the one that streams from HBM."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import _graphs, _lib  # noqa: E402
from reformer_tts_amd.dataset.audio import Resample, Tacotron2Spectrogram, resample_tables  # noqa: E402

ORIG, NEW, CHANNELS = 48000, 22050, 2
N_FFT, WIN, HOP, N_MELS = 1024, 1024, 256, 80


def utterances(n=16, seed=0):
    """n utterances of 1-10 s: int16 (frames, 2), noise at -10 dBFS in both channels (different in each)."""
    g = torch.Generator().manual_seed(seed)
    lens = [int(x) for x in torch.randint(ORIG, 10 * ORIG + 1, (n,), generator=g)]
    return [(torch.randn(m, CHANNELS, generator=g) * 0.3 * 32768).clamp(-32768, 32767).to(torch.int16) for m in lens]


def timed_replays(graph, args):
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.replays)
    return ms


def gpu_leg(resampler, creator, utts, dev, args):
    """-> (tables, resampled output, per-replay ms of the resample launch alone, of resample + mel)."""
    lens = [u.shape[0] for u in utts]
    tables = resampler.tables(lens)
    raw = torch.cat([u.reshape(-1) for u in utts]).to(dev)
    out = torch.empty(tables.out_offsets[-1], device=dev)
    mel_tables = creator.tables(tables.out_lengths)
    mel = torch.empty(N_MELS, mel_tables.frame_offsets[-1], device=dev)

    def one():
        resampler.forward_packed(raw, tables=tables, channels=CHANNELS, out=out)

    def both():
        one()
        creator.forward_packed(out, tables=mel_tables, out=mel)

    times = []
    for fn in (one, both):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with _graphs.capturing(graph):
            fn()
        times.append(timed_replays(graph, args))
    return tables, out, times[0], times[1]


def copy_peak_gbs(dev):
    n = 1 << 30
    src, dst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        _lib.call("rtts_peak_copy", src.data_ptr(), dst.data_ptr(), n, s)
    a.record()
    for _ in range(5):
        _lib.call("rtts_peak_copy", src.data_ptr(), dst.data_ptr(), n, s)
    b.record()
    torch.cuda.synchronize()
    return 5 * 2 * n / (a.elapsed_time(b) * 1e-3) / 1e9


def cpu_polyphase(utts, first, coef, o, w):
    """The same filter as a float32 conv1d: one output channel per phase, stride orig', the phases interleaved afterwards."""
    taps = coef.shape[0]
    lo, hi = int(first.min()), int(first.max()) + taps
    weight = torch.zeros(w, 1, hi - lo)
    for p in range(w):
        a = int(first[p]) - lo
        weight[p, 0, a:a + taps] = coef[:, p]
    out = []
    for u in utts:
        x = u[:, 0].to(torch.float32) / 32768.0
        m = -((-x.numel() * w) // o)
        blocks = -(-m // w)
        need = (blocks - 1) * o + hi                                 # one past the last input index the last block reads
        x = torch.nn.functional.pad(x, (-lo, max(need - x.numel(), 0)))
        y = torch.nn.functional.conv1d(x[None, None], weight, stride=o)[0]      # (w, >= blocks)
        out.append(y[:, :blocks].t().reshape(-1)[:m])
    return out


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--cpu-reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    resampler = Resample(ORIG, NEW).to(dev)
    creator = Tacotron2Spectrogram(NEW, N_FFT, WIN, HOP, N_MELS).to(dev)
    peak = copy_peak_gbs(dev)

    def leg(utts):
        tables, out, ms1, ms2 = gpu_leg(resampler, creator, utts, dev, args)
        frames_in, samples_out = tables.in_offsets[-1], tables.out_offsets[-1]
        nbytes = 2 * CHANNELS * frames_in + 4 * samples_out
        med = statistics.median(ms1)
        return tables, out, {
            "utterances": len(utts), "audio_s": round(frames_in / ORIG, 2), "frames_in": frames_in, "samples_out": samples_out,
            "resample_ms": stats(ms1), "resample_plus_mel_ms": stats(ms2),
            "bytes": {"pcm_in": 2 * CHANNELS * frames_in, "f32_out": 4 * samples_out},
            "gb_per_s": round(nbytes / (med * 1e-3) / 1e9, 1), "share_of_copy_peak": round(nbytes / (med * 1e-3) / 1e9 / peak, 4),
            "x_realtime": round(frames_in / ORIG / (med * 1e-3), 0),
            "gflop_per_s": round(2.0 * resampler.taps * samples_out / (med * 1e-3) / 1e9, 1)}

    utts = utterances()
    tables, out, small = leg(utts)
    small["note"] = "about 31 MB per launch: replays find it in the Infinity Cache, the rate is a cache rate"
    got = out.cpu()
    _, _, big = leg(utterances(256, seed=1))
    big["note"] = "about 0.5 GB per launch: streamed from HBM"

    cores = min(len(os.sched_getaffinity(0)), 16)
    torch.set_num_threads(cores)
    first, coef, o, w, _ = resample_tables(ORIG, NEW)
    ref = cpu_polyphase(utts, first, coef, o, w)
    cpu_s = []
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        cpu_polyphase(utts, first, coef, o, w)
        cpu_s.append(time.perf_counter() - t0)
    cpu_ms = 1e3 * statistics.median(cpu_s)
    diff = max(float((got[tables.out_offsets[i]:tables.out_offsets[i + 1]] - r).abs().max()) for i, r in enumerate(ref))
    print(json.dumps({
        "conversion": {"orig": ORIG, "new": NEW, "channels": CHANNELS, "input": "int16 interleaved", "phases": resampler.new_red,
                       "taps": resampler.taps},
        "timing": "device events around hipGraph replays", "replays_per_repeat": args.replays, "repeats": args.repeats,
        "copy_peak_gb_per_s": round(peak, 1),
        "batch_16": small, "saturated_256_utterances": big,
        "mel_shape": {"n_fft": N_FFT, "win_length": WIN, "hop": HOP, "n_mels": N_MELS, "power": 1},
        "cpu_f32_polyphase_conv1d": {"cores": cores, "ms": round(cpu_ms, 2)},
        "gpu_over_cpu": round(cpu_ms / small["resample_ms"]["median"], 1),
        "max_abs_difference_vs_cpu_f32": diff,
    }))


if __name__ == "__main__":
    main()
