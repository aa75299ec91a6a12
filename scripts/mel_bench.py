#!/usr/bin/env python3
"""Audio -> log-mel on one MI355X: 16 utterances of 1-10 s at 22.05 kHz through one ragged rtts_mel_spectrogram launch (config
shape: n_fft 1024, window 1024, hop 256, 80 mels, Tacotron-2 variant), next to the float32 torch.stft + matmul pipeline on
16 host cores (the stated baseline, not a target).

    python scripts/mel_bench.py > profiles/mel_bench.json

Kernel time: device events around ``--replays`` replays of a hipGraph that holds the one launch, ``--repeats`` times after a
warm-up; the median, minimum and maximum per-launch time are reported.  FLOP: what the algorithm needs, 2 n_fft^2 for the real
DFT of a frame plus 2 n_mels (n_fft/2 + 1) for its mel product, over the real frames only; the share of peak is against the
155 TFLOP/s measured for back-to-back v_mfma_f32_32x32x2_f32 (the kernel is bound by the f32 matrix pipe, not by bandwidth:
its audio and output bytes are reported next to it)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import _graphs  # noqa: E402
from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram, hann_window, mel_filterbank  # noqa: E402

SR, N_FFT, WIN, HOP, N_MELS = 22050, 1024, 1024, 256, 80
F32_MFMA_PEAK = 155e12


def utterances(n=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = [int(x) for x in torch.randint(SR, 10 * SR + 1, (n,), generator=g)]
    return [torch.rand(m, generator=g) - 0.5 for m in lens]


def cpu_pipeline(utts, fb32, window32):
    out = []
    for u in utts:
        mag = torch.stft(u, N_FFT, HOP, WIN, window32, center=True, pad_mode="reflect", return_complex=True).abs()
        out.append(torch.log(torch.clamp(fb32 @ mag, min=1e-5)))
    return out


def flop_of(frames):
    return 2.0 * frames * (N_FFT * N_FFT + N_MELS * (N_FFT // 2 + 1))


def gpu_leg(creator, utts, dev, args):
    """One ragged launch over ``utts`` captured into a hipGraph -> (tables, output, per-launch ms of every repeat)."""
    tables = creator.tables([u.numel() for u in utts])
    flat = torch.cat(utts).to(dev)
    out = torch.empty(N_MELS, tables.frame_offsets[-1], device=dev)
    for _ in range(3):
        creator.forward_packed(flat, tables=tables, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _graphs.capturing(graph):
        creator.forward_packed(flat, tables=tables, out=out)
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    per_launch_ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        per_launch_ms.append(a.elapsed_time(b) / args.replays)
    return tables, out, per_launch_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--cpu-reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mel_bench measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    utts = utterances()
    lens = [u.numel() for u in utts]
    creator = Tacotron2Spectrogram(SR, N_FFT, WIN, HOP, N_MELS).to(dev)
    tables, out, per_launch_ms = gpu_leg(creator, utts, dev, args)
    frames = tables.frame_offsets[-1]
    ms = statistics.median(per_launch_ms)
    flop = flop_of(frames)
    # the same launch over 16 x as many utterances: the 16 above are about one 32-frame tile per CU, so their time is set by how the
    # tiles happen to divide among 256 CUs; this leg is the kernel's steady rate
    big = utterances(16 * len(utts), seed=1)
    big_tables, _, big_ms = gpu_leg(creator, big, dev, args)
    big_frames, big_med = big_tables.frame_offsets[-1], statistics.median(big_ms)
    got = out.cpu()

    cores = min(len(os.sched_getaffinity(0)), 16)
    torch.set_num_threads(cores)
    fb32 = mel_filterbank(SR, N_FFT, N_MELS, 0.0, 8000.0, "slaney", "slaney").float()
    window32 = torch.from_numpy(hann_window(WIN, N_FFT)).float()
    ref = cpu_pipeline(utts, fb32, window32)
    cpu_s = []
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        cpu_pipeline(utts, fb32, window32)
        cpu_s.append(time.perf_counter() - t0)
    cpu_ms = 1e3 * statistics.median(cpu_s)
    # same inputs, both pipelines: the difference of the stored logs where the signal is above the clip
    diff = 0.0
    for i, r in enumerate(ref):
        g = got[:, tables.frame_offsets[i]:tables.frame_offsets[i + 1]]
        diff = max(diff, float((g - r)[r > -11.0].abs().max()))
    print(json.dumps({
        "shape": {"sample_rate": SR, "n_fft": N_FFT, "win_length": WIN, "hop": HOP, "n_mels": N_MELS, "power": 1},
        "utterances": len(lens), "audio_s": round(sum(lens) / SR, 2), "frames": frames,
        "kernel_ms": {"median": round(ms, 4), "min": round(min(per_launch_ms), 4), "max": round(max(per_launch_ms), 4),
                      "replays_per_repeat": args.replays, "repeats": args.repeats, "timing": "device events around hipGraph replays"},
        "frames_per_s": round(frames / (ms * 1e-3), 0),
        "x_realtime": round(sum(lens) / SR / (ms * 1e-3), 0),
        "algorithm_tflop": round(flop / 1e12, 5), "tflops": round(flop / (ms * 1e-3) / 1e12, 2),
        "share_of_f32_mfma_peak_155TF": round(flop / (ms * 1e-3) / F32_MFMA_PEAK, 4),
        "saturated_256_utterances": {"audio_s": round(sum(u.numel() for u in big) / SR, 1), "frames": big_frames,
                                     "kernel_ms_median": round(big_med, 4), "kernel_ms_min": round(min(big_ms), 4),
                                     "frames_per_s": round(big_frames / (big_med * 1e-3), 0),
                                     "tflops": round(flop_of(big_frames) / (big_med * 1e-3) / 1e12, 2),
                                     "share_of_f32_mfma_peak_155TF": round(flop_of(big_frames) / (big_med * 1e-3) / F32_MFMA_PEAK, 4)},
        "bytes": {"audio_in": 4 * sum(lens), "mel_out": 4 * N_MELS * frames, "dft_basis_in_cache": 4 * N_FFT * N_FFT},
        "cpu_f32_stft_matmul": {"cores": cores, "ms": round(cpu_ms, 2), "frames_per_s": round(frames / (cpu_ms * 1e-3), 0)},
        "gpu_over_cpu": round(cpu_ms / ms, 1),
        "max_abs_log_difference_vs_cpu_f32_above_clip": diff,
    }))


if __name__ == "__main__":
    main()
