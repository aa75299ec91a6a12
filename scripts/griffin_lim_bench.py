#!/usr/bin/env python3
"""Griffin-Lim vocoding on one MI355X: the 16 utterances of scripts/denoise_bench.py (1-10 s at 22.05 kHz), their log-mels (the
package's Tacotron2Spectrogram of a seeded vowel-like signal) inverted by ``griffin_lim.GriffinLim`` -- one ``rtts_gl_magnitudes``
launch, one ``rtts_gl_init`` launch and ``--iters`` ``rtts_gl_step`` launches (n_fft 1024, hop 256, momentum 0.99).

    python scripts/griffin_lim_bench.py            # writes profiles/griffin_lim_bench.json and prints it

Time: device events around ``--replays`` replays of a hipGraph that holds the whole call, ``--repeats`` times after a warm-up; a
second graph holds the call with no iteration (magnitudes and start), and the time of one iteration is the difference of the two
over ``--iters``.  Each repeat is followed by one timed pass of the same algorithm as a float32 ``torch.stft`` / ``torch.istft``
loop on the device (one utterance at a time: the reflect padding is per utterance; the same magnitudes, the previous spectrogram
kept for the momentum term as torchaudio does), host clock around the pass and a device synchronise, so the two legs alternate.
Next to them: ``synthesis.mel_round_trip_error`` of both results against the mels they were made from.  FLOP: what the algorithm
needs, two real n_fft x n_fft transforms per frame and iteration over the real frames only; a launch computes 32 / 29 of that (tiles
overlap by three frames).  The share of peak is against the 155 TFLOP/s measured for back-to-back v_mfma_f32_32x32x2_f32."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import _graphs, synthesis  # noqa: E402
from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram  # noqa: E402
from reformer_tts_amd.griffin_lim import GriffinLim  # noqa: E402

SR, N_FFT, HOP, N_MELS = 22050, 1024, 256, 80
F32_MFMA_PEAK = 155e12
MOMENTUM = 0.99


def voiced(n, seed, dev):
    """A vowel-like signal: a wandering fundamental with 29 harmonics at 1/k, a 3 Hz envelope and a little noise."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / SR
    ph = torch.rand(31, generator=g, dtype=torch.float64) * 2 * math.pi
    inst = 2 * math.pi * torch.cumsum(120.0 + 40.0 * torch.sin(2 * math.pi * 1.3 * t + ph[0]), 0) / SR
    x = sum(torch.sin(k * inst + ph[k]) / k for k in range(1, 30))
    x = x * (0.5 + 0.5 * torch.sin(2 * math.pi * 3.0 * t) ** 2) * 0.1 + 0.003 * torch.randn(n, generator=g, dtype=torch.float64)
    return x.to(torch.float32).to(dev)


def torch_griffin_lim(mags, lens, window, iters, seed):
    """torchaudio's loop in float32 on the tensors' device, one utterance at a time."""
    beta = MOMENTUM / (1.0 + MOMENTUM)
    g = torch.Generator(device=window.device).manual_seed(seed)
    out = []
    for m, n in zip(mags, lens):
        ang = torch.polar(torch.ones_like(m), 2 * math.pi * torch.rand(m.shape, generator=g, device=m.device))
        prev = None
        for _ in range(iters):
            x = torch.istft(m * ang, N_FFT, HOP, N_FFT, window, center=True, length=n)
            c = torch.stft(x, N_FFT, HOP, N_FFT, window, center=True, pad_mode="reflect", return_complex=True)
            r = c if prev is None else c - beta * prev
            prev = c
            ang = r / r.abs().clamp(min=1e-16)
        out.append(torch.istft(m * ang, N_FFT, HOP, N_FFT, window, center=True, length=n))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "griffin_lim_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("griffin_lim_bench measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    frames = [int(f) for f in torch.randint(SR // HOP, 10 * SR // HOP + 1, (16,), generator=g)]      # the draw of denoise_bench.py
    lens = [HOP * f for f in frames]
    creator = Tacotron2Spectrogram(SR, N_FFT, N_FFT, HOP, N_MELS).to(dev)
    packed_mel, foff = creator.forward_packed(torch.cat([voiced(n, 100 + i, dev) for i, n in enumerate(lens)]), lens)
    mel = torch.zeros(16, N_MELS, max(frames), device=dev)
    for i, n in enumerate(frames):
        mel[i, :, :n] = packed_mel[:, foff[i]:foff[i] + n]

    gl = GriffinLim(creator, n_iter=args.iters, momentum=MOMENTUM)
    start_only = GriffinLim(creator, n_iter=0, momentum=MOMENTUM)
    tables = gl.tables(frames)
    graphs = {}
    for name, obj in (("call", gl), ("start", start_only)):
        for _ in range(2):
            obj.forward_packed(mel, tables=tables)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with _graphs.capturing(graph):
            out, _ = obj.forward_packed(mel, tables=tables)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        graphs[name] = (graph, out)
    waves = [w.clone() for w in gl.split_packed(graphs["call"][1], synthesis.segment_offsets(frames))]

    # the same magnitudes for the torch loop: what rtts_gl_magnitudes wrote
    from reformer_tts_amd import ops
    mag = torch.empty(N_FFT // 2 + 1, tables.col_offsets[-1], device=dev)
    ops.gl_magnitudes(mel, [0] * 16, tables.device_table[3], tables.coff_host, tables.device_table[:2], 16, gl.pinv, gl.power, N_FFT, mag)
    mags = [mag[:, tables.col_offsets[i]:tables.col_offsets[i + 1]].contiguous() for i in range(16)]
    window = torch.hann_window(N_FFT, periodic=True, device=dev)
    where = "device (same magnitudes)"
    try:
        ref = torch_griffin_lim(mags, lens, window, args.iters, 0)
        torch.cuda.synchronize()
    except RuntimeError as e:                                     # no device FFT in this torch build: the host, and say so
        where = f"host, {min(len(os.sched_getaffinity(0)), 16)} cores (torch.stft did not run on the device: {str(e).splitlines()[0][:120]})"
        torch.set_num_threads(min(len(os.sched_getaffinity(0)), 16))
        mags, window = [m.cpu() for m in mags], window.cpu()
        ref = torch_griffin_lim(mags, lens, window, args.iters, 0)

    def timed(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.replays

    call_ms, start_ms, torch_ms = [], [], []
    for _ in range(args.repeats):                                 # the legs alternate
        call_ms.append(timed(graphs["call"][0]))
        start_ms.append(timed(graphs["start"][0]))
        t0 = time.perf_counter()
        torch_griffin_lim(mags, lens, window, args.iters, 0)
        torch.cuda.synchronize()
        torch_ms.append(1e3 * (time.perf_counter() - t0))

    err_kernel = synthesis.mel_round_trip_error(waves, mel, frames, creator)
    err_torch = synthesis.mel_round_trip_error([r.to(dev) for r in ref], mel, frames, creator)
    n_frames = sum(f + 1 for f in frames)
    flop_iter = 4.0 * n_frames * N_FFT * N_FFT
    ms, ms0 = statistics.median(call_ms), statistics.median(start_ms)
    per_iter = (ms - ms0) / max(args.iters, 1)
    result = {
        "shape": {"sample_rate": SR, "n_fft": N_FFT, "hop": HOP, "n_mels": N_MELS, "n_iter": args.iters, "momentum": MOMENTUM, "phase": "hash"},
        "utterances": 16, "audio_s": round(sum(lens) / SR, 2), "stft_frames": n_frames, "launches": 2 + args.iters,
        "call_ms": {"median": round(ms, 4), "min": round(min(call_ms), 4), "max": round(max(call_ms), 4), "replays_per_repeat": args.replays,
                    "repeats": args.repeats, "timing": "device events around hipGraph replays of the whole call"},
        "magnitudes_and_start_ms": {"median": round(ms0, 4), "min": round(min(start_ms), 4), "max": round(max(start_ms), 4),
                                    "timing": "the same, for the graph of the call with n_iter = 0"},
        "iteration_ms": round(per_iter, 4),
        "x_realtime": round(sum(lens) / SR / (ms * 1e-3), 0),
        "iteration_algorithm_tflop": round(flop_iter / 1e12, 5), "iteration_tflops": round(flop_iter / (per_iter * 1e-3) / 1e12, 2),
        "iteration_share_of_f32_mfma_peak_155TF": round(flop_iter / (per_iter * 1e-3) / F32_MFMA_PEAK, 4),
        "computed_over_algorithm_flop": round(32 / 29, 4),
        "torch_f32_stft_istft_loop": {"where": where, "ms_median": round(statistics.median(torch_ms), 3), "ms_min": round(min(torch_ms), 3),
                                      "timing": "host clock around one pass over the 16 utterances and a device synchronise, alternating "
                                                "with the graph's repeats"},
        "torch_over_call": round(statistics.median(torch_ms) / ms, 1),
        "mel_round_trip_error": {"kernel_mean": round(float(err_kernel.mean()), 4), "kernel_max": round(float(err_kernel.max()), 4),
                                 "torch_mean": round(float(err_torch.mean()), 4), "torch_max": round(float(err_torch.max()), 4),
                                 "what": "mean |log-mel(audio) - mel| per utterance (synthesis.mel_round_trip_error); the two loops start "
                                         "from different random phases"},
    }
    text = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
