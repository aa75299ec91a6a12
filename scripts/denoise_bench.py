#!/usr/bin/env python3
"""The vocoder denoiser on one MI355X: 16 utterances of 1-10 s at 22.05 kHz, vocoded by one ``SqueezeWave.infer_ragged`` call
(reference default configuration, seeded weights) and denoised by one ragged ``rtts_denoise`` launch (n_fft 1024, hop 256).

    python scripts/denoise_bench.py            # writes profiles/denoise_bench.json and prints it

Kernel time: device events around ``--replays`` replays of a hipGraph that holds the one launch, ``--repeats`` times after a
warm-up.  Each repeat is followed by one timed pass of the float32 ``torch.stft`` -> gain -> ``torch.istft`` pipeline over the same
device tensors (one utterance at a time: the reflect padding is per utterance), so the two legs alternate; if this torch build
cannot run the transforms on the device, that leg runs on 16 host cores and the result says so.  Next to them: the time of the
``infer_ragged`` call that produces the audio (host clock around the call and a device synchronise).  FLOP: what the algorithm
needs, two real n_fft x n_fft transforms per frame, over the real frames only; the launch computes 32 / 29 of that (tiles overlap
by three frames).  The share of peak is against the 155 TFLOP/s measured for back-to-back v_mfma_f32_32x32x2_f32."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import _graphs  # noqa: E402
from reformer_tts_amd.squeeze_wave import Denoiser, SqueezeWave, WNConfig  # noqa: E402

SR, N_FFT, HOP, N_MELS = 22050, 1024, 256, 80
F32_MFMA_PEAK = 155e12
STRENGTH = 0.1


def torch_pipeline(waves, bias, window, strength):
    out = []
    for x in waves:
        X = torch.stft(x, N_FFT, HOP, N_FFT, window, center=True, pad_mode="reflect", return_complex=True)
        mag = X.abs()
        g = torch.clamp(mag - strength * bias[:, None], min=0) / torch.clamp(mag, min=1e-30)
        out.append(torch.istft(X * g, N_FFT, HOP, N_FFT, window, center=True, length=x.numel()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "denoise_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sw = SqueezeWave(12, 128, N_MELS, 2, 16, WNConfig()).to(dev).eval()
    for wn in sw.wn_layers:                                       # end_conv is zero-initialised: give the flow something to do
        wn.end_conv.weight.data.normal_(0, 0.01)
    g = torch.Generator().manual_seed(0)
    frames = [int(f) for f in torch.randint(SR // HOP, 10 * SR // HOP + 1, (16,), generator=g)]
    lens = [HOP * f for f in frames]
    mel = ((torch.randn(16, N_MELS, max(frames), generator=g) * 2 - 5).clamp(-11.5, 2.0)).to(dev)

    # the call that produces the audio
    for _ in range(2):
        packed, waves = sw.infer_ragged(mel, frames)
    torch.cuda.synchronize()
    infer_s = []
    for _ in range(5):
        t0 = time.perf_counter()
        packed, waves = sw.infer_ragged(mel, frames)
        torch.cuda.synchronize()
        infer_s.append(time.perf_counter() - t0)

    d = Denoiser(sw)
    tables = d.tables(lens)
    out = torch.empty_like(packed)
    for _ in range(3):
        d.forward_packed(packed, tables=tables, strength=STRENGTH, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _graphs.capturing(graph):
        d.forward_packed(packed, tables=tables, strength=STRENGTH, out=out)
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()

    window = torch.hann_window(N_FFT, periodic=True, device=dev)
    where = "device (same tensors)"
    t_waves, t_bias = waves, d.bias_spec
    try:
        ref = torch_pipeline(t_waves, t_bias, window, STRENGTH)
        torch.cuda.synchronize()
    except RuntimeError as e:                                     # no device FFT in this torch build: the host, and say so
        where = f"host, {min(len(os.sched_getaffinity(0)), 16)} cores (torch.stft did not run on the device: {str(e).splitlines()[0][:120]})"
        torch.set_num_threads(min(len(os.sched_getaffinity(0)), 16))
        t_waves, t_bias, window = [w.cpu() for w in waves], d.bias_spec.cpu(), window.cpu()
        ref = torch_pipeline(t_waves, t_bias, window, STRENGTH)

    kernel_ms, torch_ms = [], []
    for _ in range(args.repeats):                                 # the two legs alternate
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        kernel_ms.append(a.elapsed_time(b) / args.replays)
        t0 = time.perf_counter()
        torch_pipeline(t_waves, t_bias, window, STRENGTH)
        torch.cuda.synchronize()
        torch_ms.append(1e3 * (time.perf_counter() - t0))

    got = SqueezeWave.split_packed(out, [0] + [sum(frames[:i + 1]) for i in range(16)])
    diff = max(float((a.cpu() - b.cpu()).abs().max()) for a, b in zip(got, ref))
    changed = max(float((a - b).abs().max()) for a, b in zip(got, waves))
    n_frames = sum(n // HOP + 1 for n in lens)
    flop = 4.0 * n_frames * N_FFT * N_FFT
    ms = statistics.median(kernel_ms)
    result = {
        "shape": {"sample_rate": SR, "n_fft": N_FFT, "hop": HOP, "strength": STRENGTH},
        "utterances": 16, "audio_s": round(sum(lens) / SR, 2), "frames": n_frames,
        "kernel_ms": {"median": round(ms, 4), "min": round(min(kernel_ms), 4), "max": round(max(kernel_ms), 4),
                      "replays_per_repeat": args.replays, "repeats": args.repeats, "timing": "device events around hipGraph replays"},
        "x_realtime": round(sum(lens) / SR / (ms * 1e-3), 0),
        "algorithm_tflop": round(flop / 1e12, 5), "tflops": round(flop / (ms * 1e-3) / 1e12, 2),
        "share_of_f32_mfma_peak_155TF": round(flop / (ms * 1e-3) / F32_MFMA_PEAK, 4),
        "computed_over_algorithm_flop": round(32 / 29, 4),
        "bytes": {"audio_in": 4 * sum(lens), "audio_out": 4 * sum(lens), "bases_in_cache": 8 * N_FFT * N_FFT},
        "torch_f32_stft_gain_istft": {"where": where, "ms_median": round(statistics.median(torch_ms), 3), "ms_min": round(min(torch_ms), 3),
                                      "timing": "host clock around one pass over the 16 utterances and a device synchronise, "
                                                "alternating with the kernel's repeats"},
        "torch_over_kernel": round(statistics.median(torch_ms) / ms, 1),
        "infer_ragged_ms": {"median": round(1e3 * statistics.median(infer_s), 2), "min": round(1e3 * min(infer_s), 2),
                            "timing": "host clock around the eager call that produces the audio and a device synchronise, 5 calls"},
        "denoise_share_of_infer_ragged": round(ms / (1e3 * statistics.median(infer_s)), 4),
        "max_abs_difference_vs_torch_f32": diff,
        "max_abs_change_of_the_audio": changed,
    }
    text = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
