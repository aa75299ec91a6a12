#!/usr/bin/env python3
"""BASELINE config #5 on one MI355X: SqueezeWave vocoder throughput (mel -> audio) and end-to-end text -> mel -> audio with
ReformerTTS.infer in front of it (random-init weights of the default configurations; 22.05 kHz audio, 256 samples per mel
frame), next to the CPU oracle of the vocoder on a bounded mel length.

    python scripts/vocoder_bench.py > gpurun_out/vocoder_bench.json
    python scripts/vocoder_bench.py --ragged-only            # only the ragged legs (16 utterances of 100-870 frames)
    python scripts/vocoder_bench.py --ragged-kernels-only    # the ragged vocoder stage alone: run it under
        rocprofv3 --kernel-trace --stats for the segment kernels' bytes/s (ragged_kernel_bytes in the JSON)
    python scripts/vocoder_bench.py --round-trip             # only mel(vocoder(mel)) against mel, per utterance
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd.model.config import baseline_model_config  # noqa: E402
from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig  # noqa: E402
from reformer_tts_amd.training import build_model  # noqa: E402

SR = 22050


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def ragged_lengths(n=16, seed=0):
    """n LJSpeech-like utterance lengths in mel frames (1.2 to 10 s at 22.05 kHz / 256), seeded."""
    g = torch.Generator().manual_seed(seed)
    return [int(x) for x in torch.randint(100, 871, (n,), generator=g)]


def ragged_legs(sw, dev, args):
    """The same 16 utterances four ways -> audio-seconds per wall-second: (a) one at a time through SqueezeWave.capture,
    one graph per distinct length (capture and replay timed apart), (b) one at a time through one capture_ragged graph,
    (c) batches of 8 through capture_ragged, (d) synthesize at B = 8 against 8 x B = 1 (text -> audio, graphed)."""
    from reformer_tts_amd import synthesis
    lens = ragged_lengths()
    g = torch.Generator().manual_seed(1)
    mels = [((torch.randn(1, 80, n, generator=g) * 2 - 5).clamp(-11.5, 2.0)).to(dev) for n in lens]
    audio_s = 256 * sum(lens) / SR
    res = {"lengths": lens, "audio_s": round(audio_s, 2)}

    def rate(dt):
        return round(audio_s / dt, 1)
    # (a) today: capture per distinct length
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runs = {n: sw.capture(1, n) for n in sorted(set(lens))}
    torch.cuda.synchronize()
    cap_s = time.perf_counter() - t0
    dt, _ = timed(lambda: [runs[n](m).clone() for n, m in zip(lens, mels)], 3)
    res["a_capture_per_length"] = {"capture_s": round(cap_s, 3), "replay_ms": round(1e3 * dt, 2), "audio_s_per_s_replay": rate(dt),
                                   "audio_s_per_s_incl_capture": rate(dt + cap_s)}
    del runs
    # (b) one at a time through one capture_ragged graph
    cap1 = synthesis.capacity_frames(max(lens))
    run1 = sw.capture_ragged(1, cap1)
    dt, _ = timed(lambda: [run1(m, [n])[0].clone() for n, m in zip(lens, mels)], 3)
    res["b_ragged_B1"] = {"capacity": cap1, "ms": round(1e3 * dt, 2), "audio_s_per_s": rate(dt)}
    # (c) batches of 8 through capture_ragged
    batches = []
    for i in range(0, len(lens), 8):
        mel = torch.zeros(8, 80, max(lens[i:i + 8]), device=dev)
        for j, m in enumerate(mels[i:i + 8]):
            mel[j, :, :m.shape[2]] = m[0]
        batches.append((mel, lens[i:i + 8]))
    caps = [synthesis.capacity_frames(sum(ls)) for _, ls in batches]
    runs8 = [sw.capture_ragged(8, c) for c in caps]
    dt, _ = timed(lambda: [r(mel, ls)[0].clone() for r, (mel, ls) in zip(runs8, batches)], 3)
    res["c_ragged_B8"] = {"capacities": caps, "ms": round(1e3 * dt, 2), "audio_s_per_s": rate(dt)}
    res["eager_infer_ragged_B8_ms"] = round(1e3 * timed(lambda: [sw.infer_ragged(mel, ls)[0] for mel, ls in batches], 2)[0], 2)
    if args.ragged_kernels_only:
        return res
    # (d) synthesize at B = 8 against 8 x B = 1: text -> mel (graphed generation, encoder cached) -> audio
    tts = build_model(baseline_model_config(), dev, seed=42)
    gp = torch.Generator().manual_seed(2)
    phonemes = [torch.randint(1, 77, (int(n) // 4,), generator=gp) for n in lens[:8]]
    kw = dict(max_len=args.tts_frames, cache_encoder=True, use_graph=True, stop_at_stop_token=False)   # random weights stop at once
    synthesis.synthesize(tts, sw, phonemes, **kw)                                   # captures
    for p in phonemes:
        synthesis.synthesize(tts, sw, [p], **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    waves, _, stop = synthesis.synthesize(tts, sw, phonemes, **kw)
    torch.cuda.synchronize()
    dt8 = time.perf_counter() - t0
    a8 = sum(w.numel() for w in waves) / SR
    t0 = time.perf_counter()
    a1 = 0
    for p in phonemes:
        a1 += sum(w.numel() for w in synthesis.synthesize(tts, sw, [p], **kw)[0]) / SR
    torch.cuda.synchronize()
    dt1 = time.perf_counter() - t0
    res["d_synthesize"] = {"max_len": args.tts_frames, "stops_B8": stop.tolist(), "B8_s": round(dt8, 3), "B8_audio_s_per_s": round(a8 / dt8, 2),
                           "8xB1_s": round(dt1, 3), "8xB1_audio_s_per_s": round(a1 / dt1, 2),
                           "note": "random-init TTS run to max_len (no stop token); generation dominates"}
    return res


def round_trip_leg(sw, dev):
    """mel -> vocoder -> audio -> log-mel against the mel that went in, for 8 of the ragged utterances: per-utterance mean
    |difference| in log units (synthesis.mel_round_trip_error, one ragged mel launch) and its wall time.  With random-init
    weights the size of the error says nothing; a trained vocoder is judged by it."""
    from reformer_tts_amd import synthesis
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram
    lens = ragged_lengths()[:8]
    g = torch.Generator().manual_seed(1)
    mel = torch.full((len(lens), 80, max(lens)), -11.5)
    for i, n in enumerate(lens):
        mel[i, :, :n] = (torch.randn(80, n, generator=g) * 2 - 5).clamp(-11.5, 2.0)
    mel = mel.to(dev)
    creator = Tacotron2Spectrogram(SR, 1024, 1024, 256, 80).to(dev)
    _, waves = sw.infer_ragged(mel, lens)
    dt, err = timed(lambda: synthesis.mel_round_trip_error(waves, mel, lens, creator), 5)
    return {"lengths": lens, "mean_abs_log_mel_error": [round(float(e), 4) for e in err.cpu()], "ms": round(1e3 * dt, 3),
            "note": "random-init vocoder: the wiring is measured, not the quality"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mel-len", type=int, default=1024)
    ap.add_argument("--tts-frames", type=int, default=200)
    ap.add_argument("--cpu-mel-len", type=int, default=64)
    ap.add_argument("--ragged-only", action="store_true", help="only the ragged legs")
    ap.add_argument("--ragged-kernels-only", action="store_true", help="ragged legs (a)-(c) only, for a rocprofv3 kernel trace")
    ap.add_argument("--round-trip", action="store_true", help="only the mel(vocoder(mel)) round-trip leg")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sw = SqueezeWave(12, 128, 80, 2, 16, WNConfig()).to(dev).eval()
    for wn in sw.wn_layers:                                   # end_conv is zero-initialised: give the flow something to do
        wn.end_conv.weight.data.normal_(0, 0.01)
    out = {"unit": "audio samples/s", "sample_rate": SR}
    if args.round_trip:
        out["round_trip"] = round_trip_leg(sw, dev)
        print(json.dumps(out))
        return
    if args.ragged_only or args.ragged_kernels_only:
        out["ragged"] = ragged_legs(sw, dev, args)
        lens = out["ragged"]["lengths"]
        # bytes moved per call of the segment kernels (one per WN layer and flow / one per batch), for a kernel-trace run
        out["ragged_kernel_bytes"] = {"depthwise_k3_seg_per_row": 256 * (4 + 2), "pack_mel_per_frame": 80 * (4 + 4),
                                      "note": "fp32 row in, bf16 row out (neighbours hit in cache); HBM peak 8 TB/s"}
        print(json.dumps(out))
        return
    for b in (1, 8):
        mel = (torch.randn(b, 80, args.mel_len) * 2 - 5).clamp(-11.5, 2.0).to(dev)
        dt, audio = timed(lambda: sw.infer(mel), 5)
        out[f"vocoder_B{b}"] = {"mel_len": args.mel_len, "ms": round(1e3 * dt, 3), "samples_per_s": round(audio.numel() / dt, 0),
                                "x_realtime": round(audio.numel() / dt / SR, 1)}
        run = sw.capture(b, args.mel_len)
        dt, audio = timed(lambda: run(mel), 20)
        out[f"vocoder_B{b}_graph"] = {"mel_len": args.mel_len, "ms": round(1e3 * dt, 3), "samples_per_s": round(audio.numel() / dt, 0),
                                      "x_realtime": round(audio.numel() / dt / SR, 1)}
    # CPU oracle of the vocoder (fp32 eager restatement of the reference), bounded
    from oracle import squeezewave_ref as sw_ref
    cores = min(len(os.sched_getaffinity(0)), 16)
    torch.set_num_threads(cores)
    sd = {k: v.detach().cpu().float() for k, v in sw.state_dict().items()}
    melc = (torch.randn(1, 80, args.cpu_mel_len) * 2 - 5).clamp(-11.5, 2.0)
    t0 = time.perf_counter()
    with torch.no_grad():
        a = sw_ref.infer(sd, sw_ref.default_cfg(), melc)
    dtc = time.perf_counter() - t0
    out["vocoder_cpu_oracle"] = {"mel_len": args.cpu_mel_len, "ms": round(1e3 * dtc, 1), "samples_per_s": round(a.numel() / dtc, 0),
                                 "x_realtime": round(a.numel() / dtc / SR, 2), "cores": cores}
    # end to end: text -> mel (ReformerTTS.infer, encoder cached) -> audio
    tts = build_model(baseline_model_config(), dev, seed=42)
    ph = torch.randint(1, 77, (1, 200), generator=torch.Generator().manual_seed(0))

    def e2e():
        spec, _ = tts.infer(ph, max_len=args.tts_frames, stop_at_stop_token=False, cache_encoder=True)
        return sw.infer(spec)
    def e2e_graph():
        spec, _ = tts.infer(ph, max_len=args.tts_frames, stop_at_stop_token=False, cache_encoder=True, use_graph=True)
        return sw.infer(spec)
    dtg, audio = timed(e2e_graph, 1)
    out["text_to_audio_B1_graph"] = {"frames": args.tts_frames, "ms": round(1e3 * dtg, 1), "samples_per_s": round(audio.numel() / dtg, 0),
                                     "x_realtime": round(audio.numel() / dtg / SR, 2), "note": "one hipGraph replay per frame (captures included)"}
    dt, audio = timed(e2e, 1)
    out["text_to_audio_B1"] = {"frames": args.tts_frames, "ms": round(1e3 * dt, 1), "samples_per_s": round(audio.numel() / dt, 0),
                               "x_realtime": round(audio.numel() / dt / SR, 2),
                               "note": "ReformerTTS.infer (one full decoder forward per frame, encoder cached) dominates"}
    del tts
    out["ragged"] = ragged_legs(sw, dev, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
