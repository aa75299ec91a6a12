#!/usr/bin/env python3
"""One vocoder training step on one MI355X at the reference's training shape: the default SqueezeWave configuration, B = 96
segments of 16384 samples (Lm 64, 12288 audio rows), ``VocoderTrainer.training_step`` = zero_grad + ``nll_backward`` + Adam.

    python scripts/vocoder_train_bench.py > profiles/vocoder_train_bench.json

After a warm-up, device-event timings over a window of at least ``--seconds``: the whole step, and its split into re-fold
(weight norm, bf16 casts, padding, and the host float64 log-determinants / inverses of the twelve W_k with their device -> host
copy), forward, backward and Adam.  Next to it ``model.nll`` at the same shape in eval mode (the forward-only yardstick), the
algorithmic GEMM FLOP of a step computed from the shapes with the rate they reach over the step, and the launches of a step.
There is no pass / fail threshold: the numbers are recorded.

    python scripts/vocoder_train_bench.py --graph > profiles/vocoder_train_graph_bench.json

``--graph``: three variants of the step in ONE process, interleaved round by round (each round times one step of each, so a
drift of the box hits all three alike) -- the eager step with the host float64 factorisation (``VocoderTrainer(model)``), the
eager step with the device factorisation (``logdet="device"``), and the replay of ``VocoderTrainer.capture`` -- each on a model of
its own from the same seed, plus ``rtts_sw_inv1x1_factor`` alone on the twelve W_k of the model.  Medians and ranges are
recorded; the replay is expected not to be slower than the host-mode eager step of the same run, and the JSON says whether it was."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import _lib  # noqa: E402
from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig  # noqa: E402
from reformer_tts_amd.squeeze_wave.training import VocoderTrainer  # noqa: E402


def gemm_flop(model: SqueezeWave, b: int, mel_len: int) -> float:
    """2 M N K of every 1x1 convolution of a step: forward, input gradient and weight gradient (the mel and the audio need no
    input gradient)."""
    rows, mrows = b * mel_len * model._up(), b * mel_len
    total = 0.0
    for k, (wn, inv) in enumerate(zip(model.wn_layers, model.inv_conv_layers)):
        n = inv.conv.weight.shape[0]
        c, nl, nh, n_mel = wn.n_channels, wn.n_layers, n // 2, model._n_mel()
        total += 2.0 * rows * n * n * (3 if k else 2)
        total += 2.0 * rows * nh * c * 3 + 2.0 * mrows * n_mel * 2 * c * nl * 2 + 2.0 * rows * c * 2 * nh * 3
        total += nl * (2.0 * rows * c * 2 * c + 2.0 * rows * c * c) * 3
    return total


def _model(dev):
    torch.manual_seed(0)
    model = SqueezeWave(12, 128, 80, 2, 16, WNConfig(8, 256, 3, 2)).to(dev)
    for wn in model.wn_layers:                      # the reference starts end_conv at zero; a trained one is not
        wn.end_conv.weight.data.normal_(0, 0.01)
    return model.train()


def graph_bench(args):
    from reformer_tts_amd import ops
    dev = torch.device("cuda:0")
    b, lm = args.batch, args.mel_len
    models = {k: _model(dev) for k in ("eager_host", "eager_device", "graph_replay")}
    torch.manual_seed(1)
    batch = {"spectrogram": torch.randn(b, 80, lm, device=dev), "audio": 0.1 * torch.randn(b, 256 * lm, device=dev)}
    host_t = VocoderTrainer(models["eager_host"])
    dev_t = VocoderTrainer(models["eager_device"], logdet="device")
    graph_t = VocoderTrainer(models["graph_replay"], logdet="device")
    run = graph_t.capture(b, lm)
    steps = {"eager_host": lambda: host_t.training_step(batch), "eager_device": lambda: dev_t.training_step(batch),
             "graph_replay": lambda: run(batch)}
    ev = lambda: torch.cuda.Event(enable_timing=True)     # noqa: E731

    def timed(fn):
        a, z = ev(), ev()
        t0 = time.perf_counter()
        a.record()
        loss = fn()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z), (time.perf_counter() - t0) * 1e3, float(loss)

    losses = {k: [] for k in steps}
    for _ in range(args.warmup):
        for k, fn in steps.items():
            losses[k].append(timed(fn)[2])
    times, wall = {k: [] for k in steps}, {k: [] for k in steps}
    t_end = time.perf_counter() + 3 * args.seconds
    while time.perf_counter() < t_end or len(times["graph_replay"]) < 5:
        for k, fn in steps.items():
            t, w, loss = timed(fn)
            times[k].append(t)
            wall[k].append(w)
            losses[k].append(loss)
    graph_t.check_determinants()

    # the factorisation alone: the twelve W_k of the model, one launch, device events around each launch
    ws = [c.conv.weight.detach().squeeze(-1).contiguous() for c in models["eager_device"].inv_conv_layers]
    for _ in range(5):
        ops.sw_inv1x1_factor(ws)
    lu_ms = []
    for _ in range(50):
        a, z = ev(), ev()
        a.record()
        ops.sw_inv1x1_factor(ws)
        z.record()
        torch.cuda.synchronize()
        lu_ms.append(a.elapsed_time(z))

    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}     # noqa: E731
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "what": "VocoderTrainer step, default SqueezeWave configuration: eager host-mode, eager device-mode and the captured graph, "
                "interleaved in one process (device events around each step; host_clock_* = host clock around the step and a synchronise)",
        "device": torch.cuda.get_device_name(0), "batch": b, "mel_len": lm, "audio_rows": b * lm * 2, "rounds_timed": len(times["graph_replay"]),
        **{k: stat(v) for k, v in times.items()},
        **{"host_clock_" + k: stat(v) for k, v in wall.items()},
        "replay_over_eager_host": round(med["graph_replay"] / med["eager_host"], 4),
        "replay_not_slower_than_eager_host": bool(med["graph_replay"] <= med["eager_host"]),
        "sw_inv1x1_factor_12_matrices": stat(lu_ms), "factor_sizes": [int(w.shape[0]) for w in ws],
        "segments_per_second_graph_replay": round(b / (med["graph_replay"] * 1e-3), 1),
        "loss_first": {k: v[0] for k, v in losses.items()}, "loss_last": {k: v[-1] for k, v in losses.items()},
        "device_and_graph_losses_equal": losses["eager_device"] == losses["graph_replay"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--mel-len", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--graph", action="store_true", help="time host-mode eager, device-mode eager and the captured step, interleaved")
    args = ap.parse_args()
    if args.graph:
        return graph_bench(args)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SqueezeWave(12, 128, 80, 2, 16, WNConfig(8, 256, 3, 2)).to(dev)
    for wn in model.wn_layers:                      # the reference starts end_conv at zero; a trained one is not
        wn.end_conv.weight.data.normal_(0, 0.01)
    b, lm = args.batch, args.mel_len
    batch = {"spectrogram": torch.randn(b, 80, lm, device=dev), "audio": 0.1 * torch.randn(b, 256 * lm, device=dev)}
    trainer = VocoderTrainer(model)
    ev = lambda: torch.cuda.Event(enable_timing=True)     # noqa: E731

    def whole():
        """VocoderTrainer.training_step between two events -> ms, loss"""
        a, z = ev(), ev()
        a.record()
        loss = trainer.training_step(batch)
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z), float(loss)

    def split():
        """The same calls one by one with events between them -> (fold, forward, backward, adam, fold on the host clock) ms"""
        marks = [ev() for _ in range(5)]
        model.train()
        trainer.optimizer.zero_grad()
        marks[0].record()
        t0 = time.perf_counter()
        model._fold(fold_bn=False)
        host_fold = (time.perf_counter() - t0) * 1e3
        marks[1].record()
        model.nll_backward(batch["spectrogram"], batch["audio"], _after_forward=marks[2].record)
        marks[3].record()
        trainer.optimizer.step()
        marks[4].record()
        torch.cuda.synchronize()
        t = [marks[i].elapsed_time(marks[i + 1]) for i in range(4)]
        t[1] -= t[0]                      # nll_backward folds again itself: what is left of its first part is the forward
        return t + [host_fold]

    losses = []
    for _ in range(args.warmup):
        losses.append(whole()[1])
    torch.cuda.reset_peak_memory_stats()
    steps, t_end = [], time.perf_counter() + args.seconds
    while time.perf_counter() < t_end or len(steps) < 5:
        t, loss = whole()
        steps.append(t)
        losses.append(loss)
    peak = torch.cuda.max_memory_allocated()
    splits = [split() for _ in range(5)]
    med = [statistics.median(steps)] + [statistics.median(col) for col in zip(*splits)]
    times = [[t] for t in steps]

    # launches of one step: the library's entry calls (each one or two kernels) counted here, every kernel by the profiler
    calls = [0]
    orig = _lib.call

    def counting(name, *a):
        calls[0] += 1
        return orig(name, *a)
    kernels = None
    try:
        from torch.profiler import ProfilerActivity, profile
        _lib.call = counting
        for mod in (sys.modules["reformer_tts_amd.squeeze_wave.modules"], sys.modules["reformer_tts_amd.engine"]):
            mod._lib.call = counting
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            trainer.training_step(batch)
            torch.cuda.synchronize()
        kernels = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA
                      and "memcpy" not in e.key.lower() and "memset" not in e.key.lower())
    except Exception as exc:          # the profiler is optional evidence
        kernels = f"not measured ({type(exc).__name__})"
    finally:
        _lib.call = orig

    model.eval()
    with torch.no_grad():
        for _ in range(3):
            model.nll(batch["spectrogram"], batch["audio"])
        nll_ms = []
        for _ in range(10):
            a, z = ev(), ev()
            a.record()
            model.nll(batch["spectrogram"], batch["audio"])
            z.record()
            torch.cuda.synchronize()
            nll_ms.append(a.elapsed_time(z))
    flop = gemm_flop(model, b, lm)
    print(json.dumps({
        "what": "VocoderTrainer.training_step, default SqueezeWave configuration", "device": torch.cuda.get_device_name(0),
        "batch": b, "mel_len": lm, "audio_rows": b * lm * 2, "samples_per_segment": 256 * lm, "steps_timed": len(times),
        "step_ms": round(med[0], 3), "step_ms_min": round(min(t[0] for t in times), 3), "step_ms_max": round(max(t[0] for t in times), 3),
        "refold_and_host_logdet_ms": round(med[1], 3), "refold_and_host_logdet_host_ms": round(med[5], 3),
        "forward_ms": round(med[2], 3), "backward_ms": round(med[3], 3), "adam_ms": round(med[4], 3),
        "eval_nll_ms": round(statistics.median(nll_ms), 3),
        "gemm_gflop_per_step": round(flop / 1e9, 1), "gemm_tflops_over_step": round(flop / (med[0] * 1e-3) / 1e12, 2),
        "gemm_tflops_over_forward_backward": round(flop / ((med[2] + med[3]) * 1e-3) / 1e12, 2),
        "segments_per_second": round(b / (med[0] * 1e-3), 1), "peak_memory_gb": round(peak / 2 ** 30, 2),
        "hip_entry_calls_per_step": calls[0], "kernel_launches_per_step": kernels,
        "loss_first": losses[0], "loss_last": losses[-1]}))


if __name__ == "__main__":
    main()
