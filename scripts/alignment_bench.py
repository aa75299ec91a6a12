#!/usr/bin/env python3
"""Alignment scores and monotonic alignment search on one MI355X at the validation shape: 3 decoder layers, 12 utterances, (1024,
256) attention matrices, 670-1020 frames and 120-250 phonemes per utterance.

    python scripts/alignment_bench.py > profiles/alignment_bench.json

``rtts_align_stats`` and ``rtts_align_mas`` are timed as hipGraph replays between device events (``--replays`` per region),
alternated ``--repeats`` times with what they replace: a float64 torch restatement of the statistics on the same device (masked
reductions, one ``log`` and one ``exp`` over every matrix) and a numpy monotonic alignment search on the host (frame loop, one
layer of one utterance, scaled to the 36 searches of the call).  Then ``Trainer.validate`` of the baseline model with and without
``alignment=True``.  Medians with their ranges."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from reformer_tts_amd import _graphs, ops  # noqa: E402

LAYERS, B, TQ, TK, SIGMA = 3, 12, 1024, 256, 0.2


def matrices(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(670, 1021, (B,), generator=g)
    keys = torch.randint(120, 251, (B,), generator=g)
    t = torch.arange(TQ, dtype=torch.float64)[None, :, None] / frames[:, None, None]
    k = torch.arange(TK, dtype=torch.float64)[None, None, :] / keys[:, None, None]
    mats = []
    for sharp in (30.0, 300.0, 100.0):                             # a diagonal ridge of a different width per layer, and noise
        logits = -sharp * (k - t) ** 2 + torch.randn(B, TQ, TK, generator=g, dtype=torch.float64)
        logits = logits.masked_fill(torch.arange(TK)[None, None, :] >= keys[:, None, None], float("-inf"))
        mats.append(torch.softmax(logits, dim=-1).float())
    return torch.stack(mats).to(dev), frames.to(torch.int32).to(dev), keys.to(torch.int32).to(dev)


def torch_stats(mats, n_frames, n_keys):
    """The table's six sums and the arg-max track in float64 torch on the device (no durations, no counts)."""
    a = mats.double()
    tq = torch.arange(TQ, device=a.device)
    tk = torch.arange(TK, device=a.device)
    live = (tq[None, :, None] < n_frames[:, None, None]) & (tk[None, None, :] < n_keys[:, None, None])
    a = torch.where(live[None], a, torch.zeros_like(a))
    d = tk[None, None, :] / n_keys[:, None, None].double() - tq[None, :, None] / n_frames[:, None, None].double()
    w = 1.0 - torch.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    ent = -(a * torch.log(a.clamp_min(1e-300))).sum(-1)
    peak, argmax = a.max(dim=-1)
    return torch.stack([a.sum((-1, -2)), peak.sum(-1), ent.sum(-1), (a * w[None]).sum((-1, -2))], dim=-1), argmax


def numpy_mas(a, t, k, floor=1e-30):
    c = np.log(np.maximum(a[:t, :k].astype(np.float64), floor))
    q = np.full((t, k), -np.inf)
    q[0, 0] = c[0, 0]
    move = np.full(k, -np.inf)
    for i in range(1, t):
        move[1:] = q[i - 1, :-1]
        q[i] = c[i] + np.maximum(q[i - 1], move)
    dur = np.zeros(k, dtype=np.int64)
    j = k - 1
    for i in range(t - 1, -1, -1):
        dur[j] += 1
        if i and j and q[i - 1, j - 1] > q[i - 1, j]:
            j -= 1
    return dur, q[t - 1, k - 1]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def validate_case(repeats):
    from reformer_tts_amd.model.config import baseline_model_config, baseline_training_config
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    dev = torch.device("cuda:0")
    model = build_model(baseline_model_config(), dev, seed=42)
    tcfg = baseline_training_config()
    tcfg.batch_size = B
    tr = Trainer(model, tcfg, dev)
    batch = synthetic_batch(B, TK, TQ, seed=42, device=dev)
    out = {}
    for name, kw in (("plain", {}), ("alignment", {"alignment": True})):
        for _ in range(3):
            tr.validate(batch, **kw)
        torch.cuda.synchronize()
        out[name] = []
    for _ in range(repeats):
        for name, kw in (("plain", {}), ("alignment", {"alignment": True})):
            out[name].append(timed(lambda: [tr.validate(batch, **kw) for _ in range(5)]) / 5)
    return {"validate_ms": stats(out["plain"]), "validate_alignment_ms": stats(out["alignment"]),
            "added_ms": round(statistics.median(out["alignment"]) - statistics.median(out["plain"]), 4),
            "decoder_layers": model.dec.reformer.depth, "what": "Trainer.validate of the baseline model, B 12, text 256, mel 1024, eager launches"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-validate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("alignment_bench measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    mats, n_frames, n_keys = matrices(dev)
    for _ in range(2):
        got_stats = ops.alignment_stats(mats, n_frames, n_keys, SIGMA)
        got_mas = ops.alignment_mas(mats, n_frames, n_keys)
        want_table, want_argmax = torch_stats(mats, n_frames, n_keys)
    torch.cuda.synchronize()
    graphs = []
    for fn in (lambda: ops.alignment_stats(mats, n_frames, n_keys, SIGMA), lambda: ops.alignment_mas(mats, n_frames, n_keys)):
        g = torch.cuda.CUDAGraph()
        with _graphs.capturing(g):
            keep = fn()
        graphs.append((g, keep))
    for g, _ in graphs:
        for _ in range(5):
            g.replay()
    torch.cuda.synchronize()

    def replays(g):
        return lambda: [g.replay() for _ in range(args.replays)]

    host = mats[1, 0].cpu().numpy()
    t0, k0 = int(n_frames[0]), int(n_keys[0])
    stats_ms, mas_ms, torch_ms, numpy_ms = [], [], [], []
    for _ in range(args.repeats):
        stats_ms.append(timed(replays(graphs[0][0])) / args.replays)
        torch_ms.append(timed(lambda: torch_stats(mats, n_frames, n_keys)))
        mas_ms.append(timed(replays(graphs[1][0])) / args.replays)
        start = time.perf_counter()
        want_dur, want_q = numpy_mas(host, t0, k0)
        numpy_ms.append((time.perf_counter() - start) * 1e3)
    table = got_stats[2][:, :-1, 2:6]
    rel = float(((table - want_table).abs() / want_table.abs().clamp_min(1e-30)).max())
    same_dur = bool((got_mas[0][1, 0, :k0].cpu().numpy() == want_dur).all())
    nbytes = int(sum(int(t) * int(k) for t, k in zip(n_frames.tolist(), n_keys.tolist())) * 4 * LAYERS)
    full = LAYERS * B * TQ * TK * 4
    ms = statistics.median(stats_ms)
    result = {
        "shape": {"layers": LAYERS, "B": B, "T_q": TQ, "T_k": TK, "frames": n_frames.tolist(), "keys": n_keys.tolist(), "sigma": SIGMA},
        "timing": "device events around hipGraph replays, alternated with the restatements",
        "align_stats_ms": dict(stats(stats_ms), replays_per_repeat=args.replays, repeats=args.repeats),
        "align_stats_bytes_read": nbytes, "align_stats_GBps_of_bytes_read": round(nbytes / (ms * 1e-3) / 1e9, 1),
        "align_stats_GBps_of_the_37.7MB_matrices": round(full / (ms * 1e-3) / 1e9, 1),
        "xattn_probs_mean_GBps_same_shape": 1500.0,
        "align_mas_ms": dict(stats(mas_ms), dependent_steps=int(n_frames.max()),
                             next_to="rtts_dtw_align's recurrence: 0.488 ms for 2288 dependent steps (profiles/dtw_bench.json)"),
        "torch_stats_restatement_ms": dict(stats(torch_ms), what="float64 masked reductions on the device, sums and arg-max only"),
        "numpy_mas_ms_one_search": stats(numpy_ms), "numpy_mas_ms_scaled_to_36_searches": round(statistics.median(numpy_ms) * LAYERS * B, 1),
        "max_relative_difference_of_the_sums_vs_torch": rel, "durations_equal_numpy": same_dur,
        "q_difference_vs_numpy": abs(float(got_mas[2][1, 0, 0]) - float(want_q)),
    }
    if not args.no_validate:
        result["validate"] = validate_case(args.repeats)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
