#!/usr/bin/env python3
"""Incremental against windowed generation on one MI355X: the config/baseline.yml shape with dense attention on both stacks
(3 + 3 layers, d 512, ``use_full_attn``), random weights, stop tokens ignored, ``--frames`` frames, B in {1, 12}.

    python scripts/incremental_infer_bench.py > profiles/incremental_infer_bench.json

  windowed      ``infer(use_graph=True, cache_encoder=True)``: one hipGraph replay of the decoder over the padded window per frame
  incremental   ``infer(incremental=True, use_graph=True)``: one replay of ONE captured single-row step per frame
  kernels       ``rtts_decode_self_attn`` / ``rtts_decode_cross_attn`` alone at p = frames - 1 (device events around ``--launches``
                back-to-back launches, so launch gaps count), with the bytes one launch has to read and their share of the 8 TB/s
                HBM peak

The two paths alternate round by round in one process (host clock around the call and a synchronise; the first call of each, with
its captures, is reported apart).  The paths do not generate the same frames (the postnet of the incremental path sees the sequence
end at the newest frame); both generate ``--frames`` of them.  Medians and ranges are written down.  No threshold."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import ops  # noqa: E402
from reformer_tts_amd.model.config import model_config_from_dict  # noqa: E402
from reformer_tts_amd.training import build_model  # noqa: E402

HBM_PEAK = 8.0e12


def stat(v, unit, nd=4):
    return {f"median_{unit}": round(statistics.median(v), nd), f"min_{unit}": round(min(v), nd), f"max_{unit}": round(max(v), nd), "rounds": len(v)}


def dense_baseline():
    dense = dict(implementation="hip", use_full_attn=True)
    return model_config_from_dict(dict(
        dict_size=76, num_mel_coeffs=80, scp_encoding_dropout=0.05, pad_base=256,
        enc_prenet_kwargs=dict(dropout=0.05), dec_prenet_kwargs=dict(dropout=0.05),
        enc_reformer_kwargs=dict(depth=3, attn_kwargs=dict(dense)),
        dec_reformer_kwargs=dict(depth=3, self_attn_kwargs=dict(dense, bucket_size=128)),
        postnet_kwargs=dict(depth=2, dropout=0.1)))


def launches_us(fn, n):
    for _ in range(10):
        fn()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 12])
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--text", type=int, default=150)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = build_model(dense_baseline(), dev, seed=42)
    d, heads = 512, 8
    out = {"what": "windowed against incremental generation, dense baseline shape (see the script's docstring); rounds alternate in one process",
           "device": torch.cuda.get_device_name(0), "frames": args.frames, "batches": {}}
    for b in args.batches:
        ph = torch.randint(1, 77, (b, args.text), generator=torch.Generator().manual_seed(b)).to(dev)
        paths = {"windowed": dict(use_graph=True, cache_encoder=True), "incremental": dict(use_graph=True, incremental=True)}

        def call(kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            spec, _ = model.infer(ph, max_len=args.frames, stop_at_stop_token=False, **kw)
            torch.cuda.synchronize()
            assert spec.shape[2] == args.frames
            return (time.perf_counter() - t0) * 1e3

        first = {n: call(kw) for n, kw in paths.items()}                 # captures happen here
        ms = {n: [] for n in paths}
        for _ in range(args.rounds):
            for n, kw in paths.items():
                ms[n].append(call(kw) / args.frames)
        res = {n: dict(per_frame=stat(v, "ms"), first_call_with_captures_ms=round(first[n], 1)) for n, v in ms.items()}
        res["windowed_over_incremental"] = round(statistics.median(ms["windowed"]) / statistics.median(ms["incremental"]), 2)
        # the two single-query kernels alone at the last position
        cap, tk, p = -(-args.frames // 64) * 64, -(-args.text // 256) * 256, args.frames - 1
        g = torch.Generator().manual_seed(3)
        cache = torch.randn(b, cap, 2 * d, generator=g).bfloat16().to(dev)
        row = torch.randn(128, 2 * d, generator=g).bfloat16().to(dev)
        kv = torch.randn(b, tk, 2 * d, generator=g).bfloat16().to(dev)
        pos = torch.tensor([p], dtype=torch.int32, device=dev)
        o = torch.zeros(128, d, dtype=torch.bfloat16, device=dev)
        kern = {}
        for name, t, nbytes, fn in (
                ("rtts_decode_self_attn", cap, b * p * 2 * d * 2, lambda ws, s: ops.decode_self_attn(row, cache, pos, heads, splits=s, out=o, workspace=ws, batch=b)),
                ("rtts_decode_cross_attn", tk, b * tk * 2 * d * 2, lambda ws, s: ops.decode_cross_attn(row[:, :d], kv, heads, None, splits=s, out=o, workspace=ws, batch=b))):
            s = ops.decode_attn_splits(b * heads, t)
            ws = torch.empty(b * heads * s * (64 + 4), dtype=torch.float32, device=dev)
            us = launches_us(lambda: fn(ws, s), args.launches)
            kern[name] = dict(us_per_call=round(us, 2), splits=s, bytes_read=nbytes, gb_per_s=round(nbytes / us * 1e-3, 1),
                              share_of_hbm_peak=round(nbytes / (us * 1e-6) / HBM_PEAK, 4))
        res["kernels_at_last_position"] = kern
        out["batches"][str(b)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
