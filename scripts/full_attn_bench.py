#!/usr/bin/env python3
"""Dense shared-QK attention against the LSH chain it replaces, measured (GPU box only) -> profiles/full_attn_bench.json.

1. Kernels, at the encoder shape (B 12, H 8, T 256, bucket 64) and the decoder shape (T 1024, bucket 128, causal), 8 hash rounds:
     forward : rtts_full_attn_fwd                       against  rtts_lsh_hash_sort + rtts_lsh_attn_fwd + rtts_lsh_combine_fwd
     backward: rtts_lsh_bwd_delta + rtts_full_attn_bwd  against  rtts_lsh_bwd_delta + rtts_lsh_attn_bwd + rtts_lsh_bwd_reduce
   Each side is captured into a hipGraph of ``--launches`` repetitions; the two sides replay alternately for ``--rounds`` rounds
   in one process (HIP events around each replay), the median round is reported.
2. Training step: config/baseline.yml (3 + 3 layers, B 12, 256 phonemes, 1024 frames), Trainer.train_step with ``use_full_attn``
   off / on the encoder / on both stacks, three models in one process, alternating.

usage: python scripts/full_attn_bench.py [--out profiles/full_attn_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = dict(encoder=dict(b=12, h=8, t=256, bucket=64, causal=False), decoder=dict(b=12, h=8, t=1024, bucket=128, causal=True))
N_HASHES = 8


def _event_ms(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z)


def _graph(fn, launches):
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(launches):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def kernel_graphs(b, h, t, bucket, causal, launches):
    e = h * 64
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(b, t, 2 * e, generator=g).bfloat16().to(dev)
    qk, v = qkv[..., :e], qkv[..., e:]
    dout = torch.randn(b, t, e, generator=g).bfloat16().to(dev)
    mask = torch.ones(b, t, dtype=torch.uint8, device=dev)
    for i in range(b):
        mask[i, t - 11 * i:] = 0                                 # ragged tails, as a collated batch has
    rot = torch.randn(1, 64, N_HASHES, t // bucket // 2, generator=g).to(dev)
    dqkv = torch.empty_like(qkv)
    dq = (dqkv[..., :e], dqkv[..., e:])
    st, _, _ = ops.lsh_hash_sort(qk, rot, h, bucket)
    o, lse = ops.lsh_attn_fwd(qk, v, st, h, bucket, causal, mask)
    out_l, lse_l = ops.lsh_combine_fwd(o, lse, b, h)
    out_d, lse_d = ops.full_attn_fwd(qk, v, h, causal, mask)
    keep = [qkv, dout, mask, rot, dqkv, st, out_l, lse_l, out_d, lse_d]

    def lsh_fwd():
        st_, _, _ = ops.lsh_hash_sort(qk, rot, h, bucket)
        o_, lse_ = ops.lsh_attn_fwd(qk, v, st_, h, bucket, causal, mask)
        ops.lsh_combine_fwd(o_, lse_, b, h)

    graphs = dict(
        fwd_dense=_graph(lambda: ops.full_attn_fwd(qk, v, h, causal, mask, out=out_d), launches),
        fwd_lsh=_graph(lsh_fwd, launches),
        bwd_dense=_graph(lambda: ops.full_attn_bwd(qk, v, out_d, dout, lse_d, h, causal, mask, dqkv=dq), launches),
        bwd_lsh=_graph(lambda: ops.lsh_attn_bwd(qk, v, st, out_l, dout, lse_l, h, bucket, causal, mask, dqkv=dq), launches))
    bh = b * h
    # MFMA FLOP issued: the dense kernels 2 (forward) / 7 (backward) products of 2 T^2 dh per head, the causal ones stop at the
    # diagonal tile; the LSH kernels 2 / 5 products of 2 bucket (2 bucket) dh per chunk, rounds T / bucket chunks per head
    tri = (t // 64 + 1) / (2.0 * (t // 64)) if causal else 1.0
    dense = 2.0 * t * t * 64 * bh * tri
    lsh = 2.0 * bucket * 2 * bucket * 64 * (N_HASHES * t // bucket) * bh
    flops = dict(fwd_dense=2 * dense, bwd_dense=7 * dense, fwd_lsh=2 * lsh, bwd_lsh=5 * lsh)
    return graphs, flops, keep


def bench_kernels(launches, rounds):
    out = {}
    for name, shape in SHAPES.items():
        graphs, flops, keep = kernel_graphs(launches=launches, **shape)
        us = {k: [] for k in graphs}
        for _ in range(rounds):
            for k in graphs:                                  # interleaved: one replay of every graph per round
                us[k].append(_event_ms(graphs[k].replay) / launches * 1e3)
        res = {k: dict(us_per_call_rounds=[round(x, 2) for x in v], us_median=round(statistics.median(v), 2),
                       mfma_tflops=round(flops[k] / statistics.median(v) / 1e6, 1)) for k, v in us.items()}
        res["shape"] = dict(B=shape["b"], H=shape["h"], T=shape["t"], bucket_size=shape["bucket"], n_hashes=N_HASHES, causal=shape["causal"])
        out[name] = res
        print(f"{name}: forward dense {res['fwd_dense']['us_median']:8.1f} us  LSH chain {res['fwd_lsh']['us_median']:8.1f} us   "
              f"backward dense {res['bwd_dense']['us_median']:8.1f} us  LSH chain {res['bwd_lsh']['us_median']:8.1f} us", flush=True)
        del graphs, keep
    return out


def bench_step(steps, rounds, b=12, text=256, mel=1024):
    from reformer_tts_amd.model.config import baseline_model_config, baseline_training_config
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    batch = synthetic_batch(b, text, mel, seed=42, device=dev)
    trainers = {}
    for name, enc, dec in (("lsh", False, False), ("dense_encoder", True, False), ("dense_both", True, True)):
        cfg = baseline_model_config()
        cfg.enc_reformer_kwargs.attn_kwargs.use_full_attn = enc
        cfg.dec_reformer_kwargs.self_attn_kwargs.use_full_attn = dec
        tcfg = baseline_training_config()
        tcfg.batch_size = b
        trainers[name] = Trainer(build_model(cfg, dev, seed=42), tcfg, dev)

    def run(tr):
        for _ in range(steps):
            tr.train_step(batch)

    for tr in trainers.values():                              # warm-up
        run(tr)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for _ in range(rounds):
        for k, tr in trainers.items():
            ms[k].append(_event_ms(lambda: run(tr)) / steps)
    out = {k: dict(ms_rounds=[round(x, 3) for x in v], ms_median=round(statistics.median(v), 3)) for k, v in ms.items()}
    out["shape"] = dict(B=b, text=text, mel=mel, layers="3+3", step="Trainer.train_step (eager)")
    print("training step 3+3 layers: " + "   ".join(f"{k} {v['ms_median']:.2f} ms" for k, v in out.items() if k != "shape"), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/full_attn_bench.json")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    res = dict(tool="scripts/full_attn_bench.py", device=torch.cuda.get_device_name(0), launches_per_graph=args.launches,
               kernels=bench_kernels(args.launches, args.rounds), training_step=bench_step(args.steps, args.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"wrote {args.out}")
