#!/usr/bin/env python3
"""Cross-attention with 128-wide heads, measured (GPU box only) -> profiles/xattn_dh128_bench.json.

1. Kernels: rtts_xattn_fwd and the backward chain (rtts_lsh_bwd_delta, rtts_xattn_bwd with its dq-chunk sum, rtts_sum_slabs) at
   B 12, T_q 1024, T_k 256, width 512, as dh 128 / H 4 and as dh 64 / H 8 (the same FLOPs).  Each is captured into a hipGraph of
   ``--launches`` launches; the two widths replay alternately for ``--rounds`` rounds (HIP events around each replay).
2. Training step: a 3 + 3-layer model with ``num_heads: 4`` (config/legacy/attention-depth-3-heads-4.yml of the reference) at
   B 12, 1024 mel frames, 256 phonemes: Trainer.train_step with the decoder on the explicit executor and, in the same process
   and on the same model, with the decoder's executor switched off (``use_fused = False``: the general eager path), alternating.

usage: python scripts/bench_xattn_dh128.py [--out profiles/xattn_dh128_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import _lib  # noqa: E402
from reformer_tts_amd._seeds import seed_base  # noqa: E402

dev = torch.device("cuda:0")


def _event_ms(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z)


def kernel_graphs(dh, launches, b=12, t=1024, tk=256, e=512):
    h = e // dh
    g = torch.Generator().manual_seed(0)
    q = torch.randn(b * t, e, generator=g).bfloat16().to(dev)
    kv = torch.randn(b * tk, 2 * e, generator=g).bfloat16().to(dev)
    do = torch.randn(b * t, e, generator=g).bfloat16().to(dev)
    kvalid = torch.ones(b, tk, dtype=torch.uint8, device=dev)
    kvalid[:, 200:] = 0
    o = torch.empty(b * t, e, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(b * h, t, dtype=torch.float32, device=dev)
    delta = torch.empty(b * h, t, dtype=torch.float32, device=dev)
    dq = torch.empty(b * t, e, dtype=torch.bfloat16, device=dev)
    part = torch.empty(t // 128, b * tk, 2 * e, dtype=torch.bfloat16, device=dev)
    dkv = torch.empty(b * tk, 2 * e, dtype=torch.bfloat16, device=dev)
    nkc = _lib.load().rtts_xattn_bwd_key_chunks(tk, dh)
    ws = torch.empty(nkc, b * t, e, dtype=torch.bfloat16, device=dev) if nkc > 1 else None
    sb = seed_base(dev)
    keep = (q, kv, do, kvalid, o, lse, delta, dq, part, dkv, ws, sb)

    def fwd():
        s = torch.cuda.current_stream().cuda_stream
        _lib.call("rtts_xattn_fwd", q.data_ptr(), e, kv.data_ptr(), 2 * e, kvalid.data_ptr(), b, h, t, tk, dh, o.data_ptr(), e,
                  lse.data_ptr(), 0.0, 0, sb.data_ptr(), s)

    def bwd():
        s = torch.cuda.current_stream().cuda_stream
        _lib.call("rtts_lsh_bwd_delta", o.data_ptr(), e, do.data_ptr(), e, b, h, t, dh, delta.data_ptr(), s)
        _lib.call("rtts_xattn_bwd", q.data_ptr(), e, kv.data_ptr(), 2 * e, kvalid.data_ptr(), do.data_ptr(), e, lse.data_ptr(),
                  delta.data_ptr(), b, h, t, tk, dh, dq.data_ptr(), e, part.data_ptr(), 0.0, 0, sb.data_ptr(),
                  None if ws is None else ws.data_ptr(), s)
        _lib.call("rtts_sum_slabs", part.data_ptr(), t // 128, dkv.numel(), dkv.data_ptr(), s)

    graphs = {}
    for name, fn in (("fwd", fwd), ("bwd_chain", bwd)):
        fwd()
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(launches):
                fn()
        gr.replay()
        torch.cuda.synchronize()
        graphs[name] = gr
    # 4 T_q T_k dh FLOPs per head for the forward's two products, 10 for the backward's five
    flops = dict(fwd=4.0 * b * h * t * tk * dh, bwd_chain=10.0 * b * h * t * tk * dh)
    return graphs, flops, keep, nkc


def bench_kernels(launches, rounds):
    sets = {dh: kernel_graphs(dh, launches) for dh in (128, 64)}
    out = {}
    for name in ("fwd", "bwd_chain"):
        us = {128: [], 64: []}
        for _ in range(rounds):
            for dh in (128, 64):                      # interleaved: one replay of each width per round
                us[dh].append(_event_ms(sets[dh][0][name].replay) / launches * 1e3)
        for dh in (128, 64):
            med = statistics.median(us[dh])
            out[f"{name}_dh{dh}"] = dict(us_per_launch_rounds=[round(x, 2) for x in us[dh]], us_median=round(med, 2),
                                         tflops=round(sets[dh][1][name] / med / 1e6, 1), heads=512 // dh,
                                         bwd_key_chunks=sets[dh][3])
        print(f"{name}: dh 128 / H 4 {out[name + '_dh128']['us_median']:8.1f} us    dh 64 / H 8 {out[name + '_dh64']['us_median']:8.1f} us", flush=True)
    return out


def bench_step(steps, rounds, b=12, text=256, mel=1024):
    from reformer_tts_amd.model.config import baseline_model_config, baseline_training_config
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    cfg = baseline_model_config()
    assert cfg.enc_reformer_kwargs.depth == cfg.dec_reformer_kwargs.depth == 3
    cfg.dec_reformer_kwargs.attn_kwargs.num_heads = 4
    model = build_model(cfg, dev, seed=42)
    tcfg = baseline_training_config()
    tcfg.batch_size = b
    tr = Trainer(model, tcfg, dev)
    batch = synthetic_batch(b, text, mel, seed=42, device=dev)
    dec = model.dec.reformer.layers

    def run(fused):
        dec.use_fused = fused
        for _ in range(steps):
            tr.train_step(batch)

    before = len(_lib.PATHS_LEFT)
    for fused in (True, False):                       # warm-up of both paths
        run(fused)
    torch.cuda.synchronize()
    assert dec._program is not None, "the decoder stack got no program"
    ms = {True: [], False: []}
    for _ in range(rounds):
        for fused in (True, False):
            ms[fused].append(_event_ms(lambda: run(fused)) / steps)
    dec.use_fused = True
    out = dict(executor_ms_rounds=[round(x, 3) for x in ms[True]], general_decoder_ms_rounds=[round(x, 3) for x in ms[False]],
               executor_ms_median=round(statistics.median(ms[True]), 3), general_decoder_ms_median=round(statistics.median(ms[False]), 3),
               notes_of_a_general_path=[list(p) for p in _lib.PATHS_LEFT[before:]], shape=dict(B=b, text=text, mel=mel, layers="3+3", num_heads=4))
    print(f"training step 3+3 layers, num_heads 4: executor {out['executor_ms_median']:.2f} ms   decoder on the general path "
          f"{out['general_decoder_ms_median']:.2f} ms", flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/xattn_dh128_bench.json")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    res = dict(tool="scripts/bench_xattn_dh128.py", device=torch.cuda.get_device_name(0),
               kernels=dict(shape=dict(B=12, Tq=1024, Tk=256, width=512, valid_keys=200), launches_per_graph=args.launches,
                            **bench_kernels(args.launches, args.rounds)),
               training_step=bench_step(args.steps, args.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"wrote {args.out}")
