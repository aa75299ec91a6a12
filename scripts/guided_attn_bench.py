#!/usr/bin/env python3
"""What the guided attention loss costs, measured (GPU box only) -> profiles/guided_attn_bench.json.

1. Kernels: the unguided backward chain (rtts_lsh_bwd_delta, rtts_xattn_bwd, rtts_sum_slabs) against the guided one (the same
   with rtts_xattn_guide_rows + rtts_xattn_guide_fold in front of rtts_xattn_bwd_guided) at B 12, T_q 1024, T_k 256, width 512, as
   dh 64 / H 8 and dh 128 / H 4.  Each chain is captured into a hipGraph of ``--launches`` launches; the two replay alternately
   for ``--rounds`` rounds (HIP events around each replay).
2. Training step: the eager config/baseline.yml step (3 + 3 layers, B 12, 1024 mel frames, 256 phonemes) on two trainers over the
   same model built twice, ``guided_attention_weight`` 0 and 1, alternating in one process.

No time is fixed anywhere: the comparison is the unguided chain of the same build in the same process.

usage: python scripts/guided_attn_bench.py [--out profiles/guided_attn_bench.json]"""
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


def kernel_graphs(dh, launches, b=12, t=1024, tk=256, e=512, sigma=0.2):
    h = e // dh
    g = torch.Generator().manual_seed(0)
    q = torch.randn(b * t, e, generator=g).bfloat16().to(dev)
    kv = torch.randn(b * tk, 2 * e, generator=g).bfloat16().to(dev)
    do = torch.randn(b * t, e, generator=g).bfloat16().to(dev)
    kvalid = torch.ones(b, tk, dtype=torch.uint8, device=dev)
    kvalid[:, 200:] = 0
    n_frames = torch.tensor([t - 37 * i for i in range(b)], dtype=torch.int32, device=dev)
    n_keys = torch.full((b,), 200, dtype=torch.int32, device=dev)
    o = torch.empty(b * t, e, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(b * h, t, dtype=torch.float32, device=dev)
    delta = torch.empty(b * h, t, dtype=torch.float32, device=dev)
    rows = torch.empty(b * h, t, dtype=torch.float32, device=dev)
    out = torch.empty(b + 1, dtype=torch.float64, device=dev)
    c = torch.empty(1, dtype=torch.float32, device=dev)
    dq = torch.empty(b * t, e, dtype=torch.bfloat16, device=dev)
    part = torch.empty(t // 128, b * tk, 2 * e, dtype=torch.bfloat16, device=dev)
    dkv = torch.empty(b * tk, 2 * e, dtype=torch.bfloat16, device=dev)
    nkc = _lib.load().rtts_xattn_bwd_key_chunks(tk, dh)
    ws = torch.empty(nkc, b * t, e, dtype=torch.bfloat16, device=dev) if nkc > 1 else None
    sb = seed_base(dev)
    keep = (q, kv, do, kvalid, n_frames, n_keys, o, lse, delta, rows, out, c, dq, part, dkv, ws, sb)
    _lib.call("rtts_xattn_fwd", q.data_ptr(), e, kv.data_ptr(), 2 * e, kvalid.data_ptr(), b, h, t, tk, dh, o.data_ptr(), e, lse.data_ptr(),
              0.0, 0, sb.data_ptr(), torch.cuda.current_stream().cuda_stream)

    def chain(guided):
        s = torch.cuda.current_stream().cuda_stream
        args = (q.data_ptr(), e, kv.data_ptr(), 2 * e, kvalid.data_ptr(), do.data_ptr(), e, lse.data_ptr(), delta.data_ptr(), b, h, t, tk,
                dh, dq.data_ptr(), e, part.data_ptr(), 0.0, 0, sb.data_ptr(), None if ws is None else ws.data_ptr())
        _lib.call("rtts_lsh_bwd_delta", o.data_ptr(), e, do.data_ptr(), e, b, h, t, dh, delta.data_ptr(), s)
        if guided:
            _lib.call("rtts_xattn_guide_rows", q.data_ptr(), e, kv.data_ptr(), 2 * e, kvalid.data_ptr(), lse.data_ptr(), n_frames.data_ptr(),
                      n_keys.data_ptr(), b, h, t, tk, dh, sigma, rows.data_ptr(), s)
            _lib.call("rtts_xattn_guide_fold", rows.data_ptr(), n_frames.data_ptr(), n_keys.data_ptr(), b, h, t, tk, 1.0, out.data_ptr(),
                      c.data_ptr(), s)
            _lib.call("rtts_xattn_bwd_guided", *args, rows.data_ptr(), c.data_ptr(), n_frames.data_ptr(), n_keys.data_ptr(), sigma, s)
        else:
            _lib.call("rtts_xattn_bwd", *args, s)
        _lib.call("rtts_sum_slabs", part.data_ptr(), t // 128, dkv.numel(), dkv.data_ptr(), s)

    graphs = {}
    for guided in (False, True):
        chain(guided)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(launches):
                chain(guided)
        gr.replay()
        torch.cuda.synchronize()
        graphs[guided] = gr
    return graphs, keep, float(out[-1])


def bench_kernels(launches, rounds):
    res = {}
    for dh in (64, 128):
        graphs, keep, loss = kernel_graphs(dh, launches)
        us = {False: [], True: []}
        for _ in range(rounds):
            for guided in (False, True):              # interleaved: one replay of each chain per round
                us[guided].append(_event_ms(graphs[guided].replay) / launches * 1e3)
        med = {k: statistics.median(v) for k, v in us.items()}
        res[f"dh{dh}"] = dict(heads=512 // dh, unguided_us_rounds=[round(x, 2) for x in us[False]], guided_us_rounds=[round(x, 2) for x in us[True]],
                              unguided_us_median=round(med[False], 2), guided_us_median=round(med[True], 2),
                              guided_over_unguided=round(med[True] / med[False], 3), guided_loss=round(loss, 6))
        print(f"backward chain dh {dh}: unguided {med[False]:8.1f} us   rows + fold + guided {med[True]:8.1f} us", flush=True)
    return res


def bench_step(steps, rounds, b=12, text=256, mel=1024):
    from reformer_tts_amd.model.config import baseline_model_config, baseline_training_config
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    trainers = {}
    for weight in (0.0, 1.0):                         # a model each (a trainer owns its model's flat storage), the same seed
        tcfg = baseline_training_config()
        tcfg.batch_size = b
        tcfg.guided_attention_weight = weight
        trainers[weight] = Trainer(build_model(baseline_model_config(), dev, seed=42), tcfg, dev)
    batch = synthetic_batch(b, text, mel, seed=42, device=dev)

    def run(weight):
        tr = trainers[weight]
        for _ in range(steps):
            tr.train_step(batch)

    for weight in (0.0, 1.0):                         # warm-up of both
        run(weight)
    torch.cuda.synchronize()
    ms = {0.0: [], 1.0: []}
    for _ in range(rounds):
        for weight in (0.0, 1.0):
            ms[weight].append(_event_ms(lambda: run(weight)) / steps)
    out = dict(weight0_ms_rounds=[round(x, 3) for x in ms[0.0]], weight1_ms_rounds=[round(x, 3) for x in ms[1.0]],
               weight0_ms_median=round(statistics.median(ms[0.0]), 3), weight1_ms_median=round(statistics.median(ms[1.0]), 3),
               guided_attention_loss=round(float(trainers[1.0].guided_attention_loss()), 6),
               shape=dict(B=b, text=text, mel=mel, layers="3+3", mode="eager train_step"))
    print(f"eager baseline training step: weight 0 {out['weight0_ms_median']:.2f} ms   weight 1 {out['weight1_ms_median']:.2f} ms", flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/guided_attn_bench.json")
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    res = dict(tool="scripts/guided_attn_bench.py", device=torch.cuda.get_device_name(0),
               kernels=dict(shape=dict(B=12, Tq=1024, Tk=256, width=512, valid_keys=200), launches_per_graph=args.launches,
                            **bench_kernels(args.launches, args.rounds)),
               training_step=bench_step(args.steps, args.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"wrote {args.out}")
