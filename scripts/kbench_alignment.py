#!/usr/bin/env python3
"""Attention alignments on the eval path (GPU box only): us per launch of rtts_xattn_probs_mean and its achieved bytes per second,
the general eval path's ATen sequence for the same matrices, and Trainer.validate with and without return_attention at the
baseline configuration.  HIP events; medians of several timed regions.
RTTS_LIB=<alternative build> python scripts/kbench_alignment.py   # A/B against another build on the same box
--dh 128: the kernel cases with 128-wide heads at the same model width (half the heads)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reformer_tts_amd import _lib, engine  # noqa: E402
from reformer_tts_amd._seeds import seed_base  # noqa: E402

dev = torch.device("cuda:0")
s = torch.cuda.current_stream().cuda_stream


def timed(fn, reps=50, regions=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        z.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(z) / reps * 1e3)
    return statistics.median(out)


def kernel_case(b, h, t, tk, valid_keys, dh=64):
    e = dh * h
    g = torch.Generator().manual_seed(0)
    q = torch.randn(b * t, e, generator=g).bfloat16().to(dev)
    kv = torch.randn(b * tk, 2 * e, generator=g).bfloat16().to(dev)
    kvalid = torch.ones(b, tk, dtype=torch.uint8, device=dev)
    kvalid[:, valid_keys:] = 0
    o = torch.empty(b * t, e, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(b * h, t, dtype=torch.float32, device=dev)
    a = torch.empty(b, t, tk, dtype=torch.float32, device=dev)

    def fwd():
        _lib.call("rtts_xattn_fwd", q.data_ptr(), e, kv.data_ptr(), 2 * e, kvalid.data_ptr(), b, h, t, tk, dh, o.data_ptr(), e,
                  lse.data_ptr(), 0.0, 0, seed_base(dev).data_ptr(), s)

    fwd_us = timed(fwd)
    us = timed(lambda: engine.xattn_probs_mean(q, kv, kvalid, lse, b, h, t, tk, out=a))
    # bytes that must cross HBM once: a (fp32) out; q, the k half of kv, lse, kvalid in
    nbytes = a.numel() * 4 + q.numel() * 2 + b * tk * e * 2 + lse.numel() * 4 + kvalid.numel()

    def aten():                                    # model/reformer.py's general eval path for the same matrices
        qh = q.view(b, t, h, dh).transpose(1, 2)
        kh = kv[:, :e].view(b, tk, h, dh).transpose(1, 2)
        sc = (qh.float() * dh ** -0.5) @ kh.float().transpose(-1, -2)
        sc = sc.masked_fill(~kvalid.bool()[:, None, None, :], float("-inf"))
        return torch.softmax(sc, dim=-1).mean(dim=1)

    aten_us = timed(aten, reps=10)
    err = float((aten() - a).abs().max())
    print(f"B={b} H={h} dh={dh} Tq={t} Tk={tk}: probs_mean {us:8.1f} us  {nbytes / us / 1e3:7.1f} GB/s ({nbytes / 1e6:.1f} MB)   "
          f"xattn_fwd {fwd_us:7.1f} us   ATen general path {aten_us:8.1f} us   max |HIP - ATen| {err:.1e}", flush=True)


def validate_case(b=12, text=256, mel=1024):
    from reformer_tts_amd.model.config import baseline_model_config, baseline_training_config
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    model = build_model(baseline_model_config(), dev, seed=42)
    tcfg = baseline_training_config()
    tcfg.batch_size = b
    tr = Trainer(model, tcfg, dev)
    batch = synthetic_batch(b, text, mel, seed=42, device=dev)
    plain = timed(lambda: tr.validate(batch), reps=10)
    full = timed(lambda: tr.validate(batch, return_attention=True), reps=10)
    print(f"validate B={b} text={text} mel={mel}: {plain / 1e3:7.2f} ms   return_attention=True {full / 1e3:7.2f} ms   "
          f"(+{(full - plain) / 1e3:.2f} ms, {model.dec.reformer.depth} decoder layers)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dh", type=int, default=64, choices=(64, 128), help="head width of the kernel cases; the model width stays 512")
    dh = ap.parse_args().dh
    kernel_case(12, 512 // dh, 1024, 256, 200, dh)
    kernel_case(12, 512 // dh, 4096, 256, 200, dh)
    kernel_case(12, 512 // dh, 4096, 512, 400, dh)
    validate_case()
