#!/usr/bin/env python3
"""``rtts_dtw_align`` (MCD-DTW, ``evaluation.mel_cepstral_distortion``) on one MI355X at the validation shape of
scripts/infer_validation_bench.py: B = 12, the same twelve truths of 670-1020 frames (same generator, same seed), 1024 generated
frames that never stop, 80 mels, 13 cepstral coefficients.

    python scripts/dtw_bench.py > profiles/dtw_bench.json

  call           device events around one ``ops.dtw_align`` (four kernels), workspace allocated before the clock starts
  phases         the same entry point restricted to ONE of its kernels (project, distances, recurrence, fold) on the buffers a full
                 call left behind: device events around each
  torch loop     the same recurrence -- same distances, same tie-break order, f64 -- as a torch loop over the anti-diagonals on the
                 device, all slots at once (about ten small launches per diagonal); the distance table is built before its clock starts
  numpy          the same recurrence as a float64 numpy loop over the anti-diagonals on the host, slot after slot, host clock

Rounds of the call and its phases are interleaved in one process; the two loops are slower by orders of magnitude and get fewer
rounds.  Medians and ranges are written down, and the call as a share of the generation it scores
(profiles/infer_validation_bench.json).  No threshold."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from reformer_tts_amd import _lib, evaluation, ops  # noqa: E402

PHASES = (("project", 1), ("distances", 2), ("recurrence", 4), ("fold", 8))


def stat(v, unit):
    return {f"median_{unit}": round(statistics.median(v), 3), f"min_{unit}": round(min(v), 3), f"max_{unit}": round(max(v), 3), "rounds": len(v)}


def torch_recurrence(skewed, n_len, m_len):
    """skewed (B, N + M - 1, N) f64 with skewed[b, k, i] = d_b(i, k - i), +inf where no such cell -> (cost (B,), steps (B,))."""
    b, diagonals, n = skewed.shape
    inf = torch.full((b, n + 1), float("inf"), dtype=torch.float64, device=skewed.device)
    zero = torch.zeros((b, n + 1), dtype=torch.int64, device=skewed.device)
    prev2_d, prev2_s = inf, zero
    prev1_d, prev1_s = inf.clone(), zero.clone()
    prev1_d[:, 1], prev1_s[:, 1] = skewed[:, 0, 0], 1
    last = (n_len + m_len - 2).view(b, 1)
    at = n_len.view(b, 1)
    cost, steps = prev1_d.gather(1, at), prev1_s.gather(1, at)        # slots of one cell end on diagonal 0
    for k in range(1, diagonals):
        best, s = prev2_d[:, :-1], prev2_s[:, :-1]                      # diagonal, then above, then left: strict < replaces
        up = prev1_d[:, :-1] < best
        best, s = torch.where(up, prev1_d[:, :-1], best), torch.where(up, prev1_s[:, :-1], s)
        left = prev1_d[:, 1:] < best
        best, s = torch.where(left, prev1_d[:, 1:], best), torch.where(left, prev1_s[:, 1:], s)
        cur_d, cur_s = inf.clone(), zero.clone()
        cur_d[:, 1:], cur_s[:, 1:] = best + skewed[:, k], s + 1
        done = last == k
        cost, steps = torch.where(done, cur_d.gather(1, at), cost), torch.where(done, cur_s.gather(1, at), steps)
        prev2_d, prev2_s, prev1_d, prev1_s = prev1_d, prev1_s, cur_d, cur_s
    return cost.view(b), steps.view(b)


def numpy_recurrence(d):
    """d (N, M) f64 -> (cost, steps): the recurrence by anti-diagonals on the host."""
    n, m = d.shape
    dp = np.full((n + 1, m + 1), np.inf)
    sp = np.zeros((n + 1, m + 1), dtype=np.int64)
    dp[1, 1], sp[1, 1] = d[0, 0], 1
    for k in range(1, n + m - 1):
        i = np.arange(max(0, k - m + 1), min(n - 1, k) + 1)
        j = k - i
        best, s = dp[i, j].copy(), sp[i, j].copy()
        for cd, cs in ((dp[i, j + 1], sp[i, j + 1]), (dp[i + 1, j], sp[i + 1, j])):
            take = cd < best
            best[take], s[take] = cd[take], cs[take]
        dp[i + 1, j + 1], sp[i + 1, j + 1] = best + d[i, j], s + 1
    return float(dp[n, m]), int(sp[n, m])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--generation-ms", type=float, default=None, help="default: profiles/infer_validation_bench.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    truths = []
    for _ in range(args.batch):                                 # the draws of scripts/infer_validation_bench.py, in its order
        lm, lp = int(torch.randint(600, 1025, (1,), generator=g)), int(torch.randint(50, 201, (1,), generator=g))
        torch.randint(1, 77, (lp,), generator=g)
        truths.append((torch.randn(lm, 80, generator=g) * 2 - 5).clamp(-11.5, 2.0).t().contiguous())
    lens = [t.shape[1] for t in truths]
    lm, frames, b = max(lens), args.max_len, args.batch
    gen = (torch.randn(b, 80, frames, generator=g) * 2 - 5).clamp(-11.5, 2.0).to(dev)
    stop = torch.full((b,), frames, dtype=torch.int64, device=dev)
    truth = torch.cat(truths, dim=1).to(dev)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    fo = torch.tensor(offsets, dtype=torch.int64).to(dev)
    ids = torch.arange(b, dtype=torch.int32, device=dev)
    basis = evaluation.cepstral_basis(80, 13, dev)
    need = int(_lib.load().rtts_dtw_workspace_bytes(b, frames, lm, 13))
    out = torch.empty(b + 2, dtype=torch.float64, device=dev)
    state = (torch.empty(need, dtype=torch.uint8, device=dev), out[:b], torch.empty(b, dtype=torch.int32, device=dev), out[b:])

    def kernel(phases=ops.DTW_ALL):
        return ops.dtw_align(gen, stop, truth, lm, basis=basis, frame_offsets=fo, ids=ids, _phases=phases, _state=state)

    def events(fn):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) * 1e3

    for _ in range(5):
        kernel()
    us = {"call": [], **{name: [] for name, _ in PHASES}}
    for _ in range(args.rounds):
        us["call"].append(events(kernel))
        for name, bit in PHASES:
            us[name].append(events(lambda: kernel(bit)))
    cost, steps, totals = [t.cpu() for t in kernel()]

    # the two loops, on the distances of the same projected frames (f32 distances widened, as the kernel's recurrence reads them)
    proj_g = (gen.double().transpose(1, 2) @ basis.double().t()).float()                  # (B, L, 13)
    proj_t = (truth.double().t() @ basis.double().t()).float()                            # (frames, 13)
    n_len, m_len = stop.clone(), torch.tensor(lens, dtype=torch.int64, device=dev)
    skewed = torch.full((b, frames + lm - 1, frames), float("inf"), dtype=torch.float64, device=dev)
    dists = []
    for s in range(b):
        d = (proj_g[s][:, None, :] - proj_t[offsets[s]:offsets[s + 1]][None, :, :]).pow(2).sum(-1).sqrt().double()    # (N, M)
        dists.append(d.cpu().numpy())
        i = torch.arange(frames, device=dev)[:, None].expand(frames, lens[s])
        j = torch.arange(lens[s], device=dev)[None, :].expand(frames, lens[s])
        skewed[s, (i + j).reshape(-1), i.reshape(-1)] = d.reshape(-1)
    torch_recurrence(skewed[:, :64], n_len, m_len)                                        # warm the allocator
    loop_ms, host_ms = [], []
    for _ in range(args.loop_rounds):
        loop_ms.append(events(lambda: torch_recurrence(skewed, n_len, m_len)) * 1e-3)
    t_cost, t_steps = [t.cpu() for t in torch_recurrence(skewed, n_len, m_len)]
    for _ in range(max(1, args.loop_rounds // 3)):
        t0 = time.perf_counter()
        host = [numpy_recurrence(d) for d in dists]
        host_ms.append((time.perf_counter() - t0) * 1e3)

    generation_ms = args.generation_ms
    if generation_ms is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "infer_validation_bench.json")
        generation_ms = json.load(open(path))["generation"]["median_ms"]
    med = {n: statistics.median(v) for n, v in us.items()}
    print(json.dumps({
        "what": "rtts_dtw_align (MCD-DTW) at the validation shape of scripts/infer_validation_bench.py, its four kernels one by one, and the "
                "same recurrence as a torch anti-diagonal loop on the device and as numpy on the host (see the script's docstring)",
        "device": torch.cuda.get_device_name(0), "batch": b, "mel_lengths": sorted(lens), "lm": lm, "generated_frames": frames, "n_mel": 80,
        "n_coef": 13, "workspace_mb": round(need / 2 ** 20, 1), "cells": int(sum(frames * m for m in lens)),
        "device_us": {n: stat(v, "us") for n, v in us.items()},
        "phases_sum_over_call": round(sum(med[n] for n, _ in PHASES) / med["call"], 3),
        "torch_antidiagonal_loop_device": stat(loop_ms, "ms"), "numpy_host": stat(host_ms, "ms"),
        "torch_loop_over_recurrence_kernel": round(statistics.median(loop_ms) * 1e3 / med["recurrence"], 1),
        "numpy_over_recurrence_kernel": round(statistics.median(host_ms) * 1e3 / med["recurrence"], 1),
        "generation_ms": generation_ms, "call_share_of_generation": round(med["call"] * 1e-3 / generation_ms, 6),
        "values": {"mcd_db_mean": float(totals[0]), "mcd_db_pooled": float(totals[1]), "steps": steps.tolist(),
                   "cost_max_rel_diff_torch_loop": float(((cost - t_cost).abs() / t_cost).max()),
                   "steps_equal_torch_loop": bool(torch.equal(steps.long(), t_steps)),
                   "cost_max_rel_diff_numpy": float(max(abs(c - h[0]) / h[0] for c, h in zip(cost.tolist(), host))),
                   "steps_equal_numpy": steps.tolist() == [h[1] for h in host]}}))


if __name__ == "__main__":
    main()
