#!/usr/bin/env python3
"""A/B of the two main loops of the convolutions in csrc/gemm_nt.hip in ONE process on one box (interleaved rounds, medians):
the plain loop, which fetches the input rows once per tap (rtts_debug_set_gemm_mode(21)), against the convolution form (22: the
rows of all channel blocks stay in LDS and serve the five taps; same K order, same bits), at the step's own shapes -- encoder
prenet M = 3328, postnet M = 12544 -- forward with the moments epilogue, forward fp32, and the transposed product (input
gradient), inside a replayed graph.  Where the images do not fit LDS (512 channels on the 256 x 128 tile) both columns time
the plain loop.
    python scripts/conv_taps_ab.py > profiles/conv_taps_ab.log
--once: every launch once, eagerly, on the library's pick -- what a counter pass (rocprofv3 --pmc ... -- python ... --once) wraps."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from reformer_tts_amd import _lib
from reformer_tts_amd._graphs import capturing

dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
LEAD = 8


def timed(fn, calls=20, replays=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with capturing(gr):
        for _ in range(calls):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        gr.replay()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / (calls * replays)        # us per call


def main():
    lib = _lib.load()
    rounds = 5
    # (name, B, L, C_in, C_out): M = B (L + 4) rounded up to 256 as edges.Halo does
    shapes = (("encoder prenet", 12, 256, 512, 512), ("postnet 512->512", 12, 1024, 512, 512), ("postnet 128->512", 12, 1024, 128, 512),
              ("postnet 512->128", 12, 1024, 512, 128))
    for name, b, l, ci, co in shapes:
        m = -(-(b * (l + 4)) // 256) * 256
        x = (torch.randn(m + 2 * LEAD, ci, device=dev, generator=g)).bfloat16()
        dy = (torch.randn(m + 2 * LEAD, co, device=dev, generator=g) / 8).bfloat16()
        wp = (torch.randn(co, 5 * ci, device=dev, generator=g) * (5 * ci) ** -0.5).bfloat16()
        y = torch.empty(m, co, dtype=torch.float32, device=dev)
        dx = torch.empty(m, ci, dtype=torch.bfloat16, device=dev)
        nrows = lib.rtts_gemm_nt_partial_rows(m, co)
        partial = torch.empty(max(nrows, 1), 2 * co, dtype=torch.float32, device=dev)
        s = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

        def fwd_moments():
            _lib.call("rtts_conv1d_k5_moments", x[LEAD:].data_ptr(), ci, wp.data_ptr(), 5 * ci, m, co, ci, y.data_ptr(), co, b, l, 2,
                      partial.data_ptr(), s())

        def fwd():
            _lib.call("rtts_conv1d_k5", x[LEAD:].data_ptr(), ci, wp.data_ptr(), 5 * ci, 0, m, co, ci, y.data_ptr(), co, None, 1, s())

        def dgrad():
            _lib.call("rtts_conv1d_k5", dy[LEAD:].data_ptr(), co, wp.data_ptr(), 5 * ci, 1, m, ci, co, dx.data_ptr(), ci, None, 0, s())

        if "--once" in sys.argv:
            for fn in (fwd_moments, fwd, dgrad):
                fn()
            torch.cuda.synchronize()
            continue
        for kind, fn in (("forward + moments", fwd_moments), ("forward fp32", fwd), ("input gradient", dgrad)):
            res = {21: [], 22: []}
            for _ in range(rounds):
                for mode in (21, 22):
                    _lib.call("rtts_debug_set_gemm_mode", mode)
                    try:
                        res[mode].append(timed(fn))
                    finally:
                        _lib.call("rtts_debug_set_gemm_mode", 20)
            flop = 2.0 * m * co * 5 * ci
            print(f"{name:17s} M={m:5d} {kind:17s}: " + "  ".join(
                f"{'per tap' if k == 21 else 'resident':9s} {statistics.median(v):6.1f} us (min {min(v):6.1f}, max {max(v):6.1f}) "
                f"{flop / statistics.median(v) / 1e6:4.0f} TF" for k, v in res.items()), flush=True)


if __name__ == "__main__":
    main()
