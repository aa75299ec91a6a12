#!/usr/bin/env python3
"""The generating half of a validation epoch on one MI355X: ``Trainer.validate_inference_corpus`` at config/baseline.yml shape
(B = 12, mel lengths 600-1024, random weights).  ``stop_loss_weight`` is set to 0 so that generation ignores the stop tokens
(``wrappers.py:180``) and every run generates ``--max-len`` frames.

    python scripts/infer_validation_bench.py > profiles/infer_validation_bench.json

  whole call     host clock around ``validate_inference_corpus`` and a synchronise: phoneme collate, generation (one hipGraph replay
                 per frame), ``rtts_infer_metrics``
  generation     the call's own ``concat_inference_time`` (host clock around ``infer`` and a synchronise)
  metric launch  ``ops.infer_metrics`` on the generated spectrogram against the packed corpus, INTERLEAVED round by round with the
                 literal torch sequence of ``wrappers.py:188-195`` on the same device tensors (the padded truth, mask and stop
                 indices of ``:170-172`` are built before the clock starts, as the reference builds them): device events around
                 the launches of each, and the host clock around each including the read of its two numbers

Rounds are interleaved in one process; medians and ranges are written down.  No threshold."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch.nn.functional import mse_loss  # noqa: E402

from reformer_tts_amd import ops  # noqa: E402
from reformer_tts_amd.dataset import TTSCorpus  # noqa: E402
from reformer_tts_amd.model.config import baseline_model_config, baseline_training_config  # noqa: E402
from reformer_tts_amd.training import Trainer, build_model  # noqa: E402


def stat(v, unit):
    return {f"median_{unit}": round(statistics.median(v), 3), f"min_{unit}": round(min(v), 3), f"max_{unit}": round(max(v), 3), "rounds": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    items = []
    for _ in range(args.batch):
        lm, lp = int(torch.randint(600, 1025, (1,), generator=g)), int(torch.randint(50, 201, (1,), generator=g))
        items.append(dict(phonemes=torch.randint(1, 77, (lp,), generator=g), spectrogram=(torch.randn(lm, 80, generator=g) * 2 - 5).clamp(-11.5, 2.0)))
    corpus = TTSCorpus.from_items(items, dev)
    tcfg = baseline_training_config()
    tcfg.batch_size, tcfg.lr_scheduler, tcfg.stop_loss_weight = args.batch, None, 0.0
    tr = Trainer(build_model(baseline_model_config(), dev, seed=42), tcfg, dev)
    ids = list(range(args.batch))

    def call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tr.validate_inference_corpus(corpus, ids, max_len=args.max_len, return_outputs=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    first_ms, out = call()                                    # the captures of every padded window happen here
    whole, gen = [], []
    for _ in range(args.calls):
        ms, out = call()
        whole.append(ms)
        gen.append(out["concat_inference_time"] * 1e3)

    mel_out, stop_out = out["spectrogram"], out["stop"]
    lm = max(corpus.frame_lengths)
    dev_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
    batch = corpus.collate(ids)                               # what the torch sequence needs and the kernel does not
    true_mel = batch['spectrogram'][:, 1:, :].transpose(1, 2)
    true_mask = batch["loss_mask"].transpose(1, 2)
    true_stop = batch["stop_tokens"].argmax(dim=1)

    def kernel():
        return ops.infer_metrics(mel_out, stop_out, corpus.mel, lm, frame_offsets=corpus.tables[0], ids=dev_ids, longest=lm)[2]

    def torch_lines():                                        # wrappers.py:188-195 up to the host reads
        padded_mel_out = torch.zeros_like(true_mel)
        common_mel_len = min(padded_mel_out.shape[-1], mel_out.shape[-1])
        padded_mel_out[:, :, :common_mel_len] = mel_out[:, :, :common_mel_len]
        padded_mel_out *= true_mask
        inference_pred_mse = mse_loss(padded_mel_out, true_mel)
        inference_stop_mae = torch.abs(stop_out - true_stop).to(dtype=torch.float).mean()
        return inference_pred_mse, inference_stop_mae

    def events(fn):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) * 1e3

    def host(fn, read):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        read(fn())
        return (time.perf_counter() - t0) * 1e6

    read_kernel = lambda t: t.cpu().tolist()                                          # noqa: E731  one read of both numbers
    read_torch = lambda t: (t[0].cpu().item(), t[1].cpu().item())                     # noqa: E731  the reference's two reads
    for _ in range(5):
        kernel(), torch_lines()
    dev_us = {"rtts_infer_metrics": [], "torch_lines": []}
    host_us = {"rtts_infer_metrics": [], "torch_lines": []}
    for _ in range(args.rounds):
        dev_us["rtts_infer_metrics"].append(events(kernel))
        dev_us["torch_lines"].append(events(torch_lines))
        host_us["rtts_infer_metrics"].append(host(kernel, read_kernel))
        host_us["torch_lines"].append(host(torch_lines, read_torch))
    k, t = kernel().cpu().tolist(), read_torch(torch_lines())
    read_bytes = (min(mel_out.shape[2], lm) * args.batch + sum(corpus.frame_lengths)) * corpus.n_mel * 4
    med = {n: statistics.median(v) for n, v in dev_us.items()}
    print(json.dumps({
        "what": "Trainer.validate_inference_corpus at config/baseline.yml shape and its metric launch next to the torch lines of the "
                "reference's validate_inference (see the script's docstring); rounds interleaved in one process",
        "device": torch.cuda.get_device_name(0), "batch": args.batch, "mel_lengths": sorted(corpus.frame_lengths), "lm": lm,
        "max_len": args.max_len, "generated_frames": int(mel_out.shape[2]),
        "whole_call": stat(whole, "ms"), "generation": stat(gen, "ms"), "first_call_with_captures_ms": round(first_ms, 1),
        "whole_minus_generation_ms": round(statistics.median(whole) - statistics.median(gen), 3),
        "metric_launch_device": {n: stat(v, "us") for n, v in dev_us.items()},
        "metric_launch_host_with_reads": {n: stat(v, "us") for n, v in host_us.items()},
        "torch_lines_over_rtts_infer_metrics_device": round(med["torch_lines"] / med["rtts_infer_metrics"], 2),
        "metric_bytes_read": read_bytes, "metric_gb_per_s": round(read_bytes / med["rtts_infer_metrics"] * 1e-3, 1),
        "values": {"rtts_infer_metrics": k, "torch_lines_fp32": list(t)}}))


if __name__ == "__main__":
    main()
