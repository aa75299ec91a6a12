"""Writes tests/golden/hf_lsh_attn.npz: forward and backward goldens of HuggingFace's ``LSHSelfAttention`` -- the layer the
reference binds for ``implementation="huggingface_transformers"`` (its ``reformer_tts/model/reformer.py:201-220``) -- run in
fp32 on the CPU, train mode, dropout 0, with the config mapping of that wrapper.

    python tests/golden/make_hf_lsh_golden.py            # needs `transformers`

Per case of ``tests/hf_lsh_ref.CASES``:
  <tag>/meta        B, H, T, chunk, n_hashes, causal, n_buckets, seed
  <tag>/rot         the rotations HuggingFace drew (``torch.manual_seed(seed)`` before the forward), (H, dh, R, n_buckets / 2) f32
  <tag>/buckets     its offset buckets (B, H, R * T), int16
  <tag>/sorted_idx  its ``sorted_bucket_idx % T`` (B, H, R * T), int16
  <tag>/rows        the rows of out / dx that are stored (``hf_lsh_ref.stored_rows``)
  <tag>/out, dx     layer output and input gradient at those rows, (B, len(rows), d)
  <tag>/dwqk, dwv   gradients of ``query_key.weight`` and ``value.weight`` (sums over every row)
  <tag>/mask        (B, T) 1 = valid, or (0, T) for a case without a mask
The other inputs (x, the two weights, the upstream gradient: bf16-representable, the gradient zero on masked rows) are NOT
stored: ``hf_lsh_ref.case_inputs(tag)`` regenerates them from ``numpy.random.RandomState(seed)`` (a frozen stream), and
<tag>/input_sha256 pins their bytes.  Results are stored as float16 (11 significant bits: 2.4e-4 relative, a fortieth of the bf16 device path's
tolerance; the range is asserted).  Both choices keep the file under the size of the largest fixture of this directory.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import hf_lsh_ref as ref  # noqa: E402


def to_f16(a: np.ndarray) -> np.ndarray:
    """float32 -> float16; values must sit inside its normal range where it matters (largest below 6e4, and what falls under
    6e-5 -- absolute error 6e-8 -- is noise at the scale the tests compare on)."""
    assert np.abs(a).max() < 6e4 and np.abs(a).max() > 1e-2
    return a.astype(np.float16)


def run_case(tag: str):
    """-> dict of the arrays of one case (keys without the tag)."""
    from transformers import ReformerConfig
    from transformers.models.reformer.modeling_reformer import LSHSelfAttention as HF
    b, h, t, chunk, r, causal, lengths, seed = ref.CASES[tag]
    d = h * ref.DH
    inp = ref.case_inputs(tag)
    cfg = ReformerConfig(hidden_size=d, is_decoder=causal, num_attention_heads=h, num_hashes=r,
                         lsh_attention_probs_dropout_prob=0.0, lsh_attn_chunk_length=chunk, attention_head_size=d // h)
    layer = HF(cfg)
    with torch.no_grad():
        layer.query_key.weight.copy_(torch.from_numpy(inp["wqk"]))
        layer.value.weight.copy_(torch.from_numpy(inp["wv"]))
    layer.train()
    x = torch.from_numpy(inp["x"]).requires_grad_()
    mask = None if inp["mask"] is None else torch.from_numpy(inp["mask"])
    torch.manual_seed(seed)
    res = layer(x, attention_mask=mask)
    nb = layer.num_buckets
    assert nb == ref.num_buckets(t, chunk) and nb <= ref.bucket_limit(chunk)
    torch.manual_seed(seed)
    rot = torch.randn(h, d // h, r, nb // 2)                                  # what _hash_vectors drew
    buckets = res.buckets.reshape(b, h, r * t)
    sidx, _ = layer._get_sorted_bucket_idx_and_undo_sorted_bucket_idx(t, buckets, r)
    res.hidden_states.backward(torch.from_numpy(inp["dout"]))
    rows = ref.stored_rows(t)
    return {
        "meta": np.array([b, h, t, chunk, r, int(causal), nb, seed], dtype=np.int64),
        "rot": rot.numpy(),
        "buckets": buckets.numpy().astype(np.int16),
        "sorted_idx": (sidx % t).numpy().astype(np.int16),
        "rows": rows.astype(np.int32),
        "out": to_f16(res.hidden_states.detach().numpy()[:, rows]),
        "dx": to_f16(x.grad.numpy()[:, rows]),
        "dwqk": to_f16(layer.query_key.weight.grad.numpy()),
        "dwv": to_f16(layer.value.weight.grad.numpy()),
        "mask": np.zeros((0, t), dtype=np.uint8) if inp["mask"] is None else inp["mask"].astype(np.uint8),
        "input_sha256": ref.inputs_digest(inp),
    }


def main():
    torch.set_num_threads(4)
    out = {}
    for tag in ref.CASES:
        for k, v in run_case(tag).items():
            out[f"{tag}/{k}"] = v
        print(tag, "n_buckets", int(out[f"{tag}/meta"][6]), "max bucket", int(out[f"{tag}/buckets"].max()))
    path = os.path.join(HERE, "hf_lsh_attn.npz")
    np.savez_compressed(path, **out)
    print("hf_lsh_attn.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
