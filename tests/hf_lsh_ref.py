"""Numpy restatement of the integer stages of HuggingFace's ``LSHSelfAttention`` (transformers,
``models/reformer/modeling_reformer.py``: ``_set_num_buckets``, ``_hash_vectors``, ``_stable_argsort``) -- what
``rtts_lsh_hash_sort_hf`` computes on the device -- and the seeded inputs of ``tests/golden/hf_lsh_attn.npz``.

TEST INFRASTRUCTURE.  The projection chain is ``oracle/lsh_int`` (the k-ordered fp32 fmaf chain of the C twin), so the device
kernel is compared bit for bit; HuggingFace's own buckets (fp32 einsum) are pinned by the fixture up to near-ties.

What differs from the ``hip`` branch's hash (``oracle/lsh_int.hash_buckets`` + ``sort_buckets`` on their own):
  * the bucket count is ``2 ** ((2 * (T // chunk)).bit_length() - 1)``, not ``T // chunk``;
  * rotations are per head and shared over the batch: (H, dh, n_hashes, n_buckets / 2);
  * with a mask, masked tokens take the extra bucket ``n_buckets`` and round r is offset by ``r * (n_buckets + 1)``.
The sort is the same stable (bucket, position) order.
"""
from __future__ import annotations

import numpy as np

from oracle import lsh_int

DH = 64
MAX_POSITION_EMBEDDINGS = 4096          # ReformerConfig's default, which the reference's wrapper leaves alone

# tag -> (B, H, T, chunk, n_hashes, causal, valid lengths per batch row | None, seed)
CASES = {
    "a": (2, 2, 256, 64, 4, False, (201, 256), 11),      # 8 buckets + 1
    "b": (1, 2, 512, 64, 4, True, (443,), 12),           # 16 + 1
    "c": (1, 2, 1024, 128, 2, True, None, 13),           # 16
    "d": (1, 2, 384, 64, 2, True, None, 14),             # 2 * 6 = 12 chunks -> 8 buckets
}


def num_buckets(t: int, chunk: int) -> int:
    """``_set_num_buckets``: the largest power of two <= 2 * (T // chunk)."""
    return 2 ** ((2 * (t // chunk)).bit_length() - 1)


def bucket_limit(chunk: int, max_position_embeddings: int = MAX_POSITION_EMBEDDINGS) -> int:
    """Above this count HuggingFace factorises the hash."""
    return 2 * max(int((max_position_embeddings // chunk) ** 0.5), chunk)


def bf16_round(a: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 value (ties to even), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def case_inputs(tag: str):
    """-> dict(x (B,T,d), wqk (d,d), wv (d,d), mask (B,T) bool | None, dout (B,T,d)): bf16-representable float32 drawn from
    ``numpy.random.RandomState(seed)`` (a frozen stream), so the fixture does not have to carry them.  ``dout`` is zero on
    masked rows."""
    b, h, t, chunk, r, causal, lengths, seed = CASES[tag]
    d = h * DH
    rs = np.random.RandomState(seed)
    x = bf16_round(rs.standard_normal((b, t, d)).astype(np.float32))
    wqk = bf16_round((0.5 / np.sqrt(d)) * rs.standard_normal((d, d)).astype(np.float32))
    wv = bf16_round((1.0 / np.sqrt(d)) * rs.standard_normal((d, d)).astype(np.float32))
    dout = bf16_round(rs.standard_normal((b, t, d)).astype(np.float32))
    mask = None
    if lengths is not None:
        mask = np.arange(t)[None, :] < np.asarray(lengths)[:, None]
        dout = dout * mask[:, :, None].astype(np.float32)
    return dict(x=x, wqk=wqk, wv=wv, mask=mask, dout=dout)


def inputs_digest(inp) -> np.ndarray:
    """SHA-256 over the bytes of x, wqk, wv, dout (float32, C order) and the mask: what the fixture keeps of the inputs."""
    import hashlib
    h = hashlib.sha256()
    for k in ("x", "wqk", "wv", "dout"):
        h.update(np.ascontiguousarray(inp[k], dtype=np.float32).tobytes())
    h.update(b"" if inp["mask"] is None else np.ascontiguousarray(inp["mask"], dtype=np.uint8).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def stored_rows(t: int) -> np.ndarray:
    """Rows of ``out`` and ``dx`` the fixture stores: all of them below T = 512, every (T // 128)-th from there on (the
    fixture has to stay under the repository's size limit; the two weight gradients sum over every row)."""
    return np.arange(0, t, 1 if t < 512 else t // 128)


def hash_buckets(qk: np.ndarray, rot: np.ndarray, mask, n_buckets: int) -> np.ndarray:
    """qk (B, H, T, dh) f32, rot (H, dh, R, n_buckets / 2) f32, mask (B, T) bool | None -> HuggingFace's offset buckets
    (B * H, R, T) int32: round r offset by r * n_buckets, or by r * (n_buckets + 1) with masked tokens in bucket
    ``n_buckets`` when a mask is given."""
    b, h, t, dh = qk.shape
    hh, dh2, r, half = rot.shape
    assert hh == h and dh2 == dh and 2 * half == n_buckets
    out = np.empty((b, h, r, t), dtype=np.int32)
    for i in range(b):
        out[i] = lsh_int.hash_buckets(qk[i], rot)             # rotation row = head
    out -= (np.arange(r, dtype=np.int32) * n_buckets)[None, None, :, None]
    stride = n_buckets
    if mask is not None:
        stride = n_buckets + 1
        out = np.where(np.asarray(mask, dtype=bool)[:, None, None, :], out, np.int32(n_buckets))
    out = out + (np.arange(r, dtype=np.int32) * stride)[None, None, :, None]
    return np.ascontiguousarray(out.reshape(b * h, r, t).astype(np.int32))


def sort_buckets(buckets: np.ndarray, stride: int):
    """Offset buckets (BH, R, T) with round stride ``stride`` -> st (sorted slot -> token), undo (token -> slot), per round:
    the stable argsort of ``_stable_argsort`` taken modulo T."""
    return lsh_int.sort_buckets(buckets, stride)


def sees_another_token(st: np.ndarray, chunk: int, causal: bool, mask, h: int) -> np.ndarray:
    """st (B * H, R, T) -> bool (B * H, T): does the token, as a query, reach a key other than itself in some round?  (Its own
    chunk and the one before it on the ring of all R * T / chunk chunks; masked keys and, with ``causal``, later positions do
    not count.)  A row that does not attends to itself alone at the self-mask fill value, where fp32 rounds the logsumexp on
    a 4e-3 (-5e4) or 8e-3 (-1e5) grid: implementations legitimately differ there (oracle/lsh_ref.py)."""
    bh, r, t = st.shape
    pos = st.reshape(bh, r * t // chunk, chunk).astype(np.int64)
    keys = np.concatenate([pos, np.roll(pos, 1, axis=1)], axis=2)                        # (BH, chunks, 2 chunk)
    ok = keys[:, :, None, :] != pos[:, :, :, None]
    if causal:
        ok &= keys[:, :, None, :] < pos[:, :, :, None]
    if mask is not None:
        valid = np.repeat(np.asarray(mask, dtype=bool), h, axis=0)                        # (BH, T)
        ok &= np.take_along_axis(valid, keys.reshape(bh, -1), axis=1).reshape(keys.shape)[:, :, None, :]
    sees = ok.any(axis=3).reshape(bh, r, t)                                               # per sorted slot
    out = np.zeros((bh, t), dtype=bool)
    for i in range(r):
        np.logical_or.at(out, (np.arange(bh)[:, None], st[:, i]), sees[:, i])
    return out


def heads_first(a: np.ndarray, h: int) -> np.ndarray:
    """(B, T, H * dh) -> (B, H, T, dh)."""
    b, t, d = a.shape
    return np.ascontiguousarray(a.reshape(b, t, h, d // h).transpose(0, 2, 1, 3))
