"""Tensor-level wrappers of the C ABI: shape/dtype/device checks on the host, raw
pointers and the current HIP stream handed to librtts_hip.so.  PyTorch is used for
device memory and streams only."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib


class _Timing:
    """Optional HIP-event timing of named launches on the stream they are launched on (bench.py's roofline legs).  Off by
    default; events are resolved in ``summary`` after a device sync.  A tag is enabled by name or by prefix
    (``enable("rtts_gemm_nt")`` records every ``rtts_gemm_nt/<shape>``)."""

    def __init__(self):
        self.tags = ()
        self.records = {}

    def enable(self, *tags: str):
        self.tags, self.records = tuple(tags), {}

    def disable(self):
        self.tags = ()

    def start(self, tag: str):
        if not self.tags or not any(tag == t or tag.startswith(t + "/") for t in self.tags):
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return (tag, ev)

    def stop(self, started, work: float):
        if started is None:
            return
        tag, ev = started
        end = torch.cuda.Event(enable_timing=True)
        end.record(torch.cuda.current_stream())
        self.records.setdefault(tag, []).append((ev, end, work))

    def summary(self, tag: str):
        """-> (average launch ms, launches, algorithmic work per launch) over every record whose tag is ``tag`` or starts
        with ``tag + "/"``."""
        recs = [r for k, v in self.records.items() if k == tag or k.startswith(tag + "/") for r in v]
        if not recs:
            return 0.0, 0, 0.0
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b, _ in recs]
        return sum(ms) / len(ms), len(ms), sum(f for _, _, f in recs) / len(ms)


TIMING = _Timing()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _check_rows(x: torch.Tensor, name: str) -> int:
    """(B, T, W) bf16 view whose last dim is contiguous and whose (B,T) dims collapse to rows."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3):
        raise ValueError(f"{name}: expected a CUDA bfloat16 (B,T,W) tensor, got {x.dtype} {tuple(x.shape)} on {x.device}")
    if x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        raise ValueError(f"{name}: rows must be contiguous with a single row stride, got strides {x.stride()}")
    return x.stride(1)


def lsh_hash_sort(qk: torch.Tensor, rotations: torch.Tensor, heads: int, bucket_size: int,
                  want_buckets: bool = False, want_undo: bool = False):
    """qk (B,T,H*dh) bf16, rotations (1|B*H, dh, R, nb/2) f32 -> st (B*H,R,T) i32 [, buckets, undo]."""
    ld = _check_rows(qk, "qk")
    b, t, d = qk.shape
    dh = d // heads
    if t % (2 * bucket_size) != 0:
        raise AssertionError(f"Sequence length ({t}) needs to be divisible by target bucket size  x 2 - {bucket_size * 2}")
    if not (rotations.is_cuda and rotations.dtype == torch.float32 and rotations.is_contiguous() and rotations.dim() == 4):
        raise ValueError("rotations: expected a contiguous CUDA float32 (rows, dh, n_hashes, n_buckets/2) tensor")
    rows, rdh, n_hashes, half = rotations.shape
    if rdh != dh or 2 * half != t // bucket_size or rows not in (1, b * heads):
        raise ValueError(f"rotations shape {tuple(rotations.shape)} does not match dh={dh}, n_buckets={t // bucket_size}")
    st = torch.empty(b * heads, n_hashes, t, dtype=torch.int32, device=qk.device)
    buckets = torch.empty_like(st) if want_buckets else None
    undo = torch.empty_like(st) if want_undo else None
    ev = TIMING.start(f"rtts_lsh_hash_sort/nb{t // bucket_size}")
    _lib.call("rtts_lsh_hash_sort", qk.data_ptr(), ld, rotations.data_ptr(), rows, b, heads, t, dh, n_hashes, bucket_size,
              _ptr(buckets), st.data_ptr(), _ptr(undo), _stream())
    # SURVEY.md 8(d), per token and head: hash reads dh*2 B and writes n_hashes*4 B of bucket ids, the sort reads and writes
    # n_hashes*(4+4) B (permutation + inverse) -- the algorithm's bytes, whatever the fused kernel keeps on chip
    TIMING.stop(ev, float(b * heads * t) * (dh * 2 + n_hashes * 4 + n_hashes * 8))
    return st, buckets, undo


def lsh_hash_sort_hf(qk: torch.Tensor, rotations: torch.Tensor, heads: int, chunk: int, n_buckets: int,
                     mask: Optional[torch.Tensor] = None, want_buckets: bool = False, want_undo: bool = False):
    """HuggingFace's hash and sort: qk (B,T,H*dh) bf16, rotations (H, dh, R, n_buckets/2) f32 (per head, shared over the batch),
    mask (B,T) 1 = valid or None -> st (B*H,R,T) i32 [, buckets, undo].  With a mask the masked tokens share bucket
    ``n_buckets`` and the round offsets of ``buckets`` are r * (n_buckets + 1)."""
    ld = _check_rows(qk, "qk")
    b, t, d = qk.shape
    dh = d // heads
    if not (rotations.is_cuda and rotations.dtype == torch.float32 and rotations.is_contiguous() and rotations.dim() == 4):
        raise ValueError("rotations: expected a contiguous CUDA float32 (heads, dh, n_hashes, n_buckets/2) tensor")
    rows, rdh, n_hashes, half = rotations.shape
    if rows != heads or rdh != dh or (2 * half != n_buckets and n_buckets % 2 == 0):
        raise ValueError(f"rotations shape {tuple(rotations.shape)} does not match heads={heads}, dh={dh}, n_buckets={n_buckets}")
    mask = _check_mask(mask, b, t, qk.device)
    st = torch.empty(b * heads, n_hashes, t, dtype=torch.int32, device=qk.device)
    buckets = torch.empty_like(st) if want_buckets else None
    undo = torch.empty_like(st) if want_undo else None
    ev = TIMING.start(f"rtts_lsh_hash_sort_hf/nb{n_buckets}")
    _lib.call("rtts_lsh_hash_sort_hf", qk.data_ptr(), ld, rotations.data_ptr(), _ptr(mask), b, heads, t, dh, n_hashes, chunk, n_buckets,
              _ptr(buckets), st.data_ptr(), _ptr(undo), _stream())
    TIMING.stop(ev, float(b * heads * t) * (dh * 2 + n_hashes * 4 + n_hashes * 8))
    return st, buckets, undo


def _check_mask(mask: Optional[torch.Tensor], b: int, t: int, device) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    if mask.shape != (b, t):
        raise ValueError(f"input_mask: expected shape {(b, t)}, got {tuple(mask.shape)}")
    return mask.to(device=device, dtype=torch.uint8).contiguous()


def _drop_args(drop, device):
    """(p, seed) | None -> (p, seed, device seed word) of a counter-hash dropout site."""
    if not drop or drop[0] <= 0.0:
        return 0.0, 0, None
    from ._seeds import seed_base
    return float(drop[0]), int(drop[1]) & 0xFFFFFFFF, seed_base(device).data_ptr()


def lsh_attn_fwd(qk, v, st, heads: int, bucket_size: int, causal: bool, mask=None, drop=None):
    """-> o (B*H,R,T,dh) bf16, lse (B*H,R,T) f32; rows already at unsorted positions.  ``drop`` = (p, seed): dropout on the
    attention probabilities (the layer's ``dropout`` knob); pass the same pair to ``lsh_attn_bwd``."""
    ld = _check_rows(qk, "qk")
    if _check_rows(v, "v") != ld or v.shape != qk.shape:
        raise ValueError("qk and v must share shape and row stride")
    b, t, d = qk.shape
    dh = d // heads
    n_hashes = st.shape[1]
    if st.shape != (b * heads, n_hashes, t) or st.dtype != torch.int32 or not st.is_contiguous():
        raise ValueError("st: expected contiguous int32 (B*H, n_hashes, T)")
    mask = _check_mask(mask, b, t, qk.device)
    o = torch.empty(b * heads, n_hashes, t, dh, dtype=torch.bfloat16, device=qk.device)
    lse = torch.empty(b * heads, n_hashes, t, dtype=torch.float32, device=qk.device)
    ev = TIMING.start(f"rtts_lsh_attn_fwd/bs{bucket_size}")
    _lib.call("rtts_lsh_attn_fwd", qk.data_ptr(), v.data_ptr(), ld, st.data_ptr(), _ptr(mask), b, heads, t, dh, n_hashes,
              bucket_size, int(causal), o.data_ptr(), lse.data_ptr(), *_drop_args(drop, qk.device), _stream())
    # two MFMA products (Q K^T and P V) of 2*bs*(2bs)*dh FLOP per chunk, n_hashes*T/bs chunks per head
    TIMING.stop(ev, 2.0 * 2.0 * bucket_size * (2 * bucket_size) * dh * (n_hashes * t // bucket_size) * b * heads)
    return o, lse


def lsh_combine_fwd(o, lse, batch: int, heads: int, out: Optional[torch.Tensor] = None):
    """-> out (B,T,H*dh) bf16 (merged heads), lse_tot (B*H,T) f32."""
    bh, n_hashes, t, dh = o.shape
    if out is None:
        out = torch.empty(batch, t, heads * dh, dtype=torch.bfloat16, device=o.device)
    ld_out = _check_rows(out, "out")
    lse_tot = torch.empty(bh, t, dtype=torch.float32, device=o.device)
    _lib.call("rtts_lsh_combine_fwd", o.data_ptr(), lse.data_ptr(), batch, heads, t, dh, n_hashes, out.data_ptr(), ld_out,
              lse_tot.data_ptr(), _stream())
    return out, lse_tot


def lsh_attn_bwd(qk, v, st, out, dout, lse_tot, heads: int, bucket_size: int, causal: bool, mask=None,
                 dqkv: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, drop=None, delta: Optional[torch.Tensor] = None):
    """Backward of hash-sorted attention + round combine.  -> dqk, dv (B,T,H*dh) bf16.  ``delta`` (B*H, T) fp32 = rowsum(out *
    dout) per head when the caller already has it (the to_out input-gradient GEMM's epilogue 5), else computed here."""
    ld = _check_rows(qk, "qk")
    if _check_rows(v, "v") != ld:
        raise ValueError("qk and v must share a row stride")
    ld_out, ld_do = _check_rows(out, "out"), _check_rows(dout, "dout")
    b, t, d = qk.shape
    dh = d // heads
    n_hashes = st.shape[1]
    mask = _check_mask(mask, b, t, qk.device)
    dev = qk.device
    if delta is None:
        delta = torch.empty(b * heads, t, dtype=torch.float32, device=dev)
        _lib.call("rtts_lsh_bwd_delta", out.data_ptr(), ld_out, dout.data_ptr(), ld_do, b, heads, t, dh, delta.data_ptr(), _stream())
    elif delta.shape != (b * heads, t) or delta.dtype != torch.float32 or not delta.is_contiguous():
        raise ValueError("delta: expected contiguous fp32 (B*H, T)")
    dqk_part = torch.empty(_lib.load().rtts_lsh_bwd_qk_slots(), b * heads, n_hashes, t, dh, dtype=torch.bfloat16, device=dev)
    dv_part = torch.empty(2, b * heads, n_hashes, t, dh, dtype=torch.bfloat16, device=dev)
    # the walking kernel writes most key rows once (slot 0 only) and flags the few that have a slot-1 partner
    walks = _lib.load().rtts_lsh_attn_bwd_run_length(b, heads, t, n_hashes, bucket_size) > 0
    flags = torch.empty(b * heads, n_hashes, t, dtype=torch.uint8, device=dev) if walks else None
    ev = TIMING.start(f"rtts_lsh_attn_bwd/bs{bucket_size}")
    _lib.call("rtts_lsh_attn_bwd", qk.data_ptr(), v.data_ptr(), ld, st.data_ptr(), _ptr(mask), dout.data_ptr(), ld_do,
              lse_tot.data_ptr(), delta.data_ptr(), b, heads, t, dh, n_hashes, bucket_size, int(causal), dqk_part.data_ptr(),
              dv_part.data_ptr(), _ptr(flags), *_drop_args(drop, dev), _stream())
    # five MFMA products of 2*bs*(2bs)*dh FLOP per chunk, n_hashes*T/bs chunks per head
    TIMING.stop(ev, 5.0 * 2.0 * bucket_size * (2 * bucket_size) * dh * (n_hashes * t // bucket_size) * b * heads)
    if dqkv is None:
        dqk = torch.empty(b, t, d, dtype=torch.bfloat16, device=dev)
        dv = torch.empty(b, t, d, dtype=torch.bfloat16, device=dev)
    else:
        dqk, dv = dqkv
    ld_d = _check_rows(dqk, "dqk")
    if _check_rows(dv, "dv") != ld_d:
        raise ValueError("dqk and dv must share a row stride")
    _lib.call("rtts_lsh_bwd_reduce", dqk_part.data_ptr(), dv_part.data_ptr(), b, heads, t, dh, n_hashes, dqk.data_ptr(),
              dv.data_ptr(), ld_d, _ptr(flags), _stream())
    return dqk, dv


def full_attn_max_t(dh: int = 64) -> int:
    """Longest sequence the dense shared-QK kernels take at head width ``dh`` (-1: width not built)."""
    return int(_lib.load().rtts_full_attn_max_t(int(dh)))


def full_attn_fwd(qk, v, heads: int, causal: bool, mask=None, drop=None, out: Optional[torch.Tensor] = None):
    """Dense shared-QK attention (the layer's ``use_full_attn`` / ``T <= full_attn_thres`` branch).  qk, v (B,T,H*dh) bf16 with a
    common row stride -> out (B,T,H*dh) bf16 (merged heads), lse (B*H,T) f32.  ``drop`` = (p, seed) as ``lsh_attn_fwd``."""
    ld = _check_rows(qk, "qk")
    if _check_rows(v, "v") != ld or v.shape != qk.shape:
        raise ValueError("qk and v must share shape and row stride")
    b, t, d = qk.shape
    dh = d // heads
    mask = _check_mask(mask, b, t, qk.device)
    if out is None:
        out = torch.empty(b, t, d, dtype=torch.bfloat16, device=qk.device)
    ld_out = _check_rows(out, "out")
    lse = torch.empty(b * heads, t, dtype=torch.float32, device=qk.device)
    ev = TIMING.start(f"rtts_full_attn_fwd/t{t}")
    _lib.call("rtts_full_attn_fwd", qk.data_ptr(), v.data_ptr(), ld, _ptr(mask), b, heads, t, dh, int(causal), out.data_ptr(), ld_out,
              lse.data_ptr(), *_drop_args(drop, qk.device), _stream())
    # two MFMA products (Q K^T and P V) of 2*T*T*dh FLOP per head (a causal call works about half of them)
    TIMING.stop(ev, 2.0 * 2.0 * t * t * dh * b * heads)
    return out, lse


def full_attn_bwd(qk, v, out, dout, lse, heads: int, causal: bool, mask=None,
                  dqkv: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, drop=None, delta: Optional[torch.Tensor] = None):
    """Backward of ``full_attn_fwd``.  -> dqk, dv (B,T,H*dh) bf16.  ``delta`` (B*H, T) fp32 = rowsum(out * dout) per head when the
    caller already has it (the to_out input-gradient GEMM's epilogue), else computed here from ``out``."""
    ld = _check_rows(qk, "qk")
    if _check_rows(v, "v") != ld:
        raise ValueError("qk and v must share a row stride")
    ld_do = _check_rows(dout, "dout")
    b, t, d = qk.shape
    dh = d // heads
    mask = _check_mask(mask, b, t, qk.device)
    dev = qk.device
    if delta is None:
        ld_out = _check_rows(out, "out")
        delta = torch.empty(b * heads, t, dtype=torch.float32, device=dev)
        _lib.call("rtts_lsh_bwd_delta", out.data_ptr(), ld_out, dout.data_ptr(), ld_do, b, heads, t, dh, delta.data_ptr(), _stream())
    elif delta.shape != (b * heads, t) or delta.dtype != torch.float32 or not delta.is_contiguous():
        raise ValueError("delta: expected contiguous fp32 (B*H, T)")
    if lse.shape != (b * heads, t) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError("lse: expected contiguous fp32 (B*H, T)")
    nbytes = int(_lib.load().rtts_full_attn_bwd_workspace(b, heads, t, dh))
    if nbytes < 0:
        raise _lib.RttsError(f"rtts_full_attn_bwd: T={t}, dh={dh} is outside the dense kernels' envelope "
                             f"(T a multiple of 64 from 64 to {full_attn_max_t(64)}, dh 64)")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    if dqkv is None:
        dqk = torch.empty(b, t, d, dtype=torch.bfloat16, device=dev)
        dv = torch.empty(b, t, d, dtype=torch.bfloat16, device=dev)
    else:
        dqk, dv = dqkv
    ld_d = _check_rows(dqk, "dqk")
    if _check_rows(dv, "dv") != ld_d:
        raise ValueError("dqk and dv must share a row stride")
    ev = TIMING.start(f"rtts_full_attn_bwd/t{t}")
    _lib.call("rtts_full_attn_bwd", qk.data_ptr(), v.data_ptr(), ld, _ptr(mask), dout.data_ptr(), ld_do, lse.data_ptr(), delta.data_ptr(),
              b, heads, t, dh, int(causal), dqk.data_ptr(), dv.data_ptr(), ld_d, ws.data_ptr(), *_drop_args(drop, dev), _stream())
    # seven MFMA products of 2*T*T*dh FLOP per head: S and dP in both passes, dV, G, dQ
    TIMING.stop(ev, 7.0 * 2.0 * t * t * dh * b * heads)
    return dqk, dv


def decode_attn_splits(bh: int, t: int) -> int:
    """The library's pick of workgroups per (batch, head) for the single-query kernels over ``t`` cache rows / keys (-1: a size
    the calls reject).  A host function of its arguments only."""
    return int(_lib.load().rtts_decode_attn_splits(int(bh), int(t)))


def _decode_rows(x: torch.Tensor, name: str, width: int) -> int:
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] == width and x.stride(1) == 1):
        raise ValueError(f"{name}: expected CUDA bfloat16 rows (B, {width}) with unit column stride, got {x.dtype} {tuple(x.shape)}")
    return x.stride(0)


def _decode_ws(who: str, bh: int, t: int, dh: int, splits: int, workspace, device):
    if splits == 0:
        splits = decode_attn_splits(bh, t)
    nbytes = int(_lib.load().rtts_decode_attn_workspace(bh, max(splits, 1), dh)) if splits >= 0 else -1
    if nbytes < 0:
        raise _lib.RttsError(f"{who}: B*H={bh}, T={t}, dh={dh}, splits={splits} is outside the single-query kernels' envelope")
    if splits == 1:
        return splits, None
    if workspace is None:
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    elif workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.numel() * 4 < nbytes or workspace.device != device:
        raise ValueError(f"{who}: workspace must be contiguous fp32 of at least {nbytes} bytes")
    return splits, workspace


def decode_self_attn(row: torch.Tensor, cache: torch.Tensor, pos: torch.Tensor, heads: int, cap: Optional[int] = None, splits: int = 0,
                     out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, batch: Optional[int] = None):
    """One new position of dense shared-QK attention against a frame cache.  row (>= B, 2*H*64) bf16 = [qk | v]; cache (B, rows,
    2*H*64) bf16; ``pos`` a device int32 scalar p = rows already cached (read on the device).  Appends ``row`` at cache[:, p] and
    returns o (rows of ``row``, H*64) bf16 = row p of ``full_attn_fwd`` (causal, no mask).  ``cap`` (default: the cache's rows)
    bounds the positions; p outside [0, cap) writes nothing to the cache and gives NaN.  ``batch``: utterances when ``row`` /
    ``out`` carry filler rows behind them."""
    b = cache.shape[0] if batch is None else int(batch)
    d2 = cache.shape[2]
    ld_cache = _check_rows(cache, "cache")
    ld_row = _decode_rows(row, "row", d2)
    e = d2 // 2
    dh = e // heads
    cap = cache.shape[1] if cap is None else int(cap)
    if cap > cache.shape[1] or row.shape[0] < b or b > cache.shape[0]:
        raise ValueError(f"decode_self_attn: cap={cap} / batch={b} exceed the cache {tuple(cache.shape)} or the rows {tuple(row.shape)}")
    if not (pos.is_cuda and pos.dtype == torch.int32 and pos.numel() == 1):
        raise ValueError("pos: expected a CUDA int32 scalar")
    if out is None:
        out = torch.empty(row.shape[0], e, dtype=torch.bfloat16, device=row.device)
    ld_o = _decode_rows(out, "out", e)
    splits, workspace = _decode_ws("rtts_decode_self_attn", b * heads, cap, dh, int(splits), workspace, row.device)
    ev = TIMING.start(f"rtts_decode_self_attn/cap{cap}")
    _lib.call("rtts_decode_self_attn", row.data_ptr(), ld_row, cache.data_ptr(), ld_cache, cache.stride(0), pos.data_ptr(), b, heads, cap, dh,
              out.data_ptr(), ld_o, splits, _ptr(workspace), _stream())
    TIMING.stop(ev, 0.0)
    return out


def decode_cross_attn(q: torch.Tensor, kv: torch.Tensor, heads: int, kvalid: Optional[torch.Tensor] = None, splits: int = 0,
                      out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, batch: Optional[int] = None):
    """One query per utterance against projected encoder keys.  q (>= B, H*dh) bf16; kv (B, T_k, 2*H*dh) bf16 = [k | v]; kvalid
    (B, T_k) 1 = attend, or None -> o (rows of ``q``, H*dh) bf16 with the arithmetic of ``rtts_xattn_fwd``."""
    b = kv.shape[0] if batch is None else int(batch)
    tk, e = kv.shape[1], kv.shape[2] // 2
    ld_kv = _check_rows(kv, "kv")
    ld_q = _decode_rows(q, "q", e)
    dh = e // heads
    if q.shape[0] < b or b > kv.shape[0]:
        raise ValueError(f"decode_cross_attn: batch={b} exceeds q {tuple(q.shape)} or kv {tuple(kv.shape)}")
    kvalid = _check_mask(kvalid, b, tk, q.device)
    if out is None:
        out = torch.empty(q.shape[0], e, dtype=torch.bfloat16, device=q.device)
    ld_o = _decode_rows(out, "out", e)
    splits, workspace = _decode_ws("rtts_decode_cross_attn", b * heads, tk, dh, int(splits), workspace, q.device)
    ev = TIMING.start(f"rtts_decode_cross_attn/tk{tk}")
    _lib.call("rtts_decode_cross_attn", q.data_ptr(), ld_q, kv.data_ptr(), ld_kv, _ptr(kvalid), b, heads, tk, dh, out.data_ptr(), ld_o, splits,
              _ptr(workspace), _stream())
    TIMING.stop(ev, 0.0)
    return out


def mel_spectrogram(audio: torch.Tensor, sample_offsets_host, frame_offsets_host, offsets: torch.Tensor, nseg: int,
                    dft_basis: torch.Tensor, mel_basis: torch.Tensor, n_fft: int, hop: int, power: int, clip: float,
                    out: torch.Tensor) -> torch.Tensor:
    """audio: the utterances end to end (flat f32); offsets: (2, nseg + 1) i64 device table [sample offsets; frame offsets] and the
    same values as two host ``ctypes.c_int64`` arrays; dft_basis (n_fft, n_fft) f32, mel_basis (n_mels, n_fft/2 + 1) f32 ->
    out (n_mels, >= total frames) f32 = the log-mel rows, one ``rtts_mel_spectrogram`` launch on the current stream."""
    for name, t in (("audio", audio), ("dft_basis", dft_basis), ("mel_basis", mel_basis), ("out", out)):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise _lib.RttsError(f"mel_spectrogram runs on the GPU only: {name} must be a CUDA float32 tensor "
                                 f"(got {t.dtype} on {t.device})")
    if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.shape == (2, nseg + 1) and offsets.is_contiguous()):
        raise ValueError(f"offsets: expected a contiguous CUDA int64 (2, {nseg + 1}) table")
    n_mels = mel_basis.shape[0]
    if not (audio.dim() == 1 and audio.is_contiguous() and dft_basis.is_contiguous() and mel_basis.is_contiguous()
            and tuple(dft_basis.shape) == (n_fft, n_fft) and tuple(mel_basis.shape) == (n_mels, n_fft // 2 + 1)
            and out.dim() == 2 and out.shape[0] == n_mels and out.stride(1) == 1):
        raise ValueError("mel_spectrogram: audio flat, dft_basis (n_fft, n_fft), mel_basis (n_mels, n_fft/2 + 1), out (n_mels, frames) rows")
    if audio.numel() < sample_offsets_host[nseg] or out.shape[1] < frame_offsets_host[nseg]:
        raise ValueError(f"mel_spectrogram: {audio.numel()} samples / {out.shape[1]} output frames for offsets ending at "
                         f"{sample_offsets_host[nseg]} / {frame_offsets_host[nseg]}")
    frames = frame_offsets_host[nseg]
    ev = TIMING.start(f"rtts_mel_spectrogram/n{n_fft}")
    _lib.call("rtts_mel_spectrogram", audio.data_ptr(), sample_offsets_host, frame_offsets_host, offsets[0].data_ptr(),
              offsets[1].data_ptr(), nseg, dft_basis.data_ptr(), mel_basis.data_ptr(), n_fft, hop, n_mels, power, clip,
              out.data_ptr(), out.stride(0), _stream())
    TIMING.stop(ev, 2.0 * frames * (n_fft * n_fft + n_mels * (n_fft // 2 + 1)))
    return out


def resample(audio: torch.Tensor, in_offsets_host, out_offsets_host, offsets: torch.Tensor, nseg: int, first: torch.Tensor,
             taps_table: torch.Tensor, orig_red: int, new_red: int, out: torch.Tensor, channels: int = 1) -> torch.Tensor:
    """audio: the utterances end to end, flat f32 (mono) or flat int16 (``channels`` interleaved, channel 0 is taken); offsets:
    (2, nseg + 1) i64 device table [input frame offsets; output offsets] and the same values as two host ``ctypes.c_int64``
    arrays; first (new_red,) i32 and taps_table (taps, new_red) f32 from ``dataset.audio.resample_tables`` -> out, flat f32 of
    >= out_offsets[nseg] samples: one ``rtts_resample`` launch on the current stream."""
    if not (audio.is_cuda and audio.dtype in (torch.float32, torch.int16)):
        raise _lib.RttsError(f"resample runs on the GPU only: audio must be a CUDA float32 or int16 tensor (got {audio.dtype} on {audio.device})")
    for name, t, dt in (("first", first, torch.int32), ("taps_table", taps_table, torch.float32), ("out", out, torch.float32)):
        if not (t.is_cuda and t.dtype == dt):
            raise _lib.RttsError(f"resample runs on the GPU only: {name} must be a CUDA {dt} tensor (got {t.dtype} on {t.device})")
    if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.shape == (2, nseg + 1) and offsets.is_contiguous()):
        raise ValueError(f"offsets: expected a contiguous CUDA int64 (2, {nseg + 1}) table")
    if not (audio.dim() == 1 and audio.is_contiguous() and out.dim() == 1 and out.is_contiguous() and first.is_contiguous()
            and taps_table.dim() == 2 and taps_table.is_contiguous() and tuple(first.shape) == (new_red,)
            and taps_table.shape[1] == new_red):
        raise ValueError("resample: audio and out flat, first (new_red,), taps_table (taps, new_red)")
    if audio.numel() < in_offsets_host[nseg] * channels or out.numel() < out_offsets_host[nseg]:
        raise ValueError(f"resample: {audio.numel()} input values / {out.numel()} output samples for offsets ending at "
                         f"{in_offsets_host[nseg]} frames of {channels} channel(s) / {out_offsets_host[nseg]}")
    taps = taps_table.shape[0]
    ev = TIMING.start(f"rtts_resample/{orig_red}to{new_red}")
    _lib.call("rtts_resample", audio.data_ptr(), 0 if audio.dtype == torch.float32 else 1, channels, in_offsets_host, out_offsets_host,
              offsets[0].data_ptr(), offsets[1].data_ptr(), nseg, first.data_ptr(), taps_table.data_ptr(), orig_red, new_red, taps,
              out.data_ptr(), _stream())
    TIMING.stop(ev, 2.0 * taps * out_offsets_host[nseg])
    return out


def denoise(audio: torch.Tensor, sample_offsets_host, offsets: torch.Tensor, nseg: int, dft_basis: torch.Tensor,
            idft_basis: torch.Tensor, bias: torch.Tensor, strength: float, n_fft: int, hop: int, out: torch.Tensor) -> torch.Tensor:
    """audio: the utterances end to end (flat f32); offsets: (nseg + 1,) i64 device table of sample offsets and the same values as
    a host ``ctypes.c_int64`` array; dft_basis / idft_basis (n_fft, n_fft) f32 from ``dataset.audio``; bias (n_fft/2 + 1,) f32 ->
    out, flat f32 over the same offsets (it must not overlap audio) = each utterance with ``strength * bias`` taken off its STFT
    magnitudes: one ``rtts_denoise`` launch on the current stream."""
    for name, t in (("audio", audio), ("dft_basis", dft_basis), ("idft_basis", idft_basis), ("bias", bias), ("out", out)):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise _lib.RttsError(f"denoise runs on the GPU only: {name} must be a CUDA float32 tensor (got {t.dtype} on {t.device})")
    if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.shape == (nseg + 1,) and offsets.is_contiguous()):
        raise ValueError(f"offsets: expected a contiguous CUDA int64 ({nseg + 1},) table")
    if not (audio.dim() == 1 and audio.is_contiguous() and out.dim() == 1 and out.is_contiguous() and dft_basis.is_contiguous()
            and idft_basis.is_contiguous() and tuple(dft_basis.shape) == (n_fft, n_fft) and tuple(idft_basis.shape) == (n_fft, n_fft)):
        raise ValueError("denoise: audio and out flat, dft_basis and idft_basis (n_fft, n_fft)")
    if not (bias.dim() == 1 and bias.is_contiguous() and bias.numel() == n_fft // 2 + 1):
        raise ValueError(f"denoise: bias must hold n_fft / 2 + 1 = {n_fft // 2 + 1} magnitudes (got shape {tuple(bias.shape)})")
    if audio.numel() < sample_offsets_host[nseg] or out.numel() < sample_offsets_host[nseg]:
        raise ValueError(f"denoise: {audio.numel()} input / {out.numel()} output samples for offsets ending at {sample_offsets_host[nseg]}")
    frames = sum((sample_offsets_host[s + 1] - sample_offsets_host[s]) // hop + 1 for s in range(nseg)) if hop > 0 else 0
    ev = TIMING.start(f"rtts_denoise/n{n_fft}")
    _lib.call("rtts_denoise", audio.data_ptr(), sample_offsets_host, offsets.data_ptr(), nseg, dft_basis.data_ptr(), idft_basis.data_ptr(),
              bias.data_ptr(), float(strength), n_fft, hop, out.data_ptr(), _stream())
    TIMING.stop(ev, 4.0 * frames * n_fft * n_fft)
    return out


def _gl_check(who: str, tensors, offsets: torch.Tensor, nseg: int, mag: torch.Tensor, col_offsets_host, n_fft: int) -> None:
    """The checks the three Griffin-Lim ops share: device and dtype by name, the (2, nseg + 1) offset table, mag's rows."""
    for name, t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise _lib.RttsError(f"{who} runs on the GPU only: {name} must be a CUDA float32 tensor "
                                 f"(got {getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')})")
    if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.shape == (2, nseg + 1) and offsets.is_contiguous()):
        raise ValueError(f"offsets: expected a contiguous CUDA int64 (2, {nseg + 1}) table [sample offsets; column offsets]")
    if not (mag.dim() == 2 and mag.shape[0] == n_fft // 2 + 1 and mag.stride(1) == 1 and mag.stride(0) >= mag.shape[1]):
        raise ValueError(f"{who}: mag must be (n_fft / 2 + 1 = {n_fft // 2 + 1}, columns) rows (got shape {tuple(mag.shape)})")
    if col_offsets_host[0] < 0 or mag.shape[1] < col_offsets_host[nseg]:
        raise ValueError(f"{who}: mag has {mag.shape[1]} columns for col_offsets from {col_offsets_host[0]} to {col_offsets_host[nseg]}")


def gl_magnitudes(mel: torch.Tensor, mel_start_host, mel_start: torch.Tensor, col_offsets_host, offsets: torch.Tensor, nseg: int,
                  pinv: torch.Tensor, power: int, n_fft: int, mag: torch.Tensor) -> torch.Tensor:
    """Step 1 of Griffin-Lim (``rtts_gl_magnitudes``): mel = log-mel, f32, read in place -- (nseg, n_mels, L) of any strides, or packed
    (n_mels, sum L); utterance s starts at frame ``mel_start[s]`` of it (i64 (nseg,) on the device, the same values as host ints) and
    has ``col_offsets[s+1] - col_offsets[s] - 1`` frames; offsets: (2, nseg + 1) i64 device table [sample offsets; column offsets],
    the column offsets also as a host ``ctypes.c_int64`` array; pinv (n_fft/2 + 1, n_mels) f32 -> mag (n_fft/2 + 1, >= columns) f32
    = max(0, pinv @ exp(mel))^(1/power), column L of an utterance repeating column L - 1.  One launch on the current stream."""
    _gl_check("gl_magnitudes", (("mel", mel), ("pinv", pinv), ("mag", mag)), offsets, nseg, mag, col_offsets_host, n_fft)
    if not (pinv.dim() == 2 and pinv.is_contiguous() and pinv.shape[0] == n_fft // 2 + 1):
        raise ValueError(f"gl_magnitudes: pinv must be contiguous (n_fft / 2 + 1, n_mels) (got shape {tuple(pinv.shape)})")
    n_mels = pinv.shape[1]
    if mel.dim() == 3 and mel.shape[0] == nseg and mel.shape[1] == n_mels:
        sb, sc, st = mel.stride()
    elif mel.dim() == 2 and mel.shape[0] == n_mels:
        sb, (sc, st) = 0, mel.stride()
    else:
        raise ValueError(f"gl_magnitudes: mel must be ({nseg}, {n_mels}, L) or packed ({n_mels}, frames) (got shape {tuple(mel.shape)})")
    if min(sb, sc, st) < 0:
        raise ValueError("gl_magnitudes: mel must not have negative strides")
    if not (mel_start.is_cuda and mel_start.dtype == torch.int64 and mel_start.dim() == 1 and mel_start.numel() >= nseg
            and mel_start.is_contiguous() and len(mel_start_host) >= nseg):
        raise ValueError(f"mel_start: expected a contiguous CUDA int64 table of {nseg} first frames and the same values on the host")
    for s in range(nseg):
        frames = col_offsets_host[s + 1] - col_offsets_host[s] - 1
        if frames < 0 or mel_start_host[s] < 0 or mel_start_host[s] + frames > mel.shape[-1]:
            raise ValueError(f"gl_magnitudes: utterance {s} of {frames} frames from frame {mel_start_host[s]} does not lie in mel of "
                             f"{mel.shape[-1]} frames (mel_start / col_offsets)")
    ev = TIMING.start(f"rtts_gl_magnitudes/n{n_fft}")
    _lib.call("rtts_gl_magnitudes", mel.data_ptr(), sb, sc, st, mel_start.data_ptr(), col_offsets_host, offsets[1].data_ptr(), nseg,
              pinv.data_ptr(), n_mels, int(power), n_fft, mag.data_ptr(), mag.stride(0), _stream())
    TIMING.stop(ev, 2.0 * col_offsets_host[nseg] * n_mels * (n_fft // 2 + 1))
    return mag


def _gl_audio(who: str, buffers, sample_offsets_host, nseg: int, dft_basis: torch.Tensor, idft_basis: torch.Tensor, n_fft: int) -> None:
    for name, t in buffers:
        if not (t.dim() == 1 and t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be flat and contiguous (got shape {tuple(t.shape)})")
        if sample_offsets_host[0] < 0 or t.numel() < sample_offsets_host[nseg]:
            raise ValueError(f"{who}: {name} has {t.numel()} samples for sample_offsets ending at {sample_offsets_host[nseg]}")
    if not (dft_basis.is_contiguous() and idft_basis.is_contiguous() and tuple(dft_basis.shape) == (n_fft, n_fft)
            and tuple(idft_basis.shape) == (n_fft, n_fft)):
        raise ValueError(f"{who}: dft_basis and idft_basis must be contiguous (n_fft, n_fft)")


def gl_init(mag: torch.Tensor, col_offsets_host, sample_offsets_host, offsets: torch.Tensor, nseg: int, dft_basis: torch.Tensor,
            idft_basis: torch.Tensor, phase: str, seed: int, n_fft: int, hop: int, out: torch.Tensor) -> torch.Tensor:
    """Step 2 of Griffin-Lim (``rtts_gl_init``): mag from ``gl_magnitudes``; offsets: (2, nseg + 1) i64 device table [sample offsets;
    column offsets] and the same values as two host ``ctypes.c_int64`` arrays; phase "hash" (phases from ``rtts_drop_hash(seed, .)``)
    or "zero" -> out, flat f32: utterance s = iSTFT(mag e^{i phi}) over its sample offsets, zeros where it has fewer than three
    frames.  One launch on the current stream."""
    if phase not in ("hash", "zero"):
        raise ValueError(f"gl_init: phase must be 'hash' or 'zero' (got {phase!r})")
    _gl_check("gl_init", (("mag", mag), ("dft_basis", dft_basis), ("idft_basis", idft_basis), ("out", out)), offsets, nseg, mag,
              col_offsets_host, n_fft)
    _gl_audio("gl_init", (("out", out),), sample_offsets_host, nseg, dft_basis, idft_basis, n_fft)
    ev = TIMING.start(f"rtts_gl_init/n{n_fft}")
    _lib.call("rtts_gl_init", mag.data_ptr(), mag.stride(0), col_offsets_host, offsets[1].data_ptr(), sample_offsets_host,
              offsets[0].data_ptr(), nseg, dft_basis.data_ptr(), idft_basis.data_ptr(), 1 if phase == "hash" else 0,
              int(seed) & 0xFFFFFFFF, n_fft, hop, out.data_ptr(), _stream())
    TIMING.stop(ev, 2.0 * col_offsets_host[nseg] * n_fft * n_fft)
    return out


def gl_step(cur: torch.Tensor, prev: Optional[torch.Tensor], beta: float, mag: torch.Tensor, col_offsets_host, sample_offsets_host,
            offsets: torch.Tensor, nseg: int, dft_basis: torch.Tensor, idft_basis: torch.Tensor, n_fft: int, hop: int,
            out: torch.Tensor) -> torch.Tensor:
    """One Griffin-Lim iteration (``rtts_gl_step``): out = iSTFT(mag R / |R|), R = STFT(cur - beta prev), per utterance over the
    sample offsets; ``prev`` may be None (the first iteration, or beta = 0).  ``out`` may overlap neither ``cur`` nor ``prev``.
    Tables as for ``gl_init``.  One launch on the current stream."""
    tensors = [("cur", cur), ("mag", mag), ("dft_basis", dft_basis), ("idft_basis", idft_basis), ("out", out)]
    buffers = [("cur", cur), ("out", out)]
    if prev is not None:
        tensors.append(("prev", prev))
        buffers.append(("prev", prev))
    _gl_check("gl_step", tensors, offsets, nseg, mag, col_offsets_host, n_fft)
    _gl_audio("gl_step", buffers, sample_offsets_host, nseg, dft_basis, idft_basis, n_fft)
    ev = TIMING.start(f"rtts_gl_step/n{n_fft}")
    _lib.call("rtts_gl_step", cur.data_ptr(), _ptr(prev), float(beta), mag.data_ptr(), mag.stride(0), col_offsets_host,
              offsets[1].data_ptr(), sample_offsets_host, offsets[0].data_ptr(), nseg, dft_basis.data_ptr(), idft_basis.data_ptr(), n_fft,
              hop, out.data_ptr(), _stream())
    TIMING.stop(ev, 4.0 * col_offsets_host[nseg] * n_fft * n_fft)
    return out


def sw_inv1x1_factor(weights) -> Tuple[list, torch.Tensor]:
    """The invertible 1x1 convolutions of a SqueezeWave factored on the device: ``weights`` = CUDA float32 (n, n) contiguous
    matrices, 1 <= n <= 128 -> (their inverses, fp32 rounded once from the float64 elimination; slogdet (len, 2) float64 on the
    device = {sign, log|det|} per matrix, sign 0 / -inf / an all-NaN inverse for a singular one).  One ``rtts_sw_inv1x1_factor``
    launch per 16 matrices on the current stream; nothing is read back and no table is copied to the device (the addresses
    travel in the kernel's argument block), so the call can be captured into a graph."""
    weights = list(weights)
    if not weights:
        raise ValueError("sw_inv1x1_factor: no matrices")
    for i, w in enumerate(weights):
        if not (torch.is_tensor(w) and w.is_cuda and w.dtype == torch.float32):
            raise _lib.RttsError(f"sw_inv1x1_factor runs on the GPU only: weights[{i}] must be a CUDA float32 tensor "
                                 f"(got {getattr(w, 'dtype', type(w).__name__)} on {getattr(w, 'device', 'the host')})")
        if not (w.dim() == 2 and w.shape[0] == w.shape[1] and w.is_contiguous()):
            raise ValueError(f"sw_inv1x1_factor: weights[{i}] must be a contiguous square matrix (got {tuple(w.shape)})")
    dev = weights[0].device
    for i, w in enumerate(weights):
        if w.device != dev:
            raise ValueError(f"sw_inv1x1_factor: weights[{i}] is on {w.device}, weights[0] on {dev}: one launch, one device")
    inv = [torch.empty_like(w) for w in weights]
    slogdet = torch.empty(len(weights), 2, dtype=torch.float64, device=dev)
    step = _lib.SW_FACTOR_MAX_COUNT
    for lo in range(0, len(weights), step):
        ws, outs = weights[lo:lo + step], inv[lo:lo + step]
        cnt = len(ws)
        _lib.call("rtts_sw_inv1x1_factor", (C.c_void_p * cnt)(*[w.data_ptr() for w in ws]), (C.c_int * cnt)(*[w.shape[0] for w in ws]), cnt,
                  (C.c_void_p * cnt)(*[o.data_ptr() for o in outs]), slogdet[lo:].data_ptr(), _stream())
    return inv, slogdet


def sw_draw_segments(audio: torch.Tensor, sample_offsets: torch.Tensor, mel: torch.Tensor, frame_offsets: torch.Tensor,
                     order: Optional[torch.Tensor], state: Optional[torch.Tensor], seed: int, picks_in: Optional[torch.Tensor],
                     batch: int, seg_frames: int, hop: int, n_audio_channels: int, audio_rows: torch.Tensor, mel_rows: torch.Tensor,
                     picks_out: torch.Tensor):
    """One vocoder training batch drawn from a device-resident corpus (``rtts_sw_draw_segments``): audio = the utterances end to
    end, flat f32 or int16; sample_offsets / frame_offsets int64 (n_utt + 1,); mel f32 (n_mel, frames) rows as
    ``rtts_mel_spectrogram`` writes them; order int32 (n_order,) and state int64 (2,) = {cursor, epoch_seed}, or picks_in int32
    (batch, 2) = {utterance, hop} in their place -> audio_rows f32 (batch * seg_frames * hop / C, C), mel_rows f32
    (batch * seg_frames, >= n_mel) channels-last, picks_out int32 (batch, 2).  All on one device; one launch on the current
    stream, nothing read back, so the call can be captured into a graph."""
    named = (("audio", audio, (torch.float32, torch.int16)), ("sample_offsets", sample_offsets, (torch.int64,)), ("mel", mel, (torch.float32,)),
             ("frame_offsets", frame_offsets, (torch.int64,)), ("order", order, (torch.int32,)), ("state", state, (torch.int64,)),
             ("picks_in", picks_in, (torch.int32,)), ("audio_rows", audio_rows, (torch.float32,)), ("mel_rows", mel_rows, (torch.float32,)),
             ("picks_out", picks_out, (torch.int32,)))
    dev = audio.device if torch.is_tensor(audio) else None
    for name, t, dts in named:
        if t is None and name in ("order", "state", "picks_in"):
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype in dts and t.device == dev):
            raise _lib.RttsError(f"sw_draw_segments runs on the GPU only: {name} must be a CUDA {' or '.join(str(d) for d in dts)} tensor on "
                                 f"{dev} (got {getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')})")
    if picks_in is None and (order is None or state is None):
        raise ValueError("sw_draw_segments: a drawn batch needs order and state (or give picks_in)")
    n_utt = sample_offsets.numel() - 1
    s = seg_frames * hop
    if not (audio.dim() == 1 and audio.is_contiguous() and sample_offsets.dim() == 1 and sample_offsets.is_contiguous() and n_utt >= 1
            and tuple(frame_offsets.shape) == (n_utt + 1,) and frame_offsets.is_contiguous() and mel.dim() == 2 and mel.stride(1) == 1):
        raise ValueError("sw_draw_segments: audio flat, sample_offsets and frame_offsets (n_utt + 1,), mel (n_mel, frames) rows")
    n_mel = mel.shape[0]
    if not ((order is None or (order.dim() == 1 and order.is_contiguous())) and (state is None or (tuple(state.shape) == (2,) and state.is_contiguous()))
            and (picks_in is None or (tuple(picks_in.shape) == (batch, 2) and picks_in.is_contiguous()))
            and tuple(picks_out.shape) == (batch, 2) and picks_out.is_contiguous()):
        raise ValueError(f"sw_draw_segments: order (n_order,), state (2,), picks_in / picks_out ({batch}, 2), all contiguous")
    if not (audio_rows.is_contiguous() and audio_rows.numel() == batch * s and mel_rows.dim() == 2 and mel_rows.shape[0] == batch * seg_frames
            and mel_rows.shape[1] >= n_mel and mel_rows.stride(1) == 1):
        raise ValueError(f"sw_draw_segments: audio_rows holds {audio_rows.numel()} values for {batch} x {s} samples, mel_rows is "
                         f"{tuple(mel_rows.shape)} for ({batch * seg_frames}, >= {n_mel})")
    ev = TIMING.start("rtts_sw_draw_segments")
    _lib.call("rtts_sw_draw_segments", audio.data_ptr(), 0 if audio.dtype == torch.float32 else 1, audio.numel(), sample_offsets.data_ptr(),
              mel.data_ptr(), mel.stride(0), frame_offsets.data_ptr(), n_utt, _ptr(order), 0 if order is None else order.numel(), _ptr(state),
              int(seed) & 0xFFFFFFFF, _ptr(picks_in), batch, seg_frames, hop, n_audio_channels, n_mel, audio_rows.data_ptr(), mel_rows.data_ptr(),
              mel_rows.stride(0), picks_out.data_ptr(), _stream())
    TIMING.stop(ev, 0.0)
    return audio_rows, mel_rows, picks_out


def tts_collate(mel: torch.Tensor, frame_offsets: torch.Tensor, phoneme_ids: torch.Tensor, phoneme_offsets: torch.Tensor, ids: torch.Tensor,
                lm: int, *, phonemes: Optional[torch.Tensor] = None, spectrogram_input: Optional[torch.Tensor] = None,
                valid_in: Optional[int] = None, spectrogram_target: Optional[torch.Tensor] = None, stop_tokens: Optional[torch.Tensor] = None,
                loss_mask: Optional[torch.Tensor] = None, valid_len: Optional[torch.Tensor] = None, noise_std: float = 0.0,
                seed: int = 0) -> None:
    """One text-to-spectrogram batch collated from a device-resident corpus (``rtts_tts_collate``): mel f32 (n_mel, frames) rows as
    ``rtts_mel_spectrogram`` writes them with frame_offsets int64 (n + 1,); phoneme_ids int32 flat with phoneme_offsets int64
    (n + 1,); ids int32 (B,) ON THE DEVICE (a slice of an uploaded plan); ``lm`` the batch's longest utterance, a host int ->
    the outputs given, each written in full, padding included: phonemes int64 (B, LP), spectrogram_input f32 (B, R_in, n_mel)
    live below row ``valid_in`` (default R_in), spectrogram_target f32 (B, R, n_mel), stop_tokens f32 (B, R), loss_mask f32
    (B, R, n_mel), valid_len int32 (1,) = lm.  ``noise_std`` > 0: Gaussian noise on the live input frames, keyed by
    (seed, slot, frame, channel).  All on one device; one launch on the current stream, nothing read back."""
    named = (("mel", mel, torch.float32, False), ("frame_offsets", frame_offsets, torch.int64, False), ("phoneme_ids", phoneme_ids, torch.int32, False),
             ("phoneme_offsets", phoneme_offsets, torch.int64, False), ("ids", ids, torch.int32, False), ("phonemes", phonemes, torch.int64, True),
             ("spectrogram_input", spectrogram_input, torch.float32, True), ("spectrogram_target", spectrogram_target, torch.float32, True),
             ("stop_tokens", stop_tokens, torch.float32, True), ("loss_mask", loss_mask, torch.float32, True), ("valid_len", valid_len, torch.int32, True))
    dev = mel.device if torch.is_tensor(mel) else None
    for name, t, dt, optional in named:
        if t is None and optional:
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.device == dev):
            raise _lib.RttsError(f"tts_collate runs on the GPU only: {name} must be a CUDA {dt} tensor on {dev} "
                                 f"(got {getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')})")
    n_utt = frame_offsets.numel() - 1
    if not (mel.dim() == 2 and mel.is_contiguous() and frame_offsets.dim() == 1 and frame_offsets.is_contiguous() and n_utt >= 1
            and phoneme_ids.dim() == 1 and phoneme_ids.is_contiguous() and tuple(phoneme_offsets.shape) == (n_utt + 1,)
            and phoneme_offsets.is_contiguous() and ids.dim() == 1 and ids.is_contiguous()):
        raise ValueError("tts_collate: mel (n_mel, frames) contiguous, phoneme_ids flat, frame_offsets and phoneme_offsets (n + 1,), ids (B,)")
    n_mel, b = mel.shape[0], ids.numel()
    want = dict(phonemes=(b, None), spectrogram_input=(b, None, n_mel), spectrogram_target=(b, None, n_mel), stop_tokens=(b, None),
                loss_mask=(b, None, n_mel), valid_len=(1,))
    for name, t, _, optional in named:
        if optional and t is not None:
            w = want[name]
            if not (t.is_contiguous() and t.dim() == len(w) and all(x is None or x == s for x, s in zip(w, t.shape))):
                raise ValueError(f"tts_collate: {name} must be contiguous of shape {tuple('*' if x is None else x for x in w)}, got {tuple(t.shape)}")

    def rows(t):
        return 0 if t is None else t.shape[1]
    r_in = rows(spectrogram_input)
    ev = TIMING.start("rtts_tts_collate")
    _lib.call("rtts_tts_collate", mel.data_ptr(), mel.shape[1], frame_offsets.data_ptr(), phoneme_ids.data_ptr(), phoneme_ids.numel(),
              phoneme_offsets.data_ptr(), n_utt, ids.data_ptr(), b, n_mel, int(lm), _ptr(phonemes), rows(phonemes), _ptr(spectrogram_input), r_in,
              r_in if valid_in is None else int(valid_in), _ptr(spectrogram_target), rows(spectrogram_target), _ptr(stop_tokens), rows(stop_tokens),
              _ptr(loss_mask), rows(loss_mask), _ptr(valid_len), float(noise_std or 0.0), int(seed) & 0xFFFFFFFF, _stream())
    TIMING.stop(ev, 0.0)


def _scored_operands(who: str, gen, gen_stop, truth, *, gen_frames_last, truth_frames_last, frame_offsets, ids, starts, lengths, extra=()):
    """The operand checks ``infer_metrics`` and ``dtw_align`` share (csrc/score_common.h holds the library's side): one truth
    description, dtypes, one device, either layout of ``gen`` and ``truth``, (B,) index tensors -> (b, n_mel, frames, gs_mel, gs_t,
    t_frames, ts_mel, ts_t, n_utt, dev).  ``extra``: further (name, tensor, dtype, optional) rows for the dtype and device passes."""
    corpus, padded = frame_offsets is not None, (starts is not None or lengths is not None)
    if corpus == padded or (padded and (starts is None or lengths is None)) or (ids is not None and not corpus):
        raise ValueError(f"{who}: describe the truth by frame_offsets (+ ids) or by starts + lengths: exactly one of the two")
    named = (("gen", gen, torch.float32, False), ("gen_stop", gen_stop, torch.int64, True), ("truth", truth, torch.float32, False), *extra,
             ("frame_offsets", frame_offsets, torch.int64, True), ("ids", ids, torch.int32, True), ("starts", starts, torch.int64, True),
             ("lengths", lengths, torch.int32, True))
    for name, t, dt, optional in named:
        if t is None and optional:
            continue
        if not (torch.is_tensor(t) and t.dtype == dt):
            raise ValueError(f"{who}: {name} must be a {dt} tensor (got {getattr(t, 'dtype', type(t).__name__)})")
    dev = gen.device
    for name, t, dt, optional in named:
        if t is not None and not (t.is_cuda and t.device == dev):
            raise _lib.RttsError(f"{who} runs on the GPU only: {name} must be a CUDA {dt} tensor on {dev} (got one on {t.device})")
    if gen.dim() != 3 or truth.dim() != 2:
        raise ValueError(f"{who}: gen must be 3-D and truth 2-D (got {tuple(gen.shape)} and {tuple(truth.shape)})")
    b = gen.shape[0]
    n_mel, frames, gs_mel, gs_t = (gen.shape[1], gen.shape[2], gen.stride(1), gen.stride(2)) if gen_frames_last else \
        (gen.shape[2], gen.shape[1], gen.stride(2), gen.stride(1))
    t_mel, t_frames, ts_mel, ts_t = (truth.shape[0], truth.shape[1], truth.stride(0), truth.stride(1)) if truth_frames_last else \
        (truth.shape[1], truth.shape[0], truth.stride(1), truth.stride(0))
    if t_mel != n_mel:
        raise ValueError(f"{who}: gen has {n_mel} mel channels, truth {t_mel}")
    for name, t in (("gen_stop", gen_stop), ("ids", ids), ("starts", starts), ("lengths", lengths)):
        if t is not None and not (tuple(t.shape) == (b,) and t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be contiguous of shape ({b},), got {tuple(t.shape)}")
    n_utt = 0
    if corpus:
        n_utt = frame_offsets.numel() - 1
        if not (frame_offsets.dim() == 1 and frame_offsets.is_contiguous() and n_utt >= 1):
            raise ValueError(f"{who}: frame_offsets must be contiguous of shape (n + 1,), n >= 1")
    return b, n_mel, frames, gs_mel, gs_t, t_frames, ts_mel, ts_t, n_utt, dev


def infer_metrics(gen: torch.Tensor, gen_stop: Optional[torch.Tensor], truth: torch.Tensor, lm: int, *, gen_frames_last: bool = True,
                  truth_frames_last: bool = True, frame_offsets: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None,
                  starts: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None, longest: int = 0):
    """B generated spectrograms scored against their truths in place (``rtts_infer_metrics``): ``gen`` f32 3-D with any strides,
    (B, n_mel, L) as ``ReformerTTS.infer`` returns it or, with ``gen_frames_last=False``, (B, T, n_mel) as the teacher-forced
    forward does; ``gen_stop`` int64 (B,) or None; ``truth`` f32 2-D, (n_mel, frames) as a ``TTSCorpus`` packs it or, with
    ``truth_frames_last=False``, (frames, n_mel) rows.  Slot b's truth frames are named by exactly one of ``frame_offsets`` int64
    (n + 1,) with ``ids`` int32 (B,) (None: slot b is utterance b), or ``starts`` int64 (B,) with ``lengths`` int32 (B,), all ON THE
    DEVICE.  ``lm``: the batch's longest truth, a host int; ``longest``: the longest length where the host knows it (checked
    against ``lm``), else 0.  -> (sse f64 (B,), stop_err f64 (B,), totals f64 (2,) = [Σ sse / (B n_mel lm), mean stop_err]);
    ``gen_stop=None`` leaves stop_err and totals[1] zero.  One call on the current stream, nothing read back: capturable."""
    b, n_mel, frames, gs_mel, gs_t, t_frames, ts_mel, ts_t, n_utt, dev = _scored_operands(
        "infer_metrics", gen, gen_stop, truth, gen_frames_last=gen_frames_last, truth_frames_last=truth_frames_last, frame_offsets=frame_offsets,
        ids=ids, starts=starts, lengths=lengths)
    lm = int(lm)
    tiles = _lib.load().rtts_infer_metrics_tiles(lm)
    out = torch.empty(2 * b + 2 + b * tiles, dtype=torch.float64, device=dev)
    sse, stop_err, totals, partials = out[:b], out[b:2 * b], out[2 * b:2 * b + 2], out[2 * b + 2:]
    ev = TIMING.start("rtts_infer_metrics")
    _lib.call("rtts_infer_metrics", gen.data_ptr() if frames else None, gen.stride(0), gs_mel, gs_t, frames, _ptr(gen_stop), truth.data_ptr(),
              ts_mel, ts_t, t_frames, _ptr(frame_offsets), n_utt, _ptr(ids), _ptr(starts), _ptr(lengths), b, n_mel, lm, int(longest),
              partials.data_ptr(), sse.data_ptr(), stop_err.data_ptr(), totals.data_ptr(), _stream())
    TIMING.stop(ev, 0.0)
    return sse, stop_err, totals


DTW_ALL = 15           # RTTS_DTW_ALL of include/rtts.h: project | distances | recurrence | fold


def dtw_max_frames() -> int:
    """The largest ``L`` and ``lm`` ``dtw_align`` takes (``rtts_dtw_max_frames``)."""
    return int(_lib.load().rtts_dtw_max_frames())


def dtw_align(gen: torch.Tensor, gen_stop: Optional[torch.Tensor], truth: torch.Tensor, lm: int, *, basis: Optional[torch.Tensor] = None,
              gen_frames_last: bool = True, truth_frames_last: bool = True, frame_offsets: Optional[torch.Tensor] = None,
              ids: Optional[torch.Tensor] = None, starts: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
              _phases: int = DTW_ALL, _state=None):
    """B generated spectrograms aligned to their truths by dynamic time warping (``rtts_dtw_align``), with the operands of
    ``infer_metrics``: ``gen`` f32 3-D with any strides, (B, n_mel, L) or, with ``gen_frames_last=False``, (B, T, n_mel);
    ``gen_stop`` int64 (B,) or None; ``truth`` f32 2-D, (n_mel, frames) or, with ``truth_frames_last=False``, (frames, n_mel) rows,
    slot b's frames named by exactly one of ``frame_offsets`` (+ ``ids``) or ``starts`` + ``lengths``, all ON THE DEVICE.  Slot b
    compares its first min(gen_stop[b], L) generated frames (L without ``gen_stop``) with its own truth frames; ``lm`` is a host
    upper bound of the truth lengths.  ``basis`` f32 (n_proj, n_mel) contiguous or None: the linear projection every compared
    frame goes through before the Euclidean frame distance (``evaluation.cepstral_basis`` makes the result an MCD in dB).
    -> (cost f64 (B,) = the summed distance along the optimal path, steps int32 (B,) = the path's length, totals f64 (2,) =
    [mean_b cost/steps, Σ cost / Σ steps]).  A slot that cannot be scored (no generated frame, a bad description, a non-finite
    compared value) has cost NaN and steps 0, and makes the totals NaN.  One call on the current stream, nothing read back:
    capturable.  ``_phases`` / ``_state``: scripts/dtw_bench.py times the four kernels one by one on a previous call's buffers."""
    b, n_mel, frames, gs_mel, gs_t, t_frames, ts_mel, ts_t, n_utt, dev = _scored_operands(
        "dtw_align", gen, gen_stop, truth, gen_frames_last=gen_frames_last, truth_frames_last=truth_frames_last, frame_offsets=frame_offsets,
        ids=ids, starts=starts, lengths=lengths, extra=(("basis", basis, torch.float32, True),))
    n_proj = n_mel
    if basis is not None:
        if not (basis.dim() == 2 and basis.shape[1] == n_mel and basis.shape[0] >= 1 and basis.is_contiguous()):
            raise ValueError(f"dtw_align: basis must be contiguous of shape (n_proj, {n_mel}), got {tuple(basis.shape)}")
        n_proj = basis.shape[0]
    lm = int(lm)
    lib = _lib.load()
    most = int(lib.rtts_dtw_max_frames())
    for name, v in (("L", frames), ("lm", lm)):
        if v > most:
            raise ValueError(f"dtw_align: {name} = {v} frames exceeds rtts_dtw_max_frames() = {most}")
    if _state is None:
        need = int(lib.rtts_dtw_workspace_bytes(b, frames, lm, n_proj))
        if need < 0:
            raise ValueError(f"dtw_align: unsupported sizes B = {b}, L = {frames}, lm = {lm}, n_proj = {n_proj} (include/rtts.h, rtts_dtw_align)")
        out = torch.empty(b + 2, dtype=torch.float64, device=dev)
        _state = (torch.empty(need, dtype=torch.uint8, device=dev), out[:b], torch.empty(b, dtype=torch.int32, device=dev), out[b:])
    work, cost, steps, totals = _state
    ev = TIMING.start("rtts_dtw_align")
    _lib.call("rtts_dtw_align", gen.data_ptr() if frames else None, gen.stride(0), gs_mel, gs_t, frames, _ptr(gen_stop), truth.data_ptr(),
              ts_mel, ts_t, t_frames, _ptr(frame_offsets), n_utt, _ptr(ids), _ptr(starts), _ptr(lengths), b, n_mel, lm, _ptr(basis), n_proj,
              work.data_ptr(), work.numel(), int(_phases), cost.data_ptr(), steps.data_ptr(), totals.data_ptr(), _stream())
    TIMING.stop(ev, 0.0)
    return cost, steps, totals


PITCH_MAX_LAG = 512    # RTTS_PITCH_MAX_LAG of include/rtts.h
PITCH_WINDOW = 1024    # the integration window of rtts_pitch_yin


def pitch_yin(audio: torch.Tensor, sample_offsets_host, frame_offsets_host, offsets: torch.Tensor, nseg: int, hop: int, tau_min: int,
              tau_max: int, threshold: float, sample_rate: float, f0: torch.Tensor, aperiodicity: torch.Tensor,
              cmnd: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """audio: the utterances end to end (flat f32); offsets: (2, nseg + 1) i64 device table [sample offsets; frame offsets] and the
    same values as two host ``ctypes.c_int64`` arrays (what ``dataset.audio.MelTables`` holds) -> f0 and aperiodicity, flat f32
    of >= frame_offsets[nseg] values, one per frame of the mel grid, and, when given, cmnd (>= frame_offsets[nseg],
    PITCH_MAX_LAG + 1) f32 = every frame's d': one ``rtts_pitch_yin`` launch on the current stream."""
    for name, t in (("audio", audio), ("f0", f0), ("aperiodicity", aperiodicity), ("cmnd", cmnd)):
        if t is None and name == "cmnd":
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise _lib.RttsError(f"pitch_yin runs on the GPU only: {name} must be a CUDA float32 tensor "
                                 f"(got {getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')})")
    if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.shape == (2, nseg + 1) and offsets.is_contiguous()):
        raise ValueError(f"offsets: expected a contiguous CUDA int64 (2, {nseg + 1}) table")
    if not (audio.dim() == 1 and audio.is_contiguous() and f0.dim() == 1 and f0.is_contiguous() and aperiodicity.dim() == 1
            and aperiodicity.is_contiguous()):
        raise ValueError("pitch_yin: audio, f0 and aperiodicity must be flat")
    frames = frame_offsets_host[nseg]
    if audio.numel() < sample_offsets_host[nseg] or f0.numel() < frames or aperiodicity.numel() < frames:
        raise ValueError(f"pitch_yin: {audio.numel()} samples / {f0.numel()} and {aperiodicity.numel()} output frames for offsets ending at "
                         f"{sample_offsets_host[nseg]} / {frames}")
    if cmnd is not None and not (cmnd.dim() == 2 and cmnd.is_contiguous() and cmnd.shape[1] == PITCH_MAX_LAG + 1 and cmnd.shape[0] >= frames):
        raise ValueError(f"pitch_yin: cmnd must be contiguous of shape (>= {frames}, {PITCH_MAX_LAG + 1}), got {tuple(cmnd.shape)}")
    ev = TIMING.start(f"rtts_pitch_yin/hop{hop}")
    _lib.call("rtts_pitch_yin", audio.data_ptr(), sample_offsets_host, frame_offsets_host, offsets[0].data_ptr(), offsets[1].data_ptr(), nseg,
              int(hop), int(tau_min), int(tau_max), float(threshold), float(sample_rate), f0.data_ptr(), aperiodicity.data_ptr(), _ptr(cmnd),
              _stream())
    TIMING.stop(ev, 3.0 * frames * PITCH_WINDOW * PITCH_MAX_LAG)
    return f0, aperiodicity


def f0_compare(f0_a: torch.Tensor, offsets_a: torch.Tensor, f0_b: torch.Tensor, offsets_b: torch.Tensor, gross: float = 0.2,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two packed F0 contours, ``f0_a`` against the reference ``f0_b``: flat f32, each with its own int64 (B + 1,) frame-offset
    table ON THE DEVICE -> f64 (B + 1, 5): per utterance [frames compared, voiced in both, sum of squared cents over those, gross
    errors among those, voicing differences], the last row their sums.  A NaN frame makes its row and the last row NaN.  One
    ``rtts_f0_compare`` launch on the current stream, nothing read back: capturable."""
    named = (("f0_a", f0_a, torch.float32), ("offsets_a", offsets_a, torch.int64), ("f0_b", f0_b, torch.float32),
             ("offsets_b", offsets_b, torch.int64))
    for name, t, dt in named:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt):
            raise _lib.RttsError(f"f0_compare runs on the GPU only: {name} must be a CUDA {dt} tensor "
                                 f"(got {getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')})")
        if not (t.dim() == 1 and t.is_contiguous() and t.device == f0_a.device):
            raise ValueError(f"f0_compare: {name} must be flat, contiguous and on {f0_a.device}")
    nseg = offsets_a.numel() - 1
    if nseg < 1 or offsets_b.numel() != nseg + 1:
        raise ValueError(f"f0_compare: the offset tables hold {offsets_a.numel()} and {offsets_b.numel()} entries; both must hold B + 1, B >= 1")
    if out is None:
        out = torch.empty(nseg + 1, 5, dtype=torch.float64, device=f0_a.device)
    elif not (out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (nseg + 1, 5) and out.is_contiguous()):
        raise ValueError(f"f0_compare: out must be a contiguous CUDA float64 ({nseg + 1}, 5) tensor")
    ev = TIMING.start("rtts_f0_compare")
    _lib.call("rtts_f0_compare", f0_a.data_ptr(), offsets_a.data_ptr(), f0_b.data_ptr(), offsets_b.data_ptr(), nseg, float(gross), out.data_ptr(),
              _stream())
    TIMING.stop(ev, 0.0)
    return out


ALIGN_MAX_TQ, ALIGN_MAX_TK, ALIGN_MAX_MAT = 4096, 2048, 64    # the envelope of rtts_align_stats / rtts_align_mas (include/rtts.h)


def _align_operand(who: str, mats, n_frames: torch.Tensor, n_keys: torch.Tensor):
    """The common operand of the two alignment entries: a 4-D f32 (L, B, T_q, T_k) tensor or a list of L (B, T_q, T_k) matrices
    -> (tensor that owns the memory, base pointer, sm, sb, st, L, B, T_q, T_k).  A list whose members already lie one fixed
    distance apart in one buffer (``xattn_probs_mean(out=buf[l])``) is read in place; any other list is stacked."""
    members = list(mats) if isinstance(mats, (list, tuple)) else [mats]
    if not members:
        raise ValueError(f"{who}: mats is an empty list")
    for name, t, dt in [("mats", m, torch.float32) for m in members] + [("n_frames", n_frames, torch.int32), ("n_keys", n_keys, torch.int32)]:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt):
            raise _lib.RttsError(f"{who} runs on the GPU only: {name} must be a CUDA {dt} tensor "
                                 f"(got {getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')})")
    dev = members[0].device
    if isinstance(mats, (list, tuple)):
        first = members[0]
        if any(m.dim() != 3 or m.shape != first.shape or m.device != dev for m in members):
            raise ValueError(f"{who}: mats must be a list of (B, T_q, T_k) matrices of one shape on one device "
                             f"(got {[tuple(m.shape) for m in members]})")
        step = (members[1].data_ptr() - first.data_ptr()) // 4 if len(members) > 1 else 0
        apart = all(m.stride() == first.stride() and m.data_ptr() - first.data_ptr() == 4 * step * i for i, m in enumerate(members))
        extent = (first.shape[0] - 1) * first.stride(0) + first.shape[1] * first.stride(1)      # of one member, in elements
        if apart and first.stride(2) == 1 and (len(members) == 1 or (step >= extent and step % 4 == 0)):
            owner, base, sm, (sb, st) = members, first.data_ptr(), step, first.stride()[:2]
        else:
            owner = torch.stack(members)
            base, (sm, sb, st) = owner.data_ptr(), owner.stride()[:3]
        n_mat, (b, tq, tk) = len(members), first.shape
    else:
        if mats.dim() != 4:
            raise ValueError(f"{who}: mats must be (L, B, T_q, T_k) or a list of (B, T_q, T_k) matrices (got {tuple(mats.shape)})")
        if mats.stride(3) != 1 and mats.shape[3] > 1:
            raise ValueError(f"{who}: mats must have a unit column stride (got strides {mats.stride()})")
        owner, base, (sm, sb, st), (n_mat, b, tq, tk) = mats, mats.data_ptr(), mats.stride()[:3], mats.shape
    for name, v, most in (("n_mat", n_mat, ALIGN_MAX_MAT), ("B", b, 65535), ("T_q", tq, ALIGN_MAX_TQ), ("T_k", tk, ALIGN_MAX_TK)):
        if not 1 <= v <= most:
            raise ValueError(f"{who}: {name} must be in 1..{most} (got {v})")
    if base % 16 or sm % 4 or sb % 4 or st % 4:
        raise ValueError(f"{who}: mats must be 16-byte aligned with strides that are multiples of 4 "
                         f"(base {base:#x}, strides {sm}, {sb}, {st})")
    for name, t in (("n_frames", n_frames), ("n_keys", n_keys)):
        if not (tuple(t.shape) == (b,) and t.is_contiguous() and t.device == dev):
            raise ValueError(f"{who}: {name} must be contiguous of shape ({b},) on {dev}, got {tuple(t.shape)}")
    return owner, base, int(sm), int(sb), int(st), int(n_mat), int(b), int(tq), int(tk)


def alignment_stats(mats, n_frames: torch.Tensor, n_keys: torch.Tensor, sigma: float = 0.2) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The arg-max track and the sums behind the alignment scores of L attention matrices (``rtts_align_stats``): ``mats`` f32
    (L, B, T_q, T_k) or a list of L (B, T_q, T_k) matrices, ``n_frames`` / ``n_keys`` int32 (B,) ON THE DEVICE (slot b uses frames
    below n_frames[b] and keys below n_keys[b]) -> (argmax int32 (L, B, T_q), dur_argmax int32 (L, B, T_k), table f64
    (L, B + 1, 8) = per slot [T, K, sum a, sum max, sum entropy, sum a w, monotone steps, covered keys], the last row the sums).
    A slot that cannot be scored is NaN / 0 / -1 and makes the last row NaN.  Nothing read back: capturable."""
    if not float(sigma) > 0.0:
        raise ValueError(f"alignment_stats: sigma must be positive (got {sigma})")
    owner, base, sm, sb, st, n_mat, b, tq, tk = _align_operand("alignment_stats", mats, n_frames, n_keys)
    dev = n_frames.device
    need = int(_lib.load().rtts_align_stats_workspace(n_mat, b, tq, tk))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    argmax = torch.empty(n_mat, b, tq, dtype=torch.int32, device=dev)
    dur = torch.empty(n_mat, b, tk, dtype=torch.int32, device=dev)
    table = torch.empty(n_mat, b + 1, 8, dtype=torch.float64, device=dev)
    ev = TIMING.start("rtts_align_stats")
    _lib.call("rtts_align_stats", base, sm, sb, st, n_mat, b, tq, tk, n_frames.data_ptr(), n_keys.data_ptr(), float(sigma), argmax.data_ptr(),
              dur.data_ptr(), table.data_ptr(), work.data_ptr(), work.numel(), _stream())
    TIMING.stop(ev, 0.0)
    return argmax, dur, table


def alignment_mas(mats, n_frames: torch.Tensor, n_keys: torch.Tensor, floor: float = 1e-30,
                  return_path: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """Monotonic alignment search over L attention matrices (``rtts_align_mas``), operands as ``alignment_stats`` -> (durations
    int32 (L, B, T_k): >= 1 below n_keys[b], summing to n_frames[b], 0 beyond; path int32 (L, B, T_q) = k(t), -1 beyond, or None
    without ``return_path``; scores f64 (L, B + 1, 2) = [log-probability of the path, sum_t a[t, k(t)]], the last row the sums).
    A slot that cannot be scored (as ``alignment_stats``, or fewer frames than keys) is 0 / -1 / NaN.  Nothing read back."""
    if not float(floor) > 0.0:
        raise ValueError(f"alignment_mas: floor must be positive (got {floor})")
    owner, base, sm, sb, st, n_mat, b, tq, tk = _align_operand("alignment_mas", mats, n_frames, n_keys)
    dev = n_frames.device
    need = int(_lib.load().rtts_align_mas_workspace(n_mat, b, tq, tk))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    dur = torch.empty(n_mat, b, tk, dtype=torch.int32, device=dev)
    path = torch.empty(n_mat, b, tq, dtype=torch.int32, device=dev) if return_path else None
    scores = torch.empty(n_mat, b + 1, 2, dtype=torch.float64, device=dev)
    ev = TIMING.start("rtts_align_mas")
    _lib.call("rtts_align_mas", base, sm, sb, st, n_mat, b, tq, tk, n_frames.data_ptr(), n_keys.data_ptr(), float(floor), dur.data_ptr(),
              _ptr(path), scores.data_ptr(), work.data_ptr(), work.numel(), _stream())
    TIMING.stop(ev, 0.0)
    return dur, path, scores


def xattn_guide_loss(q: torch.Tensor, kv: torch.Tensor, kvalid: Optional[torch.Tensor], lse: torch.Tensor, n_frames: torch.Tensor,
                     n_keys: torch.Tensor, heads: int, sigma: float = 0.2, coef: float = 1.0,
                     rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Guided attention loss of one ``rtts_xattn_fwd`` call (its q (B*T_q, H*dh) bf16, kv (B*T_k, 2*H*dh) bf16, kvalid u8 (B, T_k) or
    None and lse f32 (B*H, T_q)): ``rtts_xattn_guide_rows`` + ``rtts_xattn_guide_fold``.  ``n_frames`` / ``n_keys`` int32 (B,) ON
    THE DEVICE -> (rows f32 (B*H, T_q) = sum_k P W, out f64 (B + 1,) = per utterance mean off-diagonal mass and, last, the loss
    sum rows / (H sum_b T_b), c f32 (1,) = coef / (H sum_b T_b)): the operands ``rtts_xattn_bwd_guided`` takes.  W is the guided
    attention weight of Tachibana et al., 1 - exp(-(k / K_b - t / T_b)^2 / (2 sigma^2)); the loss is the mean over ROWS (frames),
    in [0, 1] -- ESPnet's guided attention loss averages over the T_b K_b cells instead, which is smaller by a factor of about K.
    Nothing read back: capturable."""
    if not float(sigma) > 0.0:
        raise ValueError(f"xattn_guide_loss: sigma must be positive (got {sigma})")
    for name, t, dt in (("q", q, torch.bfloat16), ("kv", kv, torch.bfloat16), ("lse", lse, torch.float32), ("n_frames", n_frames, torch.int32),
                        ("n_keys", n_keys, torch.int32)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt):
            raise _lib.RttsError(f"xattn_guide_loss runs on the GPU only: {name} must be a CUDA {dt} tensor "
                                 f"(got {getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')})")
    b = int(n_frames.shape[0])
    e = q.shape[-1]
    if q.dim() != 2 or kv.dim() != 2 or kv.shape[1] != 2 * e or e % heads or q.shape[0] % b or kv.shape[0] % b or q.stride(1) != 1 or kv.stride(1) != 1:
        raise ValueError(f"xattn_guide_loss: q must be (B*T_q, H*dh) and kv (B*T_k, 2*H*dh) with unit column strides "
                         f"(got {tuple(q.shape)}, {tuple(kv.shape)}, B = {b}, H = {heads})")
    tq, tk = q.shape[0] // b, kv.shape[0] // b
    if tuple(lse.shape) != (b * heads, tq) or not lse.is_contiguous() or tuple(n_keys.shape) != (b,) or not n_frames.is_contiguous() \
            or not n_keys.is_contiguous():
        raise ValueError(f"xattn_guide_loss: lse must be contiguous ({b * heads}, {tq}) and n_frames, n_keys contiguous ({b},)")
    if kvalid is not None and not (kvalid.is_cuda and kvalid.dtype == torch.uint8 and tuple(kvalid.shape) == (b, tk) and kvalid.is_contiguous()):
        raise ValueError(f"xattn_guide_loss: kvalid must be a contiguous CUDA uint8 ({b}, {tk}) tensor")
    dev = q.device
    if rows is None:
        rows = torch.empty(b * heads, tq, dtype=torch.float32, device=dev)
    out = torch.empty(b + 1, dtype=torch.float64, device=dev)
    c = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.call("rtts_xattn_guide_rows", q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), _ptr(kvalid), lse.data_ptr(), n_frames.data_ptr(),
              n_keys.data_ptr(), b, heads, tq, tk, e // heads, float(sigma), rows.data_ptr(), _stream())
    _lib.call("rtts_xattn_guide_fold", rows.data_ptr(), n_frames.data_ptr(), n_keys.data_ptr(), b, heads, tq, tk, float(coef), out.data_ptr(),
              c.data_ptr(), _stream())
    return rows, out, c
