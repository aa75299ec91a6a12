"""``implementation="huggingface_transformers"`` of the LSH self-attention layer: the second branch of the reference's
wrapper (``reformer_tts/model/reformer.py:201-220``), which builds ``transformers``' ``LSHSelfAttention`` from
``heads -> num_attention_heads``, ``n_hashes -> num_hashes``, ``bucket_size -> lsh_attn_chunk_length``,
``dropout -> lsh_attention_probs_dropout_prob``, ``causal -> is_decoder``, ``attention_head_size = dim // heads`` and returns
``output.hidden_states``.  Same parameter names (``query_key``, ``value``: both (d, d), no bias, NO output projection), the
arithmetic in librtts_hip.so.

What that layer computes differently from ``reformer_pytorch``'s (``lsh_attention.py``), and where it runs here:
  * hashing (``rtts_lsh_hash_sort_hf``, csrc/lsh_hash_hf.hip): the bucket count is ``2 ** ((2 * (T // chunk)).bit_length() - 1)``,
    set by the first forward that hashes and kept afterwards (``num_buckets``); rotations are per head, shared over the batch,
    drawn from the default generator; with a mask the masked tokens share one extra bucket;
  * attention: keys are ``qk * rsqrt(mean(qk^2) + 1e-6) / sqrt(dh)`` and queries are unscaled, so the logit is
    ``q.k / sqrt(|k|^2 + dh * 1e-6)`` -- ``sqrt(dh)`` = 8 times the logit of ``rtts_lsh_attn_fwd`` (``q.k / (8 |k|)``) up to the
    epsilon.  The attention kernels are therefore fed ``8 * qk``: the factor sits in the bf16 cast of ``query_key.weight``
    (exact: a power of two), and the gradient of the unscaled weight picks the same factor up through the GEMMs.  The mask
    and self-mask fill values differ (-1e9 / -1e5 against -FLT_MAX / -5e4) without effect on a row that sees another token;
    HuggingFace masks keys only, so its masked QUERY rows differ from this layer's (the reference's loss masks them).
  * every other knob of the ``hip`` branch (``post_attn_dropout`` included) is ignored, as the reference ignores it here.
Outside this path, as on the ``hip`` branch: ``T <= chunk`` (HuggingFace's dense attention) and more buckets than
``2 * max(int(sqrt(max_position_embeddings // chunk)), chunk)`` (its factorised hash) raise ``NotImplementedError``.

The recompute protocol is ``LSHSelfAttention``'s (this class derives from it, so the trainer's rotation pool, per-rank seeds
and graph mode reach it unchanged).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import ops
from .._seeds import next_seed
from .lsh_attention import LSHSelfAttention, _LSHAttnFn, _project

QK_SCALE = 8.0            # sqrt(dh) at dh = 64


class HFLSHSelfAttention(LSHSelfAttention):
    hf = True

    def __init__(self, dim, heads=8, bucket_size=64, n_hashes=8, causal=False, dropout=0.0, num_buckets: Optional[int] = None,
                 max_position_embeddings: int = 4096, seed=0, **ignored):
        nn.Module.__init__(self)
        if dim % heads != 0:
            raise AssertionError("dimensions must be divisible by number of heads")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        if dim // heads != 64:
            raise NotImplementedError(f"implementation='huggingface_transformers' is built for dim/heads == 64 (got {dim // heads})")
        self.dim, self.heads, self.bucket_size, self.n_hashes, self.causal = dim, heads, bucket_size, n_hashes, causal
        self.full_attn_thres = bucket_size          # T <= chunk is HuggingFace's dense path
        self.max_position_embeddings = max_position_embeddings
        self.num_buckets = None
        if num_buckets is not None:
            self.num_buckets = self._check_buckets(int(num_buckets))
        self.query_key = nn.Linear(dim, dim, bias=False)
        self.value = nn.Linear(dim, dim, bias=False)
        self.dropout = float(dropout)        # on the attention probabilities: a counter-hash mask inside the kernels
        self._attn_drop = None
        self.seed = seed
        self._gen: Optional[torch.Generator] = None
        self._saved: Optional[tuple] = None
        self.forced_rotations: Optional[torch.Tensor] = None  # tests: use these instead of sampling
        self.forced_st: Optional[torch.Tensor] = None         # tests: use this permutation instead of hashing
        self.last_st: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ bucket count
    def bucket_limit(self) -> int:
        """The count above which HuggingFace factorises the hash."""
        return 2 * max(int((self.max_position_embeddings // self.bucket_size) ** 0.5), self.bucket_size)

    def _check_buckets(self, nb: int) -> int:
        if nb % 2 != 0 or nb < 2:
            raise AssertionError(f"There should be an even number of buckets, but `self.num_buckets`: {nb}")
        if nb > 256:
            raise NotImplementedError(f"num_buckets = {nb}: rtts_lsh_hash_sort_hf is built for at most 256 buckets")
        return nb

    def resolve_num_buckets(self, t: int) -> int:
        """``_set_num_buckets``: set on the first forward that hashes, sticky afterwards."""
        if self.num_buckets is None:
            nb = 2 ** ((2 * (t // self.bucket_size)).bit_length() - 1)
            if nb > self.bucket_limit():
                raise NotImplementedError(
                    f"T = {t} at chunk length {self.bucket_size} gives {nb} buckets, more than the limit of {self.bucket_limit()} "
                    "(2 * max(int(sqrt(max_position_embeddings // chunk)), chunk)) above which HuggingFace factorises the hash: "
                    "the factorised hash is outside the HIP path")
            self.num_buckets = self._check_buckets(nb)
        return self.num_buckets

    def _rotation_rows(self, x) -> int:
        return self.heads                    # per head, shared over the batch

    def check_length(self, t: int) -> None:
        if t <= self.bucket_size:
            raise NotImplementedError("dense attention (T <= chunk length) is outside the HIP path")
        if t % self.bucket_size != 0:
            raise AssertionError(f"Sequence length ({t}) needs to be divisible by the chunk length {self.bucket_size}")

    def hash_sort(self, qk, rot, mask):
        """-> st: the test hook's permutation, or ``rtts_lsh_hash_sort_hf`` on ``qk`` (a power-of-two multiple of the
        projection hashes like the projection: the argmax does not see the scale)."""
        if self.forced_st is not None:
            return self.forced_st
        return ops.lsh_hash_sort_hf(qk, rot, self.heads, self.bucket_size, self.num_buckets, mask)[0]

    def forward(self, x, input_mask=None, recompute: bool = False, **_):
        b, t, e = x.shape
        self.check_length(t)
        nb = self.resolve_num_buckets(t)
        # (B,T,2d) = [8 qk | v]: ONE product over the stacked weights; the multiplication is part of the autograd graph, so the
        # gradient of query_key.weight carries the factor
        qkv = _project(x.to(torch.bfloat16).reshape(b * t, e), None, self.query_key.weight * QK_SCALE, self.value.weight).view(b, t, 2 * e)
        mask = None if input_mask is None else input_mask.to(torch.uint8)
        state = self._generator_state(x.device)
        saved, st = self._saved, None
        grad_on = torch.is_grad_enabled()        # read here: the block below runs under no_grad
        with torch.no_grad():
            # always drawn, also when the permutation is re-used: the generator must end up where the forward left it
            rot = self._rotations(x, nb, default_generator=True)
            replay = (self.training and grad_on and saved is not None and saved[1].shape[0] == b * self.heads
                      and saved[1].shape[2] == t and (recompute or (state is not None and saved[0] == state)))
            if replay and recompute:
                st = saved[1]
            else:
                st = self.hash_sort(qkv[..., :e], rot, mask)
                if replay:
                    sig = self._signature(x)
                    same = (sig - saved[2]).abs().max() <= 1e-3 * saved[2].abs().max()
                    st = torch.where(same, saved[1], st)
            drop = None
            if self.training and self.dropout > 0.0:
                drop = self._attn_drop if (replay and self._attn_drop is not None) else (self.dropout, next_seed())
            if replay:
                self._saved = None
            elif self.training and not grad_on:
                self._saved = (state, st, self._signature(x))      # reversible forward: kept for the recompute
                self._attn_drop = drop
        self.last_st = st
        out = _LSHAttnFn.apply(qkv, st, mask, self.heads, self.bucket_size, self.causal, drop)
        return out.float()                   # no output projection, no output dropout: `output.hidden_states`
