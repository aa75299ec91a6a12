"""float64 definition of the single-query attention kernels (csrc/decode.hip: rtts_decode_self_attn, rtts_decode_cross_attn), with
an emulation of their split schedule, and their first-order error bounds (no GPU anywhere in this file).

Self mode, per (sample, head), the new row (q = k_p, v_p) at position p against cache rows k_j, v_j, j < p, all in R^64:

    s_j = (q . k_j) * 0.125 / max(|k_j|, 1e-12)  for j < p        s_p = -5e4
    P = softmax over j <= p                                       o = sum_j P_j v_j

which is row p of ``full_attn_ref.reference(..., causal=True)`` without a mask; p = 0 gives o = v_0.

Cross mode, one query q in R^dh against T_k keys:  s_j = q . k_j / sqrt(dh); keys with kvalid = 0 have P = 0 exactly; a sample
without a valid key has o = NaN.

Split schedule.  Key tiles of 64 are dealt round-robin over S splits (split s takes tiles s, s + S, ...); each split keeps a
partial (m, l, acc) = (maximum logit, sum exp(s - m), sum exp(s - m) v) over ITS keys -- (-FLT_MAX, 0, 0) when it got none; in
self mode split 0 also takes position p itself.  The fold: M = max_s m_s, w_s = exp(m_s - M), o = sum_s w_s acc_s / sum_s w_s l_s.

Error bound.  u = 2^-8 (bf16).  The decode kernels keep P and the P V sum in fp32 and round only o on store: |err| <= u |o| <=
u sum_j P_j |v_j|.  The tests hold them to ``full_attn_ref``'s bound for the same row, 2 u sum_j P_j |v_j| (self), and to
u |o| + 2 u sum_j P_j |v_j| (cross, the bound of tests/xattn_ref.py for rtts_xattn_fwd's row)."""
import math

import torch

TILE = 64
U = 2.0 ** -8
SELF = -5e4
FMAX = float(torch.finfo(torch.float32).max)


def self_logits(row_qk, cache_qk, p: int):
    """row_qk (..., 64), cache_qk (..., >= p, 64) float64 -> logits (..., p + 1): j < p from the cache, j = p the self fill."""
    k = cache_qk[..., :p, :]
    nrm = k.norm(dim=-1).clamp_min(1e-12)
    s = (k @ row_qk.unsqueeze(-1)).squeeze(-1) * 0.125 / nrm
    return torch.cat([s, torch.full_like(row_qk[..., :1], SELF)], dim=-1)


def self_attn(row_qk, row_v, cache_qk, cache_v, p: int):
    """(B, H, 64) rows, (B, H, cap, 64) caches (rows >= p are never looked at) -> dict o, b_o (B, H, 64) float64."""
    row_qk, row_v, cache_qk, cache_v = (x.double() for x in (row_qk, row_v, cache_qk, cache_v))
    s = self_logits(row_qk, cache_qk, p)
    v = torch.cat([cache_v[..., :p, :], row_v.unsqueeze(-2)], dim=-2)
    pr = torch.softmax(s, dim=-1)
    return dict(o=(pr.unsqueeze(-2) @ v).squeeze(-2), b_o=2 * U * (pr.unsqueeze(-2) @ v.abs()).squeeze(-2), p=pr)


def cross_logits(q, k, kvalid=None):
    """q (B, H, dh), k (B, H, Tk, dh), kvalid (B, Tk) bool or None -> logits (B, H, Tk), -inf at invalid keys."""
    s = (k @ q.unsqueeze(-1)).squeeze(-1) / math.sqrt(q.shape[-1])
    if kvalid is not None:
        s = s.masked_fill(~kvalid[:, None, :].bool(), float("-inf"))
    return s


def cross_attn(q, k, v, kvalid=None):
    """-> dict o (NaN for a sample without valid keys), pv = sum P |v|, and the bound b_o = u |o| + 2 u sum P |v|."""
    q, k, v = (x.double() for x in (q, k, v))
    s = cross_logits(q, k, kvalid)
    pr = torch.softmax(s, dim=-1)                       # all -inf -> NaN, as the kernels give
    o = (pr.unsqueeze(-2) @ v).squeeze(-2)
    pv = (pr.unsqueeze(-2) @ v.abs()).squeeze(-2)
    return dict(o=o, pv=pv, b_o=U * o.abs() + 2 * U * pv, p=pr)


def split_fold(s, v, splits: int, self_last: bool):
    """The kernels' schedule in float64: logits s (..., n) (-inf = skipped key), values v (..., n, dh).  ``self_last``: the last
    logit is position p itself, which split 0 takes whatever tile it would fall in; the others are dealt by tiles of 64.
    -> (o, partials) with partials = [(m, l, acc)] per split, m = -FLT_MAX for a split without keys."""
    n = s.shape[-1]
    nk = n - 1 if self_last else n
    parts = []
    for sp in range(splits):
        idx = [j for j in range(nk) if (j // TILE) % splits == sp]
        if self_last and sp == 0:
            idx.append(n - 1)
        shape = s.shape[:-1]
        if not idx:
            parts.append((torch.full(shape, -FMAX, dtype=s.dtype), torch.zeros(shape, dtype=s.dtype),
                          torch.zeros(*shape, v.shape[-1], dtype=s.dtype)))
            continue
        ss, vv = s[..., idx], v[..., idx, :]
        m = ss.max(dim=-1).values.clamp_min(-FMAX)                         # every key of the split skipped: as if it had none
        e = torch.exp(ss - m.unsqueeze(-1))
        parts.append((m, e.sum(-1), (e.unsqueeze(-2) @ vv).squeeze(-2)))
    big = torch.stack([m for m, _, _ in parts]).max(dim=0).values
    l = sum(torch.exp(m - big) * l_ for m, l_, _ in parts)
    acc = sum(torch.exp(m - big).unsqueeze(-1) * a for m, _, a in parts)
    return acc / l.unsqueeze(-1), parts


def postnet_tail_rows(n_convs: int) -> int:
    """Mel rows the last output row of a stack of ``n_convs`` Conv1d(k=5, pad=2) depends on."""
    return 2 * n_convs + 1
