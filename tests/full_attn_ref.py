"""float64 definition of dense shared-QK attention (csrc/full_attn.hip: rtts_full_attn_fwd, rtts_full_attn_bwd), a hand-written
float64 backward, the numpy twin of the dropout mask, per-element first-order error bounds of the kernels' roundings, and an
fp32 / bf16 torch model of the kernels' data flow with named defects (no GPU anywhere in this file).

The function is reformer_pytorch's ``FullQKAttention.forward`` as the layer of reference reformer_tts/model/reformer.py:198-217
reaches it with ``use_full_attn`` or ``T <= full_attn_thres``.  Per (sample, head), rows qk_i, v_i in R^64, i < T:

    k^_j = qk_j / max(|qk_j|, 1e-12)              s_ij = (qk_i . k^_j) / 8
    fills, in this order, each overwriting:  (a) s_ii = -5e4   (b) s_ij = -FLT_MAX unless mask_i and mask_j
                                             (c) causal: s_ij = -FLT_MAX for j > i
    P = softmax_j(s),  lse = logsumexp_j(s)       o_i = sum_j P_ij keep_ij v_j
    delta_i = o_i . dO_i                          dS = P o (keep o (dO V^T) - delta), 0 on every filled pair
    dqk_i = sum_j dS_ij k^_j / 8  +  (g_i - k^_i (k^_i . g_i)) / max(|qk_i|, 1e-12),   g_j = sum_i dS_ij qk_i / 8
    dv_j  = sum_i P_ij keep_ij dO_i

dS with dropout is P (keep dP - delta), not P keep (dP - delta): d o / d P_ij = keep_ij v_j, the softmax Jacobian then subtracts
delta_i = sum_k P_ik keep_ik dP_ik from every entry, dropped ones included (``test_backward_matches_autograd`` settles it).

A query with mask_i = 0 has every logit equal to -FLT_MAX: P_ij = 1 / T over ALL T keys (padding, the diagonal and the causal
future included), o_i = mean(keep_i o v), lse_i = -FLT_MAX + log T = -FLT_MAX in fp32 (and in float64).  P is therefore taken
from softmax (which subtracts the maximum first), never rebuilt as exp(s - lse).

``keep`` (``keep_scales``) is rebuilt from ``oracle.synth.drop_hash``: element (head, i, j), head = b H + h, has the index
(head T + i) T + j in wrapping uint32 arithmetic (full_attn.hip:158 forward, :301 backward); the effective seed is
seed + *seed_dev; kept iff hash >= int(float32(p) 2^32), a kept element carries float32(1) / (float32(1) - float32(p)).

Error bounds.  u = 2^-8 is the unit roundoff of bf16.  fp32 arithmetic between the roundings (MFMA accumulation, the column
scale, exp, the running maximum and normaliser, the fp32 workspace) is three to four orders below u and not counted.  Roundings
to bf16, with their source lines in csrc/full_attn.hip:

    o    : 2u (keep o P)|V|
             1. P~ keep, the unnormalised probability times the keep-scale, rounded before the P V MFMA (cvt_bf16x8, :170);
                a later alpha rescale multiplies the fp32 accumulator and keeps the relative error
             2. o rounded on store (at_store_rows of attn_tile.h -> pack_bf16x2, called at :184)
    delta: d_delta = sum_d B_o |dO|       delta is the rowsum over the KERNEL's rounded o, as the engine forms it
    dS   : E = u |dS| + P d_delta, 0 on filled pairs
             3. dS rounded before the G MFMA (key pass, cvt_bf16x8 :321) and dS * column scale rounded before the dQ MFMA
                (query pass, the same line); the second term is the delta error carried through dS = P (. - delta)
    dv   : u (keep o P)^T |dO| + u |dv|
             4. P keep rounded before the dV MFMA (:325)       5. dv rounded on store (:392)
    dqk  : E |K^| / 8 + (dg + |k^| (|k^| . dg)) / |qk| + u |dqk|,   dg = E^T |QK| / 8
             the key-role rows stay fp32 (workspace) until they are added to the query role;  6. dqk rounded on store (:392)

``kernel_model`` walks the key tiles of 64 with a running maximum and normaliser and rounds where the kernels round, in fp32 /
bf16 torch; tests/test_full_attn_cpu.py holds it to the bounds and requires every ``defect`` to break one."""
import numpy as np
import torch

from oracle.synth import drop_hash

DH = 64
TILE = 64
U = 2.0 ** -8
FMAX = float(torch.finfo(torch.float32).max)
SELF = -5e4
DEFECTS = ("fill_order", "lse_rebuild", "no_key_role", "fill_leak", "causal_skip")
KINDS = ("plain", "peaked", "offset")
MASKS = ("none", "ragged", "hole", "first", "one")


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def keep_scales(p: float, seed: int, seed_dev, bh: int, t: int) -> torch.Tensor:
    """(bh, t, t) float64 keep-scales of the probability dropout as the kernels draw them."""
    eff = (int(seed) + (0 if seed_dev is None else int(seed_dev))) & 0xFFFFFFFF
    key = np.arange(t, dtype=np.uint64)
    row = np.arange(bh * t, dtype=np.uint64)[:, None] * np.uint64(t)
    h = drop_hash(eff, (row + key[None, :]) & np.uint64(0xFFFFFFFF))
    thresh = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy((h >= thresh).astype(np.float64) * scale).view(bh, t, t)


def _fills(t: int, mask_b, causal: bool):
    """-> (diag, dead) bool (T, T): the -5e4 pairs that survive, and the -FLT_MAX pairs, for one sample."""
    ar = torch.arange(t)
    dead = torch.zeros(t, t, dtype=torch.bool)
    if mask_b is not None:
        dead |= ~(mask_b[:, None] & mask_b[None, :])
    if causal:
        dead |= ar[None, :] > ar[:, None]
    diag = (ar[:, None] == ar[None, :]) & ~dead
    return diag, dead


def logits(qk, mask_b, causal: bool, order: str = "reference"):
    """(H, T, 64) float64 -> filled logits (H, T, T), |q||k^| / 8 (H, T, T), k^ and the clamped norms.  ``order`` =
    'lsh' applies the self fill LAST (the LSH path's order; the ``fill_order`` defect)."""
    t = qk.shape[-2]
    nrm = qk.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    kh = qk / nrm
    s = qk @ kh.transpose(-1, -2) / 8.0
    diag, dead = _fills(t, mask_b, causal)
    neg, slf = torch.full_like(s, -FMAX), torch.full_like(s, SELF)
    if order == "lsh":
        eye = torch.eye(t, dtype=torch.bool)
        s = torch.where(eye, slf, torch.where(dead, neg, s))
    else:
        s = torch.where(dead, neg, torch.where(diag, slf, s))
    return s, kh, nrm, diag, dead


def forward_autograd(qk, v, mask, causal: bool, keep=None):
    """Differentiable float64 forward (fills are constants through torch.where): qk, v (B, H, T, 64) -> o."""
    outs = []
    for b in range(qk.shape[0]):
        s, _, _, _, _ = logits(qk[b], None if mask is None else mask[b], causal)
        p = torch.softmax(s, dim=-1)
        outs.append((p if keep is None else p * keep[b]) @ v[b])
    return torch.stack(outs)


def reference(qk, v, do, mask=None, causal=False, keep=None):
    """qk, v, do (B, H, T, 64); mask (B, T) bool or None; keep (B, H, T, T) or None.  Returns a dict of float64 tensors: o, lse,
    delta, dqk, dv, the bounds b_o, b_dqk, b_dv, and lse_scale = max over the unfilled pairs of sum_d |q_d k^_jd| / 8, + |lse| + 1
    (the scale of the fp32 error of lse; rows of masked queries are compared exactly instead)."""
    qk, v, do = (x.double() for x in (qk, v, do))
    res = {n: [] for n in ("o", "lse", "delta", "dqk", "dv", "b_o", "b_dqk", "b_dv", "lse_scale")}
    for b in range(qk.shape[0]):                         # one sample at a time: the (H, T, T) matrices of the largest case stay small
        q, vb, dob = qk[b], v[b], do[b]
        s, kh, nrm, diag, dead = logits(q, None if mask is None else mask[b], causal)
        filled = diag | dead
        p = torch.softmax(s, dim=-1)
        lse = torch.logsumexp(s, dim=-1)
        pk = p if keep is None else p * keep[b].double()
        o = pk @ vb
        b_o = 2 * U * (pk @ vb.abs())
        dp = dob @ vb.transpose(-1, -2)
        if keep is not None:
            dp = dp * keep[b].double()
        delta = (o * dob).sum(-1, keepdim=True)
        ds = (p * (dp - delta)).masked_fill(filled, 0.0)
        g = ds.transpose(-1, -2) @ q / 8.0
        live = (q.norm(dim=-1, keepdim=True) > 1e-12).double()          # below the clamp the normaliser is a constant
        dqk = ds @ kh / 8.0 + (g - live * kh * (kh * g).sum(-1, keepdim=True)) / nrm
        dv = pk.transpose(-1, -2) @ dob
        d_delta = (b_o * dob.abs()).sum(-1, keepdim=True)
        err = (U * ds.abs() + p * d_delta).masked_fill(filled, 0.0)
        dg = err.transpose(-1, -2) @ q.abs() / 8.0
        b_dqk = err @ kh.abs() / 8.0 + (dg + kh.abs() * (kh.abs() * dg).sum(-1, keepdim=True)) / nrm + U * dqk.abs()
        b_dv = U * (pk.transpose(-1, -2) @ dob.abs()) + U * dv.abs()
        aqk = (q.abs() @ kh.abs().transpose(-1, -2) / 8.0).masked_fill(filled, 0.0)
        for n, x in (("o", o), ("lse", lse), ("delta", delta.squeeze(-1)), ("dqk", dqk), ("dv", dv), ("b_o", b_o), ("b_dqk", b_dqk),
                     ("b_dv", b_dv), ("lse_scale", aqk.max(-1).values + lse.abs() + 1.0)):
            res[n].append(x)
    return {n: torch.stack(x) for n, x in res.items()}


def kernel_model(qk, v, do, mask=None, causal=False, drop=None, defect=None):
    """fp32 / bf16 model of the kernels' data flow.  ``drop`` = (p, seed, seed_dev) or None; ``defect`` switches in ONE error:
      fill_order   the self fill is applied last, as on the LSH path (a masked query then attends to itself alone)
      lse_rebuild  the backward rebuilds P = exp(s - lse) for masked queries too (1 instead of 1 / T)
      no_key_role  dqk is missing the gradient through the keys
      fill_leak    dS of the filled pairs of a valid query (diagonal, padding keys, causal future) is taken from the raw product
                   exp(q.k^ / 8 - lse) instead of the fill, and leaks into dqk
      causal_skip  a causal forward stops every query block at its diagonal tile, masked queries included
    Returns o, lse, dqk, dv (float32)."""
    assert defect is None or defect in DEFECTS
    qk, v, do = (x.float() for x in (qk, v, do))
    nb, nh, t, _ = qk.shape
    keep = None
    if drop is not None:
        keep = keep_scales(drop[0], drop[1], drop[2], nb * nh, t).float().view(nb, nh, t, t)
    out = {n: [] for n in ("o", "lse", "dqk", "dv")}
    big = torch.finfo(torch.float32).max
    for b in range(nb):
        q, vb, dob = qk[b], v[b], do[b]
        mb = None if mask is None else mask[b]
        kp = torch.ones(nh, t, t) if keep is None else keep[b]
        ss = (q * q).sum(-1, keepdim=True)
        cs = 0.125 * torch.rsqrt(ss.clamp_min(1e-24))                       # fa_col_scale
        raw = q @ q.transpose(-1, -2)
        diag, dead = _fills(t, mb, causal)
        neg, slf = torch.full_like(raw, -big), torch.full_like(raw, SELF)
        if defect == "fill_order":
            s = torch.where(torch.eye(t, dtype=torch.bool), slf, torch.where(dead, neg, raw * cs.transpose(-1, -2)))
        else:
            s = torch.where(dead, neg, torch.where(diag, slf, raw * cs.transpose(-1, -2)))
        # forward: tiles of 64 keys, running maximum and normaliser (full_attn.hip:96-181)
        m_run = torch.full((nh, t, 1), -big)
        l_run = torch.zeros(nh, t, 1)
        oacc = torch.zeros(nh, t, DH)
        rows = torch.arange(t).view(1, t, 1)
        for j0 in range(0, t, TILE):
            sl = slice(j0, j0 + TILE)
            live = torch.ones(1, t, 1, dtype=torch.bool)
            if causal:                                                       # a block stops at its diagonal tile ...
                blk_has_masked = torch.zeros(t, dtype=torch.bool)
                if mb is not None and defect != "causal_skip":               # ... unless it holds a masked query
                    blk_has_masked = (~mb).view(-1, TILE).any(-1).repeat_interleave(TILE)
                live = ((rows // TILE) * TILE + TILE > j0) | blk_has_masked.view(1, t, 1)
            sc = s[..., sl]
            m = torch.maximum(sc.max(-1, keepdim=True).values, m_run)
            alpha = torch.exp(m_run - m)
            pt = torch.exp(sc - m)
            l_new = l_run * alpha + pt.sum(-1, keepdim=True)
            o_new = oacc * alpha + bf(pt * kp[..., sl]) @ vb[..., sl, :]
            m_run = torch.where(live, m, m_run)
            l_run = torch.where(live, l_new, l_run)
            oacc = torch.where(live, o_new, oacc)
        o = bf(oacc / l_run)
        lse = torch.where(m_run == -big, m_run, m_run + torch.log(l_run)).squeeze(-1)
        # backward: P from the forward's lse, delta from the rounded o (full_attn.hip:252-337)
        delta = (o * dob).sum(-1, keepdim=True)
        qvalid = torch.ones(t, dtype=torch.bool) if mb is None else mb
        p = torch.exp(s - lse.unsqueeze(-1))
        p = torch.where(dead, torch.zeros_like(p), p)
        if defect != "lse_rebuild":
            p = torch.where(qvalid.view(1, t, 1), p, torch.full_like(p, 1.0 / t))
        else:
            p = torch.where(qvalid.view(1, t, 1), p, torch.ones_like(p))
        ds = p * ((dob @ vb.transpose(-1, -2)) * kp - delta)
        ds = ds.masked_fill(diag | dead, 0.0)
        if defect == "fill_leak":       # dS of a filled pair of a valid query taken from the product instead of the fill
            leak = torch.exp(raw * cs.transpose(-1, -2) - lse.unsqueeze(-1)) * ((dob @ vb.transpose(-1, -2)) * kp - delta)
            ds = torch.where((diag | dead) & qvalid.view(1, t, 1), leak, ds)
        pb = bf(p * kp)
        dv = bf(pb.transpose(-1, -2) @ dob)
        g = (bf(ds).transpose(-1, -2) @ q) * 0.125
        inv_n = cs * 8.0
        kh = q * inv_n
        key_role = (g - kh * (kh * g).sum(-1, keepdim=True)) * inv_n
        if defect == "no_key_role":
            key_role = torch.zeros_like(key_role)
        dqk = bf(bf(ds * cs.transpose(-1, -2)) @ q + key_role)
        for n, x in (("o", o), ("lse", lse), ("dqk", dqk), ("dv", dv)):
            out[n].append(x)
    return {n: torch.stack(x) for n, x in out.items()}


def ratios(got, ref):
    """Worst |got - ref| / bound per quantity (0 / 0 counts as 0, anything over a zero bound as inf)."""
    out = {}
    for n in ("o", "dqk", "dv"):
        if n not in got:
            continue
        err = (got[n].double() - ref[n]).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / ref["b_" + n])
        out[n] = float(ratio.max()) if not torch.isnan(ratio).any() else float("nan")
    return out


def lse_ratio(got_lse, ref, mask=None, heads=1):
    """Worst |lse - ref| / (2^-24 lse_scale) over the rows of valid queries: the C an lse bound C 2^-24 (max_j |s_ij| + |lse| + 1)
    needs.  got_lse (B, H, T)."""
    err = (got_lse.double() - ref["lse"]).abs() / (2.0 ** -24 * ref["lse_scale"])
    if mask is not None:
        err = err.masked_fill(~mask[:, None, :].expand_as(err), 0.0)
    return float(err.max())


def make_mask(pattern: str, nb: int, t: int):
    """(B, T) bool or None: 'none'; 'ragged' (another tail per sample, ending inside a tile); 'hole' (tokens 20 .. 20 + T/4 of every
    sample invalid, ragged tails on top for the odd samples); 'first' (token 0 invalid); 'one' (sample 0 keeps one valid token --
    T/2 + 3 -- the others end ragged)."""
    if pattern == "none":
        return None
    mask = torch.ones(nb, t, dtype=torch.bool)
    if pattern == "first":
        mask[:, 0] = False
        return mask
    for b in range(nb):
        mask[b, t - 5 - 17 * b - (t // 4) * (b % 2):] = False
    if pattern == "hole":
        mask[0::2] = True
        mask[:, 20:20 + t // 4] = False
    elif pattern == "one":
        mask[0] = False
        mask[0, t // 2 + 3] = True
    return mask


def make_inputs(kind: str, nb: int, nh: int, t: int, seed: int):
    """qk, v, do as float32 tensors of bf16 values, (B, H, T, 64).
      plain  : randn, qk scaled by 4 (logits ~ N(0, 1/4 |qk|^2 / 64): a few units)
      peaked : token i is close to token (37 i + 11) mod T, scaled so that this logit stands about 15 above the rest; v and do
               carry a common offset of +1, which makes delta = o . do large against its rounding noise
      offset : a common direction of length 40 added to every row puts all logits near +5 and makes the norms large"""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    qk = torch.randn(nb, nh, t, DH, generator=g) * 4.0
    v = torch.randn(nb, nh, t, DH, generator=g)
    do = torch.randn(nb, nh, t, DH, generator=g)
    if kind == "peaked":
        idx = (torch.arange(t) * 37 + 11) % t
        base = torch.randn(nb, nh, t, DH, generator=g)
        base = base / base.norm(dim=-1, keepdim=True)
        qk = 200.0 * (base + base[:, :, idx, :]) + 0.5 * qk
        v, do = v + 1.0, do + 1.0
    elif kind == "offset":
        c = torch.randn(1, 1, 1, DH, generator=g)
        qk = qk + 40.0 * c / c.norm()
    return tuple(bf(x) for x in (qk, v, do))
