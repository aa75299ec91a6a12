"""float64 oracle of dense encoder-decoder attention at a head width ``dh`` of 64 or 128 (csrc/xattn.hip templated on DH:
rtts_xattn_fwd, rtts_xattn_bwd, rtts_sum_slabs and rtts_lsh_bwd_delta), the per-element first-order error bounds of the kernels'
roundings, and an fp32 / bf16 torch model of the kernels' data flow with switchable defects.  No GPU anywhere in this file.

The width-independent helpers come from tests/xattn_ref.py (``keep_scales``, ``make_valid``, ``key_chunk``, ``bf``, ``ratios``,
``lse_ratio``); what depends on the width is restated here.  All tensors are (B, H, T, dh), bf16 VALUES lifted to float64.

Exact quantities, per (sample, head), c = 1 / sqrt(dh):

    s     = c q k^T,  padded keys -inf            P = softmax(s),  lse = logsumexp(s)
    o     = (keep o P) V                          delta = rowsum(o o dO)        (over all dh columns)
    dS    = c P o (keep o (dO V^T) - delta)
    dQ    = dS K,   dK = dS^T Q,   dV = (keep o P)^T dO

Chunking (xattn.hip xa_fwd_chunk / xa_bwd_chunk, include/rtts.h rtts_xattn_bwd_key_chunks):
    dh = 64 : forward and backward hold key_chunk(T_k) = 256 keys when T_k is a multiple of 256, else 128
    dh = 128: the backward always holds 128 keys (T_k / 128 chunks: more than one from T_k = 256 on); the forward holds 256 keys
              only when T_k == 256 and walks 128-key chunks otherwise

Error bounds, u = 2^-8 per rounding to bf16.  The DH = 128 kernels round exactly where the DH = 64 kernels do -- the plane
loop (XA_PLANES) only repeats the MFMA and store statements per 64 columns, it adds no conversion -- so the terms are those of
xattn_ref.reference; only the chunk count behind the "more than one chunk" term changes.  Source lines are csrc/xattn.hip's:

    o   : 2u (keep o P)|V|
            1. P~ keep rounded before the P V MFMA (forward, ``const bf16x8 pf = cvt_bf16x8(s[kt][o8] ...``)
            2. o rounded on store (at_store_rows: ``pk.x = pack_bf16x2(acc[dt][4 * g] * mul ...``), once per plane
    delta: d_delta = sum_d B_o |dO| over all dh columns; delta is the row sum over the KERNEL's rounded o
            (lsh_combine.hip lsh_bwd_delta_kernel<DH>), its own dh fp32 fmas are not counted
    dS  : E = u |dS| + c P d_delta
            3. dS rounded for the dK MFMA and for the dS^T image (backward, ``const bf16x8 db = cvt_bf16x8(dq_[0] ...`` and
               ``pk.x = pack_bf16x2(ds[4 * g], ds[4 * g + 1])``: the same value both times)
    dQ  : E |K| + u |dQ| + [bwd chunks > 1] u (|dS||K|)
            4. one chunk: dQ rounded on store (backward dQ epilogue, ``pk.x = pack_bf16x2(dqa[4 * g], dqa[4 * g + 1])``).  More
               chunks: every chunk's share is rounded on store by the same lines and their sum again by sum_slabs_kernel
               (``o.x = pack_bf16x2(acc[0], acc[1])``).  At dh = 128 this starts at T_k = 256.
    dK  : E^T |Q| + u sum_slabs(|dS|^T |Q|) + u |dK|
            5. every query block's slab rounded on store (at_store_rows of gacc)      6. the slab sum rounded (sum_slabs_kernel)
    dV  : 2u (keep o P)^T |dO| + u |dV|
            7. P keep rounded before the dV MFMA (``const bf16x8 pb = cvt_bf16x8(pq[0] ...``)   8. slab rounded on store
            (at_store_rows of dvacc)   9. the slab sum rounded
The score scale c is applied in fp32 (``xa_dh<DH>::scale``): float32(1 / sqrt(128)) is within 2^-25 of the exact value, four
orders of magnitude below u, and is not counted (1 / 8 is exact)."""
import math

import torch

import xattn_ref as X
from xattn_ref import bf, keep_scales, key_chunk, lse_ratio, make_valid, ratios  # noqa: F401  (re-exported for the tests)

QB = X.QB
U = X.U
KINDS = X.KINDS
DEFECTS = ("scale", "delta_half", "dq_share")


def bwd_chunk(tk: int, dh: int) -> int:
    """Keys the backward holds on chip at a time (xattn.hip xa_bwd_chunk)."""
    return 128 if dh == 128 else key_chunk(tk)


def fwd_chunk(tk: int, dh: int) -> int:
    """Keys the forward holds on chip at a time (xattn.hip xa_fwd_chunk)."""
    return (256 if tk == 256 else 128) if dh == 128 else key_chunk(tk)


def reference(q, k, v, do, valid=None, keep=None, dh=None):
    """q, do (B, H, Tq, dh); k, v (B, H, Tk, dh); valid (B, Tk) bool or None; keep (B, H, Tq, Tk) or None.  Returns a dict of
    float64 tensors: o, lse, delta, dq, dk, dv, p_mean (the head-averaged probabilities, (B, Tq, Tk)), the bounds b_o, b_dq,
    b_dk, b_dv, and lse_scale = max_j c sum_d |q_d k_jd| + |lse| + 1."""
    dh = q.shape[-1] if dh is None else dh
    assert q.shape[-1] == dh and dh in (64, 128)
    root = math.sqrt(dh)                                 # 8.0 exactly at dh = 64
    q, k, v, do = (x.double() for x in (q, k, v, do))
    nb, tk = q.shape[0], k.shape[2]
    multi = tk // bwd_chunk(tk, dh) > 1
    res = {n: [] for n in ("o", "lse", "delta", "dq", "dk", "dv", "p_mean", "b_o", "b_dq", "b_dk", "b_dv", "lse_scale")}
    for b in range(nb):
        qb, kb, vb, dob = q[b], k[b], v[b], do[b]
        s = qb @ kb.transpose(-1, -2) / root
        aqk = qb.abs() @ kb.abs().transpose(-1, -2) / root
        if valid is not None:
            pad = ~valid[b].view(1, 1, tk)
            s = s.masked_fill(pad, float("-inf"))
            aqk = aqk.masked_fill(pad, 0.0)
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse.unsqueeze(-1))
        pk = p if keep is None else p * keep[b].double()
        o = pk @ vb
        b_o = 2 * U * (pk @ vb.abs())
        dp = dob @ vb.transpose(-1, -2)
        if keep is not None:
            dp = dp * keep[b].double()
        delta = (o * dob).sum(-1, keepdim=True)
        ds = p * (dp - delta) / root
        dq, dk, dv = ds @ kb, ds.transpose(-1, -2) @ qb, pk.transpose(-1, -2) @ dob
        d_delta = (b_o * dob.abs()).sum(-1, keepdim=True)
        err = U * ds.abs() + p * d_delta / root
        b_dq = err @ kb.abs() + U * dq.abs()
        if multi:
            b_dq = b_dq + U * (ds.abs() @ kb.abs())
        b_dk = err.transpose(-1, -2) @ qb.abs() + U * (ds.abs().transpose(-1, -2) @ qb.abs()) + U * dk.abs()
        b_dv = 2 * U * (pk.transpose(-1, -2) @ dob.abs()) + U * dv.abs()
        for n, x in (("o", o), ("lse", lse), ("delta", delta.squeeze(-1)), ("dq", dq), ("dk", dk), ("dv", dv), ("p_mean", p.mean(0)),
                     ("b_o", b_o), ("b_dq", b_dq), ("b_dk", b_dk), ("b_dv", b_dv), ("lse_scale", aqk.max(-1).values + lse.abs() + 1.0)):
            res[n].append(x)
    return {n: torch.stack(x) for n, x in res.items()}


def kernel_model(q, k, v, do, valid=None, drop=None, defect=None, dh=None):
    """fp32 / bf16 model of the kernels' data flow at head width ``dh``: the forward's chunk walk (``fwd_chunk``) with a running
    maximum and normaliser, P from the forward's lse, per-chunk dQ shares (``bwd_chunk``) and per-query-block slabs, rounded
    where the kernels round.  ``drop`` = (p, seed, seed_dev) or None; ``defect`` switches in ONE deliberate error:
      scale       the score scale is 1 / 8 whatever dh is (forward and backward)
      delta_half  delta sums only the first 64 columns of a head
      dq_share    the second key chunk's share of dQ is left out of the sum (the only chunk's, if there is one chunk)
    Returns o, lse, dq, dk, dv (float32)."""
    assert defect is None or defect in DEFECTS
    dh = q.shape[-1] if dh is None else dh
    q, k, v, do = (x.float() for x in (q, k, v, do))
    nb, nh, tq, _ = q.shape
    tk = k.shape[2]
    fch, bch = fwd_chunk(tk, dh), bwd_chunk(tk, dh)
    nqb = tq // QB
    c = 0.125 if defect == "scale" else float(torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32))
    if valid is None:
        valid = torch.ones(nb, tk, dtype=torch.bool)
    if drop is None:
        keep = torch.ones(nb, nh, tq, tk)
    else:
        keep = keep_scales(drop[0], drop[1], drop[2], nb * nh, tq, tk).float().view(nb, nh, tq, tk)
    pad = ~valid.view(nb, 1, 1, tk)
    s = ((q @ k.transpose(-1, -2)) * c).masked_fill(pad, float("-inf"))
    big = torch.finfo(torch.float32).max
    m_run = torch.full((nb, nh, tq, 1), -big)
    l_run = torch.zeros(nb, nh, tq, 1)
    oacc = torch.zeros(nb, nh, tq, dh)
    for ci in range(tk // fch):
        sl = slice(ci * fch, (ci + 1) * fch)
        sc = s[..., sl]
        m = torch.maximum(sc.max(-1, keepdim=True).values, m_run)
        alpha = torch.where(m_run == -big, torch.zeros_like(m), torch.exp(m_run - m))
        pt = torch.where(torch.isinf(sc), torch.zeros_like(sc), torch.exp(sc - m))
        l_run = l_run * alpha + pt.sum(-1, keepdim=True)
        m_run = m
        oacc = oacc * alpha + bf(pt * keep[..., sl]) @ v[..., sl, :]
    o = bf(oacc / l_run)
    lse = (m_run + torch.log(l_run)).squeeze(-1)
    cols = 64 if defect == "delta_half" else dh
    delta = (o[..., :cols] * do[..., :cols]).sum(-1, keepdim=True)
    p = torch.exp(s - lse.unsqueeze(-1))
    ds = p * ((do @ v.transpose(-1, -2)) * keep - delta) * c
    dsb, pb = bf(ds), bf(p * keep)
    nch = tk // bch
    shares = [bf(dsb[..., i * bch:(i + 1) * bch] @ k[..., i * bch:(i + 1) * bch, :]) for i in range(nch)]
    if defect == "dq_share":
        shares[min(1, nch - 1)] = torch.zeros_like(shares[0])
    dq = shares[0] if nch == 1 else bf(sum(shares))
    rows = [slice(i * QB, (i + 1) * QB) for i in range(nqb)]
    slabs_k = [bf(dsb[..., r, :].transpose(-1, -2) @ q[..., r, :]) for r in rows]
    slabs_v = [bf(pb[..., r, :].transpose(-1, -2) @ do[..., r, :]) for r in rows]
    return dict(o=o, lse=lse, dq=dq, dk=bf(sum(slabs_k)), dv=bf(sum(slabs_v)))


def make_inputs(kind: str, nb: int, nh: int, tq: int, tk: int, seed: int, dh: int = 128):
    """q, k, v, do as float32 tensors of bf16 values, (B, H, T, dh): the four kinds of xattn_ref.make_inputs with their logit
    levels kept at the wider head (the peak about 30 above the rest, the offsets near +-80): a logit is q . k / sqrt(dh), so the
    constructed part of q grows with sqrt(dh / 64)."""
    assert kind in KINDS
    grow = math.sqrt(dh / 64.0)
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nb, nh, tq, dh, generator=g) * 1.5
    k = torch.randn(nb, nh, tk, dh, generator=g)
    v = torch.randn(nb, nh, tk, dh, generator=g)
    do = torch.randn(nb, nh, tq, dh, generator=g)
    if kind == "peaked":
        idx = (torch.arange(tq) * 37) % tk
        k = k * 0.3
        hit = k[:, :, idx, :]
        q = 240.0 * grow * hit / hit.pow(2).sum(-1, keepdim=True) + 0.3 * q
        v, do = v + 1.0, do + 1.0
    elif kind.startswith("offset"):
        c = torch.randn(1, 1, 1, dh, generator=g)
        c = c / c.norm()
        q = q + 25.6 * grow * c
        k = k + (25.0 if kind == "offset+" else -25.0) * c
    return tuple(bf(x) for x in (q, k, v, do))
