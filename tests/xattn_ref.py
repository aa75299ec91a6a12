"""float64 oracle of dense encoder-decoder attention (csrc/xattn.hip: rtts_xattn_fwd, rtts_xattn_bwd, rtts_sum_slabs and the
rtts_lsh_bwd_delta it borrows), the numpy twin of its dropout mask, per-element first-order error bounds of the kernels'
roundings, and an fp32 / bf16 torch model of the kernels' data flow with switchable defects (no GPU anywhere in this file).

All tensors are (B, H, T, 64); the inputs are bf16 VALUES lifted to float64, so what separates the kernels from ``reference`` is
the kernels' own arithmetic only.

Exact quantities (``reference``), per (sample, head):

    s     = q k^T / 8,  padded keys -inf          P = softmax(s),  lse = logsumexp(s)
    o     = (keep o P) V                          delta = rowsum(o o dO)
    dS    = P o (keep o (dO V^T) - delta) / 8
    dQ    = dS K,   dK = dS^T Q,   dV = (keep o P)^T dO

``keep`` (``keep_scales``) is rebuilt from ``oracle.synth.drop_hash``, never read back from a kernel: element (bh, query, key)
has the index (bh T_q + query) T_k + key (the GLOBAL key, xattn.hip:193-198 forward, :378-380 backward) in uint32 arithmetic,
the effective seed is seed + *seed_dev (:118, :258), it is kept iff hash >= int(float32(p) 2^32) (rtts_common.h
rtts_drop_thresh) and a kept element carries float32(1) / (float32(1) - float32(p)) (the launchers' ``1.f / (1.f - drop_p)``).

Error bounds.  u = 2^-8 is the unit roundoff of bf16 (half an ulp relative to the value at the bottom of a binade; 2^-9 is the
average, not the bound).  The fp32 arithmetic between the roundings (MFMA accumulation, exp, the fp32 slab sums) is three to
four orders of magnitude below u and is not counted.  Each constant below counts roundings to bf16, with their source line:

    o   : 2u (keep o P)|V|
            1. P~ keep, the unnormalised probability times the keep-scale, rounded before the P V MFMA  (cvt_bf16x8, :205)
            2. o rounded on store                                                   (at_store_rows of attn_tile.h -> pack_bf16x2)
    delta: d_delta = sum_d B_o |dO|     delta is the rowsum over the KERNEL's rounded o (lsh_combine.hip:74-77), as the engine
                                        forms it; its own 64 fp32 fmas are not counted
    dS  : E = u |dS| + P d_delta / 8
            3. dS rounded for the dK MFMA and for the dS^T image in LDS -- the same value both times   (cvt_bf16x8 :390,
               pack_bf16x2 :400-401); the second term is the delta error carried through dS = P (. - delta) / 8   (:382)
    dQ  : E |K| + u |dQ| + [chunks > 1] u (|dS||K|)
            4. one chunk: dQ rounded on store (:463-464).  More chunks: every chunk's SHARE is rounded on store (the same
               lines, u sum_c |share_c| <= u |dS||K|) and the sum of the shares is rounded again by rtts_sum_slabs (:485-488)
    dK  : E^T |Q| + u sum_slabs(|dS|^T |Q|) + u |dK|
            5. every query block's slab rounded on store (at_store_rows)          6. the slab sum rounded (:485-488)
    dV  : 2u (keep o P)^T |dO| + u |dV|
            7. P keep rounded before the dV MFMA (:389)   8. slab rounded on store (:419)   9. the slab sum rounded (:485-488)

A padded key has P = 0 and therefore dK = dV = 0 with a bound of exactly 0.  A sample without any valid key is NaN throughout
(``reference`` and nn.MultiheadAttention alike); the callers keep its rows out of the comparison.

``kernel_model`` walks the key chunks with a running maximum and normaliser, rounds where the kernels round and forms per-chunk dQ
shares and per-query-block slabs, in fp32 / bf16 torch.  tests/test_xattn_cpu.py holds it to the bounds on every input kind
(``make_inputs``) and requires each ``defect`` to break one."""
import numpy as np
import torch

from oracle.synth import drop_hash

DH = 64
QB = 128                # queries per workgroup = per dK/dV slab
U = 2.0 ** -8
DEFECTS = ("a", "b", "c", "d", "e", "f", "g")
KINDS = ("plain", "peaked", "offset+", "offset-")


def key_chunk(tk: int) -> int:
    """Keys held on chip at a time (xattn.hip xa_chunk)."""
    return 256 if tk % 256 == 0 else 128


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def keep_scales(p: float, seed: int, seed_dev, bh: int, tq: int, tk: int, local_chunk: int = 0) -> torch.Tensor:
    """(bh, tq, tk) float64 keep-scales of the probability dropout as the kernels draw them.  ``local_chunk`` > 0 is defect (a):
    the key's position within its chunk instead of the global key."""
    eff = (int(seed) + (0 if seed_dev is None else int(seed_dev))) & 0xFFFFFFFF
    key = np.arange(tk, dtype=np.uint64)
    if local_chunk:
        key = key % np.uint64(local_chunk)
    row = np.arange(bh * tq, dtype=np.uint64)[:, None] * np.uint64(tk)
    h = drop_hash(eff, (row + key[None, :]) & np.uint64(0xFFFFFFFF))
    thresh = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy((h >= thresh).astype(np.float64) * scale).view(bh, tq, tk)


def reference(q, k, v, do, valid=None, keep=None):
    """q, do (B, H, Tq, 64); k, v (B, H, Tk, 64); valid (B, Tk) bool or None; keep (B, H, Tq, Tk) or None.  Returns a dict of
    float64 tensors: o, lse, delta, dq, dk, dv, the bounds b_o, b_dq, b_dk, b_dv, and lse_scale = max_j sum_d |q_d k_jd| / 8 +
    |lse| + 1 (the scale of the fp32 error of lse)."""
    q, k, v, do = (x.double() for x in (q, k, v, do))
    nb, tk = q.shape[0], k.shape[2]
    multi = tk // key_chunk(tk) > 1
    res = {n: [] for n in ("o", "lse", "delta", "dq", "dk", "dv", "b_o", "b_dq", "b_dk", "b_dv", "lse_scale")}
    for b in range(nb):                                 # one sample at a time: the (H, Tq, Tk) matrices of the largest case stay small
        qb, kb, vb, dob = q[b], k[b], v[b], do[b]
        s = qb @ kb.transpose(-1, -2) / 8.0
        aqk = qb.abs() @ kb.abs().transpose(-1, -2) / 8.0
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
        ds = p * (dp - delta) / 8.0
        dq, dk, dv = ds @ kb, ds.transpose(-1, -2) @ qb, pk.transpose(-1, -2) @ dob
        d_delta = (b_o * dob.abs()).sum(-1, keepdim=True)
        err = U * ds.abs() + p * d_delta / 8.0
        b_dq = err @ kb.abs() + U * dq.abs()
        if multi:
            b_dq = b_dq + U * (ds.abs() @ kb.abs())
        b_dk = err.transpose(-1, -2) @ qb.abs() + U * (ds.abs().transpose(-1, -2) @ qb.abs()) + U * dk.abs()
        b_dv = 2 * U * (pk.transpose(-1, -2) @ dob.abs()) + U * dv.abs()
        for n, x in (("o", o), ("lse", lse), ("delta", delta.squeeze(-1)), ("dq", dq), ("dk", dk), ("dv", dv), ("b_o", b_o),
                     ("b_dq", b_dq), ("b_dk", b_dk), ("b_dv", b_dv), ("lse_scale", aqk.max(-1).values + lse.abs() + 1.0)):
            res[n].append(x)
    return {n: torch.stack(x) for n, x in res.items()}


def kernel_model(q, k, v, do, valid=None, drop=None, defect=None):
    """fp32 / bf16 model of the kernels' data flow.  ``drop`` = (p, seed, seed_dev) or None; ``defect`` switches in ONE
    deliberate error:
      a  the dropout index uses the key's position within its chunk      b  the alpha rescale of oacc is skipped for one chunk
      c  kvalid is read one key late                                     d  two neighbouring 32-query tiles of o are swapped
      e  dS is missing the 1/8                                           f  the last query block's slab is left out of dK
      g  delta is taken from the float64 o, times 1.02
    Returns o, lse, dq, dk, dv (float32)."""
    assert defect is None or defect in DEFECTS
    q, k, v, do = (x.float() for x in (q, k, v, do))
    nb, nh, tq, _ = q.shape
    tk = k.shape[2]
    chunk = key_chunk(tk)
    nch, nqb = tk // chunk, tq // QB
    if valid is None:
        valid = torch.ones(nb, tk, dtype=torch.bool)
    if defect == "c":
        valid = torch.cat([valid[:, 1:], valid[:, -1:]], dim=1)
    if drop is None:
        keep = torch.ones(nb, nh, tq, tk)
    else:
        keep = keep_scales(drop[0], drop[1], drop[2], nb * nh, tq, tk, local_chunk=chunk if defect == "a" else 0)
        keep = keep.float().view(nb, nh, tq, tk)
    pad = ~valid.view(nb, 1, 1, tk)
    s = ((q @ k.transpose(-1, -2)) * 0.125).masked_fill(pad, float("-inf"))
    # forward: chunk walk with a running maximum and normaliser (xattn.hip:124-216)
    big = torch.finfo(torch.float32).max
    m_run = torch.full((nb, nh, tq, 1), -big)
    l_run = torch.zeros(nb, nh, tq, 1)
    oacc = torch.zeros(nb, nh, tq, DH)
    for c in range(nch):
        sl = slice(c * chunk, (c + 1) * chunk)
        sc = s[..., sl]
        m = torch.maximum(sc.max(-1, keepdim=True).values, m_run)
        alpha = torch.where(m_run == -big, torch.zeros_like(m), torch.exp(m_run - m))
        pt = torch.where(torch.isinf(sc), torch.zeros_like(sc), torch.exp(sc - m))
        l_run = l_run * alpha + pt.sum(-1, keepdim=True)
        m_run = m
        if not (defect == "b" and c == min(1, nch - 1) and nch > 1):
            oacc = oacc * alpha
        oacc = oacc + bf(pt * keep[..., sl]) @ v[..., sl, :]
    o = bf(oacc / l_run)
    lse = (m_run + torch.log(l_run)).squeeze(-1)
    if defect == "d":
        o = torch.cat([o[..., 32:64, :], o[..., 0:32, :], o[..., 64:, :]], dim=-2)
    # backward: P from the forward's lse, delta from the rounded o (xattn.hip:341-405)
    if defect == "g":
        delta = (1.02 * (reference(q, k, v, do, valid, None if drop is None else keep)["o"] * do.double()).sum(-1, keepdim=True)).float()
    else:
        delta = (o * do).sum(-1, keepdim=True)
    p = torch.exp(s - lse.unsqueeze(-1))
    ds = p * ((do @ v.transpose(-1, -2)) * keep - delta) * (1.0 if defect == "e" else 0.125)
    dsb, pb = bf(ds), bf(p * keep)
    shares = [bf(dsb[..., c * chunk:(c + 1) * chunk] @ k[..., c * chunk:(c + 1) * chunk, :]) for c in range(nch)]
    dq = shares[0] if nch == 1 else bf(sum(shares))
    rows = [slice(i * QB, (i + 1) * QB) for i in range(nqb)]
    slabs_k = [bf(dsb[..., r, :].transpose(-1, -2) @ q[..., r, :]) for r in rows]
    slabs_v = [bf(pb[..., r, :].transpose(-1, -2) @ do[..., r, :]) for r in rows]
    if defect == "f":
        slabs_k = slabs_k[:-1] or [torch.zeros_like(slabs_k[0])]
    return dict(o=o, lse=lse, dq=dq, dk=bf(sum(slabs_k)), dv=bf(sum(slabs_v)))


def ratios(got, ref, rows=None):
    """Worst |got - ref| / bound per quantity (0 / 0 counts as 0, anything over a zero bound as inf).  ``rows``: the samples
    to look at (default all)."""
    out = {}
    for n in ("o", "dq", "dk", "dv"):
        g, r, b = got[n].double(), ref[n], ref["b_" + n]
        if rows is not None:
            g, r, b = g[rows], r[rows], b[rows]
        err = (g - r).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
        out[n] = float(ratio.max()) if not torch.isnan(ratio).any() else float("nan")
    return out


def lse_ratio(got_lse, ref, rows=None):
    """Worst |lse - ref| / (2^-24 lse_scale): the ``c`` an lse bound c 2^-24 (max_j sum_d |q_d k_jd| / 8 + |lse| + 1) needs."""
    g, r, sc = got_lse.double(), ref["lse"], ref["lse_scale"]
    if rows is not None:
        g, r, sc = g[rows], r[rows], sc[rows]
    return float(((g - r).abs() / (2.0 ** -24 * sc)).max())


def make_valid(pattern, nb: int, tk: int):
    """Key validity (B, Tk) bool, or None: 'none', 'ragged' (ends inside a chunk, another length per sample), 'first' / 'middle' /
    'last' (that whole chunk of sample 0 -- and of every other even sample -- is padding, the others end ragged), 'one'
    (exactly one valid key: key 0 in sample 0, key Tk - 1 in sample 1; with one sample: key Tk - 1), 'alternating'."""
    if pattern == "none":
        return None
    chunk = key_chunk(tk)
    nch = tk // chunk
    valid = torch.ones(nb, tk, dtype=torch.bool)
    if pattern == "alternating":
        valid[:, 1::2] = False
        valid[1::2] = ~valid[1::2]
    elif pattern == "one":
        valid[:2] = False
        valid[0, 0 if nb > 1 else tk - 1] = True
        if nb > 1:
            valid[1, tk - 1] = True
    else:
        for b in range(nb):
            valid[b, tk - 37 - 29 * b:] = False
        if pattern != "ragged":
            c = {"first": 0, "middle": nch // 2, "last": nch - 1}[pattern]
            valid[0::2] = True
            valid[0::2, c * chunk:(c + 1) * chunk] = False
    return valid


def make_inputs(kind: str, nb: int, nh: int, tq: int, tk: int, seed: int):
    """q, k, v, do as float32 tensors of bf16 values, (B, H, T, 64).
      plain   : randn, q scaled by 1.5
      peaked  : query i matches key (37 i) mod Tk with a logit about 30 above the rest, so the dominant key walks through every
                chunk (first for some queries of a block, last for others); v and do carry a common offset of +1, which makes
                delta = o . do large against its rounding noise (what defect (g) needs to be seen)
      offset+ : a common direction added to q and k puts every logit near +80   (offset-: near -80)"""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nb, nh, tq, DH, generator=g) * 1.5
    k = torch.randn(nb, nh, tk, DH, generator=g)
    v = torch.randn(nb, nh, tk, DH, generator=g)
    do = torch.randn(nb, nh, tq, DH, generator=g)
    if kind == "peaked":
        idx = (torch.arange(tq) * 37) % tk
        k = k * 0.3
        hit = k[:, :, idx, :]
        q = 240.0 * hit / hit.pow(2).sum(-1, keepdim=True) + 0.3 * q
        v, do = v + 1.0, do + 1.0
    elif kind.startswith("offset"):
        c = torch.randn(1, 1, 1, DH, generator=g)
        c = c / c.norm()
        q = q + 25.6 * c
        k = k + (25.0 if kind == "offset+" else -25.0) * c
    return tuple(bf(x) for x in (q, k, v, do))
