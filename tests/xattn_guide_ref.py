"""float64 oracle of the guided attention loss inside the cross-attention backward (csrc/xattn.hip: rtts_xattn_guide_rows,
rtts_xattn_guide_fold, rtts_xattn_bwd_guided), its per-element error bounds, and the cases the CPU and GPU tests share.  No GPU
anywhere in this file.  Head width 64 or 128, read off the inputs (tests/xattn_wide_ref.py holds the width-dependent unguided
oracle; ``make_inputs`` picks xattn_ref's or xattn_wide_ref's generator by the width).

Definition, per (sample b, head h), on bf16 VALUES lifted to float64, c_s = 1 / sqrt(dh):

    P      = softmax(c_s q k^T), padded keys 0                    (before the probability dropout)
    W[t,k] = 1 - exp(-(k / K_b - t / T_b)^2 / (2 sigma^2))  for t < T_b and k < K_b, else 0
    rows   = rowsum(P o W)                                        (0 for t >= T_b)
    out[b] = sum_{h,t} rows / (H T_b),     loss = sum_{b,h,t} rows / (H sum_b T_b),     c = coef / (H sum_b T_b)
    dS     = c_s P o (keep o (dO V^T) + c W - (delta + c rows))
    dQ = dS K,   dK = dS^T Q,   dV = (keep o P)^T dO              (dV is the unguided one)

A slot with T_b outside 1..T_q or K_b outside 1..T_k counts in no sum (its W is 0, its out[b] is 0); if no slot counts, loss = c = 0.
dS is the gradient of sum(o . dO) + coef * loss with respect to the logits: d/dS of c sum_k P_k W_k is c P o (W - rows).

Error bounds: the formulas of xattn_ref.reference / xattn_wide_ref.reference with dS replaced by the guided dS.  The kernel rounds
where the unguided kernel rounds (dS to bf16 for the dK MFMA and the dS^T image, the slabs, the shares and their sums); rows, c and
W stay fp32 (2^-24 relative, four orders of magnitude below u = 2^-8) and add no term:

    E    = u |dS| + c_s P d_delta              d_delta = sum_d B_o |dO|   (delta is the row sum over the kernel's rounded o)
    dQ   : E |K| + u |dQ| + [bwd chunks > 1] u (|dS||K|)
    dK   : E^T |Q| + u sum_slabs(|dS|^T |Q|) + u |dK|
    dV   : 2u (keep o P)^T |dO| + u |dV|"""
import math

import torch

import xattn_ref as X
import xattn_wide_ref as XW

U = X.U

# (B, H, T_q, T_k, dh, input kind, kvalid pattern, T_b per sample, K_b per sample, dropout (p, seed, seed_dev) or None).
# T_b walks {1, 127, 128, 129, T_q} and K_b {1, 128, 129, T_k - 37, T_k} so that both cross a 128 boundary (a query block, a key
# chunk); T_b = 0 (case 1, sample 2; case 5, sample 1) and K_b = T_k + 1 (case 2, sample 1; case 7, sample 0) do not count.
CASES = [
    (1, 1, 128, 128, 64, "plain", "none", (127,), (91,), None),
    (3, 2, 128, 256, 64, "peaked", "ragged", (128, 1, 0), (129, 256, 219), None),
    (3, 1, 256, 384, 64, "offset+", "none", (129, 256, 127), (128, 385, 1), (0.5, 0x9E3779B1, 7)),
    (1, 3, 384, 1152, 64, "plain", "ragged", (384,), (1115,), None),
    (3, 2, 128, 2048, 64, "offset+", "none", (128, 127, 1), (2048, 129, 2011), None),
    (3, 1, 128, 128, 128, "offset+", "ragged", (128, 0, 127), (128, 1, 91), None),
    (1, 2, 256, 256, 128, "plain", "none", (129,), (219,), None),
    (3, 1, 128, 384, 128, "peaked", "ragged", (1, 128, 127), (385, 129, 347), None),
]
IDS = [f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-dh{c[4]}-{c[5]}-{c[6]}" for c in CASES]
SIGMA = 0.2
# c = coef / (H sum_b T_b) of every case: large enough that a kernel without the guided term misses the bounds by 8x in dq and
# in dk (tests/test_xattn_guide_cpu.py asserts it).  Peaked rows are nearly one-hot, where P o (W - rows) almost cancels: at 2048
# keys a peaked case would need c in the thousands for dq, so the peaked cases are the short ones.
C_TARGET = 32.0


def counts(n_frames, n_keys, tq, tk):
    """Per slot: does it count (T_b in 1..T_q and K_b in 1..T_k)?"""
    return [1 <= int(t) <= tq and 1 <= int(k) <= tk for t, k in zip(n_frames, n_keys)]


def frames(n_frames, n_keys, tq, tk):
    return sum(int(t) for t, ok in zip(n_frames, counts(n_frames, n_keys, tq, tk)) if ok)


def case_coef(case):
    """coef of a case: C_TARGET times H sum_b T_b."""
    nb, nh, tq, tk, dh, kind, pattern, nf, nk, drop = case
    return C_TARGET * nh * frames(nf, nk, tq, tk)


def make_inputs(kind, nb, nh, tq, tk, seed, dh):
    return X.make_inputs(kind, nb, nh, tq, tk, seed) if dh == 64 else XW.make_inputs(kind, nb, nh, tq, tk, seed, dh)


def case_inputs(i):
    """-> (inputs (q, k, v, do), valid, keep (B, H, T_q, T_k) f64 or None) of CASES[i]."""
    nb, nh, tq, tk, dh, kind, pattern, nf, nk, drop = CASES[i]
    inputs = make_inputs(kind, nb, nh, tq, tk, 4242 + 17 * i, dh)
    valid = X.make_valid(pattern, nb, tk)
    keep = None if drop is None else X.keep_scales(*drop, nb * nh, tq, tk).view(nb, nh, tq, tk)
    return inputs, valid, keep


def weights(n_frames, n_keys, tq, tk, sigma):
    """W (B, T_q, T_k) float64."""
    w = torch.zeros(len(n_frames), tq, tk, dtype=torch.float64)
    for b, ok in enumerate(counts(n_frames, n_keys, tq, tk)):
        if ok:
            t, k = int(n_frames[b]), int(n_keys[b])
            tt = torch.arange(t, dtype=torch.float64).view(t, 1) / t
            kk = torch.arange(k, dtype=torch.float64).view(1, k) / k
            w[b, :t, :k] = 1.0 - torch.exp(-((kk - tt) ** 2) / (2.0 * sigma * sigma))
    return w


def reference(q, k, v, do, valid, keep, n_frames, n_keys, sigma, coef):
    """q, do (B, H, Tq, dh); k, v (B, H, Tk, dh); valid (B, Tk) bool or None; keep (B, H, Tq, Tk) or None.  Returns float64 tensors:
    o, lse, delta, p_mean (B, Tq, Tk), rows (B, H, Tq), out (B + 1,), loss, c, dq, dk, dv, the bounds b_dq, b_dk, b_dv, and
    lse_scale (as xattn_wide_ref.reference)."""
    dh = q.shape[-1]
    assert dh in (64, 128)
    root = math.sqrt(dh)
    q, k, v, do = (x.double() for x in (q, k, v, do))
    nb, nh, tq, tk = q.shape[0], q.shape[1], q.shape[2], k.shape[2]
    multi = tk // XW.bwd_chunk(tk, dh) > 1
    w = weights(n_frames, n_keys, tq, tk, sigma)
    ok = counts(n_frames, n_keys, tq, tk)
    nfr = frames(n_frames, n_keys, tq, tk)
    c = coef / (nh * nfr) if nfr else 0.0
    res = {n: [] for n in ("o", "lse", "delta", "p_mean", "rows", "dq", "dk", "dv", "b_dq", "b_dk", "b_dv", "lse_scale")}
    out = torch.zeros(nb + 1, dtype=torch.float64)
    total = 0.0
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
        rows = (p * w[b]).sum(-1, keepdim=True)
        ds = p * (dp + c * w[b] - (delta + c * rows)) / root
        dq, dk, dv = ds @ kb, ds.transpose(-1, -2) @ qb, pk.transpose(-1, -2) @ dob
        d_delta = (b_o * dob.abs()).sum(-1, keepdim=True)
        err = U * ds.abs() + p * d_delta / root
        b_dq = err @ kb.abs() + U * dq.abs()
        if multi:
            b_dq = b_dq + U * (ds.abs() @ kb.abs())
        b_dk = err.transpose(-1, -2) @ qb.abs() + U * (ds.abs().transpose(-1, -2) @ qb.abs()) + U * dk.abs()
        b_dv = 2 * U * (pk.transpose(-1, -2) @ dob.abs()) + U * dv.abs()
        if ok[b]:
            out[b] = rows.sum() / (nh * int(n_frames[b]))
            total = total + rows.sum()
        for n, x in (("o", o), ("lse", lse), ("delta", delta.squeeze(-1)), ("p_mean", p.mean(0)), ("rows", rows.squeeze(-1)), ("dq", dq),
                     ("dk", dk), ("dv", dv), ("b_dq", b_dq), ("b_dk", b_dk), ("b_dv", b_dv),
                     ("lse_scale", aqk.max(-1).values + lse.abs() + 1.0)):
            res[n].append(x)
    res = {n: torch.stack(x) for n, x in res.items()}
    loss = total / (nh * nfr) if nfr else torch.zeros((), dtype=torch.float64)
    out[nb] = loss
    res.update(out=out, loss=loss, c=c)
    return res


def autograd(q, k, v, do, valid, keep, n_frames, n_keys, sigma, coef):
    """float64 autograd of sum(o . dO) + coef * sum(P o W) / (H sum_b T_b) -> (dq, dk, dv, loss)."""
    dh = q.shape[-1]
    q, k, v = (x.double().clone().requires_grad_(True) for x in (q, k, v))
    do = do.double()
    nb, nh, tq, tk = q.shape[0], q.shape[1], q.shape[2], k.shape[2]
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if valid is not None:
        s = s.masked_fill(~valid.view(nb, 1, 1, tk), float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = (p if keep is None else p * keep.double()) @ v
    nfr = frames(n_frames, n_keys, tq, tk)
    w = weights(n_frames, n_keys, tq, tk, sigma).view(nb, 1, tq, tk)
    loss = (p * w).sum() / (nh * nfr) if nfr else (p * 0.0).sum()
    ((o * do).sum() + coef * loss).backward()
    return q.grad, k.grad, v.grad, loss.detach()


def ratios(got, ref, names=("dq", "dk", "dv")):
    """Worst |got - ref| / bound per quantity (0 / 0 counts as 0, anything over a zero bound as inf)."""
    out = {}
    for n in names:
        err = (got[n].double() - ref[n]).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / ref["b_" + n])
        out[n] = float(ratio.max()) if not torch.isnan(ratio).any() else float("nan")
    return out


def rows_ratio(got_rows, ref):
    """Worst |rows - float64| / (2^-24 lse_scale rowsum): the C a bound C 2^-24 lse_scale (row sum) needs (0 / 0 counts as 0).  The
    row sum is that of P o W; P = exp(s - lse) carries the fp32 error of its exponent, whose scale lse_scale is."""
    err = (got_rows.double() - ref["rows"]).abs()
    unit = 2.0 ** -24 * ref["lse_scale"] * ref["rows"]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / unit)
    return float(ratio.max())
