"""Constructed inputs, branch census and float64 rounding model for the LSH attention edge tests
(tests/test_lsh_edges_cpu.py, tests/test_lsh_edges_hip.py).  Plain numpy / torch on the CPU.

Three parts:

* BUILDERS.  ``st`` (B*H, R, T) int32 with every round a permutation of 0..T-1 (the attention kernels derive every mask from
  positions; they do not need the hash sort's order), padding masks, and the data kinds ``unit`` / ``ramp(A)``.
* CENSUS.  A pure function of (qk, st, mask, causal, bs) that walks the tile schedule of the forward kernels -- a wave is one
  (chunk, 32-query tile, key half), its tiles are 32 keys each in slot order -- and counts what the inputs make it meet.  It models
  the INPUTS, not the kernel's code: its job is to prove that a case reaches the branch it is listed for.
* MODEL.  The chunked forward and backward of the formulas in the header of csrc/lsh_attn_bwd.hip in float64, with a bf16 rounding
  wherever the kernels round.  With the roundings off it is the exact function (the CPU file holds it to the oracle's autograd).
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

DH = 64
B, H = 2, 2
LOG2E = 1.4426950408889634
SELF_LOGIT = -5e4
SLACK_LOG2 = 8.0            # a tile moves the running reference when it exceeds it by more than this many log2 units
RAMP_A = 80.0

FAMILIES = ("ascending", "descending", "echo", "random")

Case = namedtuple("Case", "family t bs rounds causal masked fwd_walk")


def case_id(c: Case) -> str:
    return f"{c.family}-T{c.t}-bs{c.bs}-R{c.rounds}-{'causal' if c.causal else 'full'}-{'masked' if c.masked else 'dense'}-fw{c.fwd_walk}"


def _cases():
    """{family} x {causal, not} x {masked, not} at (T=256, bs=64): all 16; at (T=512, bs=128): the 8 listed.  Rounds 2..4 (the ring
    of R * T / bs = 8, 12 or 16 chunks is divisible by the run lengths 1, 2 and 4); the walking forward runs at 4 on the masked
    cases and at 2 on the others."""
    rounds_a = {"ascending": 2, "descending": 3, "echo": 4, "random": 2}
    rounds_b = {"ascending": 3, "descending": 2, "echo": 2, "random": 4}
    out = []
    for fam in FAMILIES:
        for causal in (True, False):
            for masked in (True, False):
                out.append(Case(fam, 256, 64, rounds_a[fam], causal, masked, 4 if masked else 2))
    for fam, causal, masked in (("ascending", True, True), ("ascending", True, False), ("ascending", False, True),
                                ("descending", True, False), ("descending", False, True), ("echo", True, True),
                                ("echo", False, False), ("random", True, True)):
        out.append(Case(fam, 512, 128, rounds_b[fam], causal, masked, 4 if masked else 2))
    return out


CASES = _cases()
DATA_KINDS = ("unit", "ramp")


# ---------------------------------------------------------------------------------------------------------------- builders
def make_st(family: str, t: int, bs: int, rounds: int, seed: int = 0) -> torch.Tensor:
    """(B*H, R, T) int32.  Every (batch, head) row gets its own variant: ``ascending`` / ``descending`` are rotated by a whole number
    of chunks (row i by i chunks: every property of the family survives, but the seam -- the chunk that looks back at the far end
    of the sequence -- sits at another place of the ring and of a run), ``echo`` / ``random`` are drawn from another seed."""
    nb = t // bs
    g = torch.Generator().manual_seed(1000 + seed)
    rows = []
    for i in range(B * H):
        if family in ("ascending", "descending"):
            base = torch.arange(t) if family == "ascending" else torch.arange(t - 1, -1, -1)
            base = torch.roll(base, shifts=(i % nb) * bs)
            rows.append(base.expand(rounds, t).clone())
        elif family == "random":
            rows.append(torch.stack([torch.randperm(t, generator=g) for _ in range(rounds)]))
        elif family == "echo":
            # disjoint blocks E_0 .. E_{R-1} of bs tokens; round r begins with E_{r-1} (E_{R-1} for round 0) and ends with E_r, the
            # rest in random order between them.  The first chunk of every round then looks back at a chunk of the same tokens (in
            # another order): every query of it finds itself among the looked-back keys.  The blocks are ranges of positions taken
            # in turn from the end and from the start of the sequence (E_0 = the last bs positions, E_1 = the first bs, ...): under
            # a padding mask E_0 is a chunk of padded tokens only, each of which meets itself in both chunks, and E_1 is all valid.
            assert rounds * bs <= t
            blocks = []
            for r in range(rounds):
                lo = t - (r // 2 + 1) * bs if r % 2 == 0 else (r // 2) * bs
                blocks.append(torch.arange(lo, lo + bs))
            rs = []
            for r in range(rounds):
                head, tail = blocks[(r - 1) % rounds], blocks[r]
                used = torch.zeros(t, dtype=torch.bool)
                used[head] = True
                used[tail] = True
                rest = torch.nonzero(~used).flatten()
                rest = rest[torch.randperm(rest.numel(), generator=g)]
                rs.append(torch.cat([head[torch.randperm(bs, generator=g)], rest, tail]))
            rows.append(torch.stack(rs))
        else:
            raise ValueError(family)
    st = torch.stack(rows).to(torch.int32)
    check_st(st, t)
    return st


def check_st(st: torch.Tensor, t: int) -> None:
    """Every round of every row is a permutation of 0..T-1 (an index outside would make a kernel read out of bounds): asserted on the
    host before anything is launched."""
    assert st.dtype == torch.int32 and st.dim() == 3 and st.shape[2] == t, (st.dtype, st.shape)
    assert int(st.min()) >= 0 and int(st.max()) < t
    want = torch.arange(t, dtype=torch.int32).expand_as(st)
    assert torch.equal(st.sort(dim=-1).values, want), "a round of st is not a permutation of 0..T-1"


def make_mask(t: int, bs: int) -> torch.Tensor:
    """(B, T) bool, valid lengths (T - T//3, bs + 6): with ``ascending`` whole chunks of padded tokens, one chunk with 6 valid and
    bs - 6 padded tokens, and a valid first chunk of a round that looks back at a wholly padded chunk."""
    m = torch.zeros(B, t, dtype=torch.bool)
    for b, n in enumerate((t - t // 3, bs + 6)):
        m[b, :n] = True
    return m


def make_qkv(kind: str, t: int, seed: int = 0) -> torch.Tensor:
    """(B, T, 2*H*dh) bf16 = [qk | v].  ``unit``: randn, as in test_lsh_hip.py.  ``ramp``: in every head token i lies at angle
    pi * i / T in the plane of dimensions 0 and 1, scaled by 8 A, plus 0.02 * 8 A * randn in all 64 dimensions (logits are
    A cos(angle difference) nats: they rise or fall monotonically across a wave's key tiles under ascending / descending); v unit."""
    g = torch.Generator().manual_seed(2000 + seed)
    d = H * DH
    v = torch.randn(B, t, d, generator=g)
    if kind == "unit":
        qk = torch.randn(B, t, d, generator=g)
    elif kind == "ramp":
        amp = 8.0 * RAMP_A
        ang = math.pi * torch.arange(t, dtype=torch.float64) / t
        qk = 0.02 * amp * torch.randn(B, t, H, DH, generator=g)
        qk[..., 0] += (amp * torch.cos(ang)).float().view(1, t, 1)
        qk[..., 1] += (amp * torch.sin(ang)).float().view(1, t, 1)
        qk = qk.view(B, t, d)
    else:
        raise ValueError(kind)
    return torch.cat([qk, v], dim=-1).bfloat16()


def make_dout(t: int, seed: int = 0) -> torch.Tensor:
    return torch.randn(B, t, H * DH, generator=torch.Generator().manual_seed(3000 + seed)).bfloat16()


def heads_first(x: torch.Tensor, h: int = H) -> torch.Tensor:
    """(B, T, H*dh) -> (B*H, T, dh) float64."""
    b, t, _ = x.shape
    return x.double().reshape(b, t, h, DH).transpose(1, 2).reshape(b * h, t, DH)


def head_mask(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """(B, T) -> (B*H, T)."""
    if mask is None:
        return None
    b, t = mask.shape
    return mask.unsqueeze(1).expand(b, H, t).reshape(b * H, t)


def flat_perm(st: torch.Tensor):
    """st (BH, R, T) -> the oracle's ``sticker`` (flat source index of every sorted slot) and its inverse."""
    bh, nh, t = st.shape
    sticker = (st.long() + (torch.arange(nh) * t).view(1, nh, 1)).reshape(bh, nh * t)
    undo = torch.empty_like(sticker)
    undo.scatter_(1, sticker, torch.arange(nh * t).expand(bh, -1))
    return sticker, undo


def build(case: Case, kind: str):
    """-> dict(qkv bf16 (B,T,2Hdh), st, mask (B,T) | None, dout) of one case; deterministic."""
    seed = CASES.index(case)
    return dict(qkv=make_qkv(kind, case.t, seed), st=make_st(case.family, case.t, case.bs, case.rounds, seed),
                mask=make_mask(case.t, case.bs) if case.masked else None, dout=make_dout(case.t, seed))


# ------------------------------------------------------------------------------------------------------------------ census
CENSUS_KEYS = ("waves", "live_waves", "empty_waves", "rescales", "rescale_waves", "dead_tiles", "live_tiles", "mixed_tiles",
               "wrap_self_pairs", "self_only", "padded_chunks")


def census(qk: torch.Tensor, st: torch.Tensor, mask: Optional[torch.Tensor], causal: bool, bs: int) -> dict:
    """qk (BH, T, dh), st (BH, R, T), mask (BH, T) bool | None.  Counts over all (batch, head) rows:

    waves / live_waves / empty_waves   waves in all; with a visible key that is not the query itself; with no visible key at all,
                                       the query itself included (such a wave ends as it began and is merged)
    rescales / rescale_waves           tiles whose maximum exceeds the running reference of some query of the wave by more than 8 log2
                                       units AFTER that query has met a visible key other than itself (the reference then moves to
                                       the new maximum for the whole wave); waves with at least one such tile
    dead_tiles / live_tiles / mixed    32 x 32 tiles with every pair masked (and none the query itself) / no pair masked / the rest
    wrap_self_pairs                    (query, looked-back key) pairs that are the same token
    self_only                          (round, row) pairs whose query sees no key but itself
    padded_chunks                      chunks without a valid token

    plus ``per_round_empty`` (R,): empty waves among the chunks of each round, ``wrap_self_per_boundary``: pairs per (row, chunk)
    that has any, ``self_only_rows`` (BH, T) bool: self-only in EVERY round, and ``self_count`` (BH, T): how often such a row meets
    itself over all rounds (R, or more where a round shows it the same token in both chunks)."""
    bh_n, t, dh = qk.shape
    rounds = st.shape[1]
    nb = t // bs
    n_chunks = rounds * nb
    nt = bs // 32
    q64 = qk.double().numpy()
    stn = st.numpy().astype(np.int64)
    mk = None if mask is None else mask.numpy().astype(bool)
    big = 1 << 30
    out = dict.fromkeys(CENSUS_KEYS, 0)
    per_round_empty = np.zeros(rounds, dtype=np.int64)
    wrap_per_boundary = []
    self_only_rt = np.zeros((bh_n, rounds, t), dtype=bool)
    self_count = np.zeros((bh_n, t), dtype=np.int64)
    for bh in range(bh_n):
        norm = np.maximum(np.linalg.norm(q64[bh], axis=-1), 1e-12)
        chunks = stn[bh].reshape(n_chunks, bs)
        for c in range(n_chunks):
            qpos = chunks[c]
            kpos = np.concatenate([chunks[c], chunks[c - 1]])
            qv = np.ones(bs, bool) if mk is None else mk[bh, qpos]
            kv = np.ones(2 * bs, bool) if mk is None else mk[bh, kpos]
            if not qv.any():
                out["padded_chunks"] += 1
            qpe = np.where(qv, qpos if causal else 0, -1)
            kpe = np.where(kv, kpos if causal else 0, big)
            dead = kpe[None, :] > qpe[:, None]
            same = kpos[None, :] == qpos[:, None]
            x = (q64[bh, qpos] @ q64[bh, kpos].T) * (dh ** -0.5 * LOG2E / norm[kpos])[None, :]
            x = np.where(dead, -np.inf, x)
            x = np.where(same, SELF_LOGIT * LOG2E, x)
            seen = ~dead & ~same                      # visible keys other than the query itself
            r_idx = c // nb
            self_only_rt[bh, r_idx, qpos] = ~seen.any(axis=1)
            np.add.at(self_count[bh], qpos, same.sum(axis=1))
            wrap_pairs = int(same[:, bs:].sum())
            out["wrap_self_pairs"] += wrap_pairs
            if wrap_pairs:
                wrap_per_boundary.append(wrap_pairs)
            for qt in range(nt):
                qs = slice(qt * 32, qt * 32 + 32)
                for kh in range(2):
                    out["waves"] += 1
                    m = np.full(32, -np.inf)
                    had_rescale = False
                    wave_seen = False
                    wave_any = False
                    for tile in range(nt):
                        ks = slice(kh * bs + tile * 32, kh * bs + tile * 32 + 32)
                        d_t, s_t, x_t = dead[qs, ks], same[qs, ks], x[qs, ks]
                        if d_t.all() and not s_t.any():
                            out["dead_tiles"] += 1
                        elif not d_t.any():
                            out["live_tiles"] += 1
                        else:
                            out["mixed_tiles"] += 1
                        wave_seen |= bool(seen[qs, ks].any())
                        wave_any |= bool((~d_t | s_t).any())
                        tmax = x_t.max(axis=1)
                        fresh = m < -1e4              # nothing met yet, or only the query itself
                        moves = np.where(fresh, tmax > -np.inf, tmax > m + SLACK_LOG2)
                        if moves.any():
                            if (moves & ~fresh).any():
                                out["rescales"] += 1
                                had_rescale = True
                            m = np.maximum(m, tmax)
                    out["live_waves"] += int(wave_seen)
                    out["rescale_waves"] += int(had_rescale)
                    if not wave_any:
                        out["empty_waves"] += 1
                        per_round_empty[r_idx] += 1
    self_all = self_only_rt.all(axis=1)
    out["self_only"] = int(self_only_rt.sum())
    out["per_round_empty"] = per_round_empty
    out["wrap_self_per_boundary"] = wrap_per_boundary
    out["self_only_rows"] = torch.from_numpy(self_all)
    out["self_count"] = torch.from_numpy(self_count)
    return out


def census_of(case: Case, kind: str) -> dict:
    d = build(case, kind)
    return census(heads_first(d["qkv"][..., :H * DH]), d["st"], head_mask(d["mask"]), case.causal, case.bs)


# What every case is in the list FOR: census key -> smallest count.  test_lsh_edges_cpu.py asserts it; the GPU file builds its
# parametrize list from CASES, so the two cannot drift.
def expectations(case: Case, kind: str) -> dict:
    """-> {name: (predicate over the census, text)} of what the inputs of (case, kind) must reach."""
    assert (case.rounds * (case.t // case.bs)) % 4 == 0, "the ring must be divisible by the run lengths 1, 2 and 4"
    exp = {}
    if kind == "unit":
        exp["no rescale at unit scale (the gap this file closes)"] = lambda z: z["rescales"] == 0
    nb, nt = case.t // case.bs, case.bs // 32
    if case.family == "descending" and case.causal:
        # Every chunk but one per round looks back at a chunk wholly in the future, and inside the own chunk the keys a query may
        # see come in the order of growing distance: the ramp's logits FALL across the tiles of every live wave, so these inputs
        # cannot reach a rescale (the census counts 0) whatever the amplitude.  They are in the list for the empty key halves.
        exp["an empty key half for every chunk but one per round"] = lambda z: z["empty_waves"] >= B * H * case.rounds * (nb - 1) * nt
    elif kind == "ramp" and case.family in ("ascending", "descending"):
        exp["rescale after the first live tile in >= 1/4 of the live waves"] = lambda z: 4 * z["rescale_waves"] >= z["live_waves"] > 0
    if case.family == "ascending" and case.causal:
        exp["an empty key half in every round"] = lambda z: bool((z["per_round_empty"] >= 1).all())
        exp["wholly dead and wholly live tiles"] = lambda z: z["dead_tiles"] > 0 and z["live_tiles"] > 0
        exp["a row that sees only itself in every round"] = lambda z: int(z["self_only_rows"].sum()) >= B * H
    if case.family == "echo":
        exp["bs wrap-self pairs at every round boundary"] = lambda z: (
            len(z["wrap_self_per_boundary"]) == B * H * case.rounds and all(p == case.bs for p in z["wrap_self_per_boundary"]))
    elif case.family != "random":
        exp["no wrap-self pair"] = lambda z: z["wrap_self_pairs"] == 0
    if case.masked:
        if case.family != "random":           # a random round mixes valid and padded tokens in every chunk: the control has none
            exp["a chunk without a valid token"] = lambda z: z["padded_chunks"] >= 1
        if case.family == "echo":
            exp["a chunk of padded tokens that all meet themselves in both chunks"] = lambda z: int(
                (z["self_count"][z["self_only_rows"]] > case.rounds).sum()) >= B * H * case.bs
        exp["padded rows see only themselves"] = lambda z: int(z["self_only_rows"].sum()) >= H * ((case.t // 3) + case.t - case.bs - 6)
    return exp


# ------------------------------------------------------------------------------------------------------ float64 rounding model
def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.float().bfloat16().double()


def lsh_model(qk, v, st, bs: int, causal: bool, mask, dout, rounding: bool = True, out_given=None, lse_tot_given=None):
    """Chunked forward and backward of LSH attention in float64 (formulas: header of csrc/lsh_attn_bwd.hip).  qk, v, dout (BH, T, dh)
    float64 (bf16 values), st (BH, R, T), mask (BH, T) bool | None.  ``rounding``: a bf16 rounding wherever the kernels round --
    the probabilities before P V, o, out, P' and dS' as MFMA operands, dQ when it is parked beside the own keys' dK, the partial rows
    (own rows: dQ + dK and dV of the own keys; looked-back rows: dK and dV), the final dqk and dv.  Off: the exact function.
    -> dict(o (BH,R,T,dh), lse (BH,R,T), out, lse_tot, dqk, dv)."""
    rb = _bf16 if rounding else (lambda z: z)
    bh_n, t, dh = qk.shape
    rounds = st.shape[1]
    nb = t // bs
    n_chunks = rounds * nb
    bi = torch.arange(bh_n).view(bh_n, 1, 1)
    pos = st.long().reshape(bh_n, n_chunks, bs)
    ppos = torch.roll(pos, 1, dims=1)
    kpos = torch.cat([pos, ppos], dim=2)
    q = qk[bi, pos]                                             # (BH, C, bs, dh)
    k = qk[bi, kpos]                                            # (BH, C, 2bs, dh)
    vv = v[bi, kpos]
    kn = k.norm(dim=-1).clamp_min(1e-12)
    ksc = dh ** -0.5 / kn
    s = torch.einsum("bcqd,bckd->bcqk", q, k) * ksc.unsqueeze(2)
    valid = torch.ones(bh_n, t, dtype=torch.bool) if mask is None else mask
    qv, kv = valid[bi, pos], valid[bi, kpos]
    zero = torch.zeros_like(pos)
    qpe = torch.where(qv, pos if causal else zero, zero - 1)
    kpe = torch.where(kv, kpos if causal else torch.zeros_like(kpos), torch.full_like(kpos, 1 << 30))
    dead = kpe.unsqueeze(2) > qpe.unsqueeze(3)
    same = kpos.unsqueeze(2) == pos.unsqueeze(3)
    s = s.masked_fill(dead, -math.inf).masked_fill(same, SELF_LOGIT)
    # forward
    mx = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - mx)
    l = p.sum(dim=-1, keepdim=True)
    o_c = rb(torch.einsum("bcqk,bckd->bcqd", rb(p), vv) / l)
    lse_c = (mx + torch.log(l)).squeeze(-1)
    rnd = (torch.arange(n_chunks) // nb).view(1, n_chunks, 1).expand_as(pos)
    prnd = torch.roll(rnd, 1, dims=1)
    o = torch.zeros(bh_n, rounds, t, dh, dtype=torch.float64)
    lse = torch.zeros(bh_n, rounds, t, dtype=torch.float64)
    o[bi, rnd, pos] = o_c
    lse[bi, rnd, pos] = lse_c
    lse_tot = torch.logsumexp(lse, dim=1)
    out = rb((torch.exp(lse - lse_tot.unsqueeze(1)).unsqueeze(-1) * o).sum(dim=1))
    res = dict(o=o, lse=lse, out=out, lse_tot=lse_tot)
    if dout is None:
        return res
    # backward (of sum(out * dout)); the kernels take out and lse_tot from the forward
    out_b = out if out_given is None else out_given
    lt_b = lse_tot if lse_tot_given is None else lse_tot_given
    delta = (out_b * dout).sum(dim=-1)
    pp = torch.exp(s - lt_b[bi, pos].unsqueeze(-1))
    do = dout[bi, pos]
    dp = torch.einsum("bcqd,bckd->bcqk", do, vv)
    dv_k = torch.einsum("bcqk,bcqd->bckd", rb(pp), do)
    ds = (pp * (dp - delta[bi, pos].unsqueeze(-1))).masked_fill(same, 0.0)
    dsp = rb(ds * ksc.unsqueeze(2))
    dq = rb(torch.einsum("bcqk,bckd->bcqd", dsp, k))
    g = torch.einsum("bcqk,bcqd->bckd", dsp, q)
    khat = k / kn.unsqueeze(-1)
    dk = g - khat * (khat * g).sum(dim=-1, keepdim=True)
    dqk_p = torch.zeros(2, bh_n, rounds, t, dh, dtype=torch.float64)
    dv_p = torch.zeros(2, bh_n, rounds, t, dh, dtype=torch.float64)
    dqk_p[0][bi, rnd, pos] = rb(dq + dk[:, :, :bs])
    dqk_p[1][bi, prnd, ppos] = rb(dk[:, :, bs:])
    dv_p[0][bi, rnd, pos] = rb(dv_k[:, :, :bs])
    dv_p[1][bi, prnd, ppos] = rb(dv_k[:, :, bs:])
    res["dqk"] = rb(dqk_p.sum(dim=(0, 2)))
    res["dv"] = rb(dv_p.sum(dim=(0, 2)))
    # sum over rounds of |dQ| + |dK as an own key| + |dK as a looked-back key| (|dV| likewise): what the bf16 roundings of the parked
    # dQ and of the partial rows can move, whichever of these a kernel form adds on chip before it rounds (|a + b| <= |a| + |b|)
    mag_q = torch.zeros(2, bh_n, rounds, t, dh, dtype=torch.float64)
    mag_v = torch.zeros(2, bh_n, rounds, t, dh, dtype=torch.float64)
    mag_q[0][bi, rnd, pos] = dq.abs() + dk[:, :, :bs].abs()
    mag_q[1][bi, prnd, ppos] = dk[:, :, bs:].abs()
    mag_v[0][bi, rnd, pos] = dv_k[:, :, :bs].abs()
    mag_v[1][bi, prnd, ppos] = dv_k[:, :, bs:].abs()
    res["dqk_mag"] = mag_q.sum(dim=(0, 2))
    res["dv_mag"] = mag_v.sum(dim=(0, 2))
    return res


def exact_grads(qk, v, st, bs: int, causal: bool, mask, dout):
    """float64 autograd through oracle.lsh_ref.lsh_attention_sorted on the same permutation -> (out, o, lse, dqk, dv)."""
    from oracle import lsh_ref
    sticker, undo = flat_perm(st)
    qk_r, v_r = qk.clone().requires_grad_(), v.clone().requires_grad_()
    out, o, lse = lsh_ref.lsh_attention_sorted(qk_r, v_r, sticker, undo, bs, st.shape[1], causal, mask, return_parts=True)
    out.backward(dout)
    return out.detach(), o.detach(), lse.detach(), qk_r.grad, v_r.grad


def grad_metrics(got: torch.Tensor, ref: torch.Tensor):
    """(max, mean, rel-L2) of got - ref, the first two in units of max|ref|: the metrics of test_lsh_hip.py's backward test."""
    scale = ref.abs().max().item()
    err = (got - ref).abs()
    return err.max().item() / scale, err.mean().item() / scale, float((got - ref).norm() / ref.norm())
