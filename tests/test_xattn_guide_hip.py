"""Guided attention loss inside the cross-attention backward (csrc/xattn.hip: rtts_xattn_guide_rows, rtts_xattn_guide_fold,
rtts_xattn_bwd_guided) through the C ABI against the float64 oracle of tests/xattn_guide_ref.py.  Every call goes through
``_lib.call`` in the engine's order: rtts_xattn_fwd, rtts_lsh_bwd_delta on the kernel's own o, rows, fold, the guided backward with
the kernel's own lse, rows and c, rtts_sum_slabs -- and, from the same forward, the unguided rtts_xattn_bwd beside it.

Comparison: |got - float64| <= bound ELEMENT-WISE on dq, dk, dv with the bounds of xattn_guide_ref.py (the unguided roundings,
the guided dS); tests/test_xattn_guide_cpu.py shows that the unguided gradients miss these bounds by 8x and more on every case.
dv is bit-equal to the unguided call's.  rows is fp32 end to end: its bound is ROWS_C 2^-24 lse_scale (row sum), lse_scale =
max_j c_s sum_d |q_d k_jd| + |lse| + 1 (the scale of the fp32 error of the exponent of P).  out and c are held to 1e-6 relative.

Measured on an MI355X, worst |kernel - float64| / bound over the whole file (must be <= 1 for dq, dk, dv):
    dq 0.569   (1x1x128x128 plain, dout = 0)                dk 0.481   (1x2x256x256 dh 128 plain, dout = 0)
    dv 0.613   (3x1x256x384 offset+, dropout 0.5)           rows 1.635 in units of 2^-24 lse_scale (row sum) (3x1x128x384 dh 128 peaked)
    out 6.2e-7 relative (3x2x128x2048 offset+, the slot with T_b = 1)
ROWS_C = 7 is four times the worst rows ratio, rounded up (the margin is for another MFMA summation order and the fast exp).
The whole file runs in under 5 s."""
import re

import numpy as np
import pytest
import torch

import xattn_guide_ref as G
import xattn_ref as X
import xattn_wide_ref as XW

pytestmark = pytest.mark.gpu

ROWS_C = 7.0
SENT = -7.0                  # sentinel of every pre-filled buffer (exact in bf16)
GUARD = 4                    # guard rows in front of and behind every output


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _call(name, *args):
    from reformer_tts_amd import _lib
    _lib.call(name, *args)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Buf:
    """``rows`` x ``cols`` window at column ``col0`` of a sentinel-filled (GUARD + rows + GUARD, ld) device buffer."""

    def __init__(self, gpu, rows, cols, dtype, ld=None, col0=0, data=None):
        self.ld = cols if ld is None else ld
        self.full = torch.full((GUARD + rows + GUARD, self.ld), SENT, dtype=dtype, device=gpu)
        self.view = self.full[GUARD:GUARD + rows, col0:col0 + cols]
        self.outside = torch.ones_like(self.full, dtype=torch.bool)
        self.outside[GUARD:GUARD + rows, col0:col0 + cols] = False
        if data is not None:
            self.view.copy_(data)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def untouched(self):
        return bool((self.full[self.outside] == SENT).all())

    def unwritten(self):
        return bool((self.full == SENT).all())

    def cpu(self):
        return self.view.contiguous().cpu()


def _pack(x):
    """(B, H, T, dh) -> (B * T, H * dh) bf16, the kernels' layout."""
    nb, nh, t, dh = x.shape
    return x.transpose(1, 2).reshape(nb * t, nh * dh).bfloat16()


def _unpack(buf, nb, nh, dh):
    return buf.double().view(nb, -1, nh, dh).transpose(1, 2)


class _Chain:
    """Device copies of one case and its forward (rtts_xattn_fwd, rtts_lsh_bwd_delta); ``backward`` runs rows, fold and the guided
    backward (or the unguided one) into fresh sentinel-filled outputs.  ``wide``: q, o, dout (and dq with one key chunk) are
    column windows of buffers 64 columns wider, kv rows are 2 H dh + 8 apart."""

    def __init__(self, gpu, inputs, valid, drop=None, wide=False):
        q, k, v, do = inputs
        self.gpu = gpu
        self.nb, self.nh, self.tq, self.dh = q.shape
        self.tk = k.shape[2]
        nb, nh, tq, tk, dh = self.nb, self.nh, self.tq, self.tk, self.dh
        self.e = e = nh * dh
        self.nkc, self.nqb = tk // XW.bwd_chunk(tk, dh), tq // X.QB
        self.wide = wide
        ld, c0 = (e + 64, 32) if wide else (e, 0)
        bf16 = torch.bfloat16
        self.qb = _Buf(gpu, nb * tq, e, bf16, ld, c0, _pack(q))
        self.dob = _Buf(gpu, nb * tq, e, bf16, ld, c0, _pack(do))
        self.kvb = _Buf(gpu, nb * tk, 2 * e, bf16, 2 * e + 8 if wide else 2 * e, 0, torch.cat([_pack(k), _pack(v)], dim=1))
        self.ob = _Buf(gpu, nb * tq, e, bf16, ld, c0)
        self.lse = _Buf(gpu, nb * nh, tq, torch.float32)
        self.delta = _Buf(gpu, nb * nh, tq, torch.float32)
        self.vd = None if valid is None else valid.to(torch.uint8).to(gpu)
        self.vp = None if self.vd is None else self.vd.data_ptr()
        self.p, self.seed, seed_dev = drop if drop else (0.0, 0, None)
        self.sd = None if seed_dev is None else torch.from_numpy(np.array([seed_dev], dtype=np.uint32).view(np.int32)).to(gpu)
        self.sp = None if self.sd is None else self.sd.data_ptr()
        s = _stream()
        _call("rtts_xattn_fwd", self.qb.ptr, self.qb.ld, self.kvb.ptr, self.kvb.ld, self.vp, nb, nh, tq, tk, dh, self.ob.ptr, self.ob.ld,
              self.lse.ptr, self.p, self.seed, self.sp, s)
        _call("rtts_lsh_bwd_delta", self.ob.ptr, self.ob.ld, self.dob.ptr, self.dob.ld, nb, nh, tq, dh, self.delta.ptr, s)

    def backward(self, n_frames=None, n_keys=None, coef=1.0, sigma=G.SIGMA, launch=None):
        """Guided when ``n_frames`` is given.  ``launch(fn)``: how the launches are issued (default: directly)."""
        gpu, nb, nh, tq, tk, dh, e = self.gpu, self.nb, self.nh, self.tq, self.tk, self.dh, self.e
        bf16 = torch.bfloat16
        wide_dq = self.wide and self.nkc == 1
        dq = _Buf(gpu, nb * tq, e, bf16, e + 64 if wide_dq else e, 32 if wide_dq else 0)
        part = _Buf(gpu, self.nqb * nb * tk, 2 * e, bf16)
        ws = _Buf(gpu, self.nkc * nb * tq, e, bf16)
        dkv = _Buf(gpu, nb * tk, 2 * e, bf16)
        rows = _Buf(gpu, nb * nh, tq, torch.float32)
        out = _Buf(gpu, 1, nb + 1, torch.float64)
        c = _Buf(gpu, 1, 1, torch.float32)
        guided = n_frames is not None
        if guided:
            nf = torch.tensor(list(n_frames), dtype=torch.int32, device=gpu)
            nk = torch.tensor(list(n_keys), dtype=torch.int32, device=gpu)
        s_args = (self.qb.ptr, self.qb.ld, self.kvb.ptr, self.kvb.ld, self.vp)
        b_args = s_args + (self.dob.ptr, self.dob.ld, self.lse.ptr, self.delta.ptr, nb, nh, tq, tk, dh, dq.ptr, dq.ld, part.ptr, self.p,
                           self.seed, self.sp, ws.ptr if self.nkc > 1 else None)

        def go():
            s = _stream()
            if guided:
                _call("rtts_xattn_guide_rows", *s_args, self.lse.ptr, nf.data_ptr(), nk.data_ptr(), nb, nh, tq, tk, dh, sigma, rows.ptr, s)
                _call("rtts_xattn_guide_fold", rows.ptr, nf.data_ptr(), nk.data_ptr(), nb, nh, tq, tk, coef, out.ptr, c.ptr, s)
                _call("rtts_xattn_bwd_guided", *b_args, rows.ptr, c.ptr, nf.data_ptr(), nk.data_ptr(), sigma, s)
            else:
                _call("rtts_xattn_bwd", *b_args, s)
            _call("rtts_sum_slabs", part.ptr, self.nqb, nb * tk * 2 * e, dkv.ptr, s)
        (launch or (lambda fn: fn()))(go)
        torch.cuda.synchronize()
        for name, b in (("q", self.qb), ("dout", self.dob), ("kv", self.kvb), ("o", self.ob), ("lse", self.lse), ("delta", self.delta),
                        ("dq", dq), ("dkv_part", part), ("dq_chunks", ws), ("dkv", dkv), ("rows", rows), ("out", out), ("c", c)):
            assert b.untouched(), f"{name}: a gap column or a guard row was written"
        if self.nkc == 1:
            assert ws.unwritten(), "dq_chunks written by a one-chunk call"
        if not guided:
            assert rows.unwritten() and out.unwritten() and c.unwritten()
        return dict(dq=dq.cpu(), part=part.cpu(), dkv=dkv.cpu(), ws=ws.cpu(), rows=rows.cpu(), out=out.cpu().view(-1), c=c.cpu().view(-1))

    def tensors(self, res):
        nb, nh, dh, e = self.nb, self.nh, self.dh, self.e
        return dict(dq=_unpack(res["dq"], nb, nh, dh), dk=_unpack(res["dkv"][:, :e], nb, nh, dh), dv=_unpack(res["dkv"][:, e:], nb, nh, dh),
                    rows=res["rows"].double().view(nb, nh, -1))


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _differ(a, b, names):
    return [n for n in names if not torch.equal(_bits(a[n]), _bits(b[n]))]


GRADS = ("dq", "part", "dkv", "ws")
ALL = GRADS + ("rows", "out", "c")


def _check(tag, chain, res, ref):
    got = chain.tensors(res)
    r = G.ratios(got, ref)
    r["rows"] = G.rows_ratio(got["rows"], ref)
    rel = float(((res["out"] - ref["out"]).abs() / ref["out"].abs().clamp_min(1e-300)).masked_fill(ref["out"] == 0, 0.0).max())
    print(f"\n[parity] {tag}: worst |kernel - float64| / bound  " + "  ".join(f"{n} {x:.3f}" for n, x in r.items())
          + f"  (dq, dk, dv must be <= 1; rows is in units of 2^-24 lse_scale (row sum), must be <= {ROWS_C:g});  out rel {rel:.2e}"
          + f"  loss {float(res['out'][-1]):.6f}  c {float(res['c'][0]):.6g}")
    assert r["dq"] <= 1.0 and r["dk"] <= 1.0 and r["dv"] <= 1.0, r
    assert r["rows"] <= ROWS_C, r
    assert rel <= 1e-6 and bool((res["out"][ref["out"] == 0] == 0).all())
    assert abs(float(res["c"][0]) - ref["c"]) <= 1e-6 * abs(ref["c"])
    return r


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=G.IDS)
def test_guided_backward_within_the_bounds(gpu, i):
    nb, nh, tq, tk, dh, kind, pattern, nf, nk, drop = G.CASES[i]
    inputs, valid, keep = G.case_inputs(i)
    coef = G.case_coef(G.CASES[i])
    chain = _Chain(gpu, inputs, valid, drop)
    res = chain.backward(nf, nk, coef)
    plain = chain.backward()
    ref = G.reference(*inputs, valid, keep, nf, nk, G.SIGMA, coef)
    _check(f"{G.IDS[i]}, T_b {nf}, K_b {nk}, dropout {drop}, {chain.nkc} chunk(s)", chain, res, ref)
    e = nh * dh
    assert torch.equal(_bits(res["dkv"][:, e:].contiguous()), _bits(plain["dkv"][:, e:].contiguous())), "dv differs from rtts_xattn_bwd's"
    assert _differ(res, plain, ("dq",)) == ["dq"]
    if valid is not None:                          # padded keys: a gradient of exactly 0, in every slab
        padded = ~valid.reshape(-1)
        assert float(res["dkv"][padded].float().abs().max()) == 0.0
        assert float(res["part"].view(chain.nqb, nb * tk, 2 * e)[:, padded].float().abs().max()) == 0.0
    ok = torch.tensor(G.counts(nf, nk, tq, tk))
    got_rows = res["rows"].view(nb, nh, tq)
    assert float(got_rows[~ok].abs().max() if bool((~ok).any()) else 0.0) == 0.0
    for b in range(nb):                            # rows t >= T_b are written as 0
        if ok[b]:
            assert float(got_rows[b, :, int(nf[b]):].abs().max() if int(nf[b]) < tq else 0.0) == 0.0


@pytest.mark.parametrize("i", [0, 6], ids=[G.IDS[0], G.IDS[6]])
def test_zero_dout_leaves_the_guided_gradient_alone(gpu, i):
    """dout = 0: the unguided kernel gives exact zeros, so everything that comes out is the guided gradient.
    The cases are the plain ones.  With dout = 0 the bound loses its delta term and is u |dS| alone, and the bound counts nothing
    for rows and c being fp32.  On a one-hot row (the peaked kind: 1 - P_k is about 1e-10, below 2^-24) the true
    dS = c P (W - rows) is of order c 1e-10, finer than fp32 can hold rows itself (2^-24 W): no fp32 rows can meet u |dS| there
    (measured on 3x2x128x256 peaked with dout = 0: dq 1804 x its bound -- an absolute error of c 2^-24 per logit -- dk 0.585).
    With any dout the bound's delta term covers it (the peaked cases above)."""
    nb, nh, tq, tk, dh, kind, pattern, nf, nk, drop = G.CASES[i]
    (q, k, v, do), valid, keep = G.case_inputs(i)
    inputs = (q, k, v, torch.zeros_like(do))
    coef = G.case_coef(G.CASES[i])
    chain = _Chain(gpu, inputs, valid)
    plain = chain.backward()
    assert float(plain["dq"].float().abs().max()) == 0.0 and float(plain["dkv"].float().abs().max()) == 0.0
    res = chain.backward(nf, nk, coef)
    ref = G.reference(*inputs, valid, None, nf, nk, G.SIGMA, coef)
    assert float(ref["dq"].abs().max()) > 0.1 and float(ref["dk"].abs().max()) > 0.1          # there is something to compare
    _check(f"dout = 0, {G.IDS[i]}", chain, res, ref)
    assert float(res["dkv"][:, nh * dh:].float().abs().max()) == 0.0


@pytest.mark.parametrize("i", [2, 3, 7], ids=[G.IDS[2], G.IDS[3], G.IDS[7]])
def test_two_runs_and_a_strided_layout_are_bit_identical(gpu, i):
    nb, nh, tq, tk, dh, kind, pattern, nf, nk, drop = G.CASES[i]
    inputs, valid, keep = G.case_inputs(i)
    coef = G.case_coef(G.CASES[i])
    chain = _Chain(gpu, inputs, valid, drop)
    a = chain.backward(nf, nk, coef)
    b = chain.backward(nf, nk, coef)
    assert _differ(a, b, ALL) == []
    w = _Chain(gpu, inputs, valid, drop, wide=True).backward(nf, nk, coef)
    assert _differ(a, w, ALL) == []


def test_captured_launches_replay_bit_identically(gpu):
    """rows, fold and the guided backward read nothing on the host: one hipGraph holds them, and its replay gives the eager bits."""
    i = 1
    nb, nh, tq, tk, dh, kind, pattern, nf, nk, drop = G.CASES[i]
    inputs, valid, keep = G.case_inputs(i)
    coef = G.case_coef(G.CASES[i])
    chain = _Chain(gpu, inputs, valid)
    eager = chain.backward(nf, nk, coef)

    def captured(fn):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        graph.replay()
    replayed = chain.backward(nf, nk, coef, launch=captured)
    assert _differ(eager, replayed, ALL) == []


@pytest.mark.parametrize("dh,tk", [(64, 256), (128, 384)])
def test_no_slot_counts(gpu, dh, tk):
    """Every slot fails (T_b = 0, T_b > T_q, K_b > T_k): loss 0, c 0, rows 0, and dq, every slab and dkv bit-equal to rtts_xattn_bwd."""
    nb, nh, tq = 3, 2, 128
    inputs = G.make_inputs("plain", nb, nh, tq, tk, 5, dh)
    valid = X.make_valid("ragged", nb, tk)
    chain = _Chain(gpu, inputs, valid, (0.1, 3, 4))
    res = chain.backward((0, tq + 1, 128), (5, 5, tk + 1), 1000.0)
    plain = chain.backward()
    assert float(res["out"].abs().max()) == 0.0 and float(res["c"][0]) == 0.0 and float(res["rows"].abs().max()) == 0.0
    assert _differ(res, plain, GRADS) == []


def test_rejections_launch_nothing(gpu):
    """A null pointer, a bad stride, a shape outside the envelope or sigma <= 0 is refused by name, before any launch."""
    from reformer_tts_amd import _lib
    e = 64
    mk = lambda rows, cols, dt=torch.bfloat16: torch.full((rows, cols), SENT, dtype=dt, device=gpu)
    q, kv, do, dq = mk(128, e + 8), mk(384, 2 * e), mk(128, e), mk(128, e)
    part, ws = mk(384, 2 * e), mk(3 * 128, e)
    lse, delta, rows, c = (mk(1, 128, torch.float32) for _ in range(4))
    out = mk(1, 2, torch.float64)
    nf = torch.tensor([100], dtype=torch.int32, device=gpu)
    nk = torch.tensor([100], dtype=torch.int32, device=gpu)
    s = _stream()
    P = lambda t: t.data_ptr()

    def rows_(q_=P(q), kv_=P(kv), lse_=P(lse), nf_=P(nf), nk_=P(nk), rows__=P(rows), tq=128, tk=128, ld_q=e, sigma=0.2, dh=64):
        _call("rtts_xattn_guide_rows", q_, ld_q, kv_, 2 * e, None, lse_, nf_, nk_, 1, 1, tq, tk, dh, sigma, rows__, s)

    def fold_(rows__=P(rows), nf_=P(nf), nk_=P(nk), out_=P(out), c_=P(c), tq=128, tk=128, coef=1.0):
        _call("rtts_xattn_guide_fold", rows__, nf_, nk_, 1, 1, tq, tk, coef, out_, c_, s)

    def bwd_(q_=P(q), rows__=P(rows), c_=P(c), nf_=P(nf), nk_=P(nk), tq=128, tk=128, ld_q=e, ld_dq=e, sigma=0.2, p=0.0, ws_=None, dq_=P(dq)):
        _call("rtts_xattn_bwd_guided", q_, ld_q, P(kv), 2 * e, None, P(do), e, P(lse), P(delta), 1, 1, tq, tk, 64, dq_, ld_dq, P(part), p, 0,
              None, ws_, rows__, c_, nf_, nk_, sigma, s)

    def refuses(msg, fn, **kw):
        with pytest.raises(_lib.RttsError, match=re.escape(msg)):
            fn(**kw)

    for name, kw in (("q", "q_"), ("kv", "kv_"), ("lse", "lse_"), ("n_frames", "nf_"), ("n_keys", "nk_"), ("rows", "rows__")):
        refuses(f"rtts_xattn_guide_rows: {name} is a null pointer", rows_, **{kw: None})
    for name, kw in (("rows", "rows__"), ("n_frames", "nf_"), ("n_keys", "nk_"), ("out", "out_"), ("c_dev", "c_")):
        refuses(f"rtts_xattn_guide_fold: {name} is a null pointer", fold_, **{kw: None})
    for name, kw in (("q", "q_"), ("dq", "dq_"), ("guide_rows", "rows__"), ("c_dev", "c_"), ("n_frames", "nf_"), ("n_keys", "nk_")):
        refuses(f"rtts_xattn_bwd_guided: {name} is a null pointer", bwd_, **{kw: None})
    for fn, name in ((rows_, "rtts_xattn_guide_rows"), (bwd_, "rtts_xattn_bwd_guided")):
        for sigma in (0.0, -0.2, float("nan")):
            refuses(f"{name}: sigma must be positive and finite", fn, sigma=sigma)
        refuses(f"{name}: bad row strides", fn, ld_q=e + 4)
        refuses(f"{name}: T_q=64 must be a multiple of 128", fn, tq=64)
        for tk in (192, 2176, 0):
            refuses(f"{name}: T_k={tk} unsupported (a multiple of 128 up to 2048)", fn, tk=tk)
    refuses("rtts_xattn_guide_rows: dh=32 unsupported", rows_, dh=32)
    refuses("rtts_xattn_guide_rows: q and kv must be 16-byte aligned", rows_, q_=P(q) + 2)
    refuses("rtts_xattn_guide_fold: T_k=192 unsupported", fold_, tk=192)
    refuses("rtts_xattn_guide_fold: coef must be finite", fold_, coef=float("inf"))
    refuses("rtts_xattn_bwd_guided: bad strides", bwd_, ld_dq=e + 4)
    refuses("rtts_xattn_bwd_guided: bad arguments", bwd_, p=1.0)
    refuses("rtts_xattn_bwd_guided: buffers must be 16-byte aligned", bwd_, q_=P(q) + 2)
    refuses("rtts_xattn_bwd_guided: T_k=384 is worked in 3 key chunks: needs dq_chunks (3 x B*T_q x H*dh bf16) and ld_dq == H*dh", bwd_, tk=384)
    refuses("rtts_xattn_bwd_guided: T_k=384 is worked in 3 key chunks", bwd_, tk=384, ws_=P(ws), ld_dq=e + 8)
    torch.cuda.synchronize()
    for name, b in (("rows", rows), ("out", out), ("c", c), ("dq", dq), ("dkv_part", part), ("dq_chunks", ws)):
        assert bool((b == SENT).all()), f"{name} was written by a rejected call"
