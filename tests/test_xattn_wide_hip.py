"""Dense encoder-decoder attention with 128-wide heads (csrc/xattn.hip, DH = 128) through the C ABI against the float64 oracle
of tests/xattn_wide_ref.py.  Every call goes through ``_lib.call`` in the engine's order: rtts_xattn_fwd, rtts_lsh_bwd_delta on
the kernel's own o, rtts_xattn_bwd with the kernel's own lse, rtts_sum_slabs; every buffer is sentinel-filled with guard rows.

Comparison: |got - float64| <= bound ELEMENT-WISE on o, dq, dk, dv (per-element first-order bounds of xattn_wide_ref.py, u = 2^-8
per rounding to bf16); lse within LSE_C 2^-24 (max_j sum_d |q_d k_jd| / sqrt(dh) + |lse| + 1) with the LSE_C of
tests/test_xattn_hip.py.  Every test prints a ``[parity]`` line with the worst ratio per quantity.

At dh = 128 the backward works 128-key chunks (``rtts_xattn_bwd_key_chunks(T_k, 128) = T_k / 128``), so T_k = 256 already has two
chunks and a dq_chunks workspace; the forward holds 256 keys only at T_k = 256 and walks 128-key chunks otherwise.

Measured on an MI355X, worst |kernel - float64| / bound over the whole file (must be <= 1):
    o  0.833   (2x2x128x128 peaked, dropout 0.5, wrapping seed)      dq 0.700   (the same shape, dropout 0.15)
    dk 0.420   (2x2x128x384 peaked, dropout 0.5)                     dv 0.699   (1x3x256x512 peaked, last chunk padded)
    lse 1.875 of the 6 allowed; rtts_lsh_bwd_delta 0.009 of its bound; rtts_xattn_probs_mean within 2.7e-7 of float64, rows within
    1e-6 of 1; the dh = 64 case reproduces tests/test_xattn_hip.py's figures (dv 0.848).  The whole file runs in about 3 s."""
import re

import numpy as np
import pytest
import torch

import xattn_ref as X
import xattn_wide_ref as W

pytestmark = pytest.mark.gpu

LSE_C = 6.0                  # tests/test_xattn_hip.py
SENT = -7.0                  # sentinel of every pre-filled buffer (exact in bf16)
GUARD = 4                    # guard rows in front of and behind every output
DH = 128


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

    def cpu(self):
        return self.view.contiguous().cpu()


def _pack(x):
    """(B, H, T, dh) -> (B * T, H * dh) bf16, the kernels' layout."""
    nb, nh, t, dh = x.shape
    return x.transpose(1, 2).reshape(nb * t, nh * dh).bfloat16()


def _chain(gpu, inputs, valid, p=0.0, seed=0, seed_dev=None, wide=False, wide_dq=None):
    """fwd -> delta -> bwd -> sum_slabs on device copies of ``inputs`` = (q, k, v, do) (B, H, T, dh), dh from the inputs.
    ``wide``: q, o, dout (and dq, unless ``wide_dq`` says otherwise) are column windows of buffers 64 columns wider, kv rows are
    2 H dh + 8 apart.  Gap columns and guard rows must come back untouched.  Returns the outputs on the CPU."""
    q, k, v, do = inputs
    nb, nh, tq, dh = q.shape
    tk = k.shape[2]
    e = nh * dh
    nkc, nqb = tk // W.bwd_chunk(tk, dh), tq // W.QB
    wide_dq = wide if wide_dq is None else wide_dq
    ld, c0 = (e + 64, 32) if wide else (e, 0)
    ld_dq, c0_dq = (e + 64, 32) if wide_dq else (e, 0)
    bf16 = torch.bfloat16
    qb = _Buf(gpu, nb * tq, e, bf16, ld, c0, _pack(q))
    dob = _Buf(gpu, nb * tq, e, bf16, ld, c0, _pack(do))
    kvb = _Buf(gpu, nb * tk, 2 * e, bf16, 2 * e + 8 if wide else 2 * e, 0, torch.cat([_pack(k), _pack(v)], dim=1))
    ob = _Buf(gpu, nb * tq, e, bf16, ld, c0)
    lse = _Buf(gpu, nb * nh, tq, torch.float32)
    delta = _Buf(gpu, nb * nh, tq, torch.float32)
    dq = _Buf(gpu, nb * tq, e, bf16, ld_dq, c0_dq)
    part = _Buf(gpu, nqb * nb * tk, 2 * e, bf16)
    ws = _Buf(gpu, nkc * nb * tq, e, bf16)
    dkv = _Buf(gpu, nb * tk, 2 * e, bf16)
    vd = None if valid is None else valid.to(torch.uint8).to(gpu)
    vp = None if vd is None else vd.data_ptr()
    sd = None if seed_dev is None else torch.from_numpy(np.array([seed_dev], dtype=np.uint32).view(np.int32)).to(gpu)
    sp = None if sd is None else sd.data_ptr()
    s = _stream()
    _call("rtts_xattn_fwd", qb.ptr, qb.ld, kvb.ptr, kvb.ld, vp, nb, nh, tq, tk, dh, ob.ptr, ob.ld, lse.ptr, p, seed, sp, s)
    _call("rtts_lsh_bwd_delta", ob.ptr, ob.ld, dob.ptr, dob.ld, nb, nh, tq, dh, delta.ptr, s)
    _call("rtts_xattn_bwd", qb.ptr, qb.ld, kvb.ptr, kvb.ld, vp, dob.ptr, dob.ld, lse.ptr, delta.ptr, nb, nh, tq, tk, dh, dq.ptr, dq.ld,
          part.ptr, p, seed, sp, ws.ptr if nkc > 1 else None, s)
    _call("rtts_sum_slabs", part.ptr, nqb, nb * tk * 2 * e, dkv.ptr, s)
    torch.cuda.synchronize()
    for name, b in (("q", qb), ("dout", dob), ("kv", kvb), ("o", ob), ("lse", lse), ("delta", delta), ("dq", dq), ("dkv_part", part),
                    ("dq_chunks", ws), ("dkv", dkv)):
        assert b.untouched(), f"{name}: a gap column or a guard row was written"
    if nkc == 1:
        assert bool((ws.full == SENT).all()), "dq_chunks written by a one-chunk call"
    return dict(o=ob.cpu(), lse=lse.cpu(), delta=delta.cpu(), dq=dq.cpu(), part=part.cpu().view(nqb, nb * tk, 2 * e), dkv=dkv.cpu(),
                ws=ws.cpu(), qbuf=qb, kvbuf=kvb, vd=vd, lsebuf=lse)


def _tensors(out, nb, nh, dh):
    e = nh * dh
    un = lambda buf: buf.double().view(nb, -1, nh, dh).transpose(1, 2)
    return dict(o=un(out["o"]), dq=un(out["dq"]), dk=un(out["dkv"][:, :e]), dv=un(out["dkv"][:, e:]),
                lse=out["lse"].double().view(nb, nh, -1))


def _check(tag, out, ref, nb, nh, dh=DH, rows=None):
    got = _tensors(out, nb, nh, dh)
    r = X.ratios(got, ref, rows)
    r["lse"] = X.lse_ratio(got["lse"], ref, rows)
    print(f"\n[parity dh={dh}] {tag}: worst |kernel - float64| / bound  " + "  ".join(f"{n} {x:.3f}" for n, x in r.items())
          + f"  (o, dq, dk, dv must be <= 1; lse is in units of 2^-24 scale, must be <= {LSE_C:g})")
    assert r["o"] <= 1.0 and r["dq"] <= 1.0 and r["dk"] <= 1.0 and r["dv"] <= 1.0, r
    assert r["lse"] <= LSE_C, r
    return r


def _reference(inputs, valid, drop=None):
    q, k = inputs[0], inputs[1]
    nb, nh, tq, dh = q.shape
    keep = None if drop is None else X.keep_scales(*drop, nb * nh, tq, k.shape[2]).view(nb, nh, tq, -1)
    return W.reference(*inputs, valid, keep, dh)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b, names):
    return [n for n in names if not torch.equal(_bits(a[n]), _bits(b[n]))]


ALL = ("o", "lse", "delta", "dq", "part", "dkv", "ws")

# (B, H, T_q, T_k, input kind, kvalid pattern).  One backward chunk: T_k = 128; several: 256 (2; the forward's single-pass 256-key
# kernel), 384 (3), 512 (4), 2048 (16; the forward walks 16 chunks).  Every kind and every pattern appears with one chunk and with
# several; grids of 1, 4, 9, 6 and 1 workgroups per chunk.  With 128 keys and one sample the patterns 'first', 'middle' and 'last'
# leave the sample without a valid key (the chunk they pad is all there is): those cases check the NaN contract.
CASES = [
    (1, 1, 128, 128, "plain", "none"),
    (1, 1, 128, 128, "peaked", "ragged"),
    (1, 1, 128, 128, "offset+", "first"),
    (1, 1, 128, 128, "offset-", "middle"),
    (1, 1, 128, 128, "plain", "last"),
    (1, 1, 128, 128, "peaked", "one"),
    (1, 1, 128, 128, "offset+", "alternating"),
    (2, 2, 128, 256, "peaked", "ragged"),
    (2, 2, 128, 256, "plain", "one"),
    (3, 1, 384, 384, "offset+", "first"),
    (3, 1, 384, 384, "plain", "alternating"),
    (1, 3, 256, 512, "offset-", "middle"),
    (1, 3, 256, 512, "peaked", "last"),
    (1, 1, 128, 2048, "plain", "none"),
]


@pytest.mark.parametrize("nb,nh,tq,tk,kind,pattern", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[4]}-{c[5]}" for c in CASES])
def test_forward_and_backward_within_the_bounds(gpu, nb, nh, tq, tk, kind, pattern):
    from reformer_tts_amd import _lib
    assert _lib.load().rtts_xattn_bwd_key_chunks(tk, DH) == tk // 128
    inputs = W.make_inputs(kind, nb, nh, tq, tk, seed=1000 * nb + 100 * nh + tq + tk, dh=DH)
    valid = X.make_valid(pattern, nb, tk)
    out = _chain(gpu, inputs, valid)
    # 'first' / 'middle' / 'last' pad a whole make_valid chunk of sample 0: with 128 keys that is the sample's every key, and the
    # contract for it is NaN in data (include/rtts.h), not a bound
    empty = [] if valid is None else [b for b in range(nb) if not bool(valid[b].any())]
    rows = [b for b in range(nb) if b not in empty]
    if rows:
        _check(f"{nb}x{nh}x{tq}x{tk} {kind}, kvalid {pattern}, {tk // 128} backward chunk(s)", out, _reference(inputs, valid), nb, nh,
               rows=rows if empty else None)
    e = nh * DH
    for b in empty:
        print(f"\n[parity dh=128] {nb}x{nh}x{tq}x{tk} {kind}, kvalid {pattern}: sample {b} has no valid key -> the NaN contract")
        assert bool(torch.isnan(out["o"][b * tq:(b + 1) * tq].float()).all()) and bool(torch.isnan(out["dq"][b * tq:(b + 1) * tq].float()).all())
        assert bool((out["lse"][b * nh:(b + 1) * nh] == float("-inf")).all()) and bool(torch.isnan(out["delta"][b * nh:(b + 1) * nh]).all())
        assert bool(torch.isnan(out["dkv"][b * tk:(b + 1) * tk, :e].float()).all())
        assert float(out["dkv"][b * tk:(b + 1) * tk, e:].float().abs().max()) == 0.0
    if valid is not None:                          # padded keys of a sample that has keys: a gradient of exactly 0, in every slab
        padded = (~valid & valid.any(dim=1, keepdim=True)).reshape(-1)
        if bool(padded.any()):
            assert float(out["dkv"][padded].float().abs().max()) == 0.0 and float(out["part"][:, padded].float().abs().max()) == 0.0


@pytest.mark.parametrize("seed_dev", [None, 0xFFFFFFF0])
@pytest.mark.parametrize("tk,p", [(128, 0.15), (128, 0.5), (384, 0.15), (384, 0.5)])
def test_dropout_against_the_cpu_mask_twin(gpu, tk, p, seed_dev):
    """The keep-scales come from xattn_ref.keep_scales (oracle.synth.drop_hash), index (bh T_q + query) T_k + global key and seed
    + *seed_dev (here wrapping); lse is bit-identical to the run without dropout."""
    nb, nh, tq = 2, 2, 128
    seed = 0x9E3779B1 + tk
    inputs = W.make_inputs("peaked", nb, nh, tq, tk, seed=7 * tk + tq, dh=DH)
    valid = X.make_valid("ragged", nb, tk)
    out = _chain(gpu, inputs, valid, p, seed, seed_dev)
    _check(f"dropout {p}, seed_dev {seed_dev}: {nb}x{nh}x{tq}x{tk} peaked", out, _reference(inputs, valid, (p, seed, seed_dev)), nb, nh)
    plain = _chain(gpu, inputs, valid)
    assert not _same(out, plain, ("lse",)) and _same(out, plain, ("o", "dq", "dkv")) == ["o", "dq", "dkv"]


@pytest.mark.parametrize("tk", [128, 256])
def test_strided_rows_are_bit_identical_and_nothing_else_is_written(gpu, tk):
    """q, o, dout, dq as column windows of wider buffers and ld_kv = 2 H dh + 8: bit-identical to the compact call (``_chain``
    checks the gap columns and the guard rows of both).  More than one key chunk -- at dh = 128 that is T_k = 256 -- needs
    compact dq rows and says so, with the chunk count of this head width."""
    from reformer_tts_amd import _lib
    nb, nh, tq = 3, 3, 128
    inputs = W.make_inputs("plain", nb, nh, tq, tk, seed=tk, dh=DH)
    valid = X.make_valid("ragged", nb, tk)
    multi = tk > 128
    compact = _chain(gpu, inputs, valid, 0.15, 11, 3)
    wide = _chain(gpu, inputs, valid, 0.15, 11, 3, wide=True, wide_dq=not multi)
    assert _same(compact, wide, ALL) == []
    _check(f"strided rows, {tk} keys", wide, _reference(inputs, valid, (0.15, 11, 3)), nb, nh)
    if multi:
        with pytest.raises(_lib.RttsError, match=r"rtts_xattn_bwd: T_k=256 is worked in 2 key chunks: needs dq_chunks .* and ld_dq == H\*dh"):
            _chain(gpu, inputs, valid, wide=True, wide_dq=True)
        torch.cuda.synchronize()


@pytest.mark.parametrize("nb,nh,tq,tk,p", [(2, 2, 128, 256, 0.0), (1, 3, 256, 384, 0.5)])
def test_two_runs_are_bit_identical(gpu, nb, nh, tq, tk, p):
    inputs = W.make_inputs("peaked", nb, nh, tq, tk, seed=tk, dh=DH)
    valid = X.make_valid("ragged", nb, tk)
    a = _chain(gpu, inputs, valid, p, 3, 4)
    b = _chain(gpu, inputs, valid, p, 3, 4)
    assert _same(a, b, ALL) == []


@pytest.mark.parametrize("tq,tk,p", [(256, 384, 0.0), (128, 128, 0.5)])
def test_a_sample_without_a_valid_key(gpu, tq, tk, p):
    """Sample 1 of 3 has no valid key: what include/rtts.h states (o NaN, lse -inf, delta, dq and dk NaN, dv exactly 0), and
    samples 0 and 2 meet the bounds and are bit-identical to the same call with sample 1 unpadded."""
    nb, nh = 3, 2
    e = nh * DH
    inputs = W.make_inputs("plain", nb, nh, tq, tk, seed=tk + 1, dh=DH)
    valid = X.make_valid("ragged", nb, tk)
    valid[1] = False
    drop = (p, 21, 2) if p else None
    out = _chain(gpu, inputs, valid, p, 21, 2 if p else None)
    _check(f"sample 1 of 3 fully padded, {tk} keys, dropout {p}: samples 0 and 2", out, _reference(inputs, valid, drop), nb, nh, rows=[0, 2])
    other = valid.clone()
    other[1] = True
    out2 = _chain(gpu, inputs, other, p, 21, 2 if p else None)
    qrows = torch.cat([torch.arange(0, tq), torch.arange(2 * tq, 3 * tq)])
    krows = torch.cat([torch.arange(0, tk), torch.arange(2 * tk, 3 * tk)])
    lrows = torch.cat([torch.arange(0, nh), torch.arange(2 * nh, 3 * nh)])
    pick = lambda o: dict(o=o["o"][qrows], dq=o["dq"][qrows], lse=o["lse"][lrows], part=o["part"][:, krows], dkv=o["dkv"][krows])
    assert _same(pick(out), pick(out2), ("o", "dq", "lse", "part", "dkv")) == []
    mine = slice(tq, 2 * tq)
    assert bool(torch.isnan(out["o"][mine].float()).all()) and bool(torch.isnan(out["dq"][mine].float()).all())
    assert bool((out["lse"][nh:2 * nh] == float("-inf")).all())
    assert bool(torch.isnan(out["delta"][nh:2 * nh]).all())
    assert bool(torch.isnan(out["dkv"][tk:2 * tk, :e].float()).all())
    assert float(out["dkv"][tk:2 * tk, e:].float().abs().max()) == 0.0


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("nb,nh,t", [(1, 1, 128), (3, 3, 384)])
def test_bwd_delta_vs_float64(gpu, nb, nh, t, wide):
    """rtts_lsh_bwd_delta at dh = 128 = rowsum(o o dO) over the 128 columns of a head: 128 fused multiply-adds in fp32, so
    |delta - float64| <= 128 2^-24 sum_d |o_d||dO_d|."""
    e = nh * DH
    g = torch.Generator().manual_seed(nb + t)
    o = torch.randn(nb, nh, t, DH, generator=g) + 0.5
    do = torch.randn(nb, nh, t, DH, generator=g) + 0.5
    ob = _Buf(gpu, nb * t, e, torch.bfloat16, e + 64 if wide else e, 32 if wide else 0, _pack(o))
    dob = _Buf(gpu, nb * t, e, torch.bfloat16, e + 8 if wide else e, 8 if wide else 0, _pack(do))
    delta = _Buf(gpu, nb * nh, t, torch.float32)
    _call("rtts_lsh_bwd_delta", ob.ptr, ob.ld, dob.ptr, dob.ld, nb, nh, t, DH, delta.ptr, _stream())
    torch.cuda.synchronize()
    assert delta.untouched() and ob.untouched() and dob.untouched()
    o64, do64 = X.bf(o).double(), X.bf(do).double()
    want = (o64 * do64).sum(-1).view(nb * nh, t)
    bound = 128 * 2.0 ** -24 * (o64.abs() * do64.abs()).sum(-1).view(nb * nh, t)
    ratio = float(((delta.cpu().double() - want).abs() / bound).max())
    print(f"\n[parity dh=128] rtts_lsh_bwd_delta {nb}x{nh}x{t}, {'strided' if wide else 'compact'}: worst |delta - float64| / bound {ratio:.3f} (must be <= 1)")
    assert ratio <= 1.0


@pytest.mark.parametrize("nb,nh,tq,tk,pattern", [(1, 1, 128, 128, "none"), (2, 3, 256, 384, "ragged")])
def test_probs_mean_rows_sum_to_one_and_match_float64(gpu, nb, nh, tq, tk, pattern):
    """rtts_xattn_probs_mean at dh = 128 from the forward's own lse, into a column window of a wider sentinel-filled buffer:
    the tolerances of tests/test_alignment_hip.py::test_probs_mean_vs_float64 -- every element within 2e-4 of the float64 head
    mean, every row sums to 1 within 1e-4 -- and padded keys exactly 0."""
    inputs = W.make_inputs("plain", nb, nh, tq, tk, seed=tq + tk, dh=DH)
    valid = X.make_valid(pattern, nb, tk)
    out = _chain(gpu, inputs, valid)
    a = _Buf(gpu, nb * tq, tk, torch.float32, tk + 8, 4)
    qb, kvb = out["qbuf"], out["kvbuf"]
    _call("rtts_xattn_probs_mean", qb.ptr, qb.ld, kvb.ptr, kvb.ld, None if out["vd"] is None else out["vd"].data_ptr(), out["lsebuf"].ptr,
          nb, nh, tq, tk, DH, a.ptr, a.ld, _stream())
    torch.cuda.synchronize()
    assert a.untouched()
    got = a.cpu().double().view(nb, tq, tk)
    want = _reference(inputs, valid)["p_mean"]
    err, rows = float((got - want).abs().max()), float((got.sum(-1) - 1.0).abs().max())
    print(f"\n[parity dh=128] rtts_xattn_probs_mean {nb}x{nh}x{tq}x{tk}: max |a - float64| {err:.2e}, max |row sum - 1| {rows:.2e} (tol 2e-4, 1e-4)")
    assert err <= 2e-4 and rows <= 1e-4
    if valid is not None:
        assert float(got[~valid.view(nb, 1, tk).expand(nb, tq, tk)].abs().max()) == 0.0


def test_rejections_launch_nothing(gpu):
    """dh of 32, 96 and 256 is refused by the three entry points with the message of xa_check, before any launch;
    rtts_xattn_bwd_key_chunks gives the documented counts inside the envelope and -1 outside it."""
    from reformer_tts_amd import _lib
    e = 256
    mk = lambda rows, cols, dt=torch.bfloat16: torch.full((rows, cols), SENT, dtype=dt, device=gpu)
    q, kv, do, o, dq = mk(128, e), mk(128, 2 * e), mk(128, e), mk(128, e), mk(128, e)
    part, a = mk(128, 2 * e), mk(128, 128, torch.float32)
    lse, delta = mk(1, 128, torch.float32), mk(1, 128, torch.float32)
    s = _stream()
    for dh in (32, 96, 256):
        with pytest.raises(_lib.RttsError, match=re.escape(f"rtts_xattn_fwd: dh={dh} unsupported (this build: 64 or 128)")):
            _call("rtts_xattn_fwd", q.data_ptr(), e, kv.data_ptr(), 2 * e, None, 1, 1, 128, 128, dh, o.data_ptr(), e, lse.data_ptr(), 0.0, 0, None, s)
        with pytest.raises(_lib.RttsError, match=re.escape(f"rtts_xattn_bwd: dh={dh} unsupported (this build: 64 or 128)")):
            _call("rtts_xattn_bwd", q.data_ptr(), e, kv.data_ptr(), 2 * e, None, do.data_ptr(), e, lse.data_ptr(), delta.data_ptr(), 1, 1,
                  128, 128, dh, dq.data_ptr(), e, part.data_ptr(), 0.0, 0, None, None, s)
        with pytest.raises(_lib.RttsError, match=re.escape(f"rtts_xattn_probs_mean: dh={dh} unsupported (this build: 64 or 128)")):
            _call("rtts_xattn_probs_mean", q.data_ptr(), e, kv.data_ptr(), 2 * e, None, lse.data_ptr(), 1, 1, 128, 128, dh, a.data_ptr(), 128, s)
    torch.cuda.synchronize()
    for name, b in (("o", o), ("lse", lse), ("dq", dq), ("dkv_part", part), ("a", a)):
        assert bool((b == SENT).all()), f"{name} was written by a rejected call"
    chunks = _lib.load().rtts_xattn_bwd_key_chunks
    assert [chunks(tk, 128) for tk in (128, 256, 384, 2048)] == [1, 2, 3, 16]
    assert [chunks(tk, 64) for tk in (128, 256, 384, 640, 2048)] == [1, 1, 3, 5, 8]
    assert all(chunks(tk, 64) == _lib.load().rtts_xattn_key_chunks(tk) for tk in range(128, 2049, 128))
    assert [chunks(tk, dh) for tk, dh in ((0, 128), (64, 128), (192, 64), (2176, 128), (2176, 64), (256, 32), (256, 96), (256, 256))] == [-1] * 8


def test_width_64_through_this_harness_is_bit_identical_between_runs(gpu):
    """Regression guard for the templated kernels at the width they had before: one case of tests/test_xattn_hip.py's CASES
    through this file's harness meets its bounds and gives the same bytes twice."""
    nb, nh, tq, tk, kind, pattern = 3, 2, 256, 384, "peaked", "middle"
    inputs = X.make_inputs(kind, nb, nh, tq, tk, seed=1000 * nb + 100 * nh + tq + tk)
    valid = X.make_valid(pattern, nb, tk)
    a = _chain(gpu, inputs, valid)
    b = _chain(gpu, inputs, valid)
    assert _same(a, b, ALL) == []
    _check(f"{nb}x{nh}x{tq}x{tk} {kind}, kvalid {pattern}", a, X.reference(*inputs, valid), nb, nh, dh=64)
