"""Dense encoder-decoder attention (csrc/xattn.hip) through the C ABI against the float64 oracle of tests/xattn_ref.py, over the
whole envelope xa_check accepts.  Every call goes through ``_lib.call`` in the engine's order: rtts_xattn_fwd, rtts_lsh_bwd_delta
on the kernel's own o, rtts_xattn_bwd with the kernel's own lse, rtts_sum_slabs.

Comparison: |got - float64| <= bound ELEMENT-WISE on o, dq, dk, dv, with the per-element first-order bounds of xattn_ref.py
(u = 2^-8 per rounding to bf16, the roundings listed there with their source lines); nothing is excluded but the rows of a
sample without a valid key in the one test about it.  Every test prints a ``[parity]`` line with the worst ratio per quantity.

lse is fp32 end to end; its bound is LSE_C 2^-24 (max_j sum_d |q_d k_jd| / 8 + |lse| + 1).  The CPU fp32 model of the kernel
needs c = 2.1 (tests/test_xattn_cpu.py); the kernels on an MI355X needed 1.258 at worst over every test of this file (3x2x256x384
peaked, middle chunk padded), and LSE_C = 6 is four times that, rounded up (the margin is for another MFMA summation order and
the fast exp / log).

Measured on an MI355X, worst |kernel - float64| / bound over the whole file (must be <= 1):
    o  0.898   (3x1x128x128 peaked, dropout 0.5)        dq 0.687   (the same case)
    dk 0.524   (3x1x256x384 peaked, dropout 0.5)        dv 0.848   (3x2x256x384 peaked, middle chunk padded)
    rtts_lsh_bwd_delta 0.020 of its own bound; rtts_sum_slabs bit-exact; the whole file runs in under 5 s.
A sample without a valid key gives o = NaN, lse = -inf, delta = dq = dk = NaN and dv = 0 exactly, as include/rtts.h states."""
import re

import numpy as np
import pytest
import torch

import xattn_ref as X

pytestmark = pytest.mark.gpu

LSE_C = 6.0
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

    def cpu(self):
        return self.view.contiguous().cpu()


def _pack(x):
    """(B, H, T, 64) -> (B * T, H * 64) bf16, the kernels' layout."""
    nb, nh, t, dh = x.shape
    return x.transpose(1, 2).reshape(nb * t, nh * dh).bfloat16()


def _unpack(buf, nb, nh):
    return buf.double().view(nb, -1, nh, X.DH).transpose(1, 2)


def _chain(gpu, inputs, valid, p=0.0, seed=0, seed_dev=None, wide=False, wide_dq=None):
    """fwd -> delta -> bwd -> sum_slabs on device copies of ``inputs`` = (q, k, v, do) (B, H, T, 64).  ``wide``: q, o, dout (and dq,
    unless ``wide_dq`` says otherwise) are column windows of buffers 64 columns wider, kv rows are 2 H dh + 8 apart.  Every buffer
    is pre-filled with a sentinel; gap columns and guard rows must come back untouched.  Returns the outputs on the CPU."""
    q, k, v, do = inputs
    nb, nh, tq, _ = q.shape
    tk = k.shape[2]
    e = nh * X.DH
    nkc, nqb = tk // X.key_chunk(tk), tq // X.QB
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
    _call("rtts_xattn_fwd", qb.ptr, qb.ld, kvb.ptr, kvb.ld, vp, nb, nh, tq, tk, X.DH, ob.ptr, ob.ld, lse.ptr, p, seed, sp, s)
    _call("rtts_lsh_bwd_delta", ob.ptr, ob.ld, dob.ptr, dob.ld, nb, nh, tq, X.DH, delta.ptr, s)
    _call("rtts_xattn_bwd", qb.ptr, qb.ld, kvb.ptr, kvb.ld, vp, dob.ptr, dob.ld, lse.ptr, delta.ptr, nb, nh, tq, tk, X.DH, dq.ptr, dq.ld,
          part.ptr, p, seed, sp, ws.ptr if nkc > 1 else None, s)
    _call("rtts_sum_slabs", part.ptr, nqb, nb * tk * 2 * e, dkv.ptr, s)
    torch.cuda.synchronize()
    for name, b in (("q", qb), ("dout", dob), ("kv", kvb), ("o", ob), ("lse", lse), ("delta", delta), ("dq", dq), ("dkv_part", part),
                    ("dq_chunks", ws), ("dkv", dkv)):
        assert b.untouched(), f"{name}: a gap column or a guard row was written"
    if nkc == 1:
        assert bool((ws.full == SENT).all()), "dq_chunks written by a one-chunk call"
    out = dict(o=ob.cpu(), lse=lse.cpu(), delta=delta.cpu(), dq=dq.cpu(), part=part.cpu().view(nqb, nb * tk, 2 * e), dkv=dkv.cpu(),
               ws=ws.cpu())
    return out


def _tensors(out, nb, nh):
    e = nh * X.DH
    return dict(o=_unpack(out["o"], nb, nh), dq=_unpack(out["dq"], nb, nh), dk=_unpack(out["dkv"][:, :e], nb, nh),
                dv=_unpack(out["dkv"][:, e:], nb, nh), lse=out["lse"].double().view(nb, nh, -1))


def _check(tag, out, ref, nb, nh, rows=None):
    got = _tensors(out, nb, nh)
    r = X.ratios(got, ref, rows)
    r["lse"] = X.lse_ratio(got["lse"], ref, rows)
    print(f"\n[parity] {tag}: worst |kernel - float64| / bound  " + "  ".join(f"{n} {x:.3f}" for n, x in r.items())
          + f"  (o, dq, dk, dv must be <= 1; lse is in units of 2^-24 scale, must be <= {LSE_C:g})")
    assert r["o"] <= 1.0 and r["dq"] <= 1.0 and r["dk"] <= 1.0 and r["dv"] <= 1.0, r
    assert r["lse"] <= LSE_C, r
    return r


def _reference(inputs, valid, drop=None):
    q, k = inputs[0], inputs[1]
    nb, nh, tq, _ = q.shape
    keep = None if drop is None else X.keep_scales(*drop, nb * nh, tq, k.shape[2]).view(nb, nh, tq, -1)
    return X.reference(*inputs, valid, keep)


def _same(a, b, names):
    return [n for n in names if not torch.equal(a[n].view(torch.int16 if a[n].dtype == torch.bfloat16 else torch.int32),
                                                b[n].view(torch.int16 if b[n].dtype == torch.bfloat16 else torch.int32))]


ALL = ("o", "lse", "delta", "dq", "part", "dkv", "ws")

# (B, H, T_q, T_k, input kind, kvalid pattern): every T_k of {128, 256, 384, 640, 1024, 1152, 1920, 2048}, T_q of {128, 256, 384},
# B of {1, 3}, H of {1, 2, 3}, every input kind and kvalid pattern; grids B H T_q / 128 of 1, 3, 9, 27, 4, 6, 2, 27, 2, 6, 3,
# 12, 3 and 9 workgroups: none is a multiple of 8 (xcd_remap's remainder branch), one query block and one slab (T_q = 128), three
# slabs (T_q = 384); tests/test_model_hip.py keeps the grids that are multiples of 8
CASES = [
    (1, 1, 128, 128, "plain", "none"),
    (3, 1, 128, 256, "peaked", "ragged"),
    (1, 3, 384, 384, "plain", "first"),
    (3, 3, 384, 640, "offset+", "middle"),
    (1, 2, 256, 1024, "peaked", "last"),
    (3, 2, 128, 1152, "plain", "one"),
    (1, 1, 256, 1920, "peaked", "alternating"),
    (3, 3, 384, 2048, "plain", "ragged"),
    (1, 2, 128, 2048, "offset-", "none"),
    (3, 1, 256, 1920, "offset+", "ragged"),
    (1, 3, 128, 1024, "offset-", "alternating"),
    (3, 2, 256, 384, "peaked", "middle"),
    (1, 1, 384, 256, "offset+", "ragged"),
    (3, 3, 128, 128, "peaked", "one"),
]


@pytest.mark.parametrize("nb,nh,tq,tk,kind,pattern", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[4]}-{c[5]}" for c in CASES])
def test_forward_and_backward_within_the_bounds(gpu, nb, nh, tq, tk, kind, pattern):
    from reformer_tts_amd import _lib
    assert _lib.load().rtts_xattn_key_chunks(tk) == tk // X.key_chunk(tk)
    inputs = X.make_inputs(kind, nb, nh, tq, tk, seed=1000 * nb + 100 * nh + tq + tk)
    valid = X.make_valid(pattern, nb, tk)
    out = _chain(gpu, inputs, valid)
    ref = _reference(inputs, valid)
    _check(f"{nb}x{nh}x{tq}x{tk} {kind}, kvalid {pattern}, {tk // X.key_chunk(tk)} chunk(s), grid {nb * nh * tq // 128}", out, ref, nb, nh)
    if valid is not None:                          # padded keys: a gradient of exactly 0, in every slab
        padded = ~valid.reshape(-1)
        assert float(out["dkv"][padded].float().abs().max()) == 0.0 and float(out["part"][:, padded].float().abs().max()) == 0.0


DROP_CASES = [
    (1, 2, 256, 256, "plain", 0.1, None),          # 1 chunk
    (3, 1, 128, 128, "peaked", 0.5, 5),            # 1 chunk of 128
    (3, 1, 256, 384, "peaked", 0.5, 0xFFFFFFF0),   # 3 chunks; seed + *seed_dev wraps
    (1, 3, 128, 2048, "offset+", 0.1, 9),          # 8 chunks
    (1, 1, 256, 1920, "plain", 0.5, None),         # 15 chunks
    (3, 2, 128, 1920, "peaked", 0.1, 7),           # 15 chunks
]


@pytest.mark.parametrize("nb,nh,tq,tk,kind,p,seed_dev", DROP_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[4]}-p{c[5]}-sd{c[6]}" for c in DROP_CASES])
def test_dropout_against_the_cpu_mask_twin(gpu, nb, nh, tq, tk, kind, p, seed_dev):
    """The keep-scales come from xattn_ref.keep_scales (oracle.synth.drop_hash), not from the kernel; lse is bit-identical to
    the run without dropout."""
    seed = 0x9E3779B1 + tk
    inputs = X.make_inputs(kind, nb, nh, tq, tk, seed=7 * tk + tq + nb)
    valid = X.make_valid("ragged", nb, tk)
    out = _chain(gpu, inputs, valid, p, seed, seed_dev)
    ref = _reference(inputs, valid, (p, seed, seed_dev))
    _check(f"dropout {p}, seed_dev {seed_dev}: {nb}x{nh}x{tq}x{tk} {kind}, {tk // X.key_chunk(tk)} chunk(s)", out, ref, nb, nh)
    plain = _chain(gpu, inputs, valid)
    assert not _same(out, plain, ("lse",)) and _same(out, plain, ("o", "dq", "dkv")) == ["o", "dq", "dkv"]


@pytest.mark.parametrize("tk", [128, 256, 384])
def test_strided_rows_are_bit_identical_and_nothing_else_is_written(gpu, tk):
    """q, o, dout, dq as column windows of wider buffers and ld_kv = 2 H dh + 8: bit-identical to the compact call (``_chain``
    checks the gap columns and the guard rows of both).  More than one key chunk needs compact dq rows and says so."""
    from reformer_tts_amd import _lib
    nb, nh, tq = 3, 3, 128
    inputs = X.make_inputs("plain", nb, nh, tq, tk, seed=tk)
    valid = X.make_valid("ragged", nb, tk)
    multi = tk // X.key_chunk(tk) > 1
    compact = _chain(gpu, inputs, valid, 0.1, 11, 3)
    wide = _chain(gpu, inputs, valid, 0.1, 11, 3, wide=True, wide_dq=not multi)
    assert _same(compact, wide, ALL) == []
    _check(f"strided rows, {tk} keys", wide, _reference(inputs, valid, (0.1, 11, 3)), nb, nh)
    if multi:
        with pytest.raises(_lib.RttsError, match=r"rtts_xattn_bwd: T_k=384 is worked in 3 key chunks: needs dq_chunks .* and ld_dq == H\*dh"):
            _chain(gpu, inputs, valid, wide=True, wide_dq=True)
        torch.cuda.synchronize()


@pytest.mark.parametrize("nb,nh,tq,tk,p", [(3, 1, 128, 256, 0.0), (1, 3, 384, 1152, 0.5)])
def test_two_runs_are_bit_identical(gpu, nb, nh, tq, tk, p):
    inputs = X.make_inputs("peaked", nb, nh, tq, tk, seed=tk)
    valid = X.make_valid("ragged", nb, tk)
    a = _chain(gpu, inputs, valid, p, 3, 4)
    b = _chain(gpu, inputs, valid, p, 3, 4)
    assert _same(a, b, ALL) == []


@pytest.mark.parametrize("tq,tk,p", [(256, 640, 0.0), (128, 256, 0.5)])
def test_a_sample_without_a_valid_key(gpu, tq, tk, p):
    """Sample 1 of 3 has no valid key.  Samples 0 and 2 meet the bounds and are bit-identical (o, lse, dq, their rows of every
    dK/dV slab) to the same call with sample 1 unpadded.  Sample 1 itself is what include/rtts.h states next to rtts_xattn_fwd:
    o NaN, lse -inf, dq and dk NaN -- as nn.MultiheadAttention -- and dv exactly 0 (its P is taken as 0 where kvalid is 0)."""
    nb, nh = 3, 2
    e = nh * X.DH
    inputs = X.make_inputs("plain", nb, nh, tq, tk, seed=tk + 1)
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


@pytest.mark.parametrize("n", [8, 8 * 257])
@pytest.mark.parametrize("nslabs", [1, 2, 3, 8, 15, 16])
def test_sum_slabs_is_the_sequential_fp32_sum(gpu, nslabs, n):
    _sum_slabs(gpu, nslabs, n)


def test_sum_slabs_grid_stride_loop(gpu):
    """The grid is capped at 4096 blocks of 256 threads x 8 elements: the smallest n that enters the grid-stride loop."""
    _sum_slabs(gpu, 2, 8 * (4096 * 256 + 5))


def _sum_slabs(gpu, nslabs, n):
    g = torch.Generator().manual_seed(nslabs * 31 + n % 1000)
    part = torch.randn(nslabs, n, generator=g).bfloat16().to(gpu)
    out = torch.full((3, n), SENT, dtype=torch.bfloat16, device=gpu)          # row 1 is the output, rows 0 and 2 guard it
    _call("rtts_sum_slabs", part.data_ptr(), nslabs, n, out[1].data_ptr(), _stream())
    torch.cuda.synchronize()
    acc = torch.zeros(n, device=gpu)
    for s in range(nslabs):
        acc += part[s].float()
    assert torch.equal(out[1].view(torch.int16), acc.bfloat16().view(torch.int16))
    assert bool((out[0] == SENT).all()) and bool((out[2] == SENT).all())


def test_sum_slabs_rejections(gpu):
    from reformer_tts_amd import _lib
    part = torch.zeros(2, 64, dtype=torch.bfloat16, device=gpu)
    out = torch.full((64,), SENT, dtype=torch.bfloat16, device=gpu)
    for nslabs, n in ((2, 12), (2, 0), (0, 64), (-1, 64)):
        with pytest.raises(_lib.RttsError, match="rtts_sum_slabs: n must be a positive multiple of 8"):
            _call("rtts_sum_slabs", part.data_ptr(), nslabs, n, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("nb,nh,t", [(1, 1, 128), (3, 3, 384)])
def test_bwd_delta_vs_float64(gpu, nb, nh, t, wide):
    """rtts_lsh_bwd_delta = rowsum(o o dO) per head: 64 fused multiply-adds in fp32, so |delta - float64| <= 64 2^-24 sum_d |o_d||dO_d|."""
    e = nh * X.DH
    g = torch.Generator().manual_seed(nb + t)
    o = torch.randn(nb, nh, t, X.DH, generator=g) + 0.5
    do = torch.randn(nb, nh, t, X.DH, generator=g) + 0.5
    ob = _Buf(gpu, nb * t, e, torch.bfloat16, e + 64 if wide else e, 32 if wide else 0, _pack(o))
    dob = _Buf(gpu, nb * t, e, torch.bfloat16, e + 8 if wide else e, 8 if wide else 0, _pack(do))
    delta = _Buf(gpu, nb * nh, t, torch.float32)
    _call("rtts_lsh_bwd_delta", ob.ptr, ob.ld, dob.ptr, dob.ld, nb, nh, t, X.DH, delta.ptr, _stream())
    torch.cuda.synchronize()
    assert delta.untouched() and ob.untouched() and dob.untouched()
    o64, do64 = X.bf(o).double(), X.bf(do).double()
    want = (o64 * do64).sum(-1).view(nb * nh, t)
    bound = 64 * 2.0 ** -24 * (o64.abs() * do64.abs()).sum(-1).view(nb * nh, t)
    ratio = float(((delta.cpu().double() - want).abs() / bound).max())
    print(f"\n[parity] rtts_lsh_bwd_delta {nb}x{nh}x{t}, {'strided' if wide else 'compact'}: worst |delta - float64| / bound {ratio:.3f} (must be <= 1)")
    assert ratio <= 1.0


def test_rejections_launch_nothing(gpu):
    """Every shape, stride, pointer and rate outside the envelope is refused with its message, before any launch."""
    from reformer_tts_amd import _lib
    e = 64
    mk = lambda rows, cols, dt=torch.bfloat16: torch.full((rows, cols), SENT, dtype=dt, device=gpu)
    q, kv, do, o, dq = mk(256, e + 8), mk(2304, 2 * e), mk(256, e), mk(256, e), mk(256, e)
    part, ws = mk(2 * 2304, 2 * e), mk(18 * 256, e)
    lse, delta = mk(1, 256, torch.float32), mk(1, 256, torch.float32)
    s = _stream()

    def fwd(tq=128, tk=128, ld_q=e, qoff=0, p=0.0):
        _call("rtts_xattn_fwd", q.data_ptr() + qoff, ld_q, kv.data_ptr(), 2 * e, None, 1, 1, tq, tk, 64, o.data_ptr(), e, lse.data_ptr(), p, 0, None, s)

    def bwd(tq=128, tk=128, ld_q=e, qoff=0, p=0.0, ws_ptr=None, ld_dq=e):
        _call("rtts_xattn_bwd", q.data_ptr() + qoff, ld_q, kv.data_ptr(), 2 * e, None, do.data_ptr(), e, lse.data_ptr(), delta.data_ptr(), 1, 1,
              tq, tk, 64, dq.data_ptr(), ld_dq, part.data_ptr(), p, 0, None, ws_ptr, s)

    for fn, name in ((fwd, "rtts_xattn_fwd"), (bwd, "rtts_xattn_bwd")):
        for tk in (192, 2176, 0):
            with pytest.raises(_lib.RttsError, match=re.escape(f"{name}: T_k={tk} unsupported (a multiple of 128 up to 2048)")):
                fn(tk=tk)
        with pytest.raises(_lib.RttsError, match=re.escape(f"{name}: T_q=64 must be a multiple of 128")):
            fn(tq=64)
        with pytest.raises(_lib.RttsError, match=re.escape(f"{name}: bad row strides")):
            fn(ld_q=e + 4)
        with pytest.raises(_lib.RttsError, match=re.escape(f"{name}: buffers must be 16-byte aligned")):
            fn(qoff=2)
        with pytest.raises(_lib.RttsError, match=re.escape(f"{name}: bad arguments")):
            fn(p=1.0)
    with pytest.raises(_lib.RttsError, match=r"rtts_xattn_bwd: T_k=384 is worked in 3 key chunks: needs dq_chunks \(3 x B\*T_q x H\*dh bf16\) and ld_dq == H\*dh"):
        bwd(tk=384)
    with pytest.raises(_lib.RttsError, match=r"rtts_xattn_bwd: T_k=2048 is worked in 8 key chunks: needs dq_chunks"):
        bwd(tk=2048, ws_ptr=ws.data_ptr(), ld_dq=e + 8)
    torch.cuda.synchronize()
    for name, b in (("o", o), ("lse", lse), ("dq", dq), ("dkv_part", part), ("dq_chunks", ws)):
        assert bool((b == SENT).all()), f"{name} was written by a rejected call"
