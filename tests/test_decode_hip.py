"""Single-query attention (csrc/decode.hip) against the float64 definition of tests/decode_ref.py and against the full-window
kernels it replaces in incremental generation (rtts_full_attn_fwd, rtts_xattn_fwd).

Self mode is held, element-wise, to ``full_attn_ref``'s bound for the same row, b_o = 2 u sum_j P_j |v_j| (u = 2^-8): the decode
kernel rounds only its output (P and the P V sum stay fp32), so it has room to spare.  Cross mode is held to u |o| + 2 u sum_j P_j
|v_j|.  Against the other kernel the bound is the sum of the two kernels' bounds.  Every test prints a ``[parity]`` line with the
worst error / bound.

Measured on an MI355X, worst ratio over the file: self against float64 0.460 (logits of about +-30; 0.175 at a few units), the same
for splits 1, 2, 3 and the library's pick; self against rtts_full_attn_fwd 0.469; cross against float64 0.316, against
rtts_xattn_fwd 0.376.  The whole file (30 cases) runs in 3 s."""
import pytest
import torch

import decode_ref as D
import full_attn_ref as R

pytestmark = pytest.mark.gpu

B, H, CAP = 2, 2, 192
POSITIONS = (0, 1, 63, 64, 65, 127, 128, 191)
SCALES = {"units": 4.0, "wide": 80.0}        # logits q.k^/8 ~ N(0, (scale/8)^2): a few units, and about +-30 at three sigma


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _ops():
    from reformer_tts_amd import ops
    return ops


@pytest.fixture(scope="module")
def self_case():
    """scale -> (qkv (B, CAP, 2*H*64) bf16 on the CPU, the float64 full-window reference of the same rows)."""
    out = {}
    for name, scale in SCALES.items():
        g = torch.Generator().manual_seed(len(name))
        qk = R.bf(torch.randn(B, H, CAP, 64, generator=g) * scale)
        v = R.bf(torch.randn(B, H, CAP, 64, generator=g))
        qkv = torch.cat([qk.transpose(1, 2).reshape(B, CAP, H * 64), v.transpose(1, 2).reshape(B, CAP, H * 64)], dim=-1).bfloat16()
        out[name] = (qkv, qk, v)
    return out


def _heads(o):
    """(B, H*64) -> (B, H, 64) float64 on the CPU."""
    return o.float().cpu().double().view(B, H, 64)


def _ratio(err, bound):
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("splits", [1, 2, 3, 0])
def test_self_kernel_matches_float64(gpu, self_case, scale, splits):
    ops = _ops()
    qkv, qk, v = self_case[scale]
    worst = 0.0
    for p in POSITIONS:
        cache = qkv.to(gpu).clone()
        cache[:, p:] = float("nan")                     # rows at and beyond p must not be read
        before = cache.clone()
        row = qkv[:, p].to(gpu).contiguous()
        pos = torch.tensor([p], dtype=torch.int32, device=gpu)
        o = ops.decode_self_attn(row, cache, pos, H, splits=splits)
        ref = D.self_attn(qk[:, :, p], v[:, :, p], qk, v, p)
        got = _heads(o)
        assert torch.isfinite(got).all(), f"p={p}: a cache row at or beyond p was read"
        worst = max(worst, _ratio((got - ref["o"]).abs(), ref["b_o"]))
        # the append: row p = the new row bit for bit, every other row as it was (NaN rows compared by their bits)
        assert torch.equal(cache[:, p].view(torch.int16), row.view(torch.int16))
        keep = torch.ones(CAP, dtype=torch.bool, device=gpu)
        keep[p] = False
        assert torch.equal(cache[:, keep].view(torch.int16), before[:, keep].view(torch.int16))
        # a second call: identical bits
        cache2 = before.clone()
        o2 = ops.decode_self_attn(row, cache2, pos, H, splits=splits)
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16))
        if p == 0:
            assert torch.equal(o.view(torch.int16), row[:, H * 64:].view(torch.int16)), "p = 0: o = v_0"
    print(f"[parity] decode self {scale} splits={splits}: worst |kernel - float64| / (2u sum P|v|) = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("scale", list(SCALES))
def test_self_kernel_matches_full_window_kernel(gpu, self_case, scale):
    """Row p of rtts_full_attn_fwd (causal, no mask, T = 192) on the same [qk | v]: the two kernels differ by at most the sum of
    their bounds, (2u + 2u) sum P|v|."""
    ops = _ops()
    qkv, qk, v = self_case[scale]
    dev = qkv.to(gpu)
    full, _ = ops.full_attn_fwd(dev[..., :H * 64], dev[..., H * 64:], H, True)
    worst = 0.0
    for p in POSITIONS:
        cache = dev.clone()
        pos = torch.tensor([p], dtype=torch.int32, device=gpu)
        o = ops.decode_self_attn(dev[:, p].contiguous(), cache, pos, H)
        ref = D.self_attn(qk[:, :, p], v[:, :, p], qk, v, p)
        worst = max(worst, _ratio((_heads(o) - _heads(full[:, p])).abs(), 2 * ref["b_o"]))
    print(f"[parity] decode self vs full_attn_fwd {scale}: worst difference / (4u sum P|v|) = {worst:.3f}")
    assert worst <= 1.0


def test_self_kernel_position_guard(gpu, self_case):
    """cap = 128 on a cache tensor of 192 rows, p = 128: o is all NaN and the cache tensor is unchanged."""
    ops = _ops()
    qkv, _, _ = self_case["units"]
    for splits in (1, 2, 0):
        cache = qkv.to(gpu).clone()
        before = cache.clone()
        pos = torch.tensor([128], dtype=torch.int32, device=gpu)
        o = ops.decode_self_attn(qkv[:, 128].to(gpu).contiguous(), cache, pos, H, cap=128, splits=splits)
        assert torch.isnan(o.float()).all()
        assert torch.equal(cache.view(torch.int16), before.view(torch.int16))


def test_bad_arguments_are_named(gpu, self_case):
    from reformer_tts_amd import _lib
    qkv, _, _ = self_case["units"]
    cache = qkv.to(gpu).clone()
    row = cache[:, 0].contiguous()
    pos = torch.zeros(1, dtype=torch.int32, device=gpu)
    o = torch.empty(B, H * 64, dtype=torch.bfloat16, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    for bad, name in ((dict(cap=100), "cap"), (dict(dh=32), "dh"), (dict(splits=65), "splits"), (dict(ld_row=100), "ld_row")):
        a = dict(ld_row=2 * H * 64, cap=CAP, dh=64, splits=1)
        a.update(bad)
        with pytest.raises(_lib.RttsError, match=name):
            _lib.call("rtts_decode_self_attn", row.data_ptr(), a["ld_row"], cache.data_ptr(), 2 * H * 64, CAP * 2 * H * 64, pos.data_ptr(), B, H,
                      a["cap"], a["dh"], o.data_ptr(), H * 64, a["splits"], None, s)
    with pytest.raises(_lib.RttsError, match="workspace"):
        _lib.call("rtts_decode_self_attn", row.data_ptr(), 2 * H * 64, cache.data_ptr(), 2 * H * 64, CAP * 2 * H * 64, pos.data_ptr(), B, H, CAP, 64,
                  o.data_ptr(), H * 64, 2, None, s)
    with pytest.raises(_lib.RttsError, match="Tk"):
        _lib.call("rtts_decode_cross_attn", row.data_ptr(), H * 64, cache.data_ptr(), 2 * H * 64, None, B, H, 192, 64, o.data_ptr(), H * 64, 1, None, s)
    lib = _lib.load()
    assert lib.rtts_decode_attn_splits(4, 100) == -1 and lib.rtts_decode_attn_splits(4, 192) >= 1
    assert lib.rtts_decode_attn_workspace(4, 2, 32) == -1 and lib.rtts_decode_attn_workspace(4, 2, 64) > 0
    assert torch.equal(cache.cpu(), qkv)            # nothing was launched


# ---------------------------------------------------------------------------------------------------------- cross mode
CB = 3


def _cross_inputs(dh, tk, seed):
    heads = 128 // dh * 2                          # width 256: 4 heads of 64 or 2 of 128
    g = torch.Generator().manual_seed(seed)
    q = R.bf(torch.randn(CB, heads, dh, generator=g) * 2.0)
    k = R.bf(torch.randn(CB, heads, tk, dh, generator=g) * 2.0)
    v = R.bf(torch.randn(CB, heads, tk, dh, generator=g))
    return heads, q, k, v


def _cross_dev(gpu, q, k, v):
    cb, heads, tk, dh = k.shape
    qd = q.reshape(cb, heads * dh).bfloat16().to(gpu)
    kv = torch.cat([k.transpose(1, 2).reshape(cb, tk, heads * dh), v.transpose(1, 2).reshape(cb, tk, heads * dh)], dim=-1).bfloat16().to(gpu)
    return qd, kv


def _ragged(tk, keyless=False):
    valid = torch.ones(CB, tk, dtype=torch.bool)
    valid[0, tk - 37:] = False
    valid[1] = False
    valid[1, 70] = True                            # a single valid key, in the second tile
    if keyless:
        valid[2] = False
    else:
        valid[2, 5:tk - 3] = False
    return valid


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("tk", [128, 384])
@pytest.mark.parametrize("splits", [1, 2, 0])
def test_cross_kernel_matches_float64_and_xattn(gpu, dh, tk, splits):
    from reformer_tts_amd import _lib
    ops = _ops()
    heads, q, k, v = _cross_inputs(dh, tk, 7 * dh + tk)
    qd, kv = _cross_dev(gpu, q, k, v)
    e = heads * dh
    for valid in (None, _ragged(tk)):
        vd = None if valid is None else valid.to(gpu).to(torch.uint8)
        o = ops.decode_cross_attn(qd, kv, heads, vd, splits=splits)
        o2 = ops.decode_cross_attn(qd, kv, heads, vd, splits=splits)
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16))
        ref = D.cross_attn(q, k, v, valid)
        got = o.float().cpu().double().view(CB, heads, dh)
        r64 = _ratio((got - ref["o"]).abs(), ref["b_o"])
        if valid is not None:                       # the sample with one valid key: o = that key's value, exactly
            assert torch.equal(got[1], v[1, :, 70].double())
        # rtts_xattn_fwd at T_q = 128 with the query in row 0
        qw = torch.zeros(CB, 128, e, dtype=torch.bfloat16, device=gpu)
        qw[:, 0] = qd
        ow = torch.empty(CB * 128, e, dtype=torch.bfloat16, device=gpu)
        lse = torch.empty(CB * heads, 128, dtype=torch.float32, device=gpu)
        _lib.call("rtts_xattn_fwd", qw.data_ptr(), e, kv.data_ptr(), 2 * e, None if vd is None else vd.data_ptr(), CB, heads, 128, tk, dh,
                  ow.data_ptr(), e, lse.data_ptr(), 0.0, 0, None, torch.cuda.current_stream().cuda_stream)
        other = ow.view(CB, 128, e)[:, 0].float().cpu().double().view(CB, heads, dh)
        rx = _ratio((got - other).abs(), ref["b_o"] + 2 * D.U * ref["pv"])
        print(f"[parity] decode cross dh={dh} tk={tk} splits={splits} mask={'ragged' if valid is not None else 'none'}: "
              f"vs float64 {r64:.3f}, vs rtts_xattn_fwd {rx:.3f} (of their bounds)")
        assert r64 <= 1.0 and rx <= 1.0


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("splits", [1, 2, 0])
def test_cross_kernel_keyless_sample(gpu, dh, splits):
    ops = _ops()
    tk = 384
    heads, q, k, v = _cross_inputs(dh, tk, dh)
    qd, kv = _cross_dev(gpu, q, k, v)
    o_nan = ops.decode_cross_attn(qd, kv, heads, _ragged(tk, keyless=True).to(gpu).to(torch.uint8), splits=splits)
    o_ok = ops.decode_cross_attn(qd, kv, heads, _ragged(tk).to(gpu).to(torch.uint8), splits=splits)
    assert torch.isnan(o_nan[2].float()).all()
    assert torch.isfinite(o_ok.float()).all()
    assert torch.equal(o_nan[:2].view(torch.int16), o_ok[:2].view(torch.int16))
