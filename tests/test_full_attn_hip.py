"""Dense shared-QK attention (csrc/full_attn.hip) through the C ABI against the float64 definition of tests/full_attn_ref.py, over
the envelope fa_check accepts.  Every call goes through ``_lib.call`` in the engine's order: rtts_full_attn_fwd, rtts_lsh_bwd_delta
on the kernel's own out, rtts_full_attn_bwd with the kernel's own lse.

Comparison: |got - float64| <= bound ELEMENT-WISE on o, dqk, dv with the per-element first-order bounds of full_attn_ref.py
(u = 2^-8 per rounding to bf16, the roundings listed there with their source lines); nothing is excluded.  Every test prints a
``[parity]`` line with the worst ratio per quantity.

lse is fp32 end to end; on the rows of valid queries its bound is LSE_C 2^-24 (max_j sum_d |q_d k^_jd| / 8 + |lse| + 1), on the
rows of masked queries it must be -FLT_MAX exactly.  The CPU fp32 model of the kernel needs C = 1.61 (tests/test_full_attn_cpu.py);
LSE_C = 7 is four times that, rounded up (the margin is for another MFMA summation order and the fast exp / log / rsq).

Measured on an MI355X, worst |kernel - float64| / bound over the whole file (must be <= 1; lse in units of its scale, <= 7):
    o   0.834  (1x2x1024 peaked, hole in the middle, causal)       dqk 0.494  (1x2x192 peaked, causal, dropout 0.5)
    dv  0.937  (1x2x1024 peaked, no mask, causal)                  lse 2.02   (1x1x4096 plain, ragged, causal)
    masked queries: lse == -FLT_MAX in every case; the whole file (190 cases) runs in 6 s."""
import numpy as np
import pytest
import torch

import full_attn_ref as R

pytestmark = pytest.mark.gpu

LSE_C = 7.0
SENT = -7.0                  # sentinel of every pre-filled buffer (exact in bf16)
GUARD = 4                    # guard rows in front of and behind every output
DH = R.DH


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

    def pristine(self):
        return bool((self.full == SENT).all())

    def cpu(self):
        return self.view.contiguous().cpu()


def _pack(x):
    """(B, H, T, 64) -> (B * T, H * 64) bf16, the kernels' layout."""
    nb, nh, t, dh = x.shape
    return x.transpose(1, 2).reshape(nb * t, nh * dh).bfloat16()


def _unpack(buf, nb, nh):
    return buf.double().view(nb, -1, nh, DH).transpose(1, 2)


class _Chain:
    """Device buffers of one call, every one pre-filled with a sentinel.  ``wide``: the [qk | v] rows are 2 H dh + 64 apart and
    start at column 32, out / dout rows are H dh + 64 apart, [dqk | dv] rows 2 H dh + 64."""

    def __init__(self, gpu, inputs, mask, wide=False, seed_dev=None):
        qk, v, do = inputs
        self.nb, self.nh, self.t, _ = qk.shape
        nb, nh, t = self.nb, self.nh, self.t
        self.e = e = nh * DH
        bf16 = torch.bfloat16
        pad, c0 = (64, 32) if wide else (0, 0)
        self.qkv = _Buf(gpu, nb * t, 2 * e, bf16, 2 * e + pad, c0, torch.cat([_pack(qk), _pack(v)], dim=1))
        self.do = _Buf(gpu, nb * t, e, bf16, e + pad, c0, _pack(do))
        self.o = _Buf(gpu, nb * t, e, bf16, e + pad, c0)
        self.lse = _Buf(gpu, nb * nh, t, torch.float32)
        self.delta = _Buf(gpu, nb * nh, t, torch.float32)
        self.dqkv = _Buf(gpu, nb * t, 2 * e, bf16, 2 * e + pad, c0)
        self.ws = _Buf(gpu, nb * nh * t, DH, torch.float32)
        self.mask = None if mask is None else mask.to(torch.uint8).to(gpu)
        self.sd = None if seed_dev is None else torch.from_numpy(np.array([seed_dev], dtype=np.uint32).view(np.int32)).to(gpu)

    @property
    def mp(self):
        return None if self.mask is None else self.mask.data_ptr()

    @property
    def sp(self):
        return None if self.sd is None else self.sd.data_ptr()

    def fwd(self, causal, p=0.0, seed=0, **over):
        a = dict(qk=self.qkv.ptr, v=self.qkv.ptr + 2 * self.e, ld=self.qkv.ld, t=self.t, dh=DH, lse=self.lse.ptr)
        a.update(over)
        _call("rtts_full_attn_fwd", a["qk"], a["v"], a["ld"], self.mp, self.nb, self.nh, a["t"], a["dh"], int(causal), self.o.ptr, self.o.ld,
              a["lse"], p, seed, self.sp, _stream())

    def delta_(self):
        _call("rtts_lsh_bwd_delta", self.o.ptr, self.o.ld, self.do.ptr, self.do.ld, self.nb, self.nh, self.t, DH, self.delta.ptr, _stream())

    def bwd(self, causal, p=0.0, seed=0, **over):
        a = dict(ld=self.qkv.ld, t=self.t, dh=DH, lse=self.lse.ptr)
        a.update(over)
        _call("rtts_full_attn_bwd", self.qkv.ptr, self.qkv.ptr + 2 * self.e, a["ld"], self.mp, self.do.ptr, self.do.ld, a["lse"], self.delta.ptr,
              self.nb, self.nh, a["t"], a["dh"], int(causal), self.dqkv.ptr, self.dqkv.ptr + 2 * self.e, self.dqkv.ld, self.ws.ptr, p, seed,
              self.sp, _stream())

    def run(self, causal, p=0.0, seed=0):
        self.fwd(causal, p, seed)
        self.delta_()
        self.bwd(causal, p, seed)
        torch.cuda.synchronize()
        for name in ("qkv", "do", "o", "lse", "delta", "dqkv", "ws"):
            assert getattr(self, name).untouched(), f"{name}: a gap column or a guard row was written"
        return dict(o=self.o.cpu(), lse=self.lse.cpu(), delta=self.delta.cpu(), dqkv=self.dqkv.cpu())


def _tensors(out, nb, nh):
    e = nh * DH
    return dict(o=_unpack(out["o"], nb, nh), dqk=_unpack(out["dqkv"][:, :e], nb, nh), dv=_unpack(out["dqkv"][:, e:], nb, nh),
                lse=out["lse"].double().view(nb, nh, -1))


def _check(tag, out, ref, nb, nh, mask):
    got = _tensors(out, nb, nh)
    r = R.ratios(got, ref)
    r["lse"] = R.lse_ratio(got["lse"], ref, mask)
    print(f"\n[parity] {tag}: worst |kernel - float64| / bound  " + "  ".join(f"{n} {x:.3f}" for n, x in r.items())
          + f"  (o, dqk, dv must be <= 1; lse is in units of 2^-24 scale, must be <= {LSE_C:g})")
    assert r["o"] <= 1.0 and r["dqk"] <= 1.0 and r["dv"] <= 1.0, r
    assert r["lse"] <= LSE_C, r
    if mask is not None:                                   # masked queries: lse is -FLT_MAX exactly
        inv = (~mask)[:, None, :].expand(nb, nh, mask.shape[1])
        assert bool((got["lse"][inv] == -R.FMAX).all())
    return got


def _reference(inputs, mask, causal, drop=None):
    nb, nh, t, _ = inputs[0].shape
    keep = None if drop is None else R.keep_scales(*drop, nb * nh, t).view(nb, nh, t, t)
    return R.reference(*inputs, mask, causal, keep)


# one tile and one workgroup; two tiles; T no multiple of 128; a grid of 24 (a multiple of 8: xcd_remap's even branch) and of
# 3 x 2 x 4; three and more key tiles (the running maximum is rescaled twice); 16 tiles
SHAPES = [(1, 1, 64), (2, 2, 128), (1, 2, 192), (3, 2, 256), (2, 1, 384), (1, 2, 1024)]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("mask_kind", R.MASKS)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("nb,nh,t", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in SHAPES])
def test_forward_and_backward_within_the_bounds(gpu, nb, nh, t, causal, mask_kind, kind):
    inputs = R.make_inputs(kind, nb, nh, t, seed=1000 * nb + 100 * nh + t)
    mask = R.make_mask(mask_kind, nb, t)
    out = _Chain(gpu, inputs, mask).run(causal)
    got = _check(f"{nb}x{nh}x{t} {kind}, mask {mask_kind}, causal {causal}", out, _reference(inputs, mask, causal), nb, nh, mask)
    v = inputs[1].double()
    if causal:                                             # row 0 keeps only its -5e4 diagonal -- where token 0 is valid
        ok0 = torch.ones(nb, dtype=torch.bool) if mask is None else mask[:, 0]
        assert bool((got["lse"][ok0, :, 0] == -5e4).all())
        assert torch.equal(got["o"][ok0, :, 0], v[ok0, :, 0])
    if mask is not None:                                   # masked queries: the plain mean of all T value rows
        inv = (~mask)[:, None, :, None].expand_as(got["o"])
        mean_v = v.mean(dim=2, keepdim=True).expand_as(got["o"])
        assert float((got["o"] - mean_v)[inv].abs().max()) <= 2 * R.U * float(v.abs().mean(dim=2).max()) + 1e-12


def test_longest_sequence(gpu):
    from reformer_tts_amd import _lib
    lib = _lib.load()
    t = lib.rtts_full_attn_max_t(64)
    assert t >= 2048 and t % 64 == 0 and lib.rtts_full_attn_max_t(32) == -1 and lib.rtts_full_attn_max_t(128) == -1
    assert lib.rtts_full_attn_bwd_workspace(1, 1, t, 64) == t * 64 * 4 and lib.rtts_full_attn_bwd_workspace(1, 1, t + 64, 64) == -1
    inputs = R.make_inputs("plain", 1, 1, t, seed=t)
    mask = R.make_mask("ragged", 1, t)
    out = _Chain(gpu, inputs, mask).run(True)
    _check(f"1x1x{t} plain, ragged, causal", out, _reference(inputs, mask, True), 1, 1, mask)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_masked_query_feeds_every_dv_and_no_dqk(gpu, causal):
    """dout only on the rows of masked queries: dqk is exactly 0 everywhere, dv_j = sum_i dout_i / T for EVERY key j (padding keys
    and, under causal, the keys before and after i alike)."""
    nb, nh, t = 2, 2, 192
    qk, v, do = R.make_inputs("plain", nb, nh, t, seed=77)
    mask = R.make_mask("hole", nb, t)
    do = do * (~mask)[:, None, :, None].float()
    out = _Chain(gpu, (qk, v, do), mask).run(causal)
    got = _check(f"masked-query dout, causal {causal}", out, _reference((qk, v, do), mask, causal), nb, nh, mask)
    assert float(got["dqk"].abs().max()) == 0.0
    want = do.double().sum(dim=2, keepdim=True) / t
    assert float(want.abs().min()) > 0.0
    assert float((got["dv"] - want).abs().max()) <= 2 * R.U * float(do.abs().sum(dim=2).max()) / t + 1e-12
    assert float(got["dv"].abs().min()) > 0.0


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_strided_rows_equal_compact_rows_and_runs_repeat(gpu, causal):
    nb, nh, t = 2, 2, 192
    inputs = R.make_inputs("peaked", nb, nh, t, seed=21)
    mask = R.make_mask("ragged", nb, t)
    a = _Chain(gpu, inputs, mask).run(causal, 0.1, 17)
    b = _Chain(gpu, inputs, mask, wide=True).run(causal, 0.1, 17)
    c = _Chain(gpu, inputs, mask).run(causal, 0.1, 17)
    for n in ("o", "lse", "delta", "dqkv"):
        assert torch.equal(a[n].view(torch.int16 if a[n].dtype == torch.bfloat16 else torch.int32),
                           b[n].view(torch.int16 if b[n].dtype == torch.bfloat16 else torch.int32)), f"{n}: strided != compact"
        assert torch.equal(a[n].view(torch.int16 if a[n].dtype == torch.bfloat16 else torch.int32),
                           c[n].view(torch.int16 if c[n].dtype == torch.bfloat16 else torch.int32)), f"{n}: two runs differ"


DROP_CASES = [(2, 2, 128, False, "plain", 0.1, None), (1, 2, 192, True, "peaked", 0.5, 5), (3, 2, 256, True, "plain", 0.5, 0xFFFFFFF0),
              (2, 1, 384, False, "offset", 0.1, 9)]


@pytest.mark.parametrize("nb,nh,t,causal,kind,p,seed_dev", DROP_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-p{c[5]}-{c[6]}" for c in DROP_CASES])
def test_dropout_against_the_mask_twin(gpu, nb, nh, t, causal, kind, p, seed_dev):
    inputs = R.make_inputs(kind, nb, nh, t, seed=t + 1)
    mask = R.make_mask("hole", nb, t)
    seed = 0x12345 + t
    out = _Chain(gpu, inputs, mask, seed_dev=seed_dev).run(causal, p, seed)
    _check(f"{nb}x{nh}x{t} {kind} dropout {p} seed_dev {seed_dev}", out, _reference(inputs, mask, causal, (p, seed, seed_dev)), nb, nh, mask)


def test_rejections_launch_nothing(gpu):
    from reformer_tts_amd import _lib
    nb, nh, t = 1, 2, 128
    inputs = R.make_inputs("plain", nb, nh, t, seed=1)
    ch = _Chain(gpu, inputs, None)
    tmax = _lib.load().rtts_full_attn_max_t(64)
    bad = [dict(t=96), dict(t=tmax + 64), dict(t=0), dict(dh=32), dict(ld=2 * ch.e + 4), dict(ld=ch.e // 2), dict(lse=None)]
    for over in bad:
        with pytest.raises(_lib.RttsError, match="rtts_full_attn_fwd"):
            ch.fwd(True, **over)
        with pytest.raises(_lib.RttsError, match="rtts_full_attn_bwd"):
            ch.bwd(True, **over)
    with pytest.raises(_lib.RttsError, match="rtts_full_attn_fwd"):
        ch.fwd(False, 1.0)
    with pytest.raises(_lib.RttsError, match="16-byte"):
        ch.fwd(False, qk=ch.qkv.ptr + 2)
    torch.cuda.synchronize()
    for name in ("o", "lse", "dqkv", "ws"):
        assert getattr(ch, name).pristine(), f"{name} was written by a refused call"
