"""GPU parity of the LSH attention kernels (through the C ABI) against the oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import lsh_int, lsh_ref

pytestmark = pytest.mark.gpu


@pytest.fixture
def force_walk():
    """Force the run length of the walking kernels for the rest of the test (``rtts_debug_set_walk`` of include/rtts.h through
    ``_lib.forced_walk``: the library's launch path reads no environment variable); undone when the test ends."""
    import contextlib
    from reformer_tts_amd import _lib
    stack = contextlib.ExitStack()

    def force(fwd=None, bwd=None):
        stack.enter_context(_lib.forced_walk(fwd, bwd))
    yield force
    stack.close()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reformer_tts_amd import ops as _ops
    return _ops


def _heads_first(x, b, t, h, dh):
    """(B,T,H*dh) -> (B*H,T,dh) float32 on the CPU."""
    return x.float().cpu().view(b, t, h, dh).transpose(1, 2).reshape(b * h, t, dh)


def _make_qkv(b, t, h, dh, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, t, 2 * h * dh, generator=g) * scale).bfloat16()


def _flat_perm(st_cpu):
    bh, nh, t = st_cpu.shape
    sticker = (st_cpu.long() + (torch.arange(nh) * t).view(1, nh, 1)).reshape(bh, nh * t)
    undo = torch.empty_like(sticker)
    undo.scatter_(1, sticker, torch.arange(nh * t).expand(bh, -1))
    return sticker, undo


# ------------------------------------------------------------------ integer stages: bit-exact
@pytest.mark.parametrize("b,h,t,bs,nh,per_head", [
    (2, 2, 128, 64, 4, False), (2, 3, 256, 64, 8, True), (2, 8, 1024, 128, 8, False),
    (1, 2, 1024, 64, 8, False), (1, 2, 4096, 64, 8, False), (1, 1, 2048, 128, 3, True),
    (1, 2, 3072, 64, 4, True),      # 48 buckets: the f32-MFMA projection path with zero-padded rotation columns
])
def test_hash_sort_bit_exact(ops, b, h, t, bs, nh, per_head):
    dh = 64
    qkv = _make_qkv(b, t, h, dh, seed=t + nh)
    g = torch.Generator().manual_seed(1)
    rot = torch.randn(b * h if per_head else 1, dh, nh, t // bs // 2, generator=g)
    qkv_d = qkv.cuda()
    st, buckets, undo = ops.lsh_hash_sort(qkv_d[..., :h * dh], rot.cuda(), h, bs, want_buckets=True, want_undo=True)
    torch.cuda.synchronize()
    qk = _heads_first(qkv[..., :h * dh], b, t, h, dh)
    exp_b = lsh_int.hash_buckets(qk.numpy(), rot.numpy())
    assert np.array_equal(buckets.cpu().numpy(), exp_b)
    exp_st, exp_undo = lsh_int.sort_buckets(exp_b, t // bs)
    assert np.array_equal(st.cpu().numpy(), exp_st)
    assert np.array_equal(undo.cpu().numpy(), exp_undo)


def test_hash_sort_vs_huggingface_fixture(ops, golden_dir):
    z = np.load(os.path.join(golden_dir, "hf_lsh_int.npz"))
    for tag in ("a", "b", "c"):
        heads, t, dh, chunk, nh = (int(x) for x in z[f"{tag}/meta"])
        vec = torch.from_numpy(np.random.RandomState(5).standard_normal((2, heads, t, dh)).astype(np.float32))
        vec_bf = vec.bfloat16()
        qk = vec_bf.transpose(1, 2).reshape(2, t, heads * dh).contiguous()
        rot = torch.from_numpy(np.tile(z[f"{tag}/rot"], (2, 1, 1, 1)))
        st, buckets, _ = ops.lsh_hash_sort(qk.cuda(), rot.cuda(), heads, chunk, want_buckets=True)
        exp = z[f"{tag}/buckets"].astype(np.int32).reshape(2 * heads, nh, t)
        # the fixture hashed fp32 vectors; bf16 rounding of the input may move near-ties only
        assert (buckets.cpu().numpy() != exp).mean() < 2e-2, tag
        exp_st, _ = lsh_int.sort_buckets(buckets.cpu().numpy(), t // chunk)
        assert np.array_equal(st.cpu().numpy(), exp_st), tag


def test_hash_sort_rejects_bad_length(ops):
    qk = torch.zeros(1, 192, 128, dtype=torch.bfloat16, device="cuda")
    rot = torch.zeros(1, 64, 2, 1, device="cuda")
    with pytest.raises(AssertionError, match="divisible by target bucket size"):
        ops.lsh_hash_sort(qk, rot, 2, 64)


# ------------------------------------------------------------------ attention forward
CASES = [
    # b, h, t, bs, nh, causal, masked
    (2, 2, 128, 64, 4, False, False),
    (1, 2, 4096, 64, 8, True, True),          # BASELINE config #4 shape: 64 buckets per round
    (2, 2, 256, 64, 4, True, True),
    (1, 3, 512, 128, 2, True, False),
    (2, 2, 512, 128, 8, False, True),
    (1, 8, 1024, 128, 8, True, True),
    (2, 2, 768, 128, 4, True, True),          # 6 buckets: not a power of two (a 768-frame mel at bucket size 128)
    (1, 2, 3840, 64, 4, True, False),         # 60 buckets
    (1, 2, 384, 64, 4, False, True),          # 6 buckets at bucket size 64
]


def _run_fwd(ops, b, h, t, bs, nh, causal, masked, seed=0):
    dh = 64
    qkv = _make_qkv(b, t, h, dh, seed=seed + t)
    g = torch.Generator().manual_seed(seed + 7)
    rot = torch.randn(1, dh, nh, t // bs // 2, generator=g)
    mask = None
    if masked:
        mask = torch.ones(b, t, dtype=torch.bool)
        mask[0, t - t // 3:] = False
        if b > 1:
            mask[1, t // 2:] = False
    qkv_d = qkv.cuda()
    qk_d, v_d = qkv_d[..., :h * dh], qkv_d[..., h * dh:]
    st, _, undo = ops.lsh_hash_sort(qk_d, rot.cuda(), h, bs, want_undo=True)
    o, lse = ops.lsh_attn_fwd(qk_d, v_d, st, h, bs, causal, None if mask is None else mask.cuda())
    out, lse_tot = ops.lsh_combine_fwd(o, lse, b, h)
    torch.cuda.synchronize()
    return dict(qkv=qkv, qk_d=qk_d, v_d=v_d, st=st, undo=undo, o=o, lse=lse, out=out, lse_tot=lse_tot, mask=mask, dh=dh)


@pytest.mark.parametrize("walk", ["0", "4"])
@pytest.mark.parametrize("b,h,t,bs,nh,causal,masked", CASES)
def test_attention_forward_vs_oracle(ops, force_walk, b, h, t, bs, nh, causal, masked, walk):
    """Tolerance: inputs are identical bf16 values; the kernel rounds P to bf16 (2^-9 rel) before
    PV and o/out to bf16 on store => |err| ~ 4e-3 * max|v| on rows that see other tokens (bounds: 3x achieved).
    Rows that can only see themselves (lse ~ -5e4) sit on fp32's 4e-3 logsumexp grid, so the
    round weights legitimately differ there (see oracle/lsh_ref.py).  ``walk``: the one-chunk kernel / the walking kernel at
    runs of 4 chunks (what the decoder shape gets; these test shapes would get the one-chunk kernel by themselves)."""
    if int(walk) == 0 or (nh * (t // bs)) % int(walk) == 0:
        force_walk(fwd=int(walk))
    r = _run_fwd(ops, b, h, t, bs, nh, causal, masked)
    dh = r["dh"]
    qk = _heads_first(r["qkv"][..., :h * dh], b, t, h, dh)
    v = _heads_first(r["qkv"][..., h * dh:], b, t, h, dh)
    sticker, undo = _flat_perm(r["st"].cpu())
    m = None if r["mask"] is None else r["mask"].unsqueeze(1).expand(b, h, t).reshape(b * h, t)
    out_ref, o_ref, lse_ref = lsh_ref.lsh_attention_sorted(qk, v, sticker, undo, bs, nh, causal, m, return_parts=True)
    o, lse = r["o"].float().cpu(), r["lse"].cpu()
    out = _heads_first(r["out"], b, t, h, dh)
    lse_tot_ref = torch.logsumexp(lse_ref, dim=1)
    normal = lse_tot_ref > -1e4
    vmax = v.abs().max().item()
    e_lse = ((lse - lse_ref).abs() / (1 + lse_ref.abs())).max().item()
    e_o = (o - o_ref).abs().max().item() / vmax
    e_out = (out[normal] - out_ref[normal]).abs().max().item() / vmax
    e_mean = (out[normal] - out_ref[normal]).abs().mean().item() / vmax
    print(f"\n[lsh attention forward B={b} H={h} T={t} bs={bs} R={nh} causal={causal} masked={masked}] / max|v|: o max {e_o:.2e}, "
          f"out max {e_out:.2e} mean {e_mean:.2e}; lse max {e_lse:.2e} of 1+|lse| (tol 1.2e-2, 1.2e-2, 8e-4, 1e-3)")
    # bounds = ~3x the largest achieved error over all cases (o / out 3.9e-3 of max|v|, mean 2.4e-4, lse 3e-4): a regression
    # that triples the error fails
    torch.testing.assert_close(lse, lse_ref, rtol=1e-3, atol=1e-3)
    assert e_o < 1.2e-2 and e_out < 1.2e-2 and e_mean < 8e-4, (e_o, e_out, e_mean)
    torch.testing.assert_close(out[~normal], out_ref[~normal], rtol=1e-1, atol=1e-1)
    torch.testing.assert_close(r["lse_tot"].cpu(), lse_tot_ref, rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------ attention backward
@pytest.mark.parametrize("walk", ["0", "4", "8"])
@pytest.mark.parametrize("b,h,t,bs,nh,causal,masked", CASES)
def test_attention_backward_vs_oracle_autograd(ops, force_walk, b, h, t, bs, nh, causal, masked, walk):
    """Gradients of sum(out * dout) w.r.t. qk and v against autograd through the oracle on the same
    permutation, for both forms of the kernel (``walk``: one workgroup per chunk / workgroups walking 4 or 8 chunks -- 8 is what
    the library picks at the bench shape, the small test shapes would all get the first; the library's own pick at the bench
    shape is ``test_attention_backward_at_the_bench_shape_with_the_library_pick``).  bf16 partials and bf16 P/dS operands
    put the error at ~0.5% of the gradient scale; the bounds are 3x what is achieved."""
    if (nh * (t // bs)) % max(int(walk), 1):
        pytest.skip("the run length does not divide this ring")
    force_walk(bwd=int(walk))
    r = _run_fwd(ops, b, h, t, bs, nh, causal, masked, seed=3)
    dh = r["dh"]
    g = torch.Generator().manual_seed(11)
    dout = torch.randn(b, t, h * dh, generator=g).bfloat16()
    dqk, dv = ops.lsh_attn_bwd(r["qk_d"], r["v_d"], r["st"], r["out"], dout.cuda(), r["lse_tot"], h, bs, causal,
                               None if r["mask"] is None else r["mask"].cuda())
    torch.cuda.synchronize()
    qk = _heads_first(r["qkv"][..., :h * dh], b, t, h, dh).requires_grad_()
    v = _heads_first(r["qkv"][..., h * dh:], b, t, h, dh).requires_grad_()
    sticker, undo = _flat_perm(r["st"].cpu())
    m = None if r["mask"] is None else r["mask"].unsqueeze(1).expand(b, h, t).reshape(b * h, t)
    out_ref = lsh_ref.lsh_attention_sorted(qk, v, sticker, undo, bs, nh, causal, m)
    out_ref.backward(_heads_first(dout, b, t, h, dh))
    dqk_h, dv_h = _heads_first(dqk, b, t, h, dh), _heads_first(dv, b, t, h, dh)
    msgs = []
    for got, ref, name in ((dv_h, v.grad, "dv"), (dqk_h, qk.grad, "dqk")):
        scale = ref.abs().max().item()
        err = (got - ref).abs()
        msgs.append(f"{name} max {err.max().item() / scale:.2e} mean {err.mean().item() / scale:.2e} rel-L2 {float((got - ref).norm() / ref.norm()):.2e}")
        # ~3x the largest achieved error over all cases and both kernel forms (max 5.4e-3, mean 3e-4, rel-L2 3.2e-3)
        assert err.max().item() < 1.5e-2 * scale, (name, err.max().item(), scale)
        assert err.mean().item() < 1e-3 * scale, (name, err.mean().item(), scale)
        assert float((got - ref).norm() / ref.norm()) < 1e-2, (name, float((got - ref).norm() / ref.norm()))
    print(f"\n[lsh attention backward B={b} H={h} T={t} bs={bs} R={nh} causal={causal} masked={masked} walk={walk}] errors / max|ref|: " + "; ".join(msgs) +
          " (tol max 1.5e-2, mean 1e-3, rel-L2 1e-2)")


def test_attention_at_the_bench_shape_with_the_library_pick(ops):
    """BASELINE config #2's decoder shape (B = 12, H = 8, T = 1024, 128-row buckets, 8 rounds, causal): NOTHING forced -- the
    library's own pick is the walking forward at runs of 4 and the walking backward at runs of 8 (what ``bench.py`` times as
    ``roofline``), compared directly with the oracle and its autograd on the same permutation (about 10 s of CPU oracle)."""
    from reformer_tts_amd import _lib
    b, h, t, bs, nh, causal = 12, 8, 1024, 128, 8, True
    lib = _lib.load()
    assert _lib._WALK == [-1, -1], "a run length is forced (RTTS_LSH_*_WALK in the environment?): this test is about the library's pick"
    assert lib.rtts_lsh_attn_fwd_run_length(b, h, t, nh, bs) == 4 and lib.rtts_lsh_attn_bwd_run_length(b, h, t, nh, bs) == 8
    r = _run_fwd(ops, b, h, t, bs, nh, causal, False, seed=21)
    dh = r["dh"]
    dout = torch.randn(b, t, h * dh, generator=torch.Generator().manual_seed(17)).bfloat16()
    dqk, dv = ops.lsh_attn_bwd(r["qk_d"], r["v_d"], r["st"], r["out"], dout.cuda(), r["lse_tot"], h, bs, causal, None)
    torch.cuda.synchronize()
    qk = _heads_first(r["qkv"][..., :h * dh], b, t, h, dh).requires_grad_()
    v = _heads_first(r["qkv"][..., h * dh:], b, t, h, dh).requires_grad_()
    sticker, undo = _flat_perm(r["st"].cpu())
    out_ref, o_ref, lse_ref = lsh_ref.lsh_attention_sorted(qk, v, sticker, undo, bs, nh, causal, None, return_parts=True)
    vmax = v.abs().max().item()
    e_o = (r["o"].float().cpu() - o_ref.detach()).abs().max().item() / vmax
    e_out = (_heads_first(r["out"], b, t, h, dh) - out_ref.detach()).abs().max().item() / vmax
    torch.testing.assert_close(r["lse"].cpu(), lse_ref.detach(), rtol=1e-3, atol=1e-3)
    assert e_o < 1.2e-2 and e_out < 1.2e-2, (e_o, e_out)
    out_ref.backward(_heads_first(dout, b, t, h, dh))
    msgs = []
    for got, ref, name in ((_heads_first(dv, b, t, h, dh), v.grad, "dv"), (_heads_first(dqk, b, t, h, dh), qk.grad, "dqk")):
        scale = ref.abs().max().item()
        err = (got - ref).abs()
        rel = float((got - ref).norm() / ref.norm())
        msgs.append(f"{name} max {err.max().item() / scale:.2e} mean {err.mean().item() / scale:.2e} rel-L2 {rel:.2e}")
        assert err.max().item() < 1.5e-2 * scale and err.mean().item() < 1e-3 * scale and rel < 1e-2, (name, msgs[-1])
    print(f"\n[lsh attention at the bench shape, library's pick: forward runs of 4, backward runs of 8] o max {e_o:.2e}, out max {e_out:.2e} "
          f"of max|v|; " + "; ".join(msgs) + " (tol max 1.5e-2, mean 1e-3, rel-L2 1e-2)")


@pytest.mark.parametrize("walk", ["0", "4"])
@pytest.mark.parametrize("b,h,t,bs,nh,causal,masked", [CASES[0], CASES[2], CASES[5]])
def test_attention_probability_dropout_vs_oracle(ops, force_walk, b, h, t, bs, nh, causal, masked, walk):
    """The layer's `dropout` knob (reference reformer_tts/model/config.py:27): the chunk's softmax output
    is dropped before it meets the values, lse is that of the undropped probabilities.  The kernels draw the mask from a
    counter hash of (seed, pair index); the oracle gets the SAME mask as explicit keep-scales (oracle/synth.py rebuilds the
    hash in numpy), so forward and backward are compared like the dropout-free case: lse identical to the run without
    dropout, o / out / dqk / dv within the same bounds, and the mask really drops ~p of the pairs."""
    from oracle import synth
    from reformer_tts_amd._seeds import seed_base
    if (nh * (t // bs)) % max(int(walk), 1):
        pytest.skip("the run length does not divide this ring")
    force_walk(bwd=int(walk))
    p_drop, seed = 0.25, 0x1234567
    r = _run_fwd(ops, b, h, t, bs, nh, causal, masked, seed=9)
    dh = r["dh"]
    m_d = None if r["mask"] is None else r["mask"].cuda()
    o_d, lse_d = ops.lsh_attn_fwd(r["qk_d"], r["v_d"], r["st"], h, bs, causal, m_d, drop=(p_drop, seed))
    out_d, lse_tot_d = ops.lsh_combine_fwd(o_d, lse_d, b, h)
    torch.cuda.synchronize()
    assert torch.equal(lse_d, r["lse"]) and torch.equal(lse_tot_d, r["lse_tot"])          # dropout does not touch the normaliser
    eff_seed = (seed + int(seed_base(r["qk_d"].device).item())) & 0xFFFFFFFF
    keep = synth.attention_keep_scales(eff_seed, p_drop, b * h, nh * (t // bs), bs)
    assert abs(float((keep > 0).float().mean()) - (1 - p_drop)) < 2e-2
    qk = _heads_first(r["qkv"][..., :h * dh], b, t, h, dh).requires_grad_()
    v = _heads_first(r["qkv"][..., h * dh:], b, t, h, dh).requires_grad_()
    sticker, undo = _flat_perm(r["st"].cpu())
    m = None if r["mask"] is None else r["mask"].unsqueeze(1).expand(b, h, t).reshape(b * h, t)
    out_ref, o_ref, _ = lsh_ref.lsh_attention_sorted(qk, v, sticker, undo, bs, nh, causal, m, return_parts=True, keep=keep)
    vmax = v.abs().max().item()
    e_o = (o_d.float().cpu() - o_ref.detach()).abs().max().item() / vmax
    normal = torch.logsumexp(r["lse"].cpu(), dim=1) > -1e4
    e_out = (_heads_first(out_d, b, t, h, dh)[normal] - out_ref.detach()[normal]).abs().max().item() / vmax
    assert e_o < 1.6e-2 and e_out < 1.6e-2, (e_o, e_out)           # 1/(1-p) = 1.33 x the dropout-free bound
    # the mask did something: the dropped output differs from the plain one
    assert (o_d.float() - r["o"].float()).abs().max().item() > 0.05 * vmax
    g = torch.Generator().manual_seed(11)
    dout = torch.randn(b, t, h * dh, generator=g).bfloat16()
    dqk, dv = ops.lsh_attn_bwd(r["qk_d"], r["v_d"], r["st"], out_d, dout.cuda(), lse_tot_d, h, bs, causal, m_d, drop=(p_drop, seed))
    torch.cuda.synchronize()
    out_ref.backward(_heads_first(dout, b, t, h, dh))
    msgs = []
    for got, ref, name in ((_heads_first(dv, b, t, h, dh), v.grad, "dv"), (_heads_first(dqk, b, t, h, dh), qk.grad, "dqk")):
        scale = ref.abs().max().item()
        err = (got - ref).abs()
        rel = float((got - ref).norm() / ref.norm())
        msgs.append(f"{name} max {err.max().item() / scale:.2e} mean {err.mean().item() / scale:.2e} rel-L2 {rel:.2e}")
        assert err.max().item() < 2e-2 * scale and err.mean().item() < 1.4e-3 * scale and rel < 1.4e-2, (name, msgs[-1])
    print(f"\n[lsh attention with probability dropout {p_drop} B={b} H={h} T={t} bs={bs} R={nh} causal={causal} masked={masked} walk={walk}] "
          f"o max {e_o:.2e}, out max {e_out:.2e} of max|v|; " + "; ".join(msgs))


@pytest.mark.parametrize("drop", [None, (0.25, 77)])
@pytest.mark.parametrize("b,h,t,bs,nh,causal,masked", CASES)
def test_walking_forward_matches_the_one_chunk_kernel(ops, force_walk, b, h, t, bs, nh, causal, masked, drop):
    """lsh_attn_fwd as workgroups that walk a run of consecutive chunks (every K / V row gathered once, the next chunk's
    rows fetched while the current one is merged and stored) against the one-chunk kernel: the arithmetic of a chunk is the
    same instruction sequence in both, so o and lse must agree BIT FOR BIT for every run length that divides the ring --
    including runs that start at chunk 0 (the looked-back chunk wraps to the end of the ring), runs that cross a hash round,
    and dropout on the probabilities (same pair index)."""
    from reformer_tts_amd import _lib
    r = _run_fwd(ops, b, h, t, bs, nh, causal, masked, seed=3)
    m = None if r["mask"] is None else r["mask"].cuda()
    ring = nh * (t // bs)
    outs = {}
    for run in (0, 1, 2, 4, 8):
        if run and ring % run:
            continue
        force_walk(fwd=run)
        assert _lib.load().rtts_lsh_attn_fwd_run_length(b, h, t, nh, bs) == run
        o, lse = ops.lsh_attn_fwd(r["qk_d"], r["v_d"], r["st"], h, bs, causal, m, drop)
        torch.cuda.synchronize()
        outs[run] = (o.clone(), lse.clone())
    assert len(outs) >= 3
    for run, (o, lse) in outs.items():
        assert torch.equal(o, outs[0][0]), f"run length {run}: o differs from the one-chunk kernel"
        assert torch.equal(lse, outs[0][1]), f"run length {run}: lse differs from the one-chunk kernel"


@pytest.mark.parametrize("b,h,t,bs,nh,causal,masked", CASES)
def test_walking_backward_matches_the_one_chunk_kernel(ops, force_walk, b, h, t, bs, nh, causal, masked):
    """lsh_attn_bwd as workgroups that walk R consecutive chunks of a ring (operands of the next chunk prefetched by
    LDS-DMA, a chunk's keys worked by the same waves in their own and their looked-back step, every key row written
    once) against the one-chunk kernel: the same sums, with ONE bf16 rounding per key row where the one-chunk kernel
    rounds the own and the looked-back partial separately -- equal to a bf16 rounding of the partials, for every run
    length that divides the ring, including runs that cross a hash round and run length 1 (both slots everywhere)."""
    r = _run_fwd(ops, b, h, t, bs, nh, causal, masked, seed=5)
    dout = torch.randn(b, t, h * r["dh"], generator=torch.Generator().manual_seed(13)).bfloat16().cuda()
    m = None if r["mask"] is None else r["mask"].cuda()
    outs = {}
    ring = nh * (t // bs)
    for run in (0, 1, 2, 4, 8):
        if run and ring % run:
            continue
        force_walk(bwd=run)
        dqk, dv = ops.lsh_attn_bwd(r["qk_d"], r["v_d"], r["st"], r["out"], dout, r["lse_tot"], h, bs, causal, m)
        torch.cuda.synchronize()
        outs[run] = (dqk.float(), dv.float())
    assert len(outs) >= 3
    # (run length 1: every chunk is both ends of its run -- two partial rows per key like the one-chunk kernel, dV bit-identical;
    #  dK differs in the last fp32 bits: the projection sees k.(G + dQ) - k.dQ instead of k.G)
    assert torch.equal(outs[1][1], outs[0][1])
    worst = 0.0
    for run, (dqk, dv) in outs.items():
        for got, ref in ((dqk, outs[0][0]), (dv, outs[0][1])):
            scale = float(ref.abs().max())
            worst = max(worst, float((got - ref).abs().max()) / scale)
    print(f"\n[lsh walking backward B={b} H={h} T={t} bs={bs}] run lengths {sorted(outs)}: max |diff| / max|ref| vs the one-chunk kernel "
          f"{worst:.2e} (tol 1.2e-2: the two results differ by the bf16 roundings of their partial rows, <= 2^-8 of a row's value each)")
    assert worst < 1.2e-2


def test_strided_qkv_views(ops):
    """qk and v as the two halves of one (B,T,2d) buffer (row stride 2d) give the same result as
    separate contiguous tensors."""
    b, h, t, bs, nh, dh = 1, 2, 256, 64, 4, 64
    qkv = _make_qkv(b, t, h, dh, seed=5).cuda()
    rot = torch.randn(1, dh, nh, t // bs // 2, generator=torch.Generator().manual_seed(2)).cuda()
    qk_v, v_v = qkv[..., :h * dh], qkv[..., h * dh:]
    qk_c, v_c = qk_v.contiguous(), v_v.contiguous()
    st1, _, _ = ops.lsh_hash_sort(qk_v, rot, h, bs)
    st2, _, _ = ops.lsh_hash_sort(qk_c, rot, h, bs)
    assert torch.equal(st1, st2)
    o1, l1 = ops.lsh_attn_fwd(qk_v, v_v, st1, h, bs, True)
    o2, l2 = ops.lsh_attn_fwd(qk_c, v_c, st1, h, bs, True)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)


# ------------------------------------------------------------------ full-size properties
def test_full_size_properties(ops):
    """BASELINE config #2 decoder shape (B=12, H=8, T=1024, bucket 128, 8 rounds): size-independent
    properties -- st is a permutation of 0..T-1 per round, sorted by bucket; the attention of a
    constant V field returns the constant (softmax weights sum to one over rounds and keys);
    the backward of that field gives dqk == 0; linearity in v."""
    b, h, t, bs, nh, dh = 12, 8, 1024, 128, 8, 64
    qkv = _make_qkv(b, t, h, dh, seed=42).cuda()
    rot = torch.randn(1, dh, nh, t // bs // 2, generator=torch.Generator().manual_seed(9)).cuda()
    qk = qkv[..., :h * dh].contiguous()
    st, buckets, _ = ops.lsh_hash_sort(qk, rot, h, bs, want_buckets=True)
    assert torch.equal(st.sort(dim=-1).values, torch.arange(t, device="cuda", dtype=torch.int32).expand_as(st))
    sorted_b = buckets.gather(2, st.long())
    assert bool((sorted_b[..., 1:] >= sorted_b[..., :-1]).all())
    same = sorted_b[..., 1:] == sorted_b[..., :-1]
    assert bool((st[..., 1:][same] > st[..., :-1][same]).all())            # stable
    vconst = torch.full_like(qk, 0.75)
    o, lse = ops.lsh_attn_fwd(qk, vconst, st, h, bs, True)
    out, lse_tot = ops.lsh_combine_fwd(o, lse, b, h)
    assert bool(torch.isfinite(out.float()).all())
    torch.testing.assert_close(out.float(), torch.full_like(out, 0.75).float(), rtol=0, atol=8e-3)
    assert bool((lse_tot.unsqueeze(1) >= lse - 1e-3).all())
    v1, v2 = qkv[..., h * dh:].contiguous(), torch.flip(qkv[..., h * dh:], dims=[1]).contiguous()
    outs = []
    for vv in (v1, v2, (v1.float() + v2.float()).bfloat16()):
        o_, l_ = ops.lsh_attn_fwd(qk, vv, st, h, bs, True)
        outs.append(ops.lsh_combine_fwd(o_, l_, b, h)[0].float())
    torch.testing.assert_close(outs[2], outs[0] + outs[1], rtol=0, atol=6e-2)
    dout = torch.randn_like(out)
    dqk, dv = ops.lsh_attn_bwd(qk, vconst, st, out, dout, lse_tot, h, bs, True)
    assert dqk.float().abs().max().item() < 5e-2      # d(out)/d(qk) = 0 when V is constant
    torch.cuda.synchronize()


# ------------------------------------------------------------------ split-K weight-gradient GEMM
@pytest.mark.parametrize("m,n,k,acc", [(12288, 1024, 512, True), (3072, 512, 2048, True), (256, 128, 128, False), (1024, 2048, 512, True)])
def test_gemm_tn_vs_fp32_reference(ops, m, n, k, acc):
    """dW (+)= dY^T X against an fp32 matmul of the same bf16 values: only the accumulation order
    differs (fp32 partial tiles summed in a fixed order) => rel 1e-5-level agreement; bitwise
    reproducible run to run."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(m + n)
    a = torch.randn(m, n, generator=g).bfloat16().cuda()
    b = torch.randn(m, k, generator=g).bfloat16().cuda()
    c0 = torch.randn(n, k, generator=g).cuda()
    ws = torch.empty(16 * n * k, device="cuda")
    outs = []
    for _ in range(3):
        c = c0.clone()
        _lib.call("rtts_gemm_tn", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), m, n, k, c.data_ptr(), c.stride(0),
                  int(acc), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(c)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    ref = a.float().t() @ b.float() + (c0 if acc else 0)
    torch.testing.assert_close(outs[0], ref, rtol=2e-4, atol=2e-2)


def test_gemm_tn_grouped_matches_single_launches(ops):
    """The grouped launch (deferred weight gradients of a layer) against fp32 matmuls of the same bf16 values,
    different shapes and token counts in one grid, accumulate on and off; bitwise reproducible run to run."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(5)
    shapes = [(12288, 512, 512, 1), (12288, 1024, 512, 1), (3072, 1024, 512, 0), (12288, 2048, 512, 1), (12288, 512, 2048, 1),
              (256, 128, 128, 1), (1024, 512, 512, 0)]
    ops_ = []
    for m, n, k, acc in shapes:
        a = torch.randn(m, n, generator=g).bfloat16().cuda()
        b = torch.randn(m, k, generator=g).bfloat16().cuda()
        c0 = torch.randn(n, k, generator=g).cuda()
        ops_.append((a, b, c0, acc))
    ws = torch.empty(16 * 1024 * 1024, device="cuda")
    outs = []
    for _ in range(2):
        cs = [c0.clone() for _, _, c0, _ in ops_]
        arr = (_lib.GemmTnProblem * len(ops_))()
        for q, (a, b, _, acc), c in zip(arr, ops_, cs):
            q.a, q.lda, q.b, q.ldb, q.c, q.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0)
            q.M, q.N, q.K, q.accumulate = a.shape[0], a.shape[1], b.shape[1], acc
        _lib.call("rtts_gemm_tn_grouped", arr, len(ops_), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(cs)
    for (a, b, c0, acc), c1, c2 in zip(ops_, outs[0], outs[1]):
        assert torch.equal(c1, c2)
        ref = a.float().t() @ b.float() + (c0 if acc else 0)
        torch.testing.assert_close(c1, ref, rtol=2e-4, atol=2e-2)


def test_c_abi_rejects_bad_arguments_with_a_message(ops):
    """The C ABI validates shapes before it launches (a wrong shape must never reach a kernel): every rejection returns
    non-zero and leaves a message in rtts_last_error; the ctypes layer raises RttsError with it."""
    from reformer_tts_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    qk = torch.zeros(1, 256, 128, dtype=torch.bfloat16, device="cuda")
    rot = torch.zeros(1, 64, 2, 2, device="cuda")
    st = torch.zeros(2, 2, 256, dtype=torch.int32, device="cuda")
    # two weight gradients of one grouped launch that write the same C (buffers of the full size: refused before any launch)
    c_tn = torch.zeros(128, 128, device="cuda")
    twice = (_lib.GemmTnProblem * 2)()
    for e in twice:
        e.a, e.lda, e.b, e.ldb, e.c, e.ldc = qk.data_ptr(), 128, qk.data_ptr(), 128, c_tn.data_ptr(), 128
        e.M, e.N, e.K, e.accumulate = 256, 128, 128, 1
    # likewise two deferred column sums into one output, and two convolution weight-gradient re-layouts into one dw
    cs_twice = (_lib.ColsumJob * 2)()
    for j in cs_twice:
        j.partial, j.out, j.nrows, j.n, j.ld = c_tn.data_ptr(), c_tn.data_ptr() + 4 * 128 * 127, 8, 128, 0
    dwp, dw = torch.zeros(128, 5 * 128, device="cuda"), torch.zeros(128, 128, 5, device="cuda")
    cv_twice = (_lib.ConvPermJob * 2)()
    for j in cv_twice:
        j.w, j.wp, j.Co, j.Ci, j.CP = dwp.data_ptr(), dw.data_ptr(), 128, 128, 128
    cases = [
        # dh != 64
        (("rtts_lsh_hash_sort", qk.data_ptr(), 128, rot.data_ptr(), 1, 1, 4, 256, 32, 2, 64, None, st.data_ptr(), None, s), "dh=32 unsupported"),
        # T not divisible by 2 * bucket_size (the reference's assertion text)
        (("rtts_lsh_hash_sort", qk.data_ptr(), 128, rot.data_ptr(), 1, 1, 2, 192, 64, 2, 64, None, st.data_ptr(), None, s), "divisible by target bucket size"),
        # null output
        (("rtts_lsh_hash_sort", qk.data_ptr(), 128, rot.data_ptr(), 1, 1, 2, 256, 64, 2, 64, None, None, None, s), "null pointer"),
        # row stride not a multiple of 8
        (("rtts_lsh_hash_sort", qk.data_ptr(), 130, rot.data_ptr(), 1, 1, 2, 256, 64, 2, 64, None, st.data_ptr(), None, s), "ld_qk"),
        # unsupported bucket size in the attention kernels
        (("rtts_lsh_attn_fwd", qk.data_ptr(), qk.data_ptr(), 128, st.data_ptr(), None, 1, 2, 256, 64, 2, 32, 0, qk.data_ptr(), st.data_ptr(), 0.0, 0, None, s), "bucket_size=32"),
        # dropout probability out of range
        (("rtts_lsh_attn_fwd", qk.data_ptr(), qk.data_ptr(), 128, st.data_ptr(), None, 1, 2, 256, 64, 2, 64, 0, qk.data_ptr(), st.data_ptr(), 1.0, 0, None, s), "drop_p"),
        # weight-gradient GEMM: N not a multiple of 128
        (("rtts_gemm_tn", qk.data_ptr(), 96, qk.data_ptr(), 128, 256, 96, 128, st.data_ptr(), 128, 1, st.data_ptr(), 1 << 20, s), "128"),
        # grouped weight-gradient GEMM: two problems writing overlapping parts of C would race
        (("rtts_gemm_tn_grouped", twice, 2, None, 0, s), "overlapping"),
        (("rtts_colsum_final_grouped", cs_twice, 2, s), "overlapping"),
        (("rtts_conv_dw_unperm_grouped", cv_twice, 2, s), "overlapping"),
        # AdamW: n not a multiple of 4
        (("rtts_adamw_step", st.data_ptr(), st.data_ptr(), st.data_ptr(), st.data_ptr(), st.data_ptr(), 1022, None, st.data_ptr(), 0.9, 0.999, 1e-6,
          0.0, None, s), "multiple of 4"),
    ]
    for args, needle in cases:
        with pytest.raises(_lib.RttsError, match=needle):
            _lib.call(*args)
    torch.cuda.synchronize()
