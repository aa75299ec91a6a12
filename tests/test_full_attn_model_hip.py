"""Dense shared-QK attention above the kernels: the layer (``use_full_attn`` / ``full_attn_thres``) against float64 stage by stage,
against the LSH kernels where both compute the same function, the executor (engine.LSHExec) against the general path, across the
recompute modes and under graph replay, and the determinism an all-dense model offers."""
import numpy as np
import pytest
import torch

import full_attn_ref as R
from oracle import model_ref, synth

pytestmark = pytest.mark.gpu
U = R.U


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _layer(gpu, causal, seed=0, **kw):
    from reformer_tts_amd.model.reformer import LSHSelfAttentionWrapper
    torch.manual_seed(seed)
    lyr = LSHSelfAttentionWrapper(128, causal=causal, implementation="hip", heads=2, **kw).layer.to(gpu)
    with torch.no_grad():
        for p in lyr.parameters():                      # larger than the default init: logits of a few units, not ~0.1
            p.mul_(3.0)
    return lyr


def _heads(x2, nb, nh):
    """(B, T, H * 64) -> (B, H, T, 64) float64 on the CPU."""
    return x2.detach().double().cpu().view(nb, -1, nh, 64).transpose(1, 2)


def _within(tag, got, want, bound):
    err = (got.detach().double().cpu() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    print(f"[parity] {tag}: worst error / bound {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0, tag


@pytest.mark.parametrize("t", [128, 256])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_layer_against_float64_stage_by_stage(gpu, causal, t):
    """The layer is projection GEMM -> dense attention -> output GEMM.  ``forward`` must be bit-identical to that composition, and
    every stage of the composition is held to float64 evaluated at the stage's ACTUAL inputs: the GEMMs to one bf16 rounding of
    their exact result (u |.|, plus 2^-16 |a||w| for the fp32 accumulation), the attention to the kernel bounds of
    tests/full_attn_ref.py -- the kernel bounds carried through the two GEMMs one stage at a time, forward and backward."""
    from reformer_tts_amd.model.lsh_attention import _FullAttnFn, _project
    nb, nh, e = 2, 2, 128
    lyr = _layer(gpu, causal, use_full_attn=True)
    g = torch.Generator().manual_seed(t)
    x = torch.randn(nb, t, e, generator=g).bfloat16().float().to(gpu).requires_grad_(True)
    dy = torch.randn(nb, t, e, generator=g).bfloat16().float().to(gpu)
    mask = R.make_mask("ragged", nb, t)
    mask_d = mask.to(gpu)

    qkv = _project(x.to(torch.bfloat16).reshape(nb * t, e), None, lyr.toqk.weight, lyr.tov.weight).view(nb, t, 2 * e)
    qkv.retain_grad()
    out = _FullAttnFn.apply(qkv, mask_d.to(torch.uint8), nh, causal, None)
    out.retain_grad()
    y = _project(out.reshape(nb * t, e), lyr.to_out.bias, lyr.to_out.weight).view(nb, t, e).float()
    y.backward(dy)
    grads = {n: p.grad.clone() for n, p in lyr.named_parameters()}
    xg = x.grad.clone()
    x.grad = None
    lyr.zero_grad()
    y2 = lyr(x, input_mask=mask_d)
    y2.backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(y2, y) and torch.equal(x.grad, xg) and lyr.last_st is None
    for n, p in lyr.named_parameters():
        assert torch.equal(p.grad, grads[n]), n

    f64 = lambda z: z.detach().double().cpu()                                       # noqa: E731
    wqkv = torch.cat([f64(lyr.toqk.weight.bfloat16()), f64(lyr.tov.weight.bfloat16())])
    wo, bo = f64(lyr.to_out.weight.bfloat16()), f64(lyr.to_out.bias)
    xb, dyb = f64(x).view(nb * t, e), f64(dy).view(nb * t, e)
    acc = 2.0 ** -16
    want = xb @ wqkv.T
    _within("qkv", qkv.view(nb * t, 2 * e), want, U * want.abs() + acc * (xb.abs() @ wqkv.abs().T))
    qk_h, v_h = _heads(qkv[..., :e], nb, nh), _heads(qkv[..., e:], nb, nh)
    do_h = _heads(out.grad, nb, nh)
    ref = R.reference(qk_h, v_h, do_h, mask, causal)
    _within("out", _heads(out, nb, nh), ref["o"], ref["b_o"])
    _within("dqk", _heads(qkv.grad[..., :e], nb, nh), ref["dqk"], ref["b_dqk"])
    _within("dv", _heads(qkv.grad[..., e:], nb, nh), ref["dv"], ref["b_dv"])
    ob = f64(out).view(nb * t, e)
    want = ob @ wo.T + bo
    _within("y", y.view(nb * t, e), want, U * want.abs() + acc * (ob.abs() @ wo.abs().T + bo.abs()))
    want = dyb @ wo
    _within("dout", out.grad.view(nb * t, e), want, U * want.abs() + acc * (dyb.abs() @ wo.abs()))
    dq2 = f64(qkv.grad).view(nb * t, 2 * e)
    want = dq2 @ wqkv
    _within("dx", xg.view(nb * t, e), want, U * want.abs() + acc * (dq2.abs() @ wqkv.abs()))
    want = dq2.T @ xb
    _within("d toqk | tov", torch.cat([grads["toqk.weight"], grads["tov.weight"]]), want, acc * (dq2.abs().T @ xb.abs()))
    want = dyb.T @ ob
    _within("d to_out", grads["to_out.weight"], want, acc * (dyb.abs().T @ ob.abs()))


@pytest.mark.parametrize("t", [128, 256])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_dense_and_lsh_kernels_agree_where_they_compute_the_same(gpu, causal, t):
    """One hash round with buckets of T/2 shows every query all T keys: on the rows of valid queries the LSH kernels compute the
    dense function.  Both attention outputs sit within their own bound of float64 -- dense 2u P|V| (full_attn_ref.py), LSH 3u P|V|:
    P rounded before its P V MFMA, the round's o rounded on store, the combined out rounded on store (one round: weight 1) -- so
    they differ by at most the sum; the layer outputs by that sum carried through to_out plus their own roundings."""
    from reformer_tts_amd import ops
    nb, nh, e = 2, 2, 128
    dense = _layer(gpu, causal, use_full_attn=True)
    lsh = _layer(gpu, causal, bucket_size=t // 2, n_hashes=1, full_attn_thres=0)
    lsh.load_state_dict(dense.state_dict())
    x = torch.randn(nb, t, e, generator=torch.Generator().manual_seed(t + 1)).to(gpu)
    mask = R.make_mask("ragged", nb, t)
    mask_d = mask.to(gpu)
    with torch.no_grad():
        yd, yl = dense(x, input_mask=mask_d), lsh(x, input_mask=mask_d)
        assert dense.last_st is None and lsh.last_st is not None
        wqkv = torch.cat([dense.toqk.weight, dense.tov.weight]).bfloat16()
        qkv = (x.bfloat16().view(nb * t, e) @ wqkv.T).view(nb, t, 2 * e)
        od, _ = ops.full_attn_fwd(qkv[..., :e], qkv[..., e:], nh, causal, mask_d)
        o, lse = ops.lsh_attn_fwd(qkv[..., :e], qkv[..., e:], lsh.last_st, nh, t // 2, causal, mask_d)
        ol, _ = ops.lsh_combine_fwd(o, lse, nb, nh)
    torch.cuda.synchronize()
    ref = R.reference(_heads(qkv[..., :e], nb, nh), _heads(qkv[..., e:], nb, nh), torch.zeros(nb, nh, t, 64), mask, causal)
    pv = ref["b_o"] / (2 * U)
    sel = mask[:, None, :, None].expand(nb, nh, t, 64)
    err = (_heads(od, nb, nh) - _heads(ol, nb, nh)).abs()
    ratio = (err / (5 * U * pv))[sel]
    print(f"[parity] dense vs LSH attention output, valid rows: worst difference / (2u + 3u) P|V| {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0
    # masked queries: the dense rows are mean(v), the LSH rows v_i
    inv = ~sel
    v_h = _heads(qkv[..., e:], nb, nh)
    assert float((_heads(ol, nb, nh) - v_h)[inv].abs().max()) <= 3 * U * float(v_h.abs().max())
    assert float((_heads(od, nb, nh) - v_h.mean(2, keepdim=True).expand_as(v_h))[inv].abs().max()) <= 2 * U * float(v_h.abs().mean(2).max())
    wo = dense.to_out.weight.detach().bfloat16().double().cpu()
    b_y = (5 * U * pv).transpose(1, 2).reshape(nb * t, e) @ wo.abs().T + 2 * U * yd.double().cpu().abs().view(nb * t, e) + 1e-6
    err_y = (yd - yl).double().cpu().abs().view(nb * t, e)
    rows = mask.reshape(-1)
    assert float((err_y / b_y)[rows].max()) <= 1.0


def test_threshold_picks_the_branch_per_call(gpu):
    """full_attn_thres = 256: T = 256 runs dense (bit-identical to a use_full_attn layer, no permutation, the default generator
    untouched), T = 512 runs LSH (with forced rotations bit-identical to a layer without the threshold)."""
    kw = dict(bucket_size=64, n_hashes=4)
    thr = _layer(gpu, True, full_attn_thres=256, **kw)
    full = _layer(gpu, True, use_full_attn=True, **kw)
    plain = _layer(gpu, True, **kw)
    for other in (full, plain):
        other.load_state_dict(thr.state_dict())
    rot = torch.randn(1, 64, 4, 4, generator=torch.Generator().manual_seed(9))
    thr.forced_rotations, plain.forced_rotations = rot, rot
    g = torch.Generator().manual_seed(4)
    outs = {}
    for t in (256, 512):
        x = torch.randn(2, t, 128, generator=g).to(gpu)
        mask = R.make_mask("ragged", 2, t).to(gpu)
        other = full if t == 256 else plain
        res = []
        for lyr in (thr, other):
            xi = x.clone().requires_grad_(True)
            before = torch.cuda.get_rng_state(gpu)
            y = lyr(xi, input_mask=mask)
            if t == 256:
                assert torch.equal(torch.cuda.get_rng_state(gpu), before) and lyr.last_st is None
            else:
                assert lyr.last_st is not None
            y.square().sum().backward()
            res.append((y.detach(), xi.grad.clone(), lyr.toqk.weight.grad.clone()))
            lyr.zero_grad()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(*res)), t
        outs[t] = res[0][0]
    assert all(torch.isfinite(o).all() for o in outs.values())
    with pytest.raises(NotImplementedError, match="4096"):
        full(torch.zeros(1, 96, 128, device=gpu))


def _dense_cfg(which):
    cfg = model_ref.small_cfg()
    cfg["enc_reformer_kwargs"]["attn_kwargs"]["implementation"] = "hip"
    cfg["dec_reformer_kwargs"]["self_attn_kwargs"]["implementation"] = "hip"
    cfg["enc_reformer_kwargs"]["attn_kwargs"]["use_full_attn"] = True
    if which == "both":
        cfg["dec_reformer_kwargs"]["self_attn_kwargs"]["use_full_attn"] = True
    return cfg


def _fix_rotations(model):
    from reformer_tts_amd.model.lsh_attention import LSHSelfAttention
    for m in model.modules():
        if isinstance(m, LSHSelfAttention):
            m.forced_rotations = {nb: torch.randn(1, 64, 4, nb // 2, generator=torch.Generator().manual_seed(3)) for nb in (2, 4, 6, 8)}


@pytest.mark.parametrize("which", ["encoder", "both"])
def test_executor_matches_general_path(gpu, which):
    """tests/test_model_hip.py::test_fused_engine_matches_general_path with dense layers: same kernels for the attention cores,
    fusion differs around them => outputs within 2e-2, every gradient within 6e-2 (rel-L2), that test's tolerances."""
    from reformer_tts_amd.model import TTSLoss
    from reformer_tts_amd.model.config import model_config_from_dict
    from reformer_tts_amd.training import build_model
    cfg = _dense_cfg(which)
    cfg["enc_reformer_kwargs"]["depth"] = 2
    cfg["dec_reformer_kwargs"]["depth"] = 2
    batch = {k: v.to(gpu) for k, v in model_ref.synthetic_batch(2, 60, 200, ragged=True, seed=2).items()}
    results = []
    for fused in (True, False):
        model = build_model(model_config_from_dict(cfg), gpu)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict(synth.synth_state_dict(shapes, seed=5), strict=False)
        model.train()
        model.enc.reformer.layers.use_fused = fused
        model.dec.reformer.layers.use_fused = fused
        _fix_rotations(model)
        spec = batch["spectrogram"]
        raw, post, stop, _ = model(batch["phonemes"], spec[:, :-1], spectrogram_mask=batch["loss_mask"].mean(-1))
        res = TTSLoss(torch.tensor(5.0))(raw, post, stop.view(stop.shape[0], -1), spec[:, 1:], batch["stop_tokens"], batch["loss_mask"])
        res[0].backward()
        torch.cuda.synchronize()
        assert (model.enc.reformer.layers._program is not None) == fused
        results.append((raw.detach().float(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}))
    (raw_f, g_f), (raw_g, g_g) = results
    assert ((raw_f - raw_g).norm() / raw_g.norm()).item() < 2e-2
    worst = ("", 0.0)
    for n in g_g:
        if g_g[n].norm().item() < 1e-3:
            continue
        rel = ((g_f[n] - g_g[n]).norm() / g_g[n].norm()).item()
        if rel > worst[1]:
            worst = (n, rel)
    print(f"[parity] executor vs general path, dense on {which}: worst gradient rel-L2 {worst}")
    assert worst[1] < 6e-2, worst


@pytest.mark.parametrize("which,attn_dropout", [("encoder", 0.0), ("both", 0.2)])
def test_recompute_modes_agree(gpu, which, attn_dropout):
    """``recompute: full`` (the reference's pure recompute from the reconstructed stream) against ``stash``: gradients within 1e-2
    (tests/test_model_hip.py::test_attention_stash_matches_pure_recompute's tolerance), probability dropout included -- the dense
    recompute must redraw the forward's mask."""
    from reformer_tts_amd import _seeds, engine
    from reformer_tts_amd.model.config import TTSTrainingConfig, model_config_from_dict
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    cfg = _dense_cfg(which)
    cfg["enc_reformer_kwargs"]["attn_kwargs"]["dropout"] = attn_dropout
    cfg["dec_reformer_kwargs"]["self_attn_kwargs"]["dropout"] = attn_dropout
    batch = synthetic_batch(2, 100, 256, device=gpu)
    grads = {}
    before = engine.recompute_mode()
    try:
        for mode in ("stash", "full"):
            _seeds.reset()
            torch.manual_seed(1)
            model = build_model(model_config_from_dict(cfg), gpu)
            _fix_rotations(model)
            tr = Trainer(model, TTSTrainingConfig(batch_size=2, recompute=mode), gpu)
            model.train()
            tr.zero_grad()
            tr.forward_loss(batch)[0].backward()
            torch.cuda.synchronize()
            grads[mode] = tr.flat_g.clone()
    finally:
        engine.set_recompute(before)
    err = ((grads["stash"] - grads["full"]).norm() / grads["full"].norm()).item()
    print(f"[parity] dense on {which}, dropout {attn_dropout}: stash vs full recompute, relative gradient distance {err:.2e} (tol 1e-2)")
    assert torch.isfinite(grads["full"]).all() and err < 1e-2


@pytest.mark.parametrize("which,segmented", [("encoder", False), ("both", False), ("both", True)])
def test_graph_replay_matches_eager_steps(gpu, which, segmented):
    """tests/test_model_hip.py::test_graph_replay_matches_eager_steps with dense layers (the rotation pool serves layers that
    draw nothing): the replayed losses follow the eager trajectory to 2e-2."""
    from reformer_tts_amd.model.config import TTSTrainingConfig, model_config_from_dict
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    cfg = _dense_cfg(which)
    batch = synthetic_batch(2, 100, 256, device=gpu)
    traj = []
    for graph in (False, True):
        torch.manual_seed(1)
        model = build_model(model_config_from_dict(cfg), gpu)
        _fix_rotations(model)
        tr = Trainer(model, TTSTrainingConfig(batch_size=2, learning_rate=1e-3, warmup_steps=4, gradient_clip_val=1.0), gpu)
        if graph:
            tr.capture(batch, segmented=segmented)
            losses = [None, None] + [float(tr.replay()[0]) for _ in range(4)]
        else:
            losses = [float(tr.train_step(batch)[0]) for _ in range(6)]
        traj.append(losses)
    np.testing.assert_allclose(traj[1][2:], traj[0][2:], rtol=2e-2)
    assert traj[1][-1] < traj[1][2]


def test_all_dense_generation_is_deterministic(gpu):
    """With every LSH layer dense nothing is drawn: two graphed generations are bit-identical (the LSH mode draws new rotations
    per call and cannot offer that), and the eager loop gives the same frames as the graphed one up to its fusion."""
    from reformer_tts_amd.model.config import model_config_from_dict
    from reformer_tts_amd.training import build_model
    model = build_model(model_config_from_dict(_dense_cfg("both")), gpu)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if "running" not in k and "num_batches" not in k}
    model.load_state_dict(synth.synth_state_dict(shapes, seed=5), strict=False)       # BatchNorm keeps its initial running statistics
    ph =model_ref.synthetic_batch(2, 60, 200, ragged=True, seed=2)["phonemes"]
    kw = dict(max_len=90, stop_at_stop_token=False)       # (max_len < n_mels = 80 ends after one forward, as in the reference)
    a = model.infer(ph, use_graph=True, **kw)
    b = model.infer(ph, use_graph=True, **kw)
    c = model.infer(ph, use_graph=False, **kw)
    d = model.infer(ph, use_graph=False, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(a[0]).all() and a[0].shape == (2, 80, 90)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(c[0], d[0])
    assert float((a[0] - c[0]).abs().max()) < 2e-2 * float(c[0].abs().max())
