"""Guided attention loss where it trains: the cross-attention executor's backward with a guide context against float64 autograd,
and ``Trainer`` with ``guided_attention_weight`` -- eager steps, accumulation, ``capture`` / ``replay`` -- on the smallest model
the executors take (oracle.model_ref.small_cfg: width 128, 2 heads of 64, 1 + 1 layers; T_q 128, T_k 128, B 2, sample 1 ragged:
90 frames, 70 phonemes).  The kernels themselves are held to float64 bounds in tests/test_xattn_guide_hip.py."""
import copy
import types
from dataclasses import asdict

import numpy as np
import pytest
import torch

from oracle import model_ref

pytestmark = pytest.mark.gpu

T_B, K_B = (128, 90), (100, 70)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _cfg(num_heads=2):
    from reformer_tts_amd.model.config import model_config_from_dict
    cfg = model_ref.small_cfg()
    cfg["enc_reformer_kwargs"]["attn_kwargs"]["implementation"] = "hip"
    cfg["dec_reformer_kwargs"]["self_attn_kwargs"]["implementation"] = "hip"
    cfg["dec_reformer_kwargs"]["attn_kwargs"]["num_heads"] = num_heads
    return model_config_from_dict(cfg)


def _batch(gpu):
    from reformer_tts_amd.training import synthetic_batch
    batch = synthetic_batch(2, 100, 128, device=gpu)
    batch["phonemes"][1, K_B[1]:] = 0
    batch["loss_mask"][1, T_B[1]:] = 0
    batch["stop_tokens"][1] = 0
    batch["stop_tokens"][1, T_B[1] - 1] = 1
    return batch


def _trainer(gpu, **train_kw):
    """A fresh small model (same seed, same forced rotations every time) and its trainer."""
    from reformer_tts_amd import _seeds
    from reformer_tts_amd.model.config import TTSTrainingConfig
    from reformer_tts_amd.model.lsh_attention import LSHSelfAttention
    from reformer_tts_amd.training import Trainer, build_model
    _seeds.reset()
    torch.manual_seed(1)
    model = build_model(_cfg(), gpu)
    for m in model.modules():
        if isinstance(m, LSHSelfAttention):
            m.forced_rotations = torch.randn(1, 64, 4, 1, generator=torch.Generator().manual_seed(5))
    strip = train_kw.pop("strip_new_fields", False)
    cfg = TTSTrainingConfig(**dict(dict(batch_size=2, learning_rate=1e-3, warmup_steps=None), **train_kw))
    if strip:            # a configuration object from before the guided fields existed
        cfg = types.SimpleNamespace(**{k: v for k, v in asdict(cfg).items() if not k.startswith("guided_attention")})
    return Trainer(model, cfg, gpu)


def _census(monkeypatch):
    from reformer_tts_amd import _lib
    seen = {}
    real = _lib.call

    def counting(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    return seen


NEW_ENTRIES = ("rtts_xattn_guide_rows", "rtts_xattn_guide_fold", "rtts_xattn_bwd_guided")


@pytest.mark.parametrize("mode", ["full", "stash"])
def test_executor_backward_against_float64_autograd(gpu, mode):
    """XAttnExec forward + backward with a guide context against WithNorm(LayerNorm, nn.MultiheadAttention) in float64 with the
    guided loss through autograd (need_weights, dropout 0): d_inp, dkeys and the in_proj gradients, to the 2e-2 relative L2 of
    test_cross_attention_key_chunks_vs_autograd."""
    import xattn_guide_ref as G
    from reformer_tts_amd import engine
    from reformer_tts_amd.model.reformer import MultiheadAttentionWrapper, WithNorm
    b, t, tk, d, h = 2, 128, 128, 128, 2
    torch.manual_seed(3)
    withnorm = WithNorm(torch.nn.LayerNorm, d, MultiheadAttentionWrapper(d, None, num_heads=h, dropout=0.0)).to(gpu).train()
    with torch.no_grad():
        withnorm.norm.weight.add_(0.1 * torch.randn(d, device=gpu))
        withnorm.norm.bias.add_(0.1 * torch.randn(d, device=gpu))
        withnorm.fn.layer.in_proj_bias.add_(0.1 * torch.randn(3 * d, device=gpu))
        withnorm.fn.layer.in_proj_weight.mul_(3.0)               # logits of order 1: a softmax that is not flat
    g = torch.Generator().manual_seed(4)
    inp = torch.randn(b * t, d, generator=g).to(gpu)
    acc = torch.randn(b * t, d, generator=g).to(gpu)
    keys = torch.randn(b * tk, d, generator=g).bfloat16().to(gpu)
    d_acc = torch.randn(b * t, d, generator=g).to(gpu)
    valid = torch.ones(b, tk, dtype=torch.bool, device=gpu)
    valid[1, K_B[1]:] = False
    nf = torch.tensor(T_B, dtype=torch.int32, device=gpu)
    nk = torch.tensor(K_B, dtype=torch.int32, device=gpu)
    sigma, coef = 0.2, 32.0 * h * sum(T_B)
    out = torch.zeros(1, b + 1, dtype=torch.float64, device=gpu)
    guide = dict(n_frames=nf, n_keys=nk, sigma=sigma, coef=coef, scale=None, layers=[0], out=out)

    ex = engine.XAttnExec(withnorm)
    old = engine.set_recompute(mode)
    try:
        acc_run, d_inp = acc.clone(), torch.zeros_like(inp)
        dkeys = torch.zeros(b * tk, d, device=gpu)
        with torch.no_grad():
            ex.forward(acc_run, inp, b, t, keys_bf16=keys, kvalid=valid.view(torch.uint8))
            ex.backward(acc_run, inp, d_acc, d_inp, b, t, keys_bf16=keys, kvalid=valid.view(torch.uint8), dkeys=dkeys, guide=guide, guide_slot=0)
            engine.flush_wgrad()
        torch.cuda.synchronize()
    finally:
        engine.set_recompute(old)

    ref = copy.deepcopy(withnorm).double()
    for p in ref.parameters():
        p.grad = None
    x = inp.double().requires_grad_(True)
    kk = keys.double().requires_grad_(True)
    y = ref.norm(x).view(b, t, d).transpose(0, 1)
    kseq = kk.view(b, tk, d).transpose(0, 1)
    o, w = ref.fn.layer(y, kseq, kseq, key_padding_mask=~valid, need_weights=True, average_attn_weights=False)
    wts = G.weights(T_B, K_B, t, tk, sigma).to(gpu).view(b, 1, t, tk)
    loss = (w * wts).sum() / (h * sum(T_B))
    ((o.transpose(0, 1).reshape(b * t, d) * d_acc.double()).sum() + coef * loss).backward()
    # the guided term must matter in every compared gradient: the same autograd without it
    plain = copy.deepcopy(withnorm).double()
    x0, k0 = inp.double().requires_grad_(True), keys.double().requires_grad_(True)
    k0s = k0.view(b, tk, d).transpose(0, 1)
    o0, _ = plain.fn.layer(plain.norm(x0).view(b, t, d).transpose(0, 1), k0s, k0s, key_padding_mask=~valid, need_weights=False)
    (o0.transpose(0, 1).reshape(b * t, d) * d_acc.double()).sum().backward()

    m, mr, m0 = withnorm.fn.layer, ref.fn.layer, plain.fn.layer
    rel = lambda a, r: float((a.double() - r).norm() / r.norm())
    pairs = dict(d_inp=(d_inp, x.grad, x0.grad), dkeys=(dkeys, kk.grad, k0.grad),
                 in_proj_weight=(m.in_proj_weight.grad, mr.in_proj_weight.grad, m0.in_proj_weight.grad),
                 in_proj_bias=(m.in_proj_bias.grad[:2 * d], mr.in_proj_bias.grad[:2 * d], m0.in_proj_bias.grad[:2 * d]))
    errs = {n: rel(got, want) for n, (got, want, _) in pairs.items()}
    gaps = {n: rel(without, want) for n, (_, want, without) in pairs.items()}
    print(f"\n[parity] XAttnExec with a guide context, recompute {mode}: rel-L2 " + ", ".join(f"{n} {v:.2e}" for n, v in errs.items())
          + " (tol 2e-2); without the guided term: " + ", ".join(f"{n} {v:.2f}" for n, v in gaps.items())
          + f"; loss {float(out[0, -1]):.6f} (float64 {float(loss.detach()):.6f})")
    assert max(errs.values()) < 2e-2, errs
    assert min(gaps.values()) > 0.2, gaps
    assert abs(float(out[0, -1]) - float(loss.detach())) < 2e-2 * float(loss.detach())
    torch.testing.assert_close(acc_run, acc, rtol=0, atol=1e-5)          # the stream is reconstructed


def test_weight_zero_changes_nothing(gpu, monkeypatch):
    """flat_g after a step is bit-equal to a trainer whose configuration has no guided fields, and none of the new entries runs."""
    batch = _batch(gpu)
    seen = _census(monkeypatch)
    a = _trainer(gpu, strip_new_fields=True)
    a.train_step(batch)
    b = _trainer(gpu, guided_attention_weight=0.0, guided_attention_sigma=0.3, guided_attention_layers=[0])
    b.train_step(batch)
    torch.cuda.synchronize()
    assert torch.equal(a.flat_g, b.flat_g) and torch.equal(a.flat_p, b.flat_p)
    assert seen.get("rtts_xattn_bwd", 0) == 2 and not any(n in seen for n in NEW_ENTRIES), seen
    assert b.last_guided_attention is None and b.guided_attention_loss() is None


def test_the_guided_gradient_alone_lowers_the_guided_loss(gpu, monkeypatch):
    """Every other loss weight 0: only the guided gradient flows.  20 AdamW steps on one batch."""
    batch = _batch(gpu)
    seen = _census(monkeypatch)
    tr = _trainer(gpu, guided_attention_weight=1.0, raw_pred_loss_weight=0.0, post_pred_loss_weight=0.0, stop_loss_weight=0.0,
                  learning_rate=2e-2)
    track = []
    for _ in range(20):
        tr.train_step(batch)
        track.append(tr.guided_attention_loss())
    track = [float(x) for x in torch.stack(track).cpu()]
    print(f"\n[guided] guided_attention_loss over 20 steps: {track[0]:.4f} -> {track[-1]:.4f} (must end below {0.9 * track[0]:.4f})")
    assert tr.last_guided_attention.shape == (1, 3) and tr.last_guided_attention.dtype == torch.float64 and tr.last_guided_attention.is_cuda
    assert all(seen.get(n, 0) == 20 for n in NEW_ENTRIES) and "rtts_xattn_bwd" not in seen, seen
    assert 0.0 < track[0] <= 1.0 and track[-1] < 0.9 * track[0]


def test_accumulation_scales_the_guided_term(gpu):
    """train_accumulated([batch, batch]) with the rotations forced and every dropout 0 is train_step(batch): each micro-batch
    carries weight / 2 into the kernels."""
    batch = _batch(gpu)
    one = _trainer(gpu, guided_attention_weight=4.0)
    one.train_step(batch)
    two = _trainer(gpu, guided_attention_weight=4.0)
    two.train_accumulated([batch, batch])
    off = _trainer(gpu)
    off.train_step(batch)
    torch.cuda.synchronize()
    torch.testing.assert_close(two.flat_g, one.flat_g, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(two.last_guided_attention, one.last_guided_attention, rtol=1e-12, atol=0)
    assert float((one.flat_g - off.flat_g).norm() / off.flat_g.norm()) > 1e-2          # the term is there to be scaled


@pytest.mark.parametrize("segmented", [False, True])
def test_graph_replay_matches_eager_steps_with_the_guided_term(gpu, segmented):
    """capture + replay at weight > 0 follows the eager steps (the tolerance of test_graph_replay_matches_eager_steps), the
    guided loss included."""
    batch = _batch(gpu)
    traj = []
    for graph in (False, True):
        tr = _trainer(gpu, guided_attention_weight=2.0, warmup_steps=4, gradient_clip_val=1.0)
        steps = []
        if graph:
            tr.capture(batch, segmented=segmented)       # 2 eager warm-up steps
            for _ in range(4):
                total = tr.replay()[0]
                steps.append((float(total), float(tr.guided_attention_loss())))
        else:
            for i in range(6):
                total = tr.train_step(batch)[0]
                if i >= 2:
                    steps.append((float(total), float(tr.guided_attention_loss())))
        traj.append(steps)
    print(f"\n[guided] eager (loss, guided) {traj[0]}\n         replay {traj[1]}")
    np.testing.assert_allclose(traj[1], traj[0], rtol=2e-2)
    assert traj[1][-1][1] < traj[1][0][1]


def test_the_logged_loss_is_the_guided_score_of_the_same_matrices(gpu, monkeypatch):
    """last_guided_attention[:, B] = the frame-weighted ``guided`` sum of ops.alignment_stats over rtts_xattn_probs_mean of the
    same layer call's q, kv and lse, to 1e-5."""
    from reformer_tts_amd import engine, ops
    batch = _batch(gpu)
    tr = _trainer(gpu, guided_attention_weight=1.0, guided_attention_sigma=0.25)
    calls = []
    real = engine.XAttnExec._internals

    def recording(self, *args, **kw):
        res = real(self, *args, **kw)
        calls.append((res, args, kw))
        return res
    monkeypatch.setattr(engine.XAttnExec, "_internals", recording)
    tr.model.train()
    tr.zero_grad()
    tr.backward(tr.forward_loss(batch)[0])
    (xn, mean, rstd, w, q, kv, o, lse, g, tk), args, kw = calls[-1]          # the backward's call
    kvalid = args[4] if len(args) > 4 else kw.get("kvalid")
    b, h, t = 2, 2, 128
    mat = engine.xattn_probs_mean(q, kv, kvalid, lse, b, h, t, tk)
    nf = torch.tensor(T_B, dtype=torch.int32, device=gpu)
    nk = torch.tensor(K_B, dtype=torch.int32, device=gpu)
    table = ops.alignment_stats([mat], nf, nk, sigma=0.25)[2]
    want = table[0, :b, 5] / nf.double()
    got = tr.last_guided_attention[0]
    print(f"\n[guided] per-utterance mass {got[:b].tolist()} loss {float(got[b]):.8f}; alignment_stats {want.tolist()} "
          f"{float(table[0, :b, 5].sum() / sum(T_B)):.8f}")
    torch.testing.assert_close(got[:b], want, rtol=1e-5, atol=0)
    assert abs(float(got[b]) - float(table[0, :b, 5].sum()) / sum(T_B)) <= 1e-5 * float(got[b])


def test_a_cross_attention_outside_the_executor_is_refused(gpu):
    from reformer_tts_amd.model.config import TTSTrainingConfig
    from reformer_tts_amd.training import Trainer, build_model
    model = build_model(_cfg(num_heads=4), gpu)                      # heads of 32
    with pytest.raises(NotImplementedError, match="decoder layer 0's cross-attention"):
        Trainer(model, TTSTrainingConfig(batch_size=2, guided_attention_weight=1.0), gpu)
    Trainer(model, TTSTrainingConfig(batch_size=2), gpu)             # without the term the model trains as before
