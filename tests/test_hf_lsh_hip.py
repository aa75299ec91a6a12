"""GPU tests of ``implementation="huggingface_transformers"``: the hash / sort kernel against its numpy twin (bit for bit),
the layer against goldens produced by ``transformers``' own LSHSelfAttention (tests/golden/hf_lsh_attn.npz), and the fused
executor / captured step with the layer inside a model."""
import os

import numpy as np
import pytest
import torch

import hf_lsh_ref as ref
from oracle import model_ref, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "hf_lsh_attn.npz"))


# ------------------------------------------------------------------ (a) hash + sort: bit-exact against the twin
HASH_SHAPES = [
    # b, h, t, chunk, n_hashes, n_buckets
    (2, 2, 256, 64, 4, 8), (1, 2, 512, 64, 4, 16), (1, 2, 1024, 128, 2, 16), (1, 2, 384, 64, 2, 8),      # the fixture's shapes
    (1, 2, 4096, 64, 8, 128),            # 128 (+ 1) buckets: four column passes per round, 129 bins in 192-word counter rows
    (1, 1, 2048, 64, 2, 256),            # the count forced to the kernel's limit: 256 (+ 1) bins in 320-word rows
]


def _hash_inputs(b, h, t, r, nb, mode):
    g = torch.Generator().manual_seed(t + nb + r)
    qk = torch.randn(b, t, h * 64, generator=g).bfloat16()
    rot = torch.randn(h, 64, r, nb // 2, generator=g)
    mask = None
    if mode == "masked":
        mask = torch.ones(b, t, dtype=torch.bool)
        mask[0, t - t // 3:] = False
        mask[0, 5] = False                       # a hole inside the valid part, too
        if b > 1:
            mask[1, t // 2:] = False
    elif mode == "all_valid":
        mask = torch.ones(b, t, dtype=torch.bool)
    return qk, rot, mask


def _check_hash(gpu, b, h, t, chunk, r, nb, mode):
    from reformer_tts_amd import ops
    qk, rot, mask = _hash_inputs(b, h, t, r, nb, mode)
    st, buckets, undo = ops.lsh_hash_sort_hf(qk.to(gpu), rot.to(gpu), h, chunk, nb, None if mask is None else mask.to(gpu),
                                             want_buckets=True, want_undo=True)
    torch.cuda.synchronize()
    m = None if mask is None else mask.numpy()
    exp_b = ref.hash_buckets(ref.heads_first(qk.float().numpy(), h), rot.numpy(), m, nb)
    exp_st, exp_undo = ref.sort_buckets(exp_b, nb + (mask is not None))
    assert np.array_equal(buckets.cpu().numpy(), exp_b)
    assert np.array_equal(st.cpu().numpy(), exp_st)
    assert np.array_equal(undo.cpu().numpy(), exp_undo)
    if mode == "masked":
        assert int(exp_b.max()) == (r - 1) * (nb + 1) + nb           # the padding bucket of the last round is in use


@pytest.mark.parametrize("mode", ["none", "masked"])
@pytest.mark.parametrize("b,h,t,chunk,r,nb", HASH_SHAPES)
def test_hash_sort_hf_bit_exact(gpu, b, h, t, chunk, r, nb, mode):
    _check_hash(gpu, b, h, t, chunk, r, nb, mode)


@pytest.mark.parametrize("nb,r", [(2, 3), (4, 5), (6, 3), (12, 3), (32, 3), (48, 2), (64, 3), (96, 2), (130, 1), (254, 2)])
def test_hash_sort_hf_every_column_capacity(gpu, nb, r):
    """Bucket counts the layer would not pick by itself (the count is the caller's): every compile-time column capacity of the
    hash kernel (1 .. 128 columns per round), counts that are no power of two (zero-padded columns the argmax must ignore),
    round counts that do not fill the last pass, and every counter-row length of the sort."""
    _check_hash(gpu, 1, 2, 256, 64, r, nb, "masked")
    _check_hash(gpu, 1, 2, 256, 64, r, nb, "none")


def test_hash_sort_hf_with_a_mask_that_hides_nothing(gpu):
    """The offsets take the stride n_buckets + 1 whenever a mask is given: same sorted order, empty padding bucket."""
    _check_hash(gpu, 2, 2, 256, 64, 4, 8, "all_valid")
    from reformer_tts_amd import ops
    qk, rot, mask = _hash_inputs(2, 2, 256, 4, 8, "all_valid")
    st_m, b_m, _ = ops.lsh_hash_sort_hf(qk.to(gpu), rot.to(gpu), 2, 64, 8, mask.to(gpu), want_buckets=True)
    st_n, b_n, _ = ops.lsh_hash_sort_hf(qk.to(gpu), rot.to(gpu), 2, 64, 8, None, want_buckets=True)
    assert torch.equal(st_m, st_n)
    assert torch.equal(b_m - b_n, torch.arange(4, device=gpu, dtype=torch.int32).view(1, 4, 1).expand_as(b_m))


# ------------------------------------------------------------------ (b) bad arguments
def test_hash_sort_hf_rejects_bad_arguments(gpu):
    from reformer_tts_amd import _lib, ops
    qk = torch.zeros(1, 256, 128, dtype=torch.bfloat16, device=gpu)

    def rot(h, dh, half):
        return torch.zeros(h, dh, 2, half, device=gpu)
    with pytest.raises(_lib.RttsError, match=r"n_buckets=7 unsupported \(even, 2 \.\. 256\)"):
        ops.lsh_hash_sort_hf(qk, rot(2, 64, 3), 2, 64, 7)
    with pytest.raises(_lib.RttsError, match=r"n_buckets=258 unsupported \(even, 2 \.\. 256\)"):
        ops.lsh_hash_sort_hf(qk, rot(2, 64, 129), 2, 64, 258)
    with pytest.raises(_lib.RttsError, match=r"sequence length \(256\) must be a multiple of the chunk length \(96\)"):
        ops.lsh_hash_sort_hf(qk, rot(2, 64, 4), 2, 96, 8)
    with pytest.raises(_lib.RttsError, match=r"dh=32 unsupported"):
        ops.lsh_hash_sort_hf(qk, rot(4, 32, 4), 4, 64, 8)


# ------------------------------------------------------------------ (c), (d) the layer against HuggingFace's goldens
def _meta(z, tag):
    b, h, t, chunk, r, causal, nb, seed = (int(v) for v in z[f"{tag}/meta"])
    return b, h, t, chunk, r, bool(causal), nb, seed


def _layer(gpu, z, tag):
    from reformer_tts_amd.model.hf_lsh_attention import HFLSHSelfAttention
    b, h, t, chunk, r, causal, nb, seed = _meta(z, tag)
    inp = ref.case_inputs(tag)
    lyr = HFLSHSelfAttention(h * 64, heads=h, bucket_size=chunk, n_hashes=r, causal=causal, dropout=0.0).to(gpu)
    lyr.load_state_dict({"query_key.weight": torch.from_numpy(inp["wqk"]), "value.weight": torch.from_numpy(inp["wv"])})
    lyr.train()
    return lyr, inp


def _run_layer(gpu, lyr, inp, backward=True):
    for p in lyr.parameters():
        p.grad = None
    x = torch.from_numpy(inp["x"]).to(gpu).requires_grad_()
    mask = None if inp["mask"] is None else torch.from_numpy(inp["mask"]).to(gpu)
    out = lyr(x, input_mask=mask)
    if backward:
        out.backward(torch.from_numpy(inp["dout"]).to(gpu))
    torch.cuda.synchronize()
    return out.detach(), x.grad


@pytest.mark.parametrize("tag", list(ref.CASES))
def test_layer_vs_huggingface_golden(gpu, golden, tag):
    """The layer, fed HuggingFace's own permutation (``forced_st``), against HuggingFace's fp32 output and gradients.

    Bounds: the ones tests/test_lsh_hip.py holds the same attention kernels to against the oracle --
      forward  (test_attention_forward_vs_oracle): |out - ref| < 1.2e-2 max|v|, mean < 8e-4 max|v| on rows that see another
               token; rtol = atol = 1e-1 on rows that see only themselves (fp32's logsumexp grid at the self-mask value);
      backward (test_attention_backward_vs_oracle_autograd): max < 1.5e-2, mean < 1e-3 of max|ref|, rel-L2 < 1e-2,
               applied here to dx, d query_key.weight and d value.weight.
    Masked query rows are not compared in the forward (HuggingFace does not mask queries; the reference's loss drops them);
    the stored upstream gradient is zero there.  Unlike the oracle comparison, the device starts from the bf16 projection
    where HuggingFace keeps fp32, and the gradients pass two more bf16 GEMMs; the figures are printed before the asserts."""
    b, h, t, chunk, r, causal, nb, seed = _meta(golden, tag)
    lyr, inp = _layer(gpu, golden, tag)
    st = golden[f"{tag}/sorted_idx"].astype(np.int32).reshape(b * h, r, t)
    lyr.forced_st = torch.from_numpy(st).to(gpu)
    out, dx = _run_layer(gpu, lyr, inp)
    assert lyr.num_buckets == nb and out.dtype == torch.float32 and out.shape == (b, t, h * 64)
    rows = golden[f"{tag}/rows"]
    got = out.cpu().numpy()[:, rows].reshape(b, len(rows), h, 64)
    want = golden[f"{tag}/out"].astype(np.float32).reshape(b, len(rows), h, 64)
    valid = np.ones((b, t), dtype=bool) if inp["mask"] is None else inp["mask"]
    normal = ref.sees_another_token(st, chunk, causal, inp["mask"], h).reshape(b, h, t).transpose(0, 2, 1)     # (B, T, H)
    sel = (normal & valid[:, :, None])[:, rows]
    alone = (~normal & valid[:, :, None])[:, rows]
    vmax = float(np.abs(inp["x"].reshape(b * t, -1) @ inp["wv"].T).max())
    err = np.abs(got - want)
    e_max, e_mean = float(err[sel].max()) / vmax, float(err[sel].mean()) / vmax
    print(f"\n[hf layer {tag}] out / max|v|: max {e_max:.2e} mean {e_mean:.2e} on {int(sel.sum())} (row, head) pairs, "
          f"{int(alone.sum())} see only themselves (tol 1.2e-2, 8e-4)")
    msgs, fails = [], []
    grads = (("dx", dx.cpu().numpy()[:, rows], golden[f"{tag}/dx"]), ("dwqk", lyr.query_key.weight.grad.cpu().numpy(), golden[f"{tag}/dwqk"]),
             ("dwv", lyr.value.weight.grad.cpu().numpy(), golden[f"{tag}/dwv"]))
    for name, g, w in grads:
        w = w.astype(np.float32)
        scale = float(np.abs(w).max())
        d = np.abs(g - w)
        rel = float(np.linalg.norm(g - w) / np.linalg.norm(w))
        msgs.append(f"{name} max {d.max() / scale:.2e} mean {d.mean() / scale:.2e} rel-L2 {rel:.2e}")
        if not (d.max() < 1.5e-2 * scale and d.mean() < 1e-3 * scale and rel < 1e-2):
            fails.append(msgs[-1])
    print(f"[hf layer {tag}] gradients / max|ref|: " + "; ".join(msgs) + " (tol max 1.5e-2, mean 1e-3, rel-L2 1e-2)")
    assert e_max < 1.2e-2 and e_mean < 8e-4, (e_max, e_mean)
    if alone.any():
        np.testing.assert_allclose(got[alone], want[alone], rtol=1e-1, atol=1e-1)
    assert not fails, fails


@pytest.mark.parametrize("tag", list(ref.CASES))
def test_layer_on_its_own_hash(gpu, golden, tag):
    """With the fixture's rotations and its own hash: the permutation is what ``ops.lsh_hash_sort_hf`` gives on the layer's own
    (scaled, bf16) projection, the output is bitwise the output of the ``forced_st`` path fed that permutation, and the
    permutation differs from HuggingFace's (which hashed the fp32 projection) on few slots."""
    from reformer_tts_amd import ops
    from reformer_tts_amd.model.hf_lsh_attention import QK_SCALE
    from reformer_tts_amd.model.lsh_attention import _project
    b, h, t, chunk, r, causal, nb, seed = _meta(golden, tag)
    lyr, inp = _layer(gpu, golden, tag)
    lyr.forced_rotations = torch.from_numpy(golden[f"{tag}/rot"])
    out_own, _ = _run_layer(gpu, lyr, inp, backward=False)
    st_own = lyr.last_st.clone()
    with torch.no_grad():
        x2 = torch.from_numpy(inp["x"]).to(gpu).bfloat16().reshape(b * t, -1)
        qkv = _project(x2, None, lyr.query_key.weight * QK_SCALE, lyr.value.weight).view(b, t, -1)
        mask = None if inp["mask"] is None else torch.from_numpy(inp["mask"]).to(gpu)
        st, buckets, _ = ops.lsh_hash_sort_hf(qkv[..., :h * 64], lyr.forced_rotations.to(gpu), h, chunk, nb, mask, want_buckets=True)
    assert torch.equal(st_own, st)
    lyr.forced_st = st
    out_forced, _ = _run_layer(gpu, lyr, inp, backward=False)
    assert torch.equal(out_own, out_forced)
    share = float((buckets.cpu().numpy() != golden[f"{tag}/buckets"].astype(np.int32).reshape(b * h, r, t)).mean())
    print(f"\n[hf layer {tag}] buckets differing from HuggingFace's: {share:.2e} (cap 2e-2)")
    assert share < 2e-2


# ------------------------------------------------------------------ (e) inside a model: fused executor, captured step
def _hf_small_cfg():
    cfg = model_ref.small_cfg()
    cfg["enc_reformer_kwargs"]["attn_kwargs"]["implementation"] = "huggingface_transformers"
    cfg["dec_reformer_kwargs"]["self_attn_kwargs"]["implementation"] = "huggingface_transformers"
    return cfg


def _hf_layers(model):
    from reformer_tts_amd.model.hf_lsh_attention import HFLSHSelfAttention
    return [m for m in model.modules() if isinstance(m, HFLSHSelfAttention)]


def _force_rotations(model, seed=3):
    for layer in _hf_layers(model):
        layer.forced_rotations = {nb: torch.randn(layer.heads, 64, layer.n_hashes, nb // 2, generator=torch.Generator().manual_seed(seed))
                                  for nb in (2, 4, 8, 16)}


def test_fused_engine_matches_general_path_hf(gpu):
    """1 + 1 layers of the HuggingFace layer: the explicit executor (no output projection: the attention output enters the
    residual add, the stream gradient is the attention's output gradient) against the module path through autograd, to the
    tolerance of tests/test_model_hip.py::test_fused_engine_matches_general_path."""
    from reformer_tts_amd.model import TTSLoss
    from reformer_tts_amd.model.config import model_config_from_dict
    from reformer_tts_amd.training import build_model
    batch = {k: v.to(gpu) for k, v in model_ref.synthetic_batch(2, 60, 200, ragged=True, seed=2).items()}
    results = []
    for fused in (True, False):
        model = build_model(model_config_from_dict(_hf_small_cfg()), gpu)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict(synth.synth_state_dict(shapes, seed=5), strict=False)
        model.train()
        model.enc.reformer.layers.use_fused = fused
        model.dec.reformer.layers.use_fused = fused
        assert len(_hf_layers(model)) == 2
        _force_rotations(model)
        spec = batch["spectrogram"]
        raw, post, stop, _ = model(batch["phonemes"], spec[:, :-1], spectrogram_mask=batch["loss_mask"].mean(-1))
        res = TTSLoss(torch.tensor(5.0))(raw, post, stop.view(stop.shape[0], -1), spec[:, 1:], batch["stop_tokens"], batch["loss_mask"])
        res[0].backward()
        torch.cuda.synchronize()
        assert (model.enc.reformer.layers._program is not None) == fused
        assert [m.num_buckets for m in _hf_layers(model)] == [ref.num_buckets(m.last_st.shape[2], 64) for m in _hf_layers(model)]
        results.append((raw.detach().float(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}))
    (raw_f, g_f), (raw_g, g_g) = results
    rel_out = ((raw_f - raw_g).norm() / raw_g.norm()).item()
    worst = ("", 0.0)
    for n in g_g:
        if g_g[n].norm().item() < 1e-3:
            continue
        rel = ((g_f[n] - g_g[n]).norm() / g_g[n].norm()).item()
        if rel > worst[1]:
            worst = (n, rel)
    print(f"\n[hf fused vs general] output rel-L2 {rel_out:.2e} (tol 2e-2), worst gradient {worst[0]} {worst[1]:.2e} (tol 6e-2)")
    assert any("query_key" in n for n in g_g) and not any("to_out" in n for n in g_g)
    assert rel_out < 2e-2
    assert worst[1] < 6e-2, worst


def test_graph_replay_matches_eager_steps_hf(gpu):
    """One captured training step (T = 256 decoder frames) replayed twice against the eager steps of the same trajectory."""
    from reformer_tts_amd.model.config import TTSTrainingConfig, model_config_from_dict
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    batch = synthetic_batch(2, 100, 256, device=gpu)
    traj = []
    for graph in (False, True):
        torch.manual_seed(1)
        model = build_model(model_config_from_dict(_hf_small_cfg()), gpu)
        _force_rotations(model, seed=5)
        tr = Trainer(model, TTSTrainingConfig(batch_size=2, learning_rate=1e-3, warmup_steps=4, gradient_clip_val=1.0), gpu)
        if graph:
            tr.capture(batch, segmented=False)       # 2 eager warm-up steps (0, 1); capturing itself executes nothing
            losses = [None, None] + [float(tr.replay()[0]) for _ in range(2)]
        else:
            losses = [float(tr.train_step(batch)[0]) for _ in range(4)]
        traj.append(losses)
    print(f"\n[hf graph replay] eager {traj[0]} replayed {traj[1][2:]}")
    np.testing.assert_allclose(traj[1][2:], traj[0][2:], rtol=2e-2)
    assert traj[0][-1] < traj[0][0]


def test_huggingface_lsh_config_trains_and_synthesises(gpu):
    """The model section of the reference's config/huggingface-lsh.yml (3 + 3 layers, d = 512, chunks 64 / 128, pad_base 256):
    two ``Trainer.train_step`` calls give finite losses and move both parameters of every attention layer, and ``infer`` runs."""
    from reformer_tts_amd.model.config import TTSTrainingConfig, huggingface_lsh_model_config
    from reformer_tts_amd.training import Trainer, build_model, synthetic_batch
    torch.manual_seed(2)
    model = build_model(huggingface_lsh_model_config(), gpu)
    tr = Trainer(model, TTSTrainingConfig(batch_size=2, learning_rate=1e-3, warmup_steps=4, gradient_clip_val=1.0), gpu)
    batch = synthetic_batch(2, 100, 300, device=gpu)
    before = [(m.query_key.weight.detach().clone(), m.value.weight.detach().clone()) for m in _hf_layers(model)]
    l0 = float(tr.train_step(batch)[0])
    l1 = float(tr.train_step(batch)[0])
    assert np.isfinite(l0) and np.isfinite(l1)
    assert model.enc.reformer.layers._program is not None and model.dec.reformer.layers._program is not None      # the explicit executor
    for m, (wqk, wv) in zip(_hf_layers(model), before):
        assert bool(torch.isfinite(m.query_key.weight).all()) and bool(torch.isfinite(m.value.weight).all())
        assert not torch.equal(m.query_key.weight, wqk) and not torch.equal(m.value.weight, wv)
    assert [m.num_buckets for m in _hf_layers(model)] == [8] * 3 + [8] * 3           # T = 256 / 64 -> 8; T = 512 / 128 -> 8
    spec, stop = model.infer(batch["phonemes"][:, :40], max_len=82)
    assert spec.shape[:2] == (2, 80) and spec.shape[2] >= 1 and bool(torch.isfinite(spec).all())
