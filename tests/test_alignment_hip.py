"""Encoder-decoder attention alignments on the HIP eval path: the head-averaged probability kernel
(rtts_xattn_probs_mean) against float64, the explicit executor's attention_matrices_ against the general eval path and
against the reference's own matrices (alignment_small.npz), Trainer.validate(return_attention=True), and what must not move
(outputs, generation, launch counts)."""
import os

import numpy as np
import pytest
import torch

from oracle import model_ref, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _operands(b, h, tq, tk, masked, seed):
    g = torch.Generator().manual_seed(seed)
    e = 64 * h
    q = torch.randn(b * tq, e, generator=g).bfloat16()
    kv = (torch.randn(b * tk, 2 * e, generator=g) * 1.5).bfloat16()
    kvalid = None
    if masked:
        kvalid = torch.ones(b, tk, dtype=torch.uint8)
        lengths = [tk, 1, max(1, tk // 3)]                      # full, one key, heavy padding (prefix masks, as key_padding_mask)
        for i in range(b):
            kvalid[i, lengths[i % 3]:] = 0
        if b > 1:                                               # and one sample with holes inside
            holes = torch.rand(tk, generator=g) < 0.4
            holes[0] = False
            kvalid[b - 1][holes] = 0
    return q, kv, kvalid


def _fwd_lse(q, kv, kvalid, b, h, tq, tk, dev):
    from reformer_tts_amd import _lib
    from reformer_tts_amd._seeds import seed_base
    e = 64 * h
    o = torch.empty(b * tq, e, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(b * h, tq, dtype=torch.float32, device=dev)
    _lib.call("rtts_xattn_fwd", q.data_ptr(), e, kv.data_ptr(), 2 * e, None if kvalid is None else kvalid.data_ptr(), b, h, tq, tk, 64,
              o.data_ptr(), e, lse.data_ptr(), 0.0, 0, seed_base(dev).data_ptr(), _stream())
    return lse


def _probs_f64(q, kv, kvalid, b, h, tq, tk):
    """float64 restatement from the same bf16 operands: softmax(q k^T / 8, masked keys -inf) per head, mean over heads."""
    e = 64 * h
    qd = q.double().view(b, tq, h, 64).transpose(1, 2)
    kd = kv[:, :e].double().view(b, tk, h, 64).transpose(1, 2)
    s = qd @ kd.transpose(-1, -2) / 8.0
    if kvalid is not None:
        s = s.masked_fill(kvalid.bool().logical_not()[:, None, None, :], float("-inf"))
    return torch.softmax(s, dim=-1).mean(dim=1)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("tk", [128, 256, 384, 768, 2048])
@pytest.mark.parametrize("tq", [128, 1024])
@pytest.mark.parametrize("b", [1, 3])
def test_probs_mean_vs_float64(gpu, b, tq, tk, masked):
    """rtts_xattn_probs_mean with rtts_xattn_fwd's lse of the same operands against float64: max abs <= 2e-4, every row sums
    to 1 within 1e-4, masked keys exactly 0."""
    from reformer_tts_amd import engine
    h = 8
    q, kv, kvalid = _operands(b, h, tq, tk, masked, seed=b * 7 + tq + tk + masked)
    qd, kvd = q.to(gpu), kv.to(gpu)
    kvd_valid = None if kvalid is None else kvalid.to(gpu)
    lse = _fwd_lse(qd, kvd, kvd_valid, b, h, tq, tk, gpu)
    a = engine.xattn_probs_mean(qd, kvd, kvd_valid, lse, b, h, tq, tk)
    ref = _probs_f64(qd, kvd, kvd_valid, b, h, tq, tk)
    torch.cuda.synchronize()
    assert a.shape == (b, tq, tk) and a.dtype == torch.float32
    err = float((a.double() - ref).abs().max())
    assert err <= 2e-4, err
    assert float((a.double().sum(-1) - 1.0).abs().max()) <= 1e-4
    if kvd_valid is not None:
        assert bool((a.masked_select(kvd_valid.bool().logical_not()[:, None, :].expand_as(a)) == 0).all())


def test_probs_mean_row_stride(gpu):
    """ld_a > T_k: the kernel writes columns [0, T_k) of every row and leaves the rest alone."""
    from reformer_tts_amd import engine
    b, h, tq, tk = 2, 8, 256, 384
    q, kv, kvalid = _operands(b, h, tq, tk, True, seed=5)
    qd, kvd, kvv = q.to(gpu), kv.to(gpu), kvalid.to(gpu)
    lse = _fwd_lse(qd, kvd, kvv, b, h, tq, tk, gpu)
    wide = torch.full((b, tq, tk + 20), float("nan"), device=gpu)
    engine.xattn_probs_mean(qd, kvd, kvv, lse, b, h, tq, tk, out=wide[:, :, :tk])
    ref = _probs_f64(qd, kvd, kvv, b, h, tq, tk)
    torch.cuda.synchronize()
    assert float((wide[:, :, :tk].double() - ref).abs().max()) <= 2e-4
    assert bool(torch.isnan(wide[:, :, tk:]).all())


def test_probs_mean_rejects_bad_arguments(gpu):
    from reformer_tts_amd import _lib
    b, h = 1, 2
    q = torch.zeros(1024 * b, 64 * h, dtype=torch.bfloat16, device=gpu)
    kv = torch.zeros(4096 * b, 128 * h, dtype=torch.bfloat16, device=gpu)
    lse = torch.zeros(b * h, 1024, device=gpu)
    a = torch.zeros(b, 1024, 4096, device=gpu)

    def run(tq=128, tk=128, dh=64, lse_ptr=lse.data_ptr(), ld_a=4096):
        _lib.call("rtts_xattn_probs_mean", q.data_ptr(), 64 * h, kv.data_ptr(), 128 * h, None, lse_ptr, b, h, tq, tk, dh, a.data_ptr(),
                  ld_a, _stream())

    run()
    torch.cuda.synchronize()
    for kw, words in ((dict(dh=32), "dh"), (dict(tq=100), "T_q"), (dict(tk=64), "T_k"), (dict(tk=2176), "T_k"), (dict(tk=130), "T_k"),
                      (dict(lse_ptr=None), "NULL"), (dict(ld_a=100), "ld_a"), (dict(ld_a=130), "ld_a")):
        with pytest.raises(_lib.RttsError, match=words):
            run(**kw)


# ------------------------------------------------------------------ the executor and the model
def _cfg(which, dec_depth=2):
    from reformer_tts_amd.model.config import model_config_from_dict
    cfg = model_ref.small_cfg() if which == "small" else model_ref.cfg1()
    cfg["enc_reformer_kwargs"]["attn_kwargs"]["implementation"] = "hip"
    cfg["dec_reformer_kwargs"]["self_attn_kwargs"]["implementation"] = "hip"
    cfg["dec_reformer_kwargs"]["depth"] = dec_depth
    return model_config_from_dict(cfg)


def _lsh_layers(model):
    from reformer_tts_amd.model.lsh_attention import LSHSelfAttention
    return [m for m in model.modules() if isinstance(m, LSHSelfAttention)]


def _model(which, gpu, seed=5):
    from reformer_tts_amd.training import build_model
    model = build_model(_cfg(which), gpu)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.synth_state_dict(shapes, seed=seed), strict=False)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_((0.2 * torch.randn(buf.shape, generator=g)).to(gpu))
            elif name.endswith("running_var"):
                buf.copy_((0.5 + torch.rand(buf.shape, generator=g)).to(gpu))
    for i, layer in enumerate(_lsh_layers(model)):           # the same rotations on every path and every call
        layer.forced_rotations = {nb: torch.randn(1, 64, layer.n_hashes, nb // 2, generator=torch.Generator().manual_seed(3 + i))
                                  for nb in (2, 4, 6, 8, 10, 12, 16)}
    return model


def _eval_forward(model, batch, fused, collect=True):
    stacks = (model.enc.reformer.layers, model.dec.reformer.layers)
    model.eval()
    for st in stacks:
        st.fused_in_eval = fused
    model.dec.reformer.collect_attention = collect
    try:
        with torch.no_grad():
            spec = batch["spectrogram"]
            raw, post, stop, mats = model(batch["phonemes"], spec[:, :-1], spectrogram_mask=batch["loss_mask"].mean(-1))
            return (raw, post, stop), list(mats)
    finally:
        for st in stacks:
            st.fused_in_eval = False
        model.dec.reformer.collect_attention = True
        model.train()


@pytest.mark.parametrize("which,text,mel", [("small", 100, 200), ("small", 300, 250), ("cfg1", 150, 700), ("cfg1", 300, 400)])
def test_executor_matrices_match_general_eval_path(gpu, which, text, mel):
    """With fused_in_eval the explicit executor fills attention_matrices_: one (B, T_q padded, T_k padded) fp32 matrix per decoder
    layer, in layer order, agreeing with the general eval path's (ATen fp32 scores of the same bf16 projections) on the same
    model with the same rotations.  The two paths' decoder streams differ by bf16 rounding of the fused epilogues, which the
    logits carry into the probabilities.  Achieved on one MI355X: max abs 2.1e-4 .. 6.7e-4, mean abs 8e-6 .. 3.5e-5."""
    from reformer_tts_amd import _lib
    model = _model(which, gpu)
    batch = {k: v.to(gpu) for k, v in model_ref.synthetic_batch(2, text, mel, ragged=True, seed=text + mel).items()}
    before = len(_lib.PATHS_LEFT)
    _, fused = _eval_forward(model, batch, fused=True)
    assert len(_lib.PATHS_LEFT) == before, _lib.PATHS_LEFT[before:]
    _, general = _eval_forward(model, batch, fused=False)
    torch.cuda.synchronize()
    pad = model.pad_base
    tq, tk = -(-(batch["spectrogram"].shape[1] - 1) // pad) * pad, -(-batch["phonemes"].shape[1] // pad) * pad
    assert len(fused) == len(general) == model.dec.reformer.depth
    kvalid = (torch.nn.functional.pad(batch["phonemes"], (0, tk - batch["phonemes"].shape[1])) != 0)
    for a, r in zip(fused, general):
        assert a.shape == r.shape == (2, tq, tk) and a.dtype == torch.float32 and a.is_cuda
        assert bool((a.masked_select(~kvalid[:, None, :].expand_as(a)) == 0).all())
        d = (a - r).abs()
        print(f"{which} text {text} mel {mel}: max abs {float(d.max()):.2e} mean abs {float(d.mean()):.2e}")
        assert float(d.max()) <= 2e-2 and float(d.mean()) <= 1e-3, (float(d.max()), float(d.mean()))


def test_executor_matrices_match_reference_golden(golden_dir, gpu):
    """alignment_small.npz: the reference's ReformerTTS in eval mode, teacher-forced as validation_step calls it, on small_cfg
    with a 2-layer decoder, recorded rotations and non-trivial BatchNorm statistics.  The HIP eval forward (bf16 operands
    with fp32 accumulation; the reference is fp32 throughout) must reproduce its matrices to max abs <= 1e-2, mean abs <= 2e-4:
    a probability's relative error is its logit's absolute error, which bf16 operands (2^-9 relative) through two decoder
    layers put at a few 1e-3 on the largest logits; the fixture's float16 storage adds <= 2.5e-4.  Achieved on one MI355X:
    max abs 1.6e-3 / 5.9e-4, mean abs 1.8e-5 / 2.0e-5 (layers 0 / 1)."""
    from reformer_tts_amd import _lib
    from reformer_tts_amd.training import build_model
    z = np.load(os.path.join(golden_dir, "alignment_small.npz"))
    model = build_model(_cfg("small"), gpu)
    shapes = {k[len("shape/"):]: tuple(z[k]) for k in z.files if k.startswith("shape/")}
    missing = model.load_state_dict(synth.synth_state_dict(shapes, seed=3), strict=False)
    assert not missing.unexpected_keys
    model.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("buf/")}, strict=False)
    layers = _lsh_layers(model)
    assert len(layers) == int(z["n_rot"])                                   # one eval forward: one rotation per layer, call order
    for i, layer in enumerate(layers):
        layer.forced_rotations = torch.from_numpy(z[f"rot/{i}"])
    batch = {k[len("batch/"):]: torch.from_numpy(z[k]).to(gpu) for k in z.files if k.startswith("batch/")}
    before = len(_lib.PATHS_LEFT)
    (_, post, _), mats = _eval_forward(model, batch, fused=True)
    torch.cuda.synchronize()
    assert len(_lib.PATHS_LEFT) == before, _lib.PATHS_LEFT[before:]
    refs = [torch.from_numpy(z[f"att/{i}"].astype(np.float32)) for i in range(2)]
    assert len(mats) == len(refs)
    kvalid = torch.nn.functional.pad(batch["phonemes"], (0, refs[0].shape[2] - batch["phonemes"].shape[1])).cpu() != 0
    for i, (a, r) in enumerate(zip(mats, refs)):
        assert a.shape == r.shape
        a = a.cpu()
        d = (a - r).abs()
        print(f"layer {i}: max abs {float(d.max()):.2e} mean abs {float(d.mean()):.2e}")
        assert float(d.max()) <= 1e-2 and float(d.mean()) <= 2e-4, (i, float(d.max()), float(d.mean()))
        assert bool((a.masked_select(~kvalid[:, None, :].expand_as(a)) == 0).all())
    ref_post = torch.from_numpy(z["out/post"].astype(np.float32))
    assert float((post.cpu() - ref_post).abs().max()) < 3e-2 * float(ref_post.abs().max())


@pytest.mark.parametrize("text", [100, 300])
def test_validate_returns_trimmed_alignments(gpu, text):
    """validate(batch, return_attention=True): the same five scalars (bits) as validate(batch), plus per sample a list of per-layer
    (stop index, T_k padded) matrices equal to trim_attention_matrices of the untrimmed list; parameters and BatchNorm buffers
    untouched; no library matrix product, SDPA or general-path note during the call.  text 300: 384 keys (three 128-key chunks)."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from reformer_tts_amd import _lib
    from reformer_tts_amd.model.config import TTSTrainingConfig
    from reformer_tts_amd.training import Trainer, trim_attention_matrices
    model = _model("small", gpu)
    tr = Trainer(model, TTSTrainingConfig(batch_size=3), gpu)
    batch = {k: v.to(gpu) for k, v in model_ref.synthetic_batch(3, text, 220, ragged=True, seed=text).items()}
    snap = (tr.flat_p.clone(), {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k})
    plain = tr.validate(batch)
    tr.validate(batch, return_attention=True)          # warm-up
    seen = []

    class Census(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    before = len(_lib.PATHS_LEFT)
    with Census():
        got = tr.validate(batch, return_attention=True)
    full = list(model.dec.reformer.attention_matrices_)
    torch.cuda.synchronize()
    bad = sorted({f for f in seen if any(k in f for k in ("aten.mm", "aten.addmm", "aten.bmm", "aten.matmul", "aten.linear",
                                                          "scaled_dot_product", "aten.baddbmm", "aten._softmax"))})
    assert not bad, bad
    assert len(_lib.PATHS_LEFT) == before, _lib.PATHS_LEFT[before:]
    assert len(got) == 6 and model.training
    for x, y in zip(plain, got[:5]):
        assert torch.equal(x, y)
    assert len(full) == model.dec.reformer.depth
    tk = -(-batch["phonemes"].shape[1] // model.pad_base) * model.pad_base
    stops = batch["stop_tokens"].argmax(dim=1).tolist()
    want = trim_attention_matrices(full, batch["stop_tokens"])
    assert len(got[5]) == 3
    for i, (per_layer, ref_layer) in enumerate(zip(got[5], want)):
        assert len(per_layer) == len(full)
        for m, r in zip(per_layer, ref_layer):
            assert m.shape == (stops[i], tk) and m.is_cuda and torch.equal(m, r)
    assert torch.equal(tr.flat_p, snap[0])
    assert all(torch.equal(model.state_dict()[k], v) for k, v in snap[1].items())


def _count_calls(monkeypatch):
    from reformer_tts_amd import _lib
    counts = {}
    real = _lib.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    return counts


def test_collection_moves_nothing_else(gpu, monkeypatch):
    """Collection on or off: the eval forward's outputs are the same bits; off, the list stays empty and the probability kernel
    is never launched; the default validate() launches it neither."""
    from reformer_tts_amd.model.config import TTSTrainingConfig
    from reformer_tts_amd.training import Trainer
    model = _model("small", gpu)
    batch = {k: v.to(gpu) for k, v in model_ref.synthetic_batch(2, 120, 200, ragged=True, seed=4).items()}
    counts = _count_calls(monkeypatch)
    on, mats_on = _eval_forward(model, batch, fused=True, collect=True)
    n_on = counts.get("rtts_xattn_probs_mean", 0)
    off, mats_off = _eval_forward(model, batch, fused=True, collect=False)
    torch.cuda.synchronize()
    assert n_on == model.dec.reformer.depth and len(mats_on) == n_on
    assert counts.get("rtts_xattn_probs_mean", 0) == n_on and mats_off == []
    for x, y in zip(on, off):
        assert torch.equal(x, y)
    tr = Trainer(model, TTSTrainingConfig(batch_size=2), gpu)
    tr.validate(batch)
    assert counts.get("rtts_xattn_probs_mean", 0) == n_on
    assert model.dec.reformer.collect_attention


@pytest.mark.parametrize("use_graph", [False, True])
def test_infer_launches_no_probability_kernel(gpu, monkeypatch, use_graph):
    """Generation discards the alignments: no rtts_xattn_probs_mean launch in eager or graphed infer (nothing captured into the
    graphs), and the same spectrogram and stop indices whether the decoder's collection switch is on or off."""
    outs = []
    for collect in (True, False):
        model = _model("small", gpu)
        model.dec.reformer.collect_attention = collect
        counts = _count_calls(monkeypatch)
        ph = model_ref.synthetic_batch(2, 40, 10, seed=1)["phonemes"]
        outs.append(model.infer(ph, max_len=90, stop_at_stop_token=False, use_graph=use_graph, cache_encoder=True))
        torch.cuda.synchronize()
        assert counts.get("rtts_xattn_probs_mean", 0) == 0 and counts.get("rtts_xattn_fwd", 0) > 0
        assert model.dec.reformer.collect_attention == collect
        monkeypatch.undo()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
