"""Incremental generation (``model/incremental.py``, ``ReformerTTS.infer(incremental=True)``) on the GPU: teacher-forced parity of
every position with the full-window eval executor, the postnet tail against the postnet on the prefix, determinism and the single
graph, the stop bookkeeping against an eager loop over ``step``, the launch census and ``Trainer.validate_inference``.

Model: ``model_ref.small_cfg()`` made dense on both stacks, depth 2 + 2, postnet depth 2, ``synth.synth_state_dict`` weights; B 2, 60
phonemes (T_k 128), 70 frames (crossing the 64-key tile), capacity 128.  Tolerance of the parity tests: rel-L2 < 2e-2 per position,
``test_fused_engine_matches_general_path``'s for "same GEMMs, different fusion around the cores" -- here the GEMM rows are the same
products and only the attention cores differ.

Measured on an MI355X over the 70 positions: step against the full-window executor, worst rel-L2 3.17e-3 on mel and 1.82e-2 on the
(two) stop logits, both at p = 0; the postnet tail against the postnet on the prefix 0 (bit-identical); graphed against eager
generation 0.  The whole file runs in 5 s."""
import math

import pytest
import torch

from oracle import model_ref, synth

pytestmark = pytest.mark.gpu

B, FRAMES, CAPACITY, MAX_LEN = 2, 70, 128, 90


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _dense_cfg():
    cfg = model_ref.small_cfg()
    for stack, key in (("enc_reformer_kwargs", "attn_kwargs"), ("dec_reformer_kwargs", "self_attn_kwargs")):
        cfg[stack]["depth"] = 2
        cfg[stack][key].update(implementation="hip", use_full_attn=True)
    cfg["postnet_kwargs"] = dict(depth=2, dropout=0.0)
    return cfg


def _build(gpu):
    from reformer_tts_amd.model.config import model_config_from_dict
    from reformer_tts_amd.training import build_model
    model = build_model(model_config_from_dict(_dense_cfg()), gpu)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if "running" not in k and "num_batches" not in k}
    model.load_state_dict(synth.synth_state_dict(shapes, seed=5), strict=False)       # BatchNorm keeps its initial running statistics
    return model


@pytest.fixture(scope="module")
def env(gpu):
    model = _build(gpu)
    batch = model_ref.synthetic_batch(B, 60, 200, ragged=True, seed=2)
    return dict(model=model, phonemes=batch["phonemes"].to(gpu), spec=batch["spectrogram"][:, :FRAMES].to(gpu), out={})


def _rel(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def _teacher_forced(env):
    """Every position's (mel, mel_post, stop_logit) from ``step`` on the frames of the synthetic spectrogram, made once."""
    if "steps" not in env["out"]:
        from reformer_tts_amd.model.incremental import IncrementalDecoder
        model = env["model"]
        model.eval()
        gen = IncrementalDecoder(model, env["phonemes"], CAPACITY)
        outs = [tuple(t.clone() for t in gen.step(env["spec"][:, p])) for p in range(FRAMES)]
        torch.cuda.synchronize()
        assert int(gen.pos) == FRAMES
        env["out"]["steps"] = (gen, outs)
    return env["out"]["steps"]


def test_teacher_forced_rows_match_the_full_window_executor(env):
    from reformer_tts_amd.model.reformer_tts import pad_to_multiple
    model = env["model"]
    gen, outs = _teacher_forced(env)
    pad_ph = pad_to_multiple(env["phonemes"].unsqueeze(-1), model.pad_base).squeeze(-1)
    ph_mask = pad_ph != 0
    pad_spec = pad_to_multiple(env["spec"], model.pad_base)
    mask = torch.zeros(B, pad_spec.shape[1], dtype=torch.bool, device=pad_spec.device)
    mask[:, :FRAMES] = True
    stacks = (model.enc.reformer.layers, model.dec.reformer.layers)
    model.eval()
    for st in stacks:
        st.fused_in_eval = True
    try:
        with torch.no_grad():
            keys = model.enc(pad_ph, input_mask=ph_mask)
            mel, stop, _ = model.dec(pad_spec, keys=keys, key_padding_mask=~ph_mask, input_mask=mask)
    finally:
        for st in stacks:
            st.fused_in_eval = False
    worst = {"mel": (0.0, -1), "stop": (0.0, -1)}
    for p, (m, _, s) in enumerate(outs):
        for name, got, want in (("mel", m, mel[:, p]), ("stop", s, stop[:, p])):
            assert torch.isfinite(got).all()
            worst[name] = max(worst[name], (_rel(got, want), p))
    print(f"[parity] incremental step vs full-window executor over {FRAMES} positions: worst rel-L2 mel {worst['mel'][0]:.2e} "
          f"(p = {worst['mel'][1]}), stop logit {worst['stop'][0]:.2e} (p = {worst['stop'][1]})")
    worst = max(worst.values())
    assert worst[0] < 2e-2


def test_postnet_tail_matches_the_postnet_on_the_prefix(env):
    """mel_post[p] against mel_hist[:, :p + 1] + postnet(mel_hist[:, :p + 1]) at row p, on the incremental mel history so that
    only the tail is under test."""
    model = env["model"]
    gen, outs = _teacher_forced(env)
    hist = gen.mel_hist[:, :FRAMES]
    assert torch.equal(hist, torch.stack([m for m, _, _ in outs], dim=1))
    model.eval()
    worst = (0.0, -1)
    with torch.no_grad():
        for p, (_, mp, _) in enumerate(outs):
            want = (hist[:, :p + 1] + model.postnet(hist[:, :p + 1]))[:, p]
            worst = max(worst, (_rel(mp, want), p))
    print(f"[parity] postnet tail vs postnet on the prefix over {FRAMES} positions: worst rel-L2 {worst[0]:.2e} (p = {worst[1]})")
    assert worst[0] < 2e-2


def test_generation_is_deterministic_and_captures_one_graph(env):
    model, ph = env["model"], env["phonemes"]
    kw = dict(max_len=MAX_LEN, stop_at_stop_token=False, incremental=True)
    a = model.infer(ph, use_graph=True, **kw)
    b = model.infer(ph, use_graph=True, **kw)
    gens = list(model.__dict__["_inc_cache"].values())
    c = model.infer(ph, use_graph=False, **kw)
    torch.cuda.synchronize()
    assert a[0].shape == (B, 80, MAX_LEN) and torch.isfinite(a[0]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[1].cpu(), torch.full((B,), MAX_LEN))
    assert len(gens) == 1 and gens[0].graphs_captured == 1            # one graph for 90 frames, none more for the second call
    assert list(model.__dict__["_inc_cache"].values())[0] is gens[0]
    diff = float((a[0] - c[0]).abs().max())
    print(f"[incremental] graphed vs eager generation: max |difference| {diff:.2e} of max |.| {float(c[0].abs().max()):.2e}")
    assert diff <= 2e-2 * float(c[0].abs().max())


def test_stop_bookkeeping_is_the_reference_loop(env):
    """A stop_linear.bias chosen so that sample 0 fires at a known frame: stop indices and the cut length of the graphed generation
    equal the reference's bookkeeping run on the host over the stop logits of an eager loop over ``step``."""
    from reformer_tts_amd.model.incremental import IncrementalDecoder
    model, ph = env["model"], env["phonemes"]
    thr, every = 0.25, 8
    bias0 = model.dec.stop_linear.bias.detach().clone()
    try:
        model.eval()
        gen = IncrementalDecoder(model, ph, CAPACITY)
        frame = torch.zeros(B, 80, device=ph.device)
        logits = []
        for _ in range(MAX_LEN):
            _, frame, sl = gen.step(frame)
            logits.append(sl.reshape(B).clone())
        logits = torch.stack(logits).double().cpu()                    # (MAX_LEN, B)
        fire = int(logits[:40, 0].argmax())                            # a frame at which sample 0 can be made to cross first
        below = float(logits[:fire, 0].max()) if fire else float(logits[fire, 0]) - 2.0
        gap = float(logits[fire, 0]) - below
        assert gap > 1e-4 * abs(float(logits[fire, 0]))                # far above the fp32 rounding of logit + bias
        cut = math.log(thr / (1 - thr))                                # sigmoid(x) > thr  <=>  x > cut
        shift = cut - (float(logits[fire, 0]) - gap / 2)               # the threshold midway between that logit and every earlier one
        with torch.no_grad():
            model.dec.stop_linear.bias.add_(shift)
        shifted = logits + shift                                       # the stop head does not feed back: the frames are unchanged
        stop, cur, it = [0] * B, 1, 0
        while True:
            if it % every == 0 and all(s > 0 for s in stop):
                break
            it += 1
            for i in range(B):
                if stop[i] == 0 and float(shifted[cur - 1, i]) > cut:
                    stop[i] = cur + 1
            cur += 1
            if max(B, cur, 80) > MAX_LEN:
                break
        if all(s > 0 for s in stop):
            cur = min(cur, max(stop))
        want_stop = [s if s > 0 else MAX_LEN for s in stop]
        assert stop[0] == fire + 2
        spec, got_stop = model.infer(ph, max_len=MAX_LEN, stop_threshold=thr, stop_at_stop_token=True, check_every=every, use_graph=True,
                                     incremental=True)
        assert got_stop.cpu().tolist() == want_stop
        assert spec.shape == (B, 80, cur - 1)
    finally:
        with torch.no_grad():
            model.dec.stop_linear.bias.copy_(bias0)


def test_generation_dispatches_no_library_product(env):
    from torch.utils._python_dispatch import TorchDispatchMode
    from reformer_tts_amd import _lib
    model, ph = env["model"], env["phonemes"]
    kw = dict(max_len=MAX_LEN, stop_at_stop_token=False, incremental=True, use_graph=False)
    model.infer(ph, **kw)                                              # warm-up
    seen = []

    class Census(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    before = len(_lib.PATHS_LEFT)
    with Census():
        spec, _ = model.infer(ph, **kw)
    assert spec.shape == (B, 80, MAX_LEN)
    bad = [f for f in seen if any(k in f for k in ("aten.mm", "aten.addmm", "aten.bmm", "aten.matmul", "aten.convolution", "aten.linear"))]
    assert not bad, sorted(set(bad))
    assert len(_lib.PATHS_LEFT) == before, _lib.PATHS_LEFT[before:]


def test_validate_inference_takes_the_flag(env, gpu):
    from reformer_tts_amd.model.config import TTSTrainingConfig
    from reformer_tts_amd.training import Trainer
    model = _build(gpu)                                                # a model of its own: a Trainer re-homes the parameters
    tr = Trainer(model, TTSTrainingConfig(batch_size=B, learning_rate=1e-3, warmup_steps=None, stop_loss_weight=0.0), gpu)
    batch = {k: v.to(gpu) for k, v in model_ref.synthetic_batch(B, 60, 100, ragged=True, seed=2).items()}
    plain = tr.validate_inference(batch, max_len=MAX_LEN)
    inc = tr.validate_inference(batch, max_len=MAX_LEN, incremental=True)
    assert set(inc) == set(plain)
    for k, v in inc.items():
        if torch.is_tensor(v):
            assert torch.isfinite(v).all(), k
        else:
            assert math.isfinite(v), k
