"""tests/xattn_guide_ref.py against float64 autograd and against tests/align_ref.py, on every case the GPU tests run
(tests/test_xattn_guide_hip.py), and the materiality of those cases: the unguided gradients miss the guided bounds by at least
8x somewhere in dq and in dk, so a kernel that drops the guided term cannot pass.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import align_ref
import xattn_guide_ref as G
import xattn_wide_ref as XW


@functools.lru_cache(maxsize=None)
def _case(i):
    nf, nk = G.CASES[i][7], G.CASES[i][8]
    inputs, valid, keep = G.case_inputs(i)
    return inputs, valid, keep, G.reference(*inputs, valid, keep, nf, nk, G.SIGMA, G.case_coef(G.CASES[i]))


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=G.IDS)
def test_reference_gradients_equal_float64_autograd(i):
    nf, nk = G.CASES[i][7], G.CASES[i][8]
    inputs, valid, keep, ref = _case(i)
    dq, dk, dv, loss = G.autograd(*inputs, valid, keep, nf, nk, G.SIGMA, G.case_coef(G.CASES[i]))
    worst = {n: float((ref[n] - g).abs().max()) for n, g in (("dq", dq), ("dk", dk), ("dv", dv))}
    print(f"\n[parity] {G.IDS[i]}: worst |reference - float64 autograd|  " + "  ".join(f"{n} {x:.2e}" for n, x in worst.items())
          + f"  loss {float(ref['loss']):.6f}")
    assert max(worst.values()) <= 1e-10, worst
    assert abs(float(ref["loss"]) - float(loss)) <= 1e-12
    assert 0.0 <= float(ref["loss"]) <= 1.0


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=G.IDS)
def test_loss_is_the_frame_weighted_guided_score_of_the_head_mean(i):
    """loss = sum_b guided_b / sum_b T_b over the slots that count, guided_b = column [5] of align_ref.stats_ref on the
    head-averaged matrix; out[b] = guided_b / T_b."""
    nb, nh, tq, tk = G.CASES[i][:4]
    nf, nk = G.CASES[i][7], G.CASES[i][8]
    ref = _case(i)[3]
    guided, total = [], 0
    for b, ok in enumerate(G.counts(nf, nk, tq, tk)):
        row = align_ref.stats_ref(ref["p_mean"][b].numpy(), int(nf[b]), int(nk[b]), G.SIGMA)[2]
        if ok:
            guided.append(float(row[5]))
            total += int(nf[b])
            assert abs(float(ref["out"][b]) - row[5] / int(nf[b])) <= 1e-12
        else:
            assert np.isnan(row[5]) and float(ref["out"][b]) == 0.0
    assert abs(float(ref["loss"]) - sum(guided) / total) <= 1e-12


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=G.IDS)
def test_the_unguided_gradients_miss_the_guided_bounds(i):
    inputs, valid, keep, ref = _case(i)
    plain = XW.reference(*inputs, valid, keep)
    r = G.ratios(plain, ref)
    print(f"\n[materiality] {G.IDS[i]}: worst |unguided - guided| / bound  dq {r['dq']:.1f}  dk {r['dk']:.1f}  (must be >= 8)  c {ref['c']:g}")
    assert r["dq"] >= 8.0 and r["dk"] >= 8.0, r
    assert r["dv"] == 0.0            # dV does not see the guided term


def test_no_slot_counts():
    """Every slot fails: loss = c = 0, W = 0, and the gradients are the unguided ones."""
    nb, nh, tq, tk = 3, 2, 128, 256
    inputs = G.make_inputs("plain", nb, nh, tq, tk, 5, 64)
    valid = G.X.make_valid("ragged", nb, tk)
    ref = G.reference(*inputs, valid, None, (0, 129, 128), (5, 5, 257), G.SIGMA, 1000.0)
    plain = XW.reference(*inputs, valid, None)
    assert float(ref["loss"]) == 0.0 and ref["c"] == 0.0 and float(ref["out"].abs().max()) == 0.0
    for n in ("dq", "dk", "dv"):
        assert torch.equal(ref[n], plain[n])


# ------------------------------------------------------------------ the trainer's host logic (no GPU)
def _small_model(num_heads):
    from oracle import model_ref
    from reformer_tts_amd.model.config import model_config_from_dict
    from reformer_tts_amd.training import build_model
    cfg = model_ref.small_cfg()
    cfg["enc_reformer_kwargs"]["attn_kwargs"]["implementation"] = "hip"
    cfg["dec_reformer_kwargs"]["self_attn_kwargs"]["implementation"] = "hip"
    cfg["dec_reformer_kwargs"]["attn_kwargs"]["num_heads"] = num_heads
    return build_model(model_config_from_dict(cfg))


def test_the_plan_refuses_a_cross_attention_outside_the_executor():
    from reformer_tts_amd.model.config import TTSTrainingConfig, _merge
    from reformer_tts_amd.training import Trainer
    assert Trainer.guided_attention_plan(_small_model(4), TTSTrainingConfig()) is None            # weight 0: nothing is asked
    with pytest.raises(NotImplementedError, match="decoder layer 0's cross-attention .*num_heads 4"):
        Trainer.guided_attention_plan(_small_model(4), TTSTrainingConfig(guided_attention_weight=0.5))     # heads of 32
    cfg = _merge(TTSTrainingConfig(), dict(guided_attention_weight=0.5, guided_attention_sigma=0.3, guided_attention_layers=[0]))  # as load_yaml
    assert Trainer.guided_attention_plan(_small_model(2), cfg) == (0.5, 0.3, [0])
    assert Trainer.guided_attention_plan(_small_model(1), TTSTrainingConfig(guided_attention_weight=2.0)) == (2.0, 0.2, [0])   # heads of 128
    with pytest.raises(ValueError, match="guided_attention_layers"):
        Trainer.guided_attention_plan(_small_model(2), TTSTrainingConfig(guided_attention_weight=1.0, guided_attention_layers=[1]))
    with pytest.raises(ValueError, match="guided_attention_sigma"):
        Trainer.guided_attention_plan(_small_model(2), TTSTrainingConfig(guided_attention_weight=1.0, guided_attention_sigma=0.0))


def test_the_general_path_refuses_the_guide_context():
    """A decoder stack that leaves the executors (here: on the CPU) with a guide context raises, naming the layer."""
    model = _small_model(2).train()
    dec = model.dec.reformer
    dec.guide = dict(layers=[0])
    x, keys = torch.zeros(1, 128, 128), torch.zeros(1, 128, 128)
    with pytest.raises(NotImplementedError, match="decoder layer 0's cross-attention would run on the general"):
        dec(x, keys=keys, key_padding_mask=torch.zeros(1, 128, dtype=torch.bool), input_mask=torch.ones(1, 128, dtype=torch.bool))


def test_coef_is_the_weight_times_the_loss_scale():
    """Where coef is formed: weight / N for the 1 / N of train_accumulated; a device scalar scale stays a tensor for the device."""
    import types
    from reformer_tts_amd.training import Trainer, synthetic_batch
    batch = synthetic_batch(3, 20, 40)
    batch["loss_mask"][1, 25:] = 0
    batch["phonemes"][2, 11:] = 0
    me = types.SimpleNamespace(_guide=(1.5, 0.2, [0, 2]), last_guided_attention=None)
    for n in (1, 2, 5):
        ctx = Trainer._guide_context(me, batch, 1.0 / n)
        assert ctx["coef"] == 1.5 * (1.0 / n) and ctx["scale"] is None
    ctx = Trainer._guide_context(me, batch, None)
    assert ctx["coef"] == 1.5 and ctx["scale"] is None and ctx["sigma"] == 0.2 and ctx["layers"] == [0, 2]
    assert ctx["n_frames"].dtype == torch.int32 and ctx["n_frames"].tolist() == [40, 25, 40] and ctx["n_keys"].tolist() == [20, 20, 11]
    assert ctx["out"].shape == (2, 4) and ctx["out"].dtype == torch.float64 and me.last_guided_attention is ctx["out"]
    word = torch.tensor(0.2)
    ctx = Trainer._guide_context(me, batch, word)
    assert ctx["coef"] == 1.5 and ctx["scale"] is word
