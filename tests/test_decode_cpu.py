"""CPU side of incremental generation: the float64 reference of the single-query kernels (tests/decode_ref.py) against the
full-window reference it must reproduce row by row, the split schedule's fold, the postnet-tail claim on the package's own
PostConvNet, and the host logic of ``model/incremental.py`` (refusals, loop arithmetic).  No GPU."""
import copy

import pytest
import torch

import decode_ref as D
import full_attn_ref as R
from oracle import model_ref

POSITIONS = (0, 1, 63, 64, 65, 191)


@pytest.fixture(scope="module")
def window():
    """qk, v (B, H, 192, 64) of bf16 values and the float64 causal full-window reference, computed once."""
    qk, v, do = R.make_inputs("plain", 2, 2, 192, seed=3)
    return qk.double(), v.double(), R.reference(qk, v, do, causal=True)


@pytest.mark.parametrize("p", POSITIONS)
def test_single_query_reference_is_row_p_of_the_full_window(window, p):
    qk, v, full = window
    one = D.self_attn(qk[:, :, p], v[:, :, p], qk, v, p)
    assert float((one["o"] - full["o"][:, :, p]).abs().max()) <= 1e-12
    assert float((one["b_o"] - full["b_o"][:, :, p]).abs().max()) <= 1e-12
    if p == 0:
        assert torch.equal(one["o"], v[:, :, 0])


@pytest.mark.parametrize("splits", [1, 2, 3, 5])
def test_split_fold_equals_the_unsplit_result(window, splits):
    """p = 5: every key sits in tile 0, so every split but the first is empty -- the fold must stay finite and exact."""
    qk, v, _ = window
    p = 5
    s = D.self_logits(qk[:, :, p], qk, p)
    vals = torch.cat([v[:, :, :p], v[:, :, p:p + 1]], dim=2)
    o, parts = D.split_fold(s, vals, splits, self_last=True)
    assert torch.isfinite(o).all()
    assert all(float(l.max()) == 0.0 and float(m.max()) == -D.FMAX for m, l, _ in parts[1:])
    assert float((o - D.self_attn(qk[:, :, p], v[:, :, p], qk, v, p)["o"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("splits", [2, 3])
def test_split_fold_over_several_tiles_and_skipped_keys(window, splits):
    """Round-robin tiles at p = 191 (three tiles), and the cross form with a split whose keys are all invalid."""
    qk, v, _ = window
    p = 191
    s = D.self_logits(qk[:, :, p], qk, p)
    vals = torch.cat([v[:, :, :p], v[:, :, p:p + 1]], dim=2)
    o, _ = D.split_fold(s, vals, splits, self_last=True)
    assert float((o - D.self_attn(qk[:, :, p], v[:, :, p], qk, v, p)["o"]).abs().max()) <= 1e-12
    valid = torch.ones(2, 192, dtype=torch.bool)
    valid[:, 64:128] = False                                          # tile 1: a split that receives only skipped keys (splits = 3)
    ref = D.cross_attn(qk[:, :, 0], qk, v, valid)
    o, _ = D.split_fold(D.cross_logits(qk[:, :, 0], qk, valid), v, splits, self_last=False)
    assert torch.isfinite(o).all() and float((o - ref["o"]).abs().max()) <= 1e-12


def _postnet(depth, seed):
    from reformer_tts_amd.model.modules import PostConvNet
    torch.manual_seed(seed)
    net = PostConvNet(mel_size=8, num_hidden=16, dropout=0.1, depth=depth).double().eval()
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(torch.randn(16, generator=g).double())
            m.running_var.copy_(torch.rand(16, generator=g).double() + 0.5)
    return net


def _prefix(net, mel):
    """The postnet as its own nn.Sequential defines it (Conv1d, BatchNorm1d, Tanh, Dropout on (B, C, L)), in float64: the module's
    ``forward`` rounds its operands to bf16 and cannot serve as a 1e-12 reference."""
    return net.layers(mel.transpose(1, 2)).transpose(1, 2)


@pytest.mark.parametrize("depth", [2, 4])
def test_postnet_tail_reproduces_the_prefix_result(depth):
    """The last output row of n = depth + 1 convolutions from the last 2 n + 1 mel rows: for every p in 0 ... 2 n + 3 the tail
    evaluation equals postnet(mel[:, :p + 1])[:, p] to 1e-12 (float64, the package's PostConvNet in eval mode)."""
    from reformer_tts_amd.model.incremental import postnet_tail_reference
    net = _postnet(depth, depth)
    n = depth + 1
    mel = torch.randn(2, 2 * n + 4, 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        for p in range(2 * n + 4):
            want = _prefix(net, mel[:, :p + 1])[:, p]
            got = postnet_tail_reference(net, mel, p)
            assert float((got - want).abs().max()) <= 1e-12, p
        # one row fewer is not enough: the window is tight
        p = 2 * n + 3
        short = mel.clone()
        short[:, p - 2 * n] = 0.0
        assert float((postnet_tail_reference(net, short, p) - _prefix(net, mel[:, :p + 1])[:, p]).abs().max()) > 1e-9
    assert D.postnet_tail_rows(n) == 2 * n + 1


# ---------------------------------------------------------------------------------------------------------- host logic
def _dense_cfg():
    cfg = model_ref.small_cfg()
    cfg["enc_reformer_kwargs"]["attn_kwargs"].update(implementation="hip", use_full_attn=True)
    cfg["dec_reformer_kwargs"]["self_attn_kwargs"].update(implementation="hip", use_full_attn=True)
    return cfg


def _model(cfg):
    from reformer_tts_amd.model.config import model_config_from_dict
    from reformer_tts_amd.training import build_model
    return build_model(model_config_from_dict(cfg))


def test_refusals_name_what_is_missing():
    from reformer_tts_amd.model.incremental import IncrementalDecoder, check_supported
    model = _model(_dense_cfg())
    check_supported(model, 2, 128, 128)                               # the supported configuration passes on the host
    with pytest.raises(NotImplementedError, match="batch"):
        check_supported(model, 129, 128, 128)
    with pytest.raises(NotImplementedError, match="capacity"):
        check_supported(model, 2, 4097, 128)
    with pytest.raises(NotImplementedError, match="encoder keys"):
        check_supported(model, 2, 128, 2176)
    lsh = copy.deepcopy(_dense_cfg())
    lsh["dec_reformer_kwargs"]["self_attn_kwargs"]["use_full_attn"] = False
    with pytest.raises(NotImplementedError, match="use_full_attn"):
        check_supported(_model(lsh), 2, 128, 128)
    hf = copy.deepcopy(_dense_cfg())
    hf["dec_reformer_kwargs"]["self_attn_kwargs"]["implementation"] = "huggingface_transformers"
    with pytest.raises(NotImplementedError, match="implementation"):
        check_supported(_model(hf), 2, 128, 128)
    odd = _model(_dense_cfg())
    for m in odd.dec.reformer.modules():
        if isinstance(m, torch.nn.MultiheadAttention):
            m.add_zero_attn = True
    with pytest.raises(NotImplementedError, match="XAttnExec.supported"):
        check_supported(odd, 2, 128, 128)
    drop = _model(_dense_cfg())
    for m in drop.dec.reformer.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    with pytest.raises(NotImplementedError, match="feed-forward"):
        check_supported(drop, 2, 128, 128)
    # the constructor refuses before it touches a device
    with pytest.raises(NotImplementedError, match="capacity"):
        IncrementalDecoder(model, torch.ones(2, 60, dtype=torch.long), 5000)


def test_replace_is_refused():
    model = _model(_dense_cfg())
    with pytest.raises(ValueError, match="concat"):
        model.infer(torch.ones(2, 60, dtype=torch.long), combine_strategy="replace", incremental=True)


@pytest.mark.parametrize("b,nm,max_len", [(2, 80, 90), (2, 80, 79), (2, 80, 80), (96, 80, 90), (1, 80, 1024), (12, 80, 1000), (3, 8, 1)])
def test_loop_arithmetic_is_the_graphed_loop(b, nm, max_len):
    """Frames and capacity against the guard of ``ReformerTTS._infer_graphed`` run on the host: ``cur`` starts at 1, every
    iteration appends a frame, ``max(b, cur, n_mels) > max_len`` ends the loop; the result holds cur - 1 frames."""
    from reformer_tts_amd.model.incremental import generation_plan
    cur, its = 1, 0
    while True:
        its += 1
        cur += 1
        if max(b, cur, nm) > max_len:
            break
    steps, cap = generation_plan(b, nm, max_len)
    assert steps == its == cur - 1
    assert cap % 64 == 0 and steps <= cap < steps + 64
