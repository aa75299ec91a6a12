"""The width-parametrised cross-attention oracle of tests/xattn_wide_ref.py checked without a GPU: against float64
nn.MultiheadAttention with 128-wide heads (output, gradients and head-averaged weights), against tests/xattn_ref.py at dh = 64
(exact), its error bounds against an fp32 / bf16 model of the DH = 128 kernels' data flow (inside every bound on every input
kind; each deliberate defect breaks one), and the executor's envelope: a decoder stack whose cross-attention has 128-wide heads
gets a program from ``engine.build_program``."""
import functools

import pytest
import torch

import xattn_ref as X
import xattn_wide_ref as W


def _rel(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("tk", [128, 384])
def test_reference_equals_multihead_attention_with_128_wide_heads(tk):
    """float64 nn.MultiheadAttention(embed 256, num_heads 2) with random in/out projections and biases, key_padding_mask from
    make_valid('ragged'), need_weights=True.  The oracle gets the module's projected q, k, v and the gradient of its attention
    output; its o, dq, dk, dv are compared through the module's own (random, full-rank) projections: out = o W_o^T + b_o,
    d x_q = dq W_q, d x_k = dk W_k, d x_v = dv W_v.  Relative 1e-12."""
    nb, nh, tq, dh = 2, 2, 128, 128
    e = nh * dh
    g = torch.Generator().manual_seed(tk)
    mha = torch.nn.MultiheadAttention(e, nh, bias=True, batch_first=True).double().train()
    with torch.no_grad():
        for p in mha.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / (16.0 if p.dim() == 2 else 1.0))
    xq, xk, xv = (torch.randn(nb, t, e, generator=g, dtype=torch.float64).requires_grad_() for t in (tq, tk, tk))
    dout = torch.randn(nb, tq, e, generator=g, dtype=torch.float64)
    valid = X.make_valid("ragged", nb, tk)
    out, weights = mha(xq, xk, xv, key_padding_mask=~valid, need_weights=True)
    out.backward(dout)
    wq, wk, wv = mha.in_proj_weight.detach().split(e)
    bq, bk, bv = mha.in_proj_bias.detach().split(e)
    wo, bo = mha.out_proj.weight.detach(), mha.out_proj.bias.detach()
    heads = lambda x: x.view(nb, -1, nh, dh).transpose(1, 2)
    flat = lambda x: x.transpose(1, 2).reshape(nb, -1, e)
    q, k, v = heads(xq.detach() @ wq.t() + bq), heads(xk.detach() @ wk.t() + bk), heads(xv.detach() @ wv.t() + bv)
    ref = W.reference(q, k, v, heads(dout @ wo), valid, None, dh)
    errs = dict(o=_rel(flat(ref["o"]) @ wo.t() + bo, out.detach()), dq=_rel(flat(ref["dq"]) @ wq, xq.grad),
                dk=_rel(flat(ref["dk"]) @ wk, xk.grad), dv=_rel(flat(ref["dv"]) @ wv, xv.grad),
                weights=_rel(ref["p_mean"], weights.detach()))
    print(f"\n[reference dh=128] vs nn.MultiheadAttention, {tk} keys: " + " ".join(f"{n} {x:.1e}" for n, x in errs.items()) + " (tol 1e-12)")
    assert max(errs.values()) <= 1e-12
    assert float(ref["p_mean"][~valid.view(nb, 1, tk).expand(nb, tq, tk)].abs().max()) == 0.0


@pytest.mark.parametrize("kind,tk,pattern,drop", [("plain", 128, "ragged", None), ("peaked", 384, "middle", (0.5, 77, 3)),
                                                  ("offset-", 512, "alternating", None)])
def test_reference_at_width_64_is_xattn_ref_exactly(kind, tk, pattern, drop):
    nb, nh, tq = 2, 2, 128
    inputs = X.make_inputs(kind, nb, nh, tq, tk, seed=tk)
    for a, b in zip(inputs, W.make_inputs(kind, nb, nh, tq, tk, seed=tk, dh=64)):
        assert torch.equal(a, b)
    valid = X.make_valid(pattern, nb, tk)
    keep = None if drop is None else X.keep_scales(*drop, nb * nh, tq, tk).view(nb, nh, tq, tk)
    old, new = X.reference(*inputs, valid, keep), W.reference(*inputs, valid, keep, 64)
    for n, x in old.items():
        assert torch.equal(x, new[n]), n
    assert W.bwd_chunk(tk, 64) == W.fwd_chunk(tk, 64) == X.key_chunk(tk)


# (T_k, kvalid pattern) at dh = 128: 1, 2, 3, 4 and 16 backward chunks; the forward holds 256 keys only at T_k = 256
TK_PATTERNS = [(128, "ragged"), (256, "alternating"), (384, "first"), (512, "one"), (2048, "middle")]
DROPS = (None, (0.5, 77, 3), (0.15, 77, None))


@functools.lru_cache(maxsize=None)
def _model_ratios(kind, tk, pattern, drop, defect=None):
    nb, nh, tq, dh = 2, 1, 256, 128
    inputs = W.make_inputs(kind, nb, nh, tq, tk, seed=tk + tq, dh=dh)
    valid = X.make_valid(pattern, nb, tk)
    keep = None if drop is None else X.keep_scales(*drop, nb * nh, tq, tk).view(nb, nh, tq, tk)
    ref = W.reference(*inputs, valid, keep, dh)
    got = W.kernel_model(*inputs, valid, drop, defect, dh)
    r = X.ratios(got, ref)
    r["lse"] = X.lse_ratio(got["lse"], ref)
    return r


@pytest.mark.parametrize("kind", W.KINDS)
def test_kernel_model_stays_within_every_bound(kind):
    """Without a defect the fp32 / bf16 model of the DH = 128 kernels is inside every bound on all four input kinds, at every
    chunk count and dropout rate above."""
    worst = dict(o=0.0, dq=0.0, dk=0.0, dv=0.0, lse=0.0)
    for tk, pattern in TK_PATTERNS:
        for drop in DROPS:
            r = _model_ratios(kind, tk, pattern, drop)
            worst = {n: max(worst[n], r[n]) for n in worst}
            assert max(r[n] for n in ("o", "dq", "dk", "dv")) <= 1.0, (tk, pattern, drop, r)
    print(f"\n[model dh=128] {kind}: worst |model - float64| / bound over {len(TK_PATTERNS) * len(DROPS)} cases: "
          + " ".join(f"{n} {x:.3f}" for n, x in worst.items()))
    assert worst["lse"] <= 4.0


@pytest.mark.parametrize("tk", [256, 384])
@pytest.mark.parametrize("defect", W.DEFECTS)
def test_each_defect_breaks_a_bound(defect, tk):
    """The mistakes a second head width invites -- the 64 kernels' 1 / 8 kept as the scale, the second 64 columns of a head
    missing from delta, one 128-key chunk's dQ share dropped -- each FAIL a bound at 2 and 3 backward chunks (peaked inputs,
    ragged padding, dropout 0.5; the same case passes without the defect)."""
    clean = _model_ratios("peaked", tk, "ragged", (0.5, 77, 3))
    r = _model_ratios("peaked", tk, "ragged", (0.5, 77, 3), defect)
    broken = [n for n in ("o", "dq", "dk", "dv") if not r[n] <= 1.0]
    print(f"\n[defect {defect}] {tk} keys: " + " ".join(f"{n} {x:.3g}" for n, x in r.items()) + f" -> breaks {broken}")
    assert max(clean[n] for n in ("o", "dq", "dk", "dv")) <= 1.0
    assert broken, f"defect ({defect}) passes every bound at {tk} keys: {r}"


def test_decoder_with_128_wide_cross_attention_heads_gets_a_program():
    """embedding_dim 256, LSH heads 4 (dh 64), cross-attention num_heads 2 (dh 128): the decoder stack is translated into
    executor steps.  num_heads 8 (dh 32) still is not."""
    from oracle import model_ref
    from reformer_tts_amd import engine
    from reformer_tts_amd.model.config import model_config_from_dict
    from reformer_tts_amd.training import build_model

    def stack(num_heads):
        cfg = model_ref.small_cfg()
        cfg["embedding_dim"] = 256
        for kw in (cfg["enc_reformer_kwargs"]["attn_kwargs"], cfg["dec_reformer_kwargs"]["self_attn_kwargs"]):
            kw.update(implementation="hip", heads=4)
        cfg["dec_reformer_kwargs"]["attn_kwargs"]["num_heads"] = num_heads
        return build_model(model_config_from_dict(cfg)).dec.reformer.layers

    prog = engine.build_program(stack(2))
    assert prog is not None and any(isinstance(ex, engine.XAttnExec) for step in prog for ex in step[1:3])
    assert engine.build_program(stack(4)) is not None
    assert engine.build_program(stack(8)) is None
