"""Dense shared-QK attention without a GPU: the float64 definition of tests/full_attn_ref.py against the LSH oracle it must
agree with, its hand-written backward against autograd, the fp32 model of csrc/full_attn.hip against the error bounds (and
every named defect beyond them), and the layer's constructor surface."""
import pytest
import torch

import full_attn_ref as ref
from oracle import lsh_ref


@pytest.mark.parametrize("mask_kind", ["none", "ragged", "hole"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("t", [64, 128, 256])
def test_reference_equals_lsh_oracle_on_valid_rows(t, causal, mask_kind):
    """One hash round with two buckets of T/2 shows every query all T keys (own chunk + the previous one), whatever the
    permutation: on valid rows the dense function IS the LSH function; on rows of masked queries it is mean(v), not v_i."""
    nb, nh = 2, 2
    qk, v, do = (x.double() for x in ref.make_inputs("plain", nb, nh, t, seed=t + causal))
    mask = ref.make_mask(mask_kind, nb, t)
    r = ref.reference(qk, v, do, mask, causal)
    g = torch.Generator().manual_seed(7 * t)
    sticker = torch.stack([torch.randperm(t, generator=g) for _ in range(nb * nh)])
    undo = torch.empty_like(sticker)
    undo.scatter_(-1, sticker, torch.arange(t).expand_as(sticker))
    m_bh = None if mask is None else mask[:, None, :].expand(nb, nh, t).reshape(nb * nh, t)
    out = lsh_ref.lsh_attention_sorted(qk.reshape(nb * nh, t, 64), v.reshape(nb * nh, t, 64), sticker, undo, t // 2, 1, causal, m_bh)
    out = out.view(nb, nh, t, 64)
    valid = torch.ones(nb, t, dtype=torch.bool) if mask is None else mask
    sel = valid[:, None, :, None].expand_as(out)
    assert float((out - r["o"])[sel].abs().max()) <= 1e-12
    if mask is not None:
        inv = ~sel
        mean_v = v.mean(dim=2, keepdim=True).expand_as(out)
        assert float((r["o"] - mean_v)[inv].abs().max()) <= 1e-12
        assert float((out - v)[inv].abs().max()) <= 1e-12                    # the LSH path's own answer there
        assert bool((r["lse"][(~valid)[:, None, :].expand(nb, nh, t)] == -ref.FMAX).all())


@pytest.mark.parametrize("drop", [None, (0.3, 1234, 5)])
@pytest.mark.parametrize("mask_kind", ["none", "hole", "one"])
@pytest.mark.parametrize("causal", [False, True])
def test_backward_matches_autograd(causal, mask_kind, drop):
    nb, nh, t = 2, 2, 64
    qk, v, do = (x.double() for x in ref.make_inputs("plain", nb, nh, t, seed=3))
    mask = ref.make_mask(mask_kind, nb, t)
    keep = None if drop is None else ref.keep_scales(*drop, nb * nh, t).view(nb, nh, t, t)
    r = ref.reference(qk, v, do, mask, causal, keep)
    qa, va = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    o = ref.forward_autograd(qa, va, mask, causal, keep)
    o.backward(do)
    assert float((o.detach() - r["o"]).abs().max()) <= 1e-13
    scale = float(qa.grad.abs().max()) + 1.0
    assert float((qa.grad - r["dqk"]).abs().max()) <= 1e-12 * scale
    assert float((va.grad - r["dv"]).abs().max()) <= 1e-12


def test_edge_rows_of_the_reference():
    """Causal row 0 keeps only its -5e4 diagonal: lse = -5e4, o = v_0; a masked query's dout reaches dv of every key and no dqk."""
    nb, nh, t = 1, 1, 64
    qk, v, do = (x.double() for x in ref.make_inputs("plain", nb, nh, t, seed=5))
    r = ref.reference(qk, v, do, None, True)
    assert float(r["lse"][0, 0, 0]) == -5e4 and torch.equal(r["o"][0, 0, 0], v[0, 0, 0])
    mask = torch.ones(nb, t, dtype=torch.bool)
    mask[0, 9] = False
    do1 = torch.zeros_like(do)
    do1[0, 0, 9] = do[0, 0, 9]
    r = ref.reference(qk, v, do1, mask, True)
    assert float(r["dqk"].abs().max()) == 0.0
    assert float((r["dv"][0, 0] - do1[0, 0, 9] / t).abs().max()) <= 1e-15


MODEL_CASES = [(2, 2, 128, k, c, m, d) for k in ref.KINDS for c in (False, True) for m in ref.MASKS
               for d in (None, (0.1, 99, None))] + [(1, 2, 192, "plain", True, "hole", (0.5, 7, 11))]


@pytest.fixture(scope="module")
def model_worst():
    return {"lse": 0.0, "o": 0.0, "dqk": 0.0, "dv": 0.0}


@pytest.mark.parametrize("nb,nh,t,kind,causal,mask_kind,drop", MODEL_CASES)
def test_kernel_model_within_bounds(nb, nh, t, kind, causal, mask_kind, drop, model_worst):
    qk, v, do = ref.make_inputs(kind, nb, nh, t, seed=11)
    mask = ref.make_mask(mask_kind, nb, t)
    keep = None if drop is None else ref.keep_scales(*drop, nb * nh, t).view(nb, nh, t, t)
    r = ref.reference(qk, v, do, mask, causal, keep)
    got = ref.kernel_model(qk, v, do, mask, causal, drop)
    rat = ref.ratios(got, r)
    c = ref.lse_ratio(got["lse"], r, mask)
    for n, x in list(rat.items()) + [("lse", c)]:
        model_worst[n] = max(model_worst[n], x)
    print(f"ratios {rat} lse C {c:.2f} (worst so far {model_worst})")
    assert all(x <= 1.0 for x in rat.values()), rat
    assert c <= ref_lse_c_model()
    if mask is not None:
        inv = (~mask)[:, None, :].expand(nb, nh, t)
        assert bool((got["lse"][inv] == -ref.FMAX).all())


def ref_lse_c_model() -> float:
    """What the fp32 model may need of the lse bound's constant: the logit is one fp32 product of a 64-term fp32 dot (the bf16
    products are exact) and a column scale good to ~2 ulp, lse adds a max, an exp, a sum of T terms and a log -- a handful of
    2^-24 relative steps on |s| and |lse|.  8 covers the model; the GPU test allows 4 x that."""
    return 8.0


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_every_defect_breaks_a_bound(defect):
    nb, nh, t = 2, 2, 192
    qk, v, do = ref.make_inputs("plain", nb, nh, t, seed=13)
    mask = ref.make_mask("hole", nb, t)
    r = ref.reference(qk, v, do, mask, True)
    assert max(ref.ratios(ref.kernel_model(qk, v, do, mask, True), r).values()) <= 1.0
    rat = ref.ratios(ref.kernel_model(qk, v, do, mask, True, defect=defect), r)
    assert not all(x <= 1.0 for x in rat.values()), (defect, rat)          # NaN counts as broken


def test_keep_twin_rate_and_seed_dev():
    k = ref.keep_scales(0.5, 1, None, 4, 128)
    assert abs(float((k == 0).double().mean()) - 0.5) < 0.01 and float(k.max()) == 2.0
    assert torch.equal(ref.keep_scales(0.1, 10, 5, 2, 64), ref.keep_scales(0.1, 15, None, 2, 64))


def test_layer_constructs_with_use_full_attn():
    from reformer_tts_amd.model.lsh_attention import LSHSelfAttention
    from reformer_tts_amd.model.reformer import LSHSelfAttentionWrapper
    w = LSHSelfAttentionWrapper(128, causal=True, implementation="hip", heads=2, use_full_attn=True)
    assert type(w.layer) is LSHSelfAttention and w.layer.use_full_attn
    assert w.layer.dense(4096) and w.layer.dense(64)
    thr = LSHSelfAttentionWrapper(128, causal=False, implementation="hip", heads=2, bucket_size=64, full_attn_thres=256).layer
    assert thr.dense(256) and not thr.dense(512)
    assert not LSHSelfAttentionWrapper(128, causal=False, implementation="hip", heads=2, bucket_size=64).layer.dense(128)


def test_other_knobs_are_still_refused():
    from reformer_tts_amd.model.reformer import LSHSelfAttentionWrapper
    for knob in (dict(add_local_attn_hash=True), dict(num_mem_kv=2), dict(one_value_head=True), dict(return_attn=True),
                 dict(attend_across_buckets=False), dict(allow_duplicate_attention=False)):
        with pytest.raises(NotImplementedError, match=next(iter(knob))):
            LSHSelfAttentionWrapper(128, causal=False, implementation="hip", heads=2, use_full_attn=True, **knob)
