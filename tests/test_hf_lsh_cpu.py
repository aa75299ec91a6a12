"""HuggingFace's LSH layer on the host: the numpy restatement of its integer stages (tests/hf_lsh_ref.py) against the goldens
that ``transformers``' own ``LSHSelfAttention`` produced (tests/golden/hf_lsh_attn.npz), and the module surface of
``implementation="huggingface_transformers"`` (class, parameter names, envelopes).  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import hf_lsh_ref as ref


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "hf_lsh_attn.npz"))


def _meta(z, tag):
    b, h, t, chunk, r, causal, nb, seed = (int(v) for v in z[f"{tag}/meta"])
    return b, h, t, chunk, r, bool(causal), nb, seed


def test_fixture_cases_and_inputs(golden):
    """The fixture holds the cases of hf_lsh_ref.CASES, and the inputs that case_inputs() regenerates are the ones it was made
    from (they are not stored: see tests/golden/make_hf_lsh_golden.py)."""
    for tag, (b, h, t, chunk, r, causal, lengths, seed) in ref.CASES.items():
        assert _meta(golden, tag) == (b, h, t, chunk, r, causal, ref.num_buckets(t, chunk), seed)
        inp = ref.case_inputs(tag)
        assert np.array_equal(ref.inputs_digest(inp), golden[f"{tag}/input_sha256"]), tag
        stored_mask = golden[f"{tag}/mask"]
        assert (inp["mask"] is None and stored_mask.shape == (0, t)) or np.array_equal(stored_mask.astype(bool), inp["mask"])
        for k in ("x", "wqk", "wv", "dout"):
            assert np.array_equal(ref.bf16_round(inp[k]), inp[k]), (tag, k)            # bf16-representable
        if inp["mask"] is not None:
            assert not inp["mask"].all() and not inp["dout"][~inp["mask"]].any()         # masks something; no gradient there
        assert np.array_equal(golden[f"{tag}/rows"], ref.stored_rows(t))
    assert {t for t in "abcd"} == set(ref.CASES)
    assert [_meta(golden, t)[6] for t in "abcd"] == [8, 16, 16, 8]                       # 384 / 64 = 6 chunks -> 8 buckets
    assert int(golden["a/buckets"].max()) == 3 * 9 + 8 and int(golden["b/buckets"].max()) == 3 * 17 + 16     # the padding bucket


def test_bucket_count_and_limit():
    assert [ref.num_buckets(t, c) for t, c in ((256, 64), (512, 64), (1024, 128), (384, 64), (4096, 64), (768, 128))] == \
        [8, 16, 16, 8, 128, 8]
    assert ref.bucket_limit(64) == 128 and ref.bucket_limit(128) == 256


@pytest.mark.parametrize("tag", list(ref.CASES))
def test_restated_hash_vs_huggingface(golden, tag):
    """Buckets of the restatement on the bf16-rounded projection (what the device hashes) against HuggingFace's, which hashed
    the fp32 projection: rounding may move near-ties only -- the cap tests/test_lsh_hip.py::test_hash_sort_vs_huggingface_fixture
    uses for the same cause."""
    b, h, t, chunk, r, causal, nb, seed = _meta(golden, tag)
    inp = ref.case_inputs(tag)
    qk = ref.bf16_round(inp["x"].reshape(b * t, -1) @ inp["wqk"].T).reshape(b, t, -1)
    got = ref.hash_buckets(ref.heads_first(qk, h), golden[f"{tag}/rot"], inp["mask"], nb)
    exp = golden[f"{tag}/buckets"].astype(np.int32).reshape(b * h, r, t)
    share = float((got != exp).mean())
    print(f"\n[hf hash {tag}] mismatching share {share:.2e} (cap 2e-2)")
    assert share < 2e-2
    stride = nb + (inp["mask"] is not None)
    assert got.max() < r * stride and got.min() >= 0
    if inp["mask"] is not None:                      # masked tokens: the padding bucket of their round, exactly
        pad = (np.arange(r) * stride + nb)[None, :, None]
        m = np.repeat(~inp["mask"], h, axis=0)[:, None, :]
        assert np.array_equal(got == pad, np.broadcast_to(m, got.shape))


@pytest.mark.parametrize("tag", list(ref.CASES))
def test_restated_sort_equals_huggingface(golden, tag):
    """Given HuggingFace's own buckets, the stable counting sort is its ``sorted_bucket_idx % T`` exactly."""
    b, h, t, chunk, r, causal, nb, seed = _meta(golden, tag)
    buckets = golden[f"{tag}/buckets"].astype(np.int32).reshape(b * h, r, t)
    stride = nb + (ref.CASES[tag][6] is not None)
    st, undo = ref.sort_buckets(buckets, stride)
    assert np.array_equal(st, golden[f"{tag}/sorted_idx"].astype(np.int32).reshape(b * h, r, t))
    assert np.array_equal(np.take_along_axis(st, undo, axis=-1), np.broadcast_to(np.arange(t), st.shape))


def test_wrapper_builds_the_huggingface_class():
    from reformer_tts_amd.model.hf_lsh_attention import HFLSHSelfAttention
    from reformer_tts_amd.model.lsh_attention import LSHSelfAttention
    from reformer_tts_amd.model.reformer import LSHSelfAttentionWrapper
    from reformer_tts_amd.model.config import LSHSelfAttentionConfig
    from dataclasses import asdict
    kw = asdict(LSHSelfAttentionConfig(implementation="huggingface_transformers", heads=2, bucket_size=128, n_hashes=4, dropout=0.1,
                                       post_attn_dropout=0.15, add_local_attn_hash=True, num_mem_kv=3, use_full_attn=True))
    w = LSHSelfAttentionWrapper(128, causal=True, **kw)      # knobs the hip branch refuses are ignored here, as in the reference
    lyr = w.layer
    assert type(lyr) is HFLSHSelfAttention and w.implementation == "huggingface_transformers"
    assert (lyr.heads, lyr.bucket_size, lyr.n_hashes, lyr.causal, lyr.dropout) == (2, 128, 4, True, 0.1)
    assert lyr.num_buckets is None
    # the other two values behave as before
    assert type(LSHSelfAttentionWrapper(128, causal=False, implementation="hip", heads=2).layer) is LSHSelfAttention
    with pytest.raises(NotImplementedError):
        LSHSelfAttentionWrapper(128, causal=False, implementation="reformer_pytorch", heads=2)
    with pytest.raises(NotImplementedError, match="add_local_attn_hash"):
        LSHSelfAttentionWrapper(128, causal=False, implementation="hip", heads=2, add_local_attn_hash=True)


def test_state_dict_names_are_huggingfaces():
    from reformer_tts_amd.model.reformer import LSHSelfAttentionWrapper
    w = LSHSelfAttentionWrapper(128, causal=False, implementation="huggingface_transformers", heads=2, bucket_size=64, n_hashes=2,
                                dropout=0.0)
    sd = w.state_dict()
    assert list(sd) == ["layer.query_key.weight", "layer.value.weight"]
    assert all(tuple(v.shape) == (128, 128) for v in sd.values())
    if importlib.util.find_spec("transformers") is not None:
        from transformers import ReformerConfig
        from transformers.models.reformer.modeling_reformer import LSHSelfAttention as HF
        hf = HF(ReformerConfig(hidden_size=128, num_attention_heads=2, attention_head_size=64, num_hashes=2, lsh_attn_chunk_length=64))
        assert list(hf.state_dict()) == [k[len("layer."):] for k in sd]
        w.layer.load_state_dict(hf.state_dict())


def test_bucket_count_is_sticky_and_envelopes_raise():
    from reformer_tts_amd.model.hf_lsh_attention import HFLSHSelfAttention
    lyr = HFLSHSelfAttention(128, heads=2, bucket_size=64, n_hashes=2)
    assert lyr.resolve_num_buckets(384) == 8 and lyr.num_buckets == 8
    assert lyr.resolve_num_buckets(4096) == 8                                   # sticky: the layer keeps the first count
    assert HFLSHSelfAttention(128, heads=2, bucket_size=64, n_hashes=2, num_buckets=32).resolve_num_buckets(256) == 32
    assert HFLSHSelfAttention(128, heads=2, bucket_size=64, n_hashes=2).resolve_num_buckets(4096) == 128       # the limit itself
    # the factorised hash: 2 * (8192 // 64) = 256 buckets > 2 * max(int(sqrt(4096 // 64)), 64) = 128
    with pytest.raises(NotImplementedError, match="limit of 128"):
        HFLSHSelfAttention(128, heads=2, bucket_size=64, n_hashes=2).resolve_num_buckets(8192)
    with pytest.raises(NotImplementedError, match="256 buckets"):
        HFLSHSelfAttention(128, heads=2, bucket_size=64, n_hashes=2, num_buckets=258)
    with pytest.raises(AssertionError, match="even number of buckets"):
        HFLSHSelfAttention(128, heads=2, bucket_size=64, n_hashes=2, num_buckets=7)
    # T <= chunk is HuggingFace's dense attention: outside this path (raised before anything touches a device)
    for t in (64, 32):
        with pytest.raises(NotImplementedError, match="dense attention"):
            lyr.forward(torch.zeros(1, t, 128))
    with pytest.raises(AssertionError, match="divisible by the chunk length"):
        lyr.forward(torch.zeros(1, 96, 128))


def test_huggingface_lsh_config_builds_the_model():
    """The model section of the reference's config/huggingface-lsh.yml: 3 + 3 layers of the new class, decoder chunks of 128."""
    from reformer_tts_amd.model.config import as_kwargs, huggingface_lsh_model_config
    from reformer_tts_amd.model.hf_lsh_attention import HFLSHSelfAttention
    from reformer_tts_amd.model.reformer_tts import ReformerTTS
    model = ReformerTTS(**as_kwargs(huggingface_lsh_model_config()))
    layers = [m for m in model.modules() if isinstance(m, HFLSHSelfAttention)]
    assert [(m.bucket_size, m.causal) for m in layers] == [(64, False)] * 3 + [(128, True)] * 3
    names = [n for n, _ in model.named_parameters() if ".layer.query_key." in n or ".layer.value." in n]
    assert len(names) == 12 and not any("toqk" in n or "to_out" in n for n, _ in model.named_parameters())


def test_regenerating_a_case_reproduces_the_fixture(golden):
    """With ``transformers`` importable, the generator script's output for one case is the stored one."""
    if importlib.util.find_spec("transformers") is None:
        pytest.skip("transformers is not installed: the fixture cannot be regenerated here")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_hf_lsh_golden.py")
    spec = importlib.util.spec_from_file_location("_make_hf_lsh_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    state = torch.random.get_rng_state()           # run_case seeds the default generator
    try:
        got = mod.run_case("d")
    finally:
        torch.random.set_rng_state(state)
    for k in ("meta", "rot", "buckets", "sorted_idx", "rows", "mask", "input_sha256"):
        assert np.array_equal(got[k], golden[f"d/{k}"]), k
    for k in ("out", "dx", "dwqk", "dwv"):         # fp32 reductions may be blocked differently on another host: a few fp16 ulps
        np.testing.assert_allclose(got[k].astype(np.float32), golden[f"d/{k}"].astype(np.float32), rtol=4e-3, atol=1e-4, err_msg=k)
