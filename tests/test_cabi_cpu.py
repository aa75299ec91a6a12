"""CPU-side checks: the C-ABI library loads and exports every symbol include/rtts.h declares
(no compute calls without a GPU), and the C twin of the integer stages agrees with the PyTorch
restatement and with HuggingFace's fixtures."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import lsh_int, lsh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "rtts.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rtts_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    lib = _lib.load()
    syms = _header_symbols()
    assert len(syms) >= 8
    for s in syms:
        assert hasattr(lib, s), s
    assert set(_lib.SIGNATURES) <= set(syms)
    assert lib.rtts_version() == 1


def test_library_sources_read_no_environment():
    """the library reads no environment variable, on a launch path or anywhere else -- test-only choices
    arrive through the rtts_debug_set_* exports."""
    csrc = os.path.join(ROOT, "reformer-tts_amd", "csrc")
    files = sorted(os.listdir(csrc))
    assert len(files) >= 20
    assert [f for f in files if "getenv" in open(os.path.join(csrc, f)).read()] == []


def test_debug_setters_refuse_what_they_do_not_know():
    """Host-only calls: rtts_debug_set_gemm_tn_tiles takes 0 and 1; rtts_debug_set_gemm_mode no longer takes the launch forms
    0..3 (it keeps 9..12 and 20..22).  A refusal returns -1 and leaves a message that names the value."""
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    lib = _lib.load()
    try:
        assert lib.rtts_debug_set_gemm_tn_tiles(1) == 0
        assert lib.rtts_debug_set_gemm_tn_tiles(0) == 0
        for bad in (2, -1):
            assert lib.rtts_debug_set_gemm_tn_tiles(bad) == -1
            msg = lib.rtts_last_error().decode()
            assert "rtts_debug_set_gemm_tn_tiles" in msg and f"got {bad}" in msg
        with pytest.raises(_lib.RttsError, match="rtts_debug_set_gemm_tn_tiles"):
            _lib.call("rtts_debug_set_gemm_tn_tiles", 2)
        for mode in (0, 1, 2, 3):
            assert lib.rtts_debug_set_gemm_mode(mode) == -1
            msg = lib.rtts_last_error().decode()
            assert "rtts_debug_set_gemm_mode" in msg and f"got {mode}" in msg
        for mode in (10, 11, 12, 9, 21, 22, 20):
            assert lib.rtts_debug_set_gemm_mode(mode) == 0
    finally:
        lib.rtts_debug_set_gemm_tn_tiles(0)
        lib.rtts_debug_set_gemm_mode(9)
        lib.rtts_debug_set_gemm_mode(20)


def test_missing_library_fails_loudly(monkeypatch):
    from reformer_tts_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/librtts_hip.so")
    with pytest.raises(_lib.RttsError, match="no CPU fallback"):
        _lib.load()


@pytest.mark.parametrize("bh,t,bs,nh,per_head", [(3, 256, 64, 4, False), (2, 1024, 128, 8, True), (2, 512, 64, 2, False)])
def test_c_twin_vs_pytorch_restatement(bh, t, bs, nh, per_head):
    g = torch.Generator().manual_seed(t + nh)
    qk = torch.randn(bh, t, 64, generator=g).bfloat16().float()
    rot = torch.randn(bh if per_head else 1, 64, nh, t // bs // 2, generator=g)
    b_c = lsh_int.hash_buckets(qk.numpy(), rot.numpy())
    b_t = lsh_ref.hash_vectors(qk, rot).reshape(bh, nh, t).numpy()
    assert (b_c != b_t).mean() < 1e-3          # only exact near-ties may differ (einsum order)
    st_c, undo_c = lsh_int.sort_buckets(b_c, t // bs)
    sticker, undo = lsh_ref.sort_buckets(torch.from_numpy(b_c.reshape(bh, nh * t).astype(np.int64)), t)
    assert np.array_equal(st_c.reshape(bh, -1), (sticker % t).numpy())
    flat_undo = undo_c + (np.arange(nh, dtype=np.int32) * t)[None, :, None]
    assert np.array_equal(flat_undo.reshape(bh, -1), undo.numpy())


def test_c_twin_vs_huggingface_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "hf_lsh_int.npz"))
    for tag in ("a", "b", "c"):
        heads, t, dh, chunk, nh = (int(x) for x in z[f"{tag}/meta"])
        vec = np.random.RandomState(5).standard_normal((2, heads, t, dh)).astype(np.float32)
        rot = np.tile(z[f"{tag}/rot"], (2, 1, 1, 1))
        buckets = lsh_int.hash_buckets(vec.reshape(2 * heads, t, dh), rot)
        exp = z[f"{tag}/buckets"].astype(np.int32).reshape(2 * heads, nh, t)
        assert (buckets != exp).mean() < 1e-4, tag
        st, _ = lsh_int.sort_buckets(exp, t // chunk)
        exp_sorted = z[f"{tag}/sorted_idx"].astype(np.int32).reshape(2 * heads, nh, t) % t
        assert np.array_equal(st, exp_sorted), tag


def test_model_refuses_to_run_off_the_gpu():
    """No CPU fallback: a forward (or generation) on a CPU-resident model raises the library's own error at the door."""
    import torch
    from reformer_tts_amd import _lib
    from reformer_tts_amd.model.config import baseline_model_config
    from reformer_tts_amd.training import build_model, synthetic_batch
    cfg = baseline_model_config()
    cfg.enc_reformer_kwargs.depth = 1
    cfg.dec_reformer_kwargs.depth = 1
    model = build_model(cfg)
    batch = synthetic_batch(1, 20, 256)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model(batch["phonemes"], batch["spectrogram"][:, :-1])
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model.infer(batch["phonemes"], max_len=90)


def test_row_kernel_widths_are_all_tested():
    """tests/test_rows_hip.py's WIDTHS is exactly the width list of FR_DISPATCH_D in csrc/fused_rows.hip: a width added to the
    dispatch without its tests fails here."""
    src = open(os.path.join(ROOT, "reformer-tts_amd", "csrc", "fused_rows.hip")).read()
    body = re.search(r"#define FR_DISPATCH_D\(d, CALL\)(.*?)default:", src, flags=re.S).group(1)
    widths = tuple(int(w) for w in re.findall(r"case (\d+):", body))
    tests = open(os.path.join(ROOT, "tests", "test_rows_hip.py")).read()
    listed = re.search(r"^WIDTHS = \(([^)]*)\)", tests, flags=re.M).group(1)
    assert widths and tuple(int(w) for w in listed.split(",") if w.strip()) == widths
