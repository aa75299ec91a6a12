"""The device factorisation of the invertible 1x1 convolutions, checked without a GPU: the numpy restatement of the kernel's
algorithm (tests/sw_lu_ref.py) meets the bounds of the GPU test on the GPU test's matrices -- the inputs are fair for the
reference alone --, the C ABI declares and exports the entry point, and ``VocoderTrainer.capture`` refuses what it cannot do."""
import os
import re

import numpy as np
import pytest
import torch

import sw_lu_ref as lu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind,n", lu.CASES)
def test_restatement_meets_the_bounds(kind, n):
    w = lu.matrix(kind, n)
    inv, sign, logabs = lu.factor(w)
    same_sign, r_ld, r_inv, rsign = lu.ratios(inv, sign, logabs, w)
    print(kind, n, "sign", sign, "log-det ratio", r_ld, "inverse ratio", r_inv)
    assert same_sign and r_ld <= 1 and r_inv <= 1
    if kind == "pivoting":
        assert rsign == -1 and np.all(np.diag(w) == 0)
    if kind == "kappa1e5" and n > 1:
        assert 5e4 < np.linalg.cond(w.astype(np.float64)) < 2e5


def test_restatement_rounds_like_lapack():
    """Nearly every element of the restatement's inverse is the fp32 rounding of LAPACK's float64 inverse."""
    w = lu.matrix("orthonormal", 128)
    inv, _, _ = lu.factor(w)
    want = np.linalg.inv(w.astype(np.float64)).astype(np.float32)
    assert np.mean(inv == want) > 0.999


def test_restatement_singular_and_ties():
    inv, sign, logabs = lu.factor(lu.singular(48))
    assert sign == 0 and logabs == -np.inf and np.isnan(inv).all()
    # a tie in the first column: rows 0 and 2 both hold the largest |a|; the lowest row wins, so no exchange happens
    w = np.array([[2, 1, 0], [1, 3, 1], [-2, 0, 4]], dtype=np.float32)
    inv, sign, logabs = lu.factor(w)
    rsign, rlog = np.linalg.slogdet(w.astype(np.float64))
    assert sign == rsign and abs(logabs - rlog) < 1e-14
    assert np.allclose(inv.astype(np.float64) @ w, np.eye(3), atol=1e-6)


def test_header_declares_and_library_exports_the_entry_point():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtts.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+rtts_sw_inv1x1_factor\s*\(const float\* const\* w, const int\* n, int count,\s*float\* const\* winv, "
                     r"double\* slogdet, void\* stream\)", text)
    assert "rtts_sw_inv1x1_factor" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "rtts_sw_inv1x1_factor")


def _cpu_model():
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    return SqueezeWave(4, 16, 8, 2, 4, WNConfig(2, 32, 3, 16)).train()


def test_capture_refuses_a_cpu_model():
    from reformer_tts_amd import _lib
    from reformer_tts_amd.squeeze_wave.training import VocoderTrainer
    with pytest.raises(_lib.RttsError, match="GPU only"):
        VocoderTrainer(_cpu_model()).capture(2, 4)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        VocoderTrainer(_cpu_model(), logdet="device").capture(2, 4)


def test_capture_refuses_a_host_mode_trainer_by_name(monkeypatch):
    """The device gate comes first; with it out of the way (no GPU here) the host-mode trainer is refused by name."""
    from reformer_tts_amd import _lib
    from reformer_tts_amd.squeeze_wave.training import VocoderTrainer
    model = _cpu_model()
    monkeypatch.setattr(model, "_device", lambda what: torch.device("cpu"))
    with pytest.raises(_lib.RttsError, match="logdet='device'"):
        VocoderTrainer(model).capture(2, 4)
    with pytest.raises(ValueError, match="logdet must be 'host' or 'device'"):
        VocoderTrainer(model, logdet="gpu")


def test_device_fold_is_the_training_folds_only():
    model = _cpu_model()
    with pytest.raises(ValueError, match="logdet must be 'host' or 'device'"):
        model._fold(fold_bn=False, logdet="lapack")
    with pytest.raises(ValueError, match="training fold"):
        model._fold(fold_bn=True, logdet="device")
    from reformer_tts_amd import _lib
    with pytest.raises(_lib.RttsError, match="no device-mode fold yet"):
        model.check_determinants()
