"""Host-side checks of vocoder training (no GPU): the float64 training helper against the reference's fixture, the constants
of its rounding model, ``vocoder_segment``, the refusals of the new entry points before any launch, and their exports."""
import os
import re

import numpy as np
import pytest
import torch

import sw_train_ref as train64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtts_sw_gate_bwd", "rtts_sw_dwbn_bwd_sums", "rtts_sw_dwbn_bwd_apply", "rtts_sw_boundary_bwd",
               "rtts_sw_dwbn_bwd_partial_floats", "rtts_sw_boundary_bwd_blocks")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "squeezewave_train.npz"))


@pytest.mark.parametrize("case", train64.CASES)
def test_float64_step_reproduces_the_reference_fixture(golden_dir, fixture, case):
    """The helper's float64 loss, gradients and running statistics against what the reference's fp32 modules produced in
    ``.train()``: every gradient norm and every stored gradient to relative L2 1e-4 (the reference is fp32; 1.1e-6 / 1.7e-6 at
    worst were measured), and no parameter may be skipped: none has a zero gradient."""
    loss, grads, stats = train64.grads64(golden_dir, case, False)
    assert abs(loss - float(fixture[f"{case}/loss"])) < 1e-6
    names = [str(n) for n in fixture[f"{case}/names"]]
    norms = fixture[f"{case}/norms"]
    assert sorted(names) == sorted(grads) and len(names) == {"small": 108}.get(case, 972)
    assert norms.min() > 0
    for n, want in zip(names, norms):
        assert abs(float(grads[n].norm()) - want) <= 1e-4 * want, n
    full = [k[len(case) + 6:] for k in fixture.files if k.startswith(f"{case}/grad/")]
    assert len(full) == 7                  # BatchNorm weight, bias; depthwise weight, bias; weight_g; two invertible convolutions
    for n in full:
        want = torch.from_numpy(fixture[f"{case}/grad/{n}"])
        assert grads[n].shape == want.shape and train64.rel_l2(grads[n], want) < 1e-4, n
    p = "wn_layers.0.in_layers.0.layer.0."
    for k in ("running_mean", "running_var"):
        assert train64.rel_l2(stats[p + k], torch.from_numpy(fixture[f"{case}/stat/{p}{k}"])) < 1e-5, k
    assert int(fixture[f"{case}/stat/{p}num_batches_tracked"]) == 1


@pytest.mark.parametrize("case", train64.CASES)
def test_rounding_model_constants(golden_dir, case):
    """The constants the GPU tests take their bounds from (``MODEL_CONST``), measured again: gradient, loss, 8-step and
    running-statistics errors of the bf16 rounding model against the exact float64 step.  They are properties of the model and
    the golden inputs, not of any kernel."""
    got = train64.model_constants(golden_dir, case)
    for g, w in zip(got, train64.MODEL_CONST[case]):
        assert abs(g - w) <= 0.02 * w, (case, got, train64.MODEL_CONST[case])
    if case == "small":
        exact = train64.train64(golden_dir, case, 8, False)
        assert abs(exact[0] - 0.2191) < 1e-4 and abs(exact[-1] - 0.1481) < 1e-4 and exact[-1] < exact[0]


def test_vocoder_segment():
    """Hand-written expectations for a 4096-sample segment at hop 256 (16 frames): a 40-frame utterance cropped at hop 24, 0 and
    by the seeded default draw; a 16-frame one returned whole; a 9-frame one zero-padded at its end."""
    import random
    from reformer_tts_amd.dataset.utils import vocoder_segment
    g = torch.Generator().manual_seed(1)
    audio, spec = torch.randn(40 * 256, generator=g), torch.randn(80, 40, generator=g)
    a, s = vocoder_segment(audio, spec, 4096, 256, random_hop=24)
    assert torch.equal(a, audio[6144:10240]) and torch.equal(s, spec[:, 24:40])
    a, s = vocoder_segment(audio, spec, 4096, 256, random_hop=0)
    assert torch.equal(a, audio[:4096]) and torch.equal(s, spec[:, :16])
    random.seed(3)
    a, s = vocoder_segment(audio, spec, 4096, 256)
    random.seed(3)
    hop = random.randint(0, 24)                      # (10240 - 4096) // 256 = 24 is the last start that fits
    assert torch.equal(a, audio[256 * hop:256 * hop + 4096]) and torch.equal(s, spec[:, hop:hop + 16])
    with pytest.raises(ValueError, match="random_hop"):
        vocoder_segment(audio, spec, 4096, 256, random_hop=25)
    a, s = vocoder_segment(audio[:4096], spec[:, :16], 4096, 256)
    assert torch.equal(a, audio[:4096]) and torch.equal(s, spec[:, :16])
    a, s = vocoder_segment(audio[:2304], spec[:, :9], 4096, 256)
    assert a.shape == (4096,) and s.shape == (80, 16)
    assert torch.equal(a[:2304], audio[:2304]) and not a[2304:].any()
    assert torch.equal(s[:, :9], spec[:, :9]) and not s[:, 9:].any()


def test_backward_refuses_widths_it_does_not_tile():
    """n_channels 64 / 192 / 320 run the eval forward on the MFMA GEMMs, but the backward's weight-gradient GEMM and column sums
    tile 128, 256, 512 and 1024 only: nll_backward says so before anything else (no device needed)."""
    from reformer_tts_amd import _lib
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    for c in (64, 192, 320):
        model = SqueezeWave(2, 16, 80, 2, 4, WNConfig(1, c, 3, 16)).train()
        with pytest.raises(_lib.RttsError, match=f"n_channels {c} is not one of"):
            model.nll_backward(torch.zeros(1, 80, 2), torch.zeros(1, 512))
    for c in (32, 128):                              # toy widths (library GEMM) and tiled widths get as far as the device check
        model = SqueezeWave(2, 16, 80, 2, 4, WNConfig(1, c, 3, 16)).train()
        with pytest.raises(_lib.RttsError, match="GPU only"):
            model.nll_backward(torch.zeros(1, 80, 2), torch.zeros(1, 512))


def test_training_entry_points_refuse_off_the_gpu(golden_dir):
    from reformer_tts_amd import _lib
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    from reformer_tts_amd.squeeze_wave.training import VocoderTrainer
    cfg, sd, mel, audio = train64.load_train_case(golden_dir, "small")
    model = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                        cfg["early_return_size"], WNConfig(**cfg["wn_config"]))
    model.load_state_dict(sd, strict=False)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model.train().nll_backward(mel, audio)
    trainer = VocoderTrainer(model)
    assert isinstance(trainer.optimizer, torch.optim.Adam) and trainer.optimizer.defaults["lr"] == 4e-4 and trainer.loss_sigma == 1.0
    assert sum(len(g["params"]) for g in trainer.optimizer.param_groups) == 108
    with pytest.raises(_lib.RttsError, match="GPU only"):
        trainer.training_step({"spectrogram": mel, "audio": audio})
    assert all(p.grad is None for p in model.parameters())


def test_new_entry_points_are_declared_bound_and_exported():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtts.h")).read(), flags=re.S)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert f"`{name}`" in integration, name
        proto = re.search(rf"\bint {name}\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name


def _refused(name, args):
    """Call an entry point with dummy (never dereferenced) pointers on the null stream: it must refuse before any launch."""
    from reformer_tts_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    assert rc != 0, (name, args)
    return lib.rtts_last_error().decode()


def test_backward_kernels_refuse_bad_arguments_on_the_host():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    P = [0x1000 * (i + 1) for i in range(12)]

    def gate(pw=P[0], cond=P[1], ld_cond=512, off=0, up=2, b=1, length=8, lm=4, c=256, dacts=P[2], dpw=P[3], dcond=P[4], ld_dcond=512):
        return (pw, cond, ld_cond, off, up, b, length, lm, c, dacts, dpw, dcond, ld_dcond, None)
    for bad in (gate(c=20), gate(length=9), gate(ld_cond=256), gate(ld_dcond=500), gate(off=4), gate(dacts=None), gate(up=0)):
        assert "rtts_sw_gate_bwd: bad arguments" in _refused("rtts_sw_gate_bwd", bad)
    assert "not in place" in _refused("rtts_sw_gate_bwd", gate(dpw=P[0]))
    assert "16-byte aligned" in _refused("rtts_sw_gate_bwd", gate(dacts=P[2] + 8))

    def sums(h=P[0], dy=P[1], c=256, b=2, length=8, out=P[7], ws=P[8]):
        return (h, dy, P[2], P[3], P[4], P[5], P[6], b, length, c, out, ws, None)
    for bad in (sums(c=6), sums(c=20), sums(b=0), sums(length=0), sums(ws=None), sums(dy=None)):
        assert "rtts_sw_dwbn_bwd_sums: bad arguments" in _refused("rtts_sw_dwbn_bwd_sums", bad)

    def apply(h=P[0], dy=P[1], c=256, b=2, length=8, s=P[7], dh=P[8]):
        return (h, dy, P[2], P[3], P[4], P[5], P[6], s, b, length, c, dh, None)
    for bad in (apply(c=6), apply(c=20), apply(b=0), apply(s=None), apply(dh=None)):
        assert "rtts_sw_dwbn_bwd_apply: bad arguments" in _refused("rtts_sw_dwbn_bwd_apply", bad)
    assert "must not alias" in _refused("rtts_sw_dwbn_bwd_apply", apply(dh=P[0]))
    assert "16-byte" in _refused("rtts_sw_dwbn_bwd_apply", apply(dh=P[8] + 8))
    assert "16-byte" in _refused("rtts_sw_dwbn_bwd_sums", sums(h=P[0] + 4))
    assert "16-byte" in _refused("rtts_sw_dwbn_bwd_sums", sums(dy=P[1] + 8))

    def bnd(x=P[0], ld_x=128, wn=P[1], ld_wn=128, w=P[2], n_in=128, n_early=16, rows=40, dout=P[3], ld_dout=112, z=P[4], ld_z=128, z_col=0,
            dx=P[5], ld_dx=128, dwn=P[6], ld_dwn=128, dw=P[7], ws=P[8]):
        return (x, ld_x, wn, ld_wn, w, n_in, n_early, rows, dout, ld_dout, z, ld_z, z_col, 1.0, 1.0, dx, ld_dx, dwn, ld_dwn, dw, ws, None)
    assert "n_in must be even and <= 128 (got n_in=130)" in _refused("rtts_sw_boundary_bwd", bnd(n_in=130, ld_x=130))
    assert "n_early must be even" in _refused("rtts_sw_boundary_bwd", bnd(n_early=15))
    assert "rows > 0" in _refused("rtts_sw_boundary_bwd", bnd(rows=0))
    assert "nothing to do" in _refused("rtts_sw_boundary_bwd", bnd(wn=None, w=None, n_early=128))
    assert "leading dimensions >= n_in" in _refused("rtts_sw_boundary_bwd", bnd(ld_dwn=64))
    assert "leading dimensions >= n_in" in _refused("rtts_sw_boundary_bwd", bnd(dx=None))
    assert "not in place" in _refused("rtts_sw_boundary_bwd", bnd(dx=P[0]))
    assert "ld_z >= z_col + n_early" in _refused("rtts_sw_boundary_bwd", bnd(z_col=120))
    assert "ld_dout >= n" in _refused("rtts_sw_boundary_bwd", bnd(ld_dout=64))
    assert "ld_dout >= n" in _refused("rtts_sw_boundary_bwd", bnd(dw=None))
    assert "without W every column is early output" in _refused("rtts_sw_boundary_bwd", bnd(w=None, n_early=16))
    lib = _lib.load()
    assert lib.rtts_sw_boundary_bwd_blocks(1) == 1 and lib.rtts_sw_boundary_bwd_blocks(33) == 2 and lib.rtts_sw_boundary_bwd_blocks(1 << 20) == 256
    assert lib.rtts_sw_dwbn_bwd_partial_floats(2, 32) == 6 * 32 and lib.rtts_sw_dwbn_bwd_partial_floats(12288, 256) == 256 * 6 * 256
