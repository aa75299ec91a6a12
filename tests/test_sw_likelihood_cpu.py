"""Host-side checks of the SqueezeWave likelihood path (no GPU): the float64 helper against the reference's fixture, the
log-determinant fold, the offset / sample-count arithmetic, the refusals that happen before any launch, and
``SqueezeWaveLoss`` on hand-made tuples."""
import math
import os
import re

import numpy as np
import pytest
import torch

import sw_likelihood_ref as ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtts_sw_coupling_fwd1x1", "rtts_sw_nll_reduce", "rtts_sw_pack_audio")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "squeezewave_likelihood.npz"))


def _model(golden_dir, tag):
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    cfg, sd, mel, audio = ref64.load_case(golden_dir, tag)
    model = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                        cfg["early_return_size"], WNConfig(**cfg["wn_config"]))
    model.load_state_dict(sd, strict=False)
    return model.eval(), mel, audio


@pytest.mark.parametrize("tag", ["small", "full"])
def test_float64_forward_reproduces_the_reference_fixture(golden_dir, fixture, tag):
    """The helper's float64 forward and loss against what the reference's fp32 modules returned: z to 1e-5, loss to 1e-6
    (fp32-vs-float64 differences of 1.7e-6 and 3e-8 were measured), per-flow sums of log_s and the ragged pieces likewise."""
    cfg, sd, mel, audio = ref64.load_case(golden_dir, tag)
    out = ref64.forward64(sd, cfg, mel, audio)
    z = torch.from_numpy(fixture[f"{tag}/z"]).double()
    assert out[0].shape == z.shape
    assert float((out[0] - z).abs().max()) < 1e-5
    assert abs(float(ref64.loss64(out)) - float(fixture[f"{tag}/loss"])) < 1e-6
    ls = np.array([float(s.sum()) for s in out[1]])
    assert np.abs(ls - fixture[f"{tag}/log_s_sum"]).max() < 1e-4          # sums of ~1e4 fp32 values of size <= 0.57
    assert [tuple(s.shape) for s in out[1]] == [(z.shape[0], n, z.shape[2]) for n in _halves(cfg)]
    assert list(fixture[f"{tag}/ragged_frames"]) == ref64.RAGGED_FRAMES
    for (pmel, paudio), want in zip(ref64.ragged_pieces(mel, audio), fixture[f"{tag}/ragged"]):
        if pmel.shape[2] == 0:
            assert math.isnan(float(want))
        else:
            assert abs(float(ref64.loss64(ref64.forward64(sd, cfg, pmel, paudio))) - float(want)) < 1e-6


def _halves(cfg):
    n_half, out = cfg["n_audio_channels"] // 2, []
    for k in range(cfg["n_flows"]):
        if k % cfg["early_return_interval"] == 0 and k > 0:
            n_half -= cfg["early_return_size"] // 2
        out.append(n_half)
    return out


def test_rounding_model_stays_inside_the_inference_tolerance(golden_dir):
    """The bf16 rounding model of the executor against the float64 forward: the numbers the GPU tests take their bounds
    from (4x).  They must leave room under the inference golden's 3e-2 max / 4e-3 mean."""
    for tag in ("small", "full"):
        zmax, zmean, dloss = ref64.rounding_model_error(golden_dir, tag)
        print(tag, zmax, zmean, dloss)
        assert 0 < 4 * zmax <= 3e-2 and 0 < 4 * zmean <= 4e-3 and 0 < dloss < 1e-3, (tag, zmax, zmean, dloss)
        # the constants the GPU tests multiply by 4 are these measurements (written down to four digits)
        for got, kept in zip((zmax, zmean, dloss), ref64.MODEL_ERR[tag]):
            assert abs(got - kept) <= 1e-2 * kept, (tag, got, kept)


def test_fold_caches_forward_weights_and_float64_logdet(golden_dir):
    """_fold keeps every flow's W (fp32, contiguous) and log det W from a float64 slogdet: equal to torch.logdet of the
    float64 weight; the existing inverse cache is untouched by it."""
    model, _, _ = _model(golden_dir, "small")
    with torch.no_grad():
        for conv in model.inv_conv_layers:                               # away from orthonormal: log det != 0
            conv.conv.weight.mul_(1.3).add_(0.01)
    model._fold()
    logdet = model._logdets()
    assert len(logdet) == model.n_flows == len(model._wfwd)
    for k, conv in enumerate(model.inv_conv_layers):
        w = conv.conv.weight.detach().squeeze(-1)
        assert model._wfwd[k].dtype == torch.float32 and model._wfwd[k].is_contiguous() and torch.equal(model._wfwd[k], w)
        want = float(torch.logdet(w.double()))
        assert abs(logdet[k]) > 0.1 and abs(logdet[k] - want) <= 1e-12 * abs(want)
        assert torch.equal(model._winv[k], w.double().inverse().float())


def test_negative_determinant_is_refused_by_name(golden_dir):
    model, mel, audio = _model(golden_dir, "small")
    with torch.no_grad():
        model.inv_conv_layers[2].conv.weight[:, 0] *= -1
    with pytest.raises(ValueError, match=r"inv_conv_layers\.2: det W is negative"):
        model._logdets()
    assert len(model._fold()) == model.n_flows                           # inference does not need log det W: the fold itself stands


def test_likelihood_refuses_to_run_off_the_gpu(golden_dir):
    from reformer_tts_amd import _lib
    model, mel, audio = _model(golden_dir, "small")
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model((mel, audio))
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model.nll(mel, audio)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model.nll_ragged(mel, [24, 24], audio)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model.capture_nll_ragged(2, 64)


def test_offset_and_sample_count_arithmetic(golden_dir):
    """256 samples per mel frame; the first sample of every utterance for the three audio forms; an utterance whose audio is
    shorter than 256 * frames is refused with the numbers in the message."""
    from reformer_tts_amd.squeeze_wave.modules import segment_offsets
    model, _, _ = _model(golden_dir, "small")
    cpu = torch.device("cpu")
    assert model.samples_per_frame() == 256
    lens = [7, 0, 17, 1]
    assert segment_offsets(lens) == [0, 7, 7, 24, 25]
    flat = torch.arange(256 * 25, dtype=torch.float32)
    got, starts = model._audio_starts(flat, lens, None, cpu, "t")
    assert starts == [0, 256 * 7, 256 * 7, 256 * 24] and got.data_ptr() == flat.data_ptr()
    _, starts = model._audio_starts(torch.zeros(256 * 40), lens, [5, 3000, 0, 9000, 12345], cpu, "t")      # B + 1 offsets: the last is ignored
    assert starts == [5, 3000, 0, 9000]
    padded = torch.zeros(4, 256 * 17 + 3)
    got, starts = model._audio_starts(padded, lens, None, cpu, "t")
    assert starts == [i * (256 * 17 + 3) for i in range(4)] and got.shape == (4 * (256 * 17 + 3),)
    with pytest.raises(ValueError, match=r"utterance 2 has 17 frames = 4352 samples, its audio holds 4351"):
        model._audio_starts(torch.zeros(4, 256 * 17 - 1), lens, None, cpu, "t")
    with pytest.raises(ValueError, match=r"utterance 3 has 1 frames = 256 samples, its audio holds 255"):
        model._audio_starts(torch.zeros(256 * 25 - 1), lens, None, cpu, "t")
    with pytest.raises(ValueError, match="3 sample offsets for 4 utterances"):
        model._audio_starts(flat, lens, [0, 1, 2], cpu, "t")
    with pytest.raises(ValueError, match="negative"):
        model._ragged_lengths([3, -1], "t")
    with pytest.raises(ValueError, match=r"1\.\.1024 utterances \(got 1025\)"):
        model._ragged_lengths([1] * 1025, "t")
    with pytest.raises(ValueError, match=r"1\.\.1024 utterances \(got 0\)"):
        model._ragged_lengths([], "t")


def test_squeezewave_loss_on_hand_made_tuples():
    """[sum z^2 / (2 sigma^2) - sum log_s - sum log_det_W] / numel, in double, for tensors, 0-dim tensors and floats."""
    from reformer_tts_amd.squeeze_wave import SqueezeWaveLoss, validation_loss
    z = torch.ones(1, 2, 3)
    log_s = [torch.full((1, 1, 3), 0.5), torch.full((1, 1, 3), -0.25)]
    got = SqueezeWaveLoss(2.0)((z, log_s, [torch.tensor(0.25), 1.0]))
    assert got.dtype == torch.float32 and got.dim() == 0
    assert abs(float(got) - (6 / 8 - 1.5 + 0.75 - 0.25 - 1.0) / 6) < 1e-7
    g = torch.Generator().manual_seed(0)
    z = torch.randn(2, 8, 5, generator=g)
    log_s = [0.3 * torch.randn(2, 4, 5, generator=g) for _ in range(3)]
    ld = [torch.randn((), generator=g) for _ in range(3)]
    for sigma in (1.0, 0.6):
        want = float(ref64.loss64((z, log_s, ld), sigma))
        assert abs(float(SqueezeWaveLoss(sigma)((z, log_s, ld))) - want) <= 1e-6 * abs(want)
    with pytest.raises(ValueError, match="2 log_s tensors for 1 log-determinants"):
        SqueezeWaveLoss()((z, log_s[:2], ld[:1]))

    class Fake:                                                           # validation_loss: the mean of the batch losses
        def nll(self, mel, audio, sigma):
            return (mel.sum() + audio.sum()) * sigma
    batches = [(torch.tensor([1.0]), torch.tensor([2.0])), (torch.tensor([4.0]), torch.tensor([5.0]))]
    assert float(validation_loss(Fake(), batches, sigma=0.5)) == 3.0
    with pytest.raises(ValueError, match="no batches"):
        validation_loss(Fake(), [])


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


def test_boundary_kernel_refuses_bad_arguments_on_the_host():
    """out == x, odd n, n_in > 128 and the other shape rules of rtts_sw_coupling_fwd1x1 are refused by the entry point itself,
    with a message, before anything is launched (dummy pointers, no device needed)."""
    import __graft_entry__
    __graft_entry__.build()
    X, WN, W, OUT, Z, LS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000

    def args(x=X, ld_x=128, wn=WN, ld_wn=128, w=W, n_in=128, n_early=16, rows=40, out=OUT, ld_out=128, z=Z, ld_z=128, z_col=0, ls=LS):
        return (x, ld_x, wn, ld_wn, w, n_in, n_early, rows, out, ld_out, z, ld_z, z_col, ls, None)
    assert "not in place" in _refused("rtts_sw_coupling_fwd1x1", args(out=X))
    assert "n_in must be even and <= 128 (got n_in=130)" in _refused("rtts_sw_coupling_fwd1x1", args(n_in=130, ld_x=130, ld_wn=130))
    assert "n_in must be even" in _refused("rtts_sw_coupling_fwd1x1", args(n_in=127))
    assert "n_early must be even" in _refused("rtts_sw_coupling_fwd1x1", args(n_early=15))        # odd n = n_in - n_early
    assert "n_early must be even" in _refused("rtts_sw_coupling_fwd1x1", args(n_early=130))
    assert "ld_z >= z_col + n_early" in _refused("rtts_sw_coupling_fwd1x1", args(z_col=120))
    assert "without W every column is early output" in _refused("rtts_sw_coupling_fwd1x1", args(w=None, n_early=16))
    assert "ls_row with wn_out" in _refused("rtts_sw_coupling_fwd1x1", args(ls=None))
    assert "leading dimensions" in _refused("rtts_sw_coupling_fwd1x1", args(ld_x=64))
    assert "z must not alias" in _refused("rtts_sw_coupling_fwd1x1", args(z=OUT))
    assert "rows > 0" in _refused("rtts_sw_coupling_fwd1x1", args(rows=0))


def test_reduce_and_pack_refuse_bad_arguments_on_the_host():
    import __graft_entry__
    __graft_entry__.build()
    Z, LS, MOFF, OUT, SRC, START = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    assert "1..1024 segments (got 1025)" in _refused("rtts_sw_nll_reduce", (Z, 16, 16, LS, MOFF, 1025, 16, 0, 64, OUT, None))
    assert "1..1024 segments (got 0)" in _refused("rtts_sw_nll_reduce", (Z, 16, 16, LS, MOFF, 0, 16, 0, 64, OUT, None))
    assert "without an offset table" in _refused("rtts_sw_nll_reduce", (Z, 16, 16, LS, None, 3, 16, 20, 64, OUT, None))
    assert "bad arguments" in _refused("rtts_sw_nll_reduce", (Z, 8, 16, LS, MOFF, 3, 16, 0, 64, OUT, None))
    assert "1..1024 segments (got 1025)" in _refused("rtts_sw_pack_audio", (SRC, 100, START, MOFF, 1025, 16, 16, 64, OUT, None))
    assert "rows a multiple of upsample" in _refused("rtts_sw_pack_audio", (SRC, 100, START, MOFF, 2, 16, 16, 65, OUT, None))
    assert "bad arguments" in _refused("rtts_sw_pack_audio", (SRC, 100, None, MOFF, 2, 16, 16, 64, OUT, None))
