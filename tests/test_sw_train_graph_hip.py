"""Vocoder training without the host: ``SqueezeWave.nll_backward(logdet="device")`` (the 1x1 convolutions factored by
``rtts_sw_inv1x1_factor``) against the float64 step within the bounds of tests/test_sw_train_hip.py (4 x ``MODEL_CONST``, nothing
new), its determinism, and ``VocoderTrainer.capture`` -- the whole step as one hipGraph -- bit for bit against the eager trainer
built with the same arguments."""
import pytest
import torch

import sw_train_ref as train64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _build(golden_dir, case, gpu):
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    cfg, sd, mel, audio = train64.load_train_case(golden_dir, case)
    model = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                        cfg["early_return_size"], WNConfig(**cfg["wn_config"]))
    model.load_state_dict(sd, strict=False)
    return model.to(gpu).train(), mel.to(gpu), audio.to(gpu)


def _step(golden_dir, case, gpu, calls=1):
    """A fresh model, ``calls`` x nll_backward(logdet="device") -> (model, losses, {name: gradient on the host})."""
    model, mel, audio = _build(golden_dir, case, gpu)
    losses = [float(model.nll_backward(mel, audio, logdet="device")) for _ in range(calls)]
    torch.cuda.synchronize()
    return model, losses, {n: p.grad.detach().cpu() for n, p in model.named_parameters()}


@pytest.fixture(scope="module")
def steps(golden_dir, gpu):
    """case -> (model after one device-mode step, [loss], gradients): computed once, never modified by a test."""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _step(golden_dir, case, gpu)
        return cache[case]
    return get


# ------------------------------------------------------------------ 1. the device-mode step
@pytest.mark.parametrize("case", train64.CASES)
def test_device_mode_nll_backward_vs_float64(golden_dir, steps, case):
    """Loss, every parameter's gradient, all gradients concatenated and the running statistics against the exact float64 step:
    the bounds of tests/test_sw_train_hip.py::test_nll_backward_vs_float64, unchanged."""
    worst, concat, dloss, _, rmean, rvar = train64.MODEL_CONST[case]
    loss64, grads64, stats64 = train64.grads64(golden_dir, case, False)
    model, losses, grads = steps(case)
    assert set(grads) == set(grads64)
    errs = {n: train64.rel_l2(grads[n], grads64[n]) for n in grads64}
    cat = train64.concat_rel_l2(grads, grads64)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    serr = {k: train64.rel_l2(sd[k], stats64[k]) for k in stats64}
    wm = max(v for k, v in serr.items() if k.endswith("running_mean"))
    wv = max(v for k, v in serr.items() if k.endswith("running_var"))
    print(case, "loss diff", abs(losses[0] - loss64), "bound", 4 * dloss, "worst gradient", max(errs.values()), "bound", 4 * worst,
          "concatenated", cat, "bound", 4 * concat, "running mean / var", wm, wv, "bounds", 4 * rmean, 4 * rvar)
    assert abs(losses[0] - loss64) <= 4 * dloss
    for n, e in errs.items():
        assert e <= 4 * worst, (n, e)
    assert cat <= 4 * concat
    assert wm <= 4 * rmean and wv <= 4 * rvar
    model.check_determinants()                                                  # every determinant is positive: nothing raised
    assert model._slogdet_dev.shape == (len(model.inv_conv_layers), 2) and model._slogdet_dev.dtype == torch.float64


@pytest.mark.parametrize("case", ["small", "full/3x10"])
def test_device_mode_accumulates_and_is_deterministic(golden_dir, gpu, steps, case):
    _, losses, grads = steps(case)
    _, again_loss, again = _step(golden_dir, case, gpu)
    assert again_loss == losses
    for n, gr in grads.items():
        assert torch.equal(again[n], gr), n
    _, losses2, twice = _step(golden_dir, case, gpu, calls=2)
    assert losses2[0] == losses[0] and losses2[1] == losses[0]
    for n, gr in grads.items():
        assert torch.equal(twice[n], 2 * gr), n


# ------------------------------------------------------------------ 2. the captured trainer
def _state(model, trainer):
    """Everything a step changes, on the host: parameters, buffers, Adam's state."""
    out = {"p/" + n: p.detach().cpu() for n, p in model.named_parameters()}
    out.update({"b/" + n: b.detach().cpu() for n, b in model.named_buffers()})
    names = {id(p): n for n, p in model.named_parameters()}
    for p, st in trainer.optimizer.state.items():
        for k, v in st.items():
            out[f"adam/{names[id(p)]}/{k}"] = v.detach().cpu() if torch.is_tensor(v) else torch.tensor(v)
    return out


def _assert_same_state(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _run_pair(golden_dir, case, gpu, batches_of, n_steps, before_capture=None):
    """An eager device-mode trainer and a captured one from the same start over the same batches ->
    (eager losses, graph losses, eager (model, trainer), graph (model, trainer), run)."""
    from reformer_tts_amd.squeeze_wave.training import VocoderTrainer
    eager_m, mel, audio = _build(golden_dir, case, gpu)
    graph_m, _, _ = _build(golden_dir, case, gpu)
    batches = batches_of(mel, audio)
    eager_t, graph_t = VocoderTrainer(eager_m, logdet="device"), VocoderTrainer(graph_m, logdet="device")
    if before_capture is not None:
        before_capture(graph_m, mel, audio)
    run = graph_t.capture(mel.shape[0], mel.shape[2])
    eager = [float(eager_t.training_step(batches[i % len(batches)])) for i in range(n_steps)]
    graph = [float(run(batches[i % len(batches)])) for i in range(n_steps)]
    torch.cuda.synchronize()
    return eager, graph, (eager_m, eager_t), (graph_m, graph_t), run


def test_captured_trainer_small_eight_steps(golden_dir, gpu):
    """``small``, 8 steps on one fixed batch: every loss within 4 x MODEL_CONST of the float64 sequence; losses, parameters,
    BatchNorm statistics and Adam state bit-equal to the eager device-mode trainer; num_batches_tracked == 8 (the warm-up step of
    the capture left no trace); a wrong batch shape is refused and changes nothing."""
    eager, graph, (em, et), (gm, gt), run = _run_pair(golden_dir, "small", gpu, lambda mel, audio: [{"spectrogram": mel, "audio": audio}], 8)
    want = train64.train64(golden_dir, "small", 8, False)
    bound = 4 * train64.MODEL_CONST["small"][3]
    print("graph losses", graph, "float64", want, "bound", bound)
    for a, b in zip(graph, want):
        assert abs(a - b) <= bound, (graph, want)
    assert graph == eager
    _assert_same_state(_state(gm, gt), _state(em, et))
    tracked = [int(v) for k, v in gm.state_dict().items() if k.endswith("num_batches_tracked")]
    assert tracked and all(t == 8 for t in tracked)
    gt.check_determinants()
    # a wrong shape: refused by name, nothing touched
    before = _state(gm, gt)
    _, mel, audio = _build(golden_dir, "small", gpu)
    with pytest.raises(ValueError, match="spectrogram"):
        run({"spectrogram": mel[:, :, :-1], "audio": audio})
    with pytest.raises(ValueError, match="audio"):
        run({"spectrogram": mel, "audio": audio[:, :-256]})
    torch.cuda.synchronize()
    _assert_same_state(_state(gm, gt), before)


def test_captured_trainer_full_alternating_batches_and_fold_cache(golden_dir, gpu):
    """``full/3x10`` (the MFMA path, 60 real rows in 128-row buffers), 3 steps alternating two batches (the second: the audio
    rolled by one segment): bit-equal to the eager trainer on the same sequence, so the inputs really are copied in.
    Then the sequence in which a fold goes stale: ``.eval().nll`` BETWEEN two replays caches an inference fold under a key made of
    the parameters' ``_version``, which a replay does not raise.  After the next replay ``.eval().nll`` must be bitwise that of a
    fresh model loaded with the same state_dict -- it is only because ``run`` drops the cached fold after every replay."""
    def batches_of(mel, audio):
        return [{"spectrogram": mel, "audio": audio}, {"spectrogram": mel, "audio": torch.roll(audio, 1, dims=0).contiguous()}]

    eager, graph, (em, et), (gm, gt), run = _run_pair(golden_dir, "full/3x10", gpu, batches_of, 3)
    assert graph == eager
    _assert_same_state(_state(gm, gt), _state(em, et))
    tracked = [int(v) for k, v in gm.state_dict().items() if k.endswith("num_batches_tracked")]
    assert tracked and all(t == 3 for t in tracked)
    fresh, mel, audio = _build(golden_dir, "full/3x10", gpu)
    batch = batches_of(mel, audio)[1]
    between = gm.eval().nll(mel, audio).clone()                                  # a fold is cached now, under the current versions
    assert gm._folded is not None and gm._folded_key is not None
    versions = [p._version for p in gm.parameters()]
    gm.train()
    loss = float(run(batch))
    assert [p._version for p in gm.parameters()] == versions                    # the replay moved the parameters, not their versions
    assert loss == float(et.training_step(batch))
    _assert_same_state(_state(gm, gt), _state(em, et))
    fresh.load_state_dict(gm.state_dict())
    a, b = gm.eval().nll(mel, audio), fresh.eval().nll(mel, audio)
    assert torch.isfinite(a) and torch.equal(a, b)
    assert not torch.equal(a, between)                                          # the step did change what nll scores
    gm.train()


def test_capture_refusals(golden_dir, gpu):
    from reformer_tts_amd import _lib
    from reformer_tts_amd.squeeze_wave.training import VocoderTrainer
    model, mel, audio = _build(golden_dir, "small", gpu)
    with pytest.raises(_lib.RttsError, match="logdet='device'"):
        VocoderTrainer(model).capture(mel.shape[0], mel.shape[2])
    with pytest.raises(_lib.RttsError, match="training mode"):
        VocoderTrainer(model.eval(), logdet="device").capture(mel.shape[0], mel.shape[2])
    assert all(p.grad is None for p in model.parameters())


# ------------------------------------------------------------------ 3. determinants that have no logarithm
def test_negative_determinant(golden_dir, gpu):
    """One column of inv_conv_layers[1] flipped: the device-mode step raises nothing and returns a loss that is not finite (the
    reference's torch.logdet gives NaN); check_determinants names the flow; host mode raises before touching the device."""
    model, mel, audio = _build(golden_dir, "small", gpu)
    with torch.no_grad():
        model.inv_conv_layers[1].conv.weight[:, 0] *= -1
    loss = model.nll_backward(mel, audio, logdet="device")
    torch.cuda.synchronize()
    assert not torch.isfinite(loss)
    with pytest.raises(ValueError, match=r"inv_conv_layers\.1: det W is negative"):
        model.check_determinants()
    model.zero_grad()
    with pytest.raises(ValueError, match=r"inv_conv_layers\.1: det W is negative"):
        model.nll_backward(mel, audio)
    assert all(p.grad is None for p in model.parameters())
