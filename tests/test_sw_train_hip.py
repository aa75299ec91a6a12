"""Vocoder training on the GPU: the three backward kernels against float64, ``SqueezeWave.nll_backward`` against the float64
training step of ``tests/sw_train_ref.py``, accumulation, determinism, padding rows, ``VocoderTrainer`` and the refusals.

Kernel-level bounds: with u = 2^-24, a sum of n fp32 terms added in any order is within n u / (1 - n u) of sum |terms|; the tests
compute sum |terms| in float64 from the same (exactly representable) inputs and allow a few more u for the roundings inside a
term.  bf16 outputs add the bf16 unit roundoff (2^-8 relative).

Model-level bounds: ``sw_train_ref.MODEL_CONST`` holds the error of the bf16 rounding model against the exact float64 step
(re-measured by tests/test_sw_train_cpu.py); the bound is 4x that, this project's convention for what the model leaves out
(accumulation order, the device's exp / tanh)."""

import pytest
import torch

import sw_train_ref as train64

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
BF = 2.0 ** -8


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _gamma(n):
    return n * U / (1 - n * U)


def _bf(t):
    return t.to(torch.bfloat16)


def _ratio(got, want, tol):
    """max |got - want| / tol, element-wise (tol > 0 wherever want can differ)."""
    return float(((got.double() - want).abs() / tol.clamp_min(1e-300)).max())


# ------------------------------------------------------------------ 1. kernels through the C ABI
@pytest.mark.parametrize("c,up,b,lm", [(32, 16, 2, 3), (256, 2, 2, 5), (32, 16, 1, 1), (64, 2, 3, 171)])
def test_gate_backward_kernel_vs_float64(gpu, c, up, b, lm):
    """rtts_sw_gate_bwd: C 32 / up 16, C 256 / up 2, Lm 1, and B * Lm * C / 8 = 4104 work items (not a multiple of the
    256-thread workgroup).  |err| <= the bf16 rounding of the value (2^-8 relative) + 16 u |da| per term (the gate's derivative factors are <= 1 and
    each is a few fp32 roundings of tanhf / __expf), the conditioning row summing its `up` terms.  Measured worst ratios of
    error to bound on an MI355X: dpw 0.995, dcond 0.993 (the bf16 rounding of the output itself is most of the bound)."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(c + up + lm)
    length, rows, off, ld = up * lm, b * up * lm, 2 * c, 2 * c * 2 + 8
    pw, cond = _bf(torch.randn(rows, 2 * c, generator=g)), _bf(torch.randn(b * lm, ld, generator=g))
    da = _bf(torch.randn(rows, c, generator=g))
    pwd, condd, dad = pw.to(gpu), cond.to(gpu), da.to(gpu)
    outs = []
    for _ in range(2):
        dpw = torch.full((rows, 2 * c), float("nan"), dtype=torch.bfloat16, device=gpu)
        dcond = torch.full((b * lm, ld), float("nan"), dtype=torch.bfloat16, device=gpu)
        _lib.call("rtts_sw_gate_bwd", pwd.data_ptr(), condd.data_ptr(), ld, off, up, b, length, lm, c, dad.data_ptr(), dpw.data_ptr(),
                  dcond.data_ptr(), ld, _s())
        outs.append((dpw.cpu(), dcond.cpu()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1][:, off:off + 2 * c], outs[1][1][:, off:off + 2 * c])
    dpw, dcond = outs[0]
    assert torch.isnan(dcond[:, :off]).all() and torch.isnan(dcond[:, off + 2 * c:]).all()
    s = pw.double() + cond.double()[:, off:off + 2 * c].repeat_interleave(up, 0)
    t, sg, d = torch.tanh(s[:, :c]), torch.sigmoid(s[:, c:]), da.double()
    want = torch.cat([d * sg * (1 - t * t), d * t * sg * (1 - sg)], 1)
    mag = torch.cat([d.abs(), d.abs()], 1)
    r1 = _ratio(dpw, want, BF * want.abs() + 16 * U * mag)
    wsum, msum = want.view(b * lm, up, 2 * c).sum(1), mag.view(b * lm, up, 2 * c).sum(1)
    r2 = _ratio(dcond[:, off:off + 2 * c], wsum, BF * wsum.abs() + (up + 16) * U * msum)
    print("gate bwd ratios", r1, r2)
    assert r1 <= 1 and r2 <= 1, (r1, r2)


def _dwbn_reference(h, dy, gamma, beta, w, b, length):
    """float64 batch statistics (mean, rstd) of h over its B * L rows."""
    c = h.shape[1]
    h3, dy3 = h.double().view(b, length, c), dy.double().view(b, length, c)
    mean, var = h3.mean((0, 1)), h3.var((0, 1), unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    return mean, rstd


def _dwbn_math(h, dy, mean, rstd, gamma, beta, w, b, length):
    c = h.shape[1]
    h3, dy3 = h.double().view(b, length, c), dy.double().view(b, length, c)
    xh = (h3 - mean.double()) * rstd.double()
    u = gamma.double() * xh + beta.double()
    z = torch.zeros(b, 1, c, dtype=torch.float64)
    ua = gamma.double().abs() * xh.abs() + beta.double().abs()                     # what the roundings inside u are relative to
    up_, un = torch.cat([z, u[:, :-1]], 1), torch.cat([u[:, 1:], z], 1)            # u_{l-1}, u_{l+1}, zero outside the utterance
    upa, una = torch.cat([z, ua[:, :-1]], 1), torch.cat([ua[:, 1:], z], 1)
    dp, dn = torch.cat([z, dy3[:, :-1]], 1), torch.cat([dy3[:, 1:], z], 1)          # dy_{l-1}, dy_{l+1}
    w64 = w.double()
    parts = (w64[:, 0] * dn, w64[:, 1] * dy3, w64[:, 2] * dp)
    du, du_abs = sum(parts), sum(p.abs() for p in parts)
    terms = [dy3 * up_, dy3 * u, dy3 * un, dy3, du * xh, du]
    mags = [dy3.abs() * upa, dy3.abs() * ua, dy3.abs() * una, dy3.abs(), du_abs * xh.abs(), du_abs]
    sums = torch.stack([t.sum((0, 1)) for t in terms])
    mag = torch.stack([t.sum((0, 1)) for t in mags])
    return sums, mag, du, du_abs, xh


@pytest.mark.parametrize("c,b,length,boundary_only", [(32, 3, 20, False), (256, 3, 20, True), (32, 1, 2, False), (64, 5, 333, False)])
def test_depthwise_batchnorm_backward_kernels_vs_float64(gpu, c, b, length, boundary_only):
    """rtts_sw_dwbn_bwd_sums / _apply: B 3 x L 20 (once with dy non-zero ONLY at the first and last row of every utterance: a
    gradient carried across an utterance boundary would show in d w_0 / d w_2 and in dh of the neighbour's edge row), B 1 x L 2,
    and 1665 rows (several slabs, rows not a multiple of anything).  Sums: (m + 16) u sum |terms| with m = B L terms in a
    chain at most (a term's u = gamma xhat + beta counted as |gamma xhat| + |beta|: its roundings are relative to that, not to
    what is left after cancellation); apply (given exact sums): 16 u of the magnitudes it adds.  Measured worst ratios of
    error to bound on an MI355X: sums 0.10 (B 1 x L 2), apply 0.21 (1665 rows)."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(7 * c + length)
    m = b * length
    h = torch.randn(m, c, generator=g) * 1.5 + 0.5
    dy = _bf(torch.randn(m, c, generator=g))
    if boundary_only:
        keep = torch.zeros(b, length, 1)
        keep[:, 0], keep[:, -1] = 1, 1
        dy = (dy.view(b, length, c) * keep.to(dy.dtype)).view(m, c).contiguous()
    gamma, beta, w = torch.randn(c, generator=g), torch.randn(c, generator=g), torch.randn(c, 3, generator=g)
    mean64, rstd64 = _dwbn_reference(h, dy, gamma, beta, w, b, length)
    mean, rstd = mean64.float(), rstd64.float()                # the kernels take the statistics as given: fp32, exact inputs
    want, mag, du, du_abs, xh = _dwbn_math(h, dy, mean, rstd, gamma, beta, w, b, length)
    dev = [t.to(gpu) for t in (h, dy, mean, rstd, gamma, beta, w)]
    ptrs = [t.data_ptr() for t in dev]
    nf = _lib.load().rtts_sw_dwbn_bwd_partial_floats(m, c)
    got = []
    for _ in range(2):
        sums = torch.full((6, c), float("nan"), device=gpu)
        part = torch.full((nf,), float("nan"), device=gpu)
        _lib.call("rtts_sw_dwbn_bwd_sums", *ptrs, b, length, c, sums.data_ptr(), part.data_ptr(), _s())
        got.append(sums.cpu())
    assert torch.equal(got[0], got[1])
    r1 = _ratio(got[0], want, _gamma(m + 16) * mag + 1e-30)
    # apply, with sums given exactly (any fp32 values)
    given = torch.randn(6, c, generator=g)
    dh0 = torch.randn(m, c, generator=g)
    outs = []
    for _ in range(2):
        dh = dh0.to(gpu)
        _lib.call("rtts_sw_dwbn_bwd_apply", *ptrs, given.to(gpu).data_ptr(), b, length, c, dh.data_ptr(), _s())
        outs.append(dh.cpu())
    assert torch.equal(outs[0], outs[1])
    a = (gamma.double() * rstd.double())
    s4, s5 = given[4].double() / m, given[5].double() / m
    want_dh = dh0.double().view(b, length, c) + a * (du - s5 - xh * s4)
    tol = 16 * U * (dh0.double().abs().view(b, length, c) + a.abs() * (du_abs + s5.abs() + xh.abs() * s4.abs()))
    r2 = _ratio(outs[0].view(b, length, c), want_dh, tol)
    print("dwbn bwd ratios", r1, r2)
    assert r1 <= 1 and r2 <= 1, (r1, r2)


BOUNDARY_BWD = [  # (n_in, n_early, rows, ld_wn, coupling, convolution)
    (128, 0, 70, 128, True, True),
    (128, 16, 33, 128, True, True),            # n = 112
    (64, 16, 8300, 64, True, True),            # n = 48; 260 tiles: more than the 256 workgroups, a partial last tile
    (16, 4, 1, 16, True, True),                # n = 12: the toy width
    (112, 0, 45, 112, True, True),             # the flows after the first early output: half 56, rows of 113 words in LDS
    (112, 16, 67, 128, True, True),            # n = 96
    (48, 0, 39, 64, True, True),               # n_in 48 with the coupling, W and dW
    (48, 16, 35, 48, True, True),              # n = 32
    (16, 0, 40, 16, False, True),              # the first flow: only dW
    (48, 48, 77, 64, True, False),             # the tail: the z-seed alone
]


@pytest.mark.parametrize("n_in,n_early,rows,ld_wn,coupled,conv", BOUNDARY_BWD)
def test_boundary_backward_kernel_vs_float64(gpu, n_in, n_early, rows, ld_wn, coupled, conv):
    """rtts_sw_boundary_bwd against float64 with the inputs of the forward kernel's test (unit normal rows, 0.3 x normal WN
    output, orthonormal W): n_in in {128, 112, 64, 48, 16}, n_early in {0, 16, 4}, the first flow (wn_out NULL) and the tail (w NULL).
    dW: (rows + 16) u sum |dout_i| (|e^s x1| + |b|); dc = dout W: (n + 16) u sum |dout_i W_ik|, carried through the coupling's
    factors; the z-seed: 8 u.  Outputs outside the written blocks keep their NaN.  Measured worst ratios of error to bound on an
    MI355X (dW, dx, dwn): n_in 112: 0.04, 0.23, 0.03; n_in 48 with coupling and W: 0.04, 0.23, 0.05; n_in 128: 0.06, 0.23,
    0.03; n_in 64 over 8300 rows: 1e-4, 0.23, 0.61; n_in 16: 0.09, 0.09, 0.03; the tail: dx 0.39, dwn 0.89 (the z-seed through exp)."""
    from reformer_tts_amd import _lib
    g = torch.Generator().manual_seed(300 + n_in + n_early + rows)
    n, half, z_col = n_in - n_early, n_in // 2, 6
    x = torch.randn(rows, n_in, generator=g)
    wn = 0.3 * torch.randn(rows, ld_wn, generator=g)
    w = torch.linalg.qr(torch.randn(max(n, 1), max(n, 1), generator=g))[0].contiguous()
    dout = torch.randn(rows, max(n, 1), generator=g)
    z = torch.randn(rows, z_col + n_early + 5, generator=g)
    z_scale, inv_n = 1.0 / 1920.0, 1.0 / 3840.0
    xd, wnd, wd, doutd, zd = (t.to(gpu) for t in (x, wn, w, dout, z))
    nblk = _lib.load().rtts_sw_boundary_bwd_blocks(rows)
    runs = []
    for _ in range(2):
        nan = lambda *shape: torch.full(shape, float("nan"), device=gpu)      # noqa: E731
        dx, dwn, dw, part = nan(rows, n_in + 3), nan(rows, ld_wn + 2), nan(max(n, 1), max(n, 1)), nan(nblk * max(n, 1) ** 2)
        _lib.call("rtts_sw_boundary_bwd", xd.data_ptr(), n_in, wnd.data_ptr() if coupled else None, ld_wn, wd.data_ptr() if conv else None, n_in,
                  n_early, rows, doutd.data_ptr() if conv else None, dout.shape[1], zd.data_ptr(), z.shape[1], z_col, z_scale, inv_n,
                  dx.data_ptr() if coupled else None, dx.stride(0), dwn.data_ptr() if coupled else None, dwn.stride(0),
                  dw.data_ptr() if conv else None, part.data_ptr() if conv else None, _s())
        runs.append((dx.cpu(), dwn.cpu(), dw.cpu()))
    for a, bb in zip(runs[0], runs[1]):
        assert torch.equal(a.nan_to_num(7.0), bb.nan_to_num(7.0))
    dx, dwn, dw = runs[0]
    x64, wn64, w64, d64 = x.double(), wn.double(), w.double(), dout.double()
    es = torch.exp(wn64[:, :half])
    if coupled:
        c = torch.cat([x64[:, :half], es * x64[:, half:] + wn64[:, half:n_in]], 1)
        cmag = torch.cat([x64[:, :half].abs(), (es * x64[:, half:]).abs() + wn64[:, half:n_in].abs()], 1)
    else:
        c, cmag = x64, x64.abs()
    ratios = []
    if conv:
        ratios.append(_ratio(dw, d64.t() @ c[:, n_early:], _gamma(rows + 16) * (d64.abs().t() @ cmag[:, n_early:])))
    else:
        assert torch.isnan(dw).all()
    if coupled:
        seed = z.double()[:, z_col:z_col + n_early] * z_scale
        dc = torch.cat([seed, d64 @ w64], 1) if conv else seed
        dcmag = torch.cat([seed.abs() * 8 / (n + 16), d64.abs() @ w64.abs()], 1) if conv else seed.abs() * 8 / (n + 16)
        tol = _gamma(n + 16) * dcmag
        x1 = x64[:, half:]
        want_dx = torch.cat([dc[:, :half], dc[:, half:] * es], 1)
        ratios.append(_ratio(dx[:, :n_in], want_dx, torch.cat([tol[:, :half], tol[:, half:] * es], 1)))
        want_dwn = torch.cat([dc[:, half:] * x1 * es - inv_n, dc[:, half:]], 1)
        ratios.append(_ratio(dwn[:, :n_in], want_dwn, torch.cat([tol[:, half:] * (x1 * es).abs() + 2 * U * inv_n, tol[:, half:]], 1)))
        assert torch.isnan(dx[:, n_in:]).all() and torch.isnan(dwn[:, n_in:]).all()
    else:
        assert torch.isnan(dx).all() and torch.isnan(dwn).all()
    print("boundary bwd ratios", ratios)
    assert max(ratios) <= 1, ratios


# ------------------------------------------------------------------ 2.-7. the training step
def _build(golden_dir, case, gpu):
    from reformer_tts_amd.squeeze_wave import SqueezeWave, WNConfig
    cfg, sd, mel, audio = train64.load_train_case(golden_dir, case)
    model = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                        cfg["early_return_size"], WNConfig(**cfg["wn_config"]))
    model.load_state_dict(sd, strict=False)
    return model.to(gpu).train(), mel.to(gpu), audio.to(gpu)


def _step(golden_dir, case, gpu, calls=1):
    """A fresh model, ``calls`` x nll_backward -> (model, losses, {name: gradient on the host})."""
    model, mel, audio = _build(golden_dir, case, gpu)
    losses = [float(model.nll_backward(mel, audio)) for _ in range(calls)]
    torch.cuda.synchronize()
    return model, losses, {n: p.grad.detach().cpu() for n, p in model.named_parameters()}


@pytest.fixture(scope="module")
def steps(golden_dir, gpu):
    """case -> (model after one step, [loss], gradients): computed once, never modified by a test."""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _step(golden_dir, case, gpu)
        return cache[case]
    return get


@pytest.mark.parametrize("case", train64.CASES)
def test_nll_backward_vs_float64(golden_dir, steps, case):
    """Loss, EVERY parameter's gradient, all gradients concatenated, and every BatchNorm's running statistics against the exact
    float64 step, within 4x the rounding model's error (``MODEL_CONST``)."""
    worst, concat, dloss, _, rmean, rvar = train64.MODEL_CONST[case]
    loss64, grads64, stats64 = train64.grads64(golden_dir, case, False)
    model, losses, grads = steps(case)
    print(case, "loss diff", abs(losses[0] - loss64), "bound", 4 * dloss)
    assert set(grads) == set(grads64)
    errs = {n: train64.rel_l2(grads[n], grads64[n]) for n in grads64}
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    cat = train64.concat_rel_l2(grads, grads64)
    print(case, "worst gradients", top, "bound", 4 * worst, "concatenated", cat, "bound", 4 * concat)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    serr = {k: train64.rel_l2(sd[k], stats64[k]) for k in stats64}
    wm = max(v for k, v in serr.items() if k.endswith("running_mean"))
    wv = max(v for k, v in serr.items() if k.endswith("running_var"))
    print(case, "running mean / var", wm, wv, "bounds", 4 * rmean, 4 * rvar)
    assert abs(losses[0] - loss64) <= 4 * dloss
    for n, e in errs.items():
        assert e <= 4 * worst, (n, e)
    assert cat <= 4 * concat
    assert wm <= 4 * rmean and wv <= 4 * rvar
    tracked = [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")]
    assert tracked and all(t == 1 for t in tracked)


@pytest.mark.parametrize("case", ["small", "full/3x10"])
def test_gradients_accumulate_and_runs_are_deterministic(golden_dir, gpu, steps, case):
    """A second call without zero_grad doubles every gradient exactly; two fresh runs from the same start agree bit for bit."""
    _, losses, grads = steps(case)
    _, again_loss, again = _step(golden_dir, case, gpu)
    assert again_loss == losses
    for n, gr in grads.items():
        assert torch.equal(again[n], gr), n                               # two fresh runs: bit for bit
    _, losses2, twice = _step(golden_dir, case, gpu, calls=2)
    assert losses2[0] == losses[0] and losses2[1] == losses[0]          # training-mode statistics: the loss does not move
    for n, gr in grads.items():
        assert torch.equal(twice[n], 2 * gr), n


def test_padding_rows_do_not_reach_the_gradients(golden_dir, gpu, steps):
    """full/3x10 has 60 real rows in 128-row buffers.  With the allocator's free blocks filled with NaN beforehand (poisoned
    allocations of several times what the step needs, freed before the step) the gradients are those of the clean run, bit for bit."""
    _, losses, grads = steps("full/3x10")
    model, mel, audio = _build(golden_dir, "full/3x10", gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    model.nll_backward(mel, audio)
    torch.cuda.synchronize()
    need = torch.cuda.max_memory_allocated() - base
    del model
    torch.cuda.empty_cache()                      # what the caching allocator holds from now on is what gets poisoned below
    model, mel, audio = _build(golden_dir, "full/3x10", gpu)
    # the step's peak once over in each of the block sizes it allocates (64 KB ... 1 MB: the 128-row buffers), and once in large blocks
    nan_words = lambda n: torch.full((n,), 0x7FC07FC0, dtype=torch.int32, device=gpu)     # noqa: E731  NaN as fp32 AND as two bf16
    poison = [nan_words(size // 4) for size in (1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20) for _ in range(need // size + 1)]
    small = [nan_words(need // 32 + 1) for _ in range(8)]
    torch.cuda.synchronize()
    del poison, small
    # the poison is where the step will allocate: fresh buffers of the step's activation sizes come back as NaN
    probes = [torch.empty(128, 256, dtype=torch.bfloat16, device=gpu), torch.empty(128, 512, dtype=torch.bfloat16, device=gpu),
              torch.empty(128, 256, device=gpu), torch.empty(128, 128, device=gpu)]
    assert all(torch.isnan(t[60:]).all() for t in probes), "the allocator did not hand the poisoned blocks back"
    del probes
    loss = float(model.nll_backward(mel, audio))
    torch.cuda.synchronize()
    assert loss == losses[0]
    for n, p in model.named_parameters():
        assert torch.isfinite(p.grad).all(), n
        assert torch.equal(p.grad.cpu(), grads[n]), n


def test_vocoder_trainer_follows_the_float64_sequence(golden_dir, gpu):
    """8 Adam steps on ``small`` with one fixed batch: each loss within 4x the model's worst step difference of the float64
    sequence, the last below the first; validation_loss leaves the mode as it found it."""
    from reformer_tts_amd.squeeze_wave.training import VocoderTrainer
    model, mel, audio = _build(golden_dir, "small", gpu)
    trainer = VocoderTrainer(model)
    batch = {"spectrogram": mel, "audio": audio}
    got = [float(trainer.training_step(batch)) for _ in range(8)]
    want = train64.train64(golden_dir, "small", 8, False)
    bound = 4 * train64.MODEL_CONST["small"][3]
    print("trainer losses", got, "float64", want, "bound", bound)
    for a, b in zip(got, want):
        assert abs(a - b) <= bound, (got, want)
    assert got[-1] < got[0]
    for mode in (True, False):
        model.train(mode)
        val = trainer.validation_loss([(mel, audio)])
        assert model.training is mode and torch.isfinite(val)
    model.eval()
    assert float(trainer.validation_loss([(mel, audio)])) == float(model.nll(mel, audio))


def test_refusals(golden_dir, gpu):
    from reformer_tts_amd import _lib
    model, mel, audio = _build(golden_dir, "small", gpu)
    with pytest.raises(_lib.RttsError, match="needs training mode"):
        model.eval().nll_backward(mel, audio)
    model.train()
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model.nll_backward(mel.cpu(), audio)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        model.nll_backward(mel, audio.cpu())
    with pytest.raises(ValueError, match="audio"):
        model.nll_backward(mel, audio[:, :-256])
    with pytest.raises(_lib.RttsError, match="needs eval mode"):
        model((mel, audio))
    with pytest.raises(_lib.RttsError, match="needs eval mode"):
        model.nll(mel, audio)
    assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("case", ["small", "full/3x10"])
def test_eval_path_is_unchanged_after_a_training_step(golden_dir, gpu, steps, case):
    """After nll_backward and .eval(), nll is bitwise that of a freshly built model loaded with the same state_dict."""
    model, _, _ = steps(case)
    fresh, mel, audio = _build(golden_dir, case, gpu)
    fresh.load_state_dict(model.state_dict())
    was = model.training
    try:
        a = model.eval().nll(mel, audio)
        b = fresh.eval().nll(mel, audio)
        assert torch.isfinite(a) and torch.equal(a, b)
    finally:
        model.train(was)
