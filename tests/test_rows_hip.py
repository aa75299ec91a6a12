"""Row kernels of the stack executor called through the C-ABI, against float64 torch (reference: torch.nn.LayerNorm's backward,
reformer_tts/model/reformer.py:85-93 for the two streams that start as one input)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("m,d", [(3072, 512), (1000, 128)])
@pytest.mark.parametrize("form", ["in place", "out of place", "joining"])
def test_layer_norm_backward_forms(gpu, m, d, form):
    """rtts_ln_bwd_join: dx_out = dx_in + addend + dLN(dxn); the LayerNorm parameter gradients through the partial rows.
    'joining' is the last update of a reversible stack's backward: d(input) = g1 + g2 rides in the pass that completes g2."""
    from reformer_tts_amd import _lib
    torch.manual_seed(m + d)
    x = torch.randn(m, d, device=gpu) * 2.0 + 0.3
    gamma = torch.rand(d, device=gpu) + 0.5
    dxn = torch.randn(m, d, device=gpu).bfloat16()
    dx_in = torch.randn(m, d, device=gpu)
    addend = torch.randn(m, d, device=gpu)
    mean = x.mean(-1)
    rstd = (x.var(-1, unbiased=False) + 1e-5).rsqrt()
    # float64 reference
    x64 = x.double().requires_grad_()
    g64 = gamma.double().requires_grad_()
    b64 = torch.zeros(d, dtype=torch.float64, device=gpu, requires_grad=True)
    y = torch.nn.functional.layer_norm(x64, (d,), g64, b64, 1e-5)
    y.backward(dxn.double())
    want = dx_in.double() + x64.grad + (addend.double() if form == "joining" else 0.0)
    out = dx_in.clone() if form == "in place" else torch.empty_like(dx_in)
    src = out if form == "in place" else dx_in
    dgamma = torch.zeros(d, device=gpu)
    dbeta = torch.zeros(d, device=gpu)
    ws = torch.empty(2 * 256 * d, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("rtts_ln_bwd_join", dxn.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), src.data_ptr(),
              addend.data_ptr() if form == "joining" else None, out.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), m, d,
              None, None, 0.0, 0, None, stream)
    torch.cuda.synchronize()
    assert float((out.double() - want).abs().max() / want.abs().max()) < 2e-6
    assert float((dgamma.double() - g64.grad).norm() / g64.grad.norm()) < 1e-5
    assert float((dbeta.double() - b64.grad).norm() / b64.grad.norm()) < 1e-5
    if form == "joining":
        with pytest.raises(_lib.RttsError):          # the addend must not be the output
            _lib.call("rtts_ln_bwd_join", dxn.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), src.data_ptr(),
                      out.data_ptr(), out.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), m, d, None, None, 0.0, 0, None, stream)


@pytest.mark.parametrize("b,lp,lm", [(3, 200, 1024), (2, 256, 777), (1, 1, 1)])
def test_batch_masks_match_the_reference_sequence(gpu, b, lp, lm):
    """rtts_batch_masks against the operator sequence of reformer_tts.py:119-125 with the frame mask of wrappers.py:60
    (loss_mask.mean(-1)): padded phonemes, phoneme mask and its inverse, padded frame mask -- exact."""
    from reformer_tts_amd.model.reformer_tts import ReformerTTS, pad_to_multiple
    torch.manual_seed(b * 1000 + lp)
    pad_base, n_mels = 256, 80
    phon = torch.randint(0, 5, (b, lp), device=gpu)                        # zeros inside the text too: mask = (id != 0), not a length
    loss_mask = (torch.rand(b, lm, 1, device=gpu) > 0.3).float().expand(b, lm, n_mels).contiguous()
    loss_mask[:, lm // 2:] *= torch.rand(b, lm - lm // 2, n_mels, device=gpu)    # fractional rows: mean != 0 unless the whole row is 0
    spec = torch.randn(b, lm, n_mels, device=gpu)

    class _Stub:
        pad_base = 256
        _require_gpu = staticmethod(lambda: None)
    got = ReformerTTS._encode_inputs_fused(_Stub, phon, spec, loss_mask)
    want = ReformerTTS._encode_inputs(_Stub, phon, spec, loss_mask.mean(dim=-1))
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w)
    assert torch.equal(got[1]._rtts_not, ~want[1])
    # a strided view of the masks (frames [0, L-1) of a longer tensor), as the trainer hands it over
    longer = torch.cat([loss_mask, loss_mask[:, :1]], dim=1)
    got2 = ReformerTTS._encode_inputs_fused(_Stub, phon, spec, longer[:, :-1])
    assert torch.equal(got2[2], want[2])


def test_embedding_backward_reads_a_strided_gradient_in_place(gpu):
    """rtts_embedding_bwd_strided: dx as a (B, L, C) view of halo rows (what the convolution stack's backward hands to the embedding:
    edges.Halo.valid) gives bit for bit the gradient of the contiguous copy through rtts_embedding_bwd, with and without the
    dropout mask (keyed by the LOGICAL row); reference modules.py:17,22,56 (nn.Embedding(padding_idx=0) + Dropout)."""
    from reformer_tts_amd import _lib
    from reformer_tts_amd._seeds import seed_base
    torch.manual_seed(3)
    b, l, c, n = 5, 200, 128, 77
    halo = torch.randn(b, l + 4, c + 64, device=gpu)                 # a larger array: row stride c + 64, batch stride (l + 4) rows
    dx = halo[:, 2:2 + l, :c]
    assert not dx.is_contiguous() and dx.stride(2) == 1
    ids = torch.randint(0, n, (b * l,), device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    for p, seed in ((0.0, 0), (0.1, 4242)):
        d_ref, d_str = torch.zeros(n, c, device=gpu), torch.zeros(n, c, device=gpu)
        flat = dx.reshape(-1, c).contiguous()
        _lib.call("rtts_embedding_bwd", ids.data_ptr(), flat.data_ptr(), b * l, c, n, 0, d_ref.data_ptr(), p, seed, seed_base(gpu).data_ptr(), s)
        _lib.call("rtts_embedding_bwd_strided", ids.data_ptr(), dx.data_ptr(), dx.stride(0), dx.stride(1), l, b * l, c, n, 0, d_str.data_ptr(), p, seed,
                  seed_base(gpu).data_ptr(), s)
        torch.cuda.synchronize()
        assert torch.equal(d_ref, d_str)
        assert float(d_ref[0].abs().max()) == 0.0 and float(d_ref[1:].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------
# Every row entry point at every width of csrc/fused_rows.hip's FR_DISPATCH_D (tests/test_cabi_cpu.py checks that this
# tuple IS that list), against float64.  Column sums, casts and elementwise epilogues are compared bit for bit on inputs that
# are multiples of 2^-4 (exact in bf16, every partial sum exact in fp32); LayerNorm statistics and gradients under fp32 error
# bounds written out below.
WIDTHS = (128, 256, 384, 512, 768, 1024, 2048)
# rows: fewer than a workgroup's 4 waves, a partial last workgroup, exactly the 256-workgroup cap of the partial rows and one
# row past it (block 0 then owns rows 0..3 and 1024), several rows per wave of the grid-stride loops
ROWS = (1, 3, 5, 1023, 1024, 1025, 4099)
U = 2.0 ** -24                 # fp32 unit roundoff
PARTIAL_CAP = 256              # FR_PARTIAL_BLOCKS
_RATIOS = {}                   # largest error / bound seen per check (printed when the module ends: run with -s to see them)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k in sorted(_RATIOS):
        print(f"error/bound {k}: {_RATIOS[k]:.4f}")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _grid(shape, lo, hi, gen, dev, dtype=torch.float32):
    """Multiples of 2^-4 in [lo, hi]: exact in bf16 and fp32."""
    return (torch.randint(int(lo * 16), int(hi * 16) + 1, shape, generator=gen, device=dev).to(torch.float64) / 16).to(dtype)


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _within(name, got, want, bound):
    """|got - want| <= bound elementwise (float64); records the largest ratio."""
    err = (got.double() - want.double()).abs()
    assert not torch.isnan(got).any(), name
    ratio = float((err / bound).max())
    _RATIOS[name] = max(_RATIOS.get(name, 0.0), ratio)
    assert ratio <= 1.0, f"{name}: error {float(err.max()):.3e} exceeds its fp32 bound (ratio {ratio:.3f})"


def _bf16_ulp(v):
    """One bf16 ulp at |v| (float64): 2^(e - 8) for |v| = m * 2^e, m in [0.5, 1)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 8)


def _check_bf16(name, got, want64, e_pre):
    """bf16 output of a float64 value computed in fp32 with error <= e_pre before the rounding: within one bf16 ulp (widened
    by e_pre where the fp32 value cancels towards zero), and all but a handful equal to the round-to-nearest-even of the
    float64 value (they can differ only where the fp32 value lies on the other side of a rounding boundary)."""
    _within(name, got.double(), want64, _bf16_ulp(want64) + e_pre)
    mismatch = int((_bits(got) != _bits(want64.float().bfloat16())).sum())
    _RATIOS[name + " (fraction not RNE)"] = max(_RATIOS.get(name + " (fraction not RNE)", 0.0), mismatch / got.numel())
    assert mismatch <= 2 + 2e-3 * got.numel(), f"{name}: {mismatch} of {got.numel()} values are not the nearest bf16"


def _epl(d):
    return d // 64


def _partial_rows(m):
    return min((m + 3) // 4, PARTIAL_CAP)


def _sum_depth(m):
    """Additions on the longest path of a column sum over m rows: the rows one wave walks in the grid-stride loop, the 4-wave
    partial row, then the final reduction over the partial rows (colsum_final: nrows/4 per wave + 2 levels; the grouped
    form: <= 16 per wave in pairs + 4 levels + the 16-wave reduction)."""
    blocks = _partial_rows(m)
    return -(-m // (4 * blocks)) + 3 + -(-blocks // 4) + 8


def _drop_keep(gpu, m, d, p, seed, sd):
    """Keep-scale (0 or 1/(1-p) in fp32) of every element of an (m, d) block, read back through rtts_residual_epilogue: the flat
    index row * d + column is the key every row kernel must use."""
    from reformer_tts_amd import _lib
    x = torch.zeros(m, d, device=gpu)
    g = torch.ones(m, d, dtype=torch.bfloat16, device=gpu)
    _lib.call("rtts_residual_epilogue", x.data_ptr(), g.data_ptr(), None, 1.0, x.data_ptr(), m, d, p, seed, sd.data_ptr(), _s())
    return x


def _finalise(jobs):
    """rtts_colsum_final_grouped over [(partial tensor, byte offset in floats, nrows, n, ld, out)]."""
    from reformer_tts_amd import _lib
    arr = (_lib.ColsumJob * len(jobs))()
    for j, (partial, off, rows, n, ld, out) in zip(arr, jobs):
        j.partial, j.out, j.nrows, j.n, j.ld = partial.data_ptr() + 4 * off, out.data_ptr(), rows, n, ld
    _lib.call("rtts_colsum_final_grouped", arr, len(jobs), _s())


def _stats64(x64):
    mu = x64.mean(-1)
    var = ((x64 - mu[:, None]) ** 2).mean(-1)
    return mu, (var + 1e-5).rsqrt()


def _ln_bounds(x64, gamma64, beta64, epl):
    """fp32 error bounds of ln_fwd_kernel / residual_ln_kernel (first order, doubled for the fused multiply-adds the build may form):
    mean: EPL sequential adds per lane + 6 butterfly levels + the rounded 1/D; rstd: half the relative error of the variance
    (its sum, the rounded centred values, 1/D, + eps) + 2 ulp of rsqrtf; xn before its bf16 rounding: the centred value's
    absolute error (mean error + rounding) and rstd's relative error through gamma, + 2 roundings."""
    mu, rstd = _stats64(x64)
    e_mu = 2 * (epl + 8) * U * x64.abs().mean(-1)
    rel_rstd = 2 * ((epl + 10) / 2 + 4) * U
    xc = (x64 - mu[:, None]).abs()
    e_xn = 2 * (gamma64.abs() * rstd[:, None] * (e_mu[:, None] + U * xc) + gamma64.abs() * xc * rstd[:, None] * (rel_rstd + 2 * U)
                + U * (gamma64.abs() * xc * rstd[:, None] + beta64.abs()))
    return e_mu, rel_rstd * rstd, e_xn


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_ln_fwd_against_float64(gpu, d, m):
    """rtts_ln_fwd: xn (bf16), mean and rstd against torch.nn.functional.layer_norm in float64."""
    from reformer_tts_amd import _lib
    gen = torch.Generator(device=gpu).manual_seed(d * 7 + m)
    x = torch.randn(m, d, generator=gen, device=gpu) * 1.5 + 0.7         # non-zero mean: the centring matters
    gamma = torch.rand(d, generator=gen, device=gpu) + 0.5
    beta = torch.randn(d, generator=gen, device=gpu) * 0.3
    xn, mean, rstd = _nan((m, d), gpu, torch.bfloat16), _nan((m,), gpu), _nan((m,), gpu)
    _lib.call("rtts_ln_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), m, d, _s())
    torch.cuda.synchronize()
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    mu, rs = _stats64(x64)
    e_mu, e_rs, e_xn = _ln_bounds(x64, g64, b64, _epl(d))
    _within("ln_fwd mean", mean, mu, e_mu)
    _within("ln_fwd rstd", rstd, rs, e_rs)
    _check_bf16("ln_fwd xn", xn, torch.nn.functional.layer_norm(x64, (d,), g64, b64, 1e-5), e_xn)


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_residual_ln_against_epilogue_and_float64(gpu, d, m):
    """rtts_residual_ln: y = x + sign * dropout(g + bias) equals rtts_residual_epilogue bit for bit (sign +-1, bias present / NULL,
    in place / out of place, dropout with a device seed word), and xn / mean / rstd equal LayerNorm(y) within the fp32 bound."""
    from reformer_tts_amd import _lib
    gen = torch.Generator(device=gpu).manual_seed(d * 11 + m)
    x0 = torch.randn(m, d, generator=gen, device=gpu) + 0.4
    g = torch.randn(m, d, generator=gen, device=gpu).bfloat16()
    bias = torch.randn(d, generator=gen, device=gpu) * 0.5
    gamma = torch.rand(d, generator=gen, device=gpu) + 0.5
    beta = torch.randn(d, generator=gen, device=gpu) * 0.3
    sd = torch.tensor([17], dtype=torch.int32, device=gpu)
    for sign, with_bias, in_place, p in ((1.0, True, True, 0.0), (-1.0, False, False, 0.0), (-1.0, True, False, 0.15),
                                         (1.0, False, True, 0.15)):
        b = bias if with_bias else None
        want_y = _nan((m, d), gpu)
        _lib.call("rtts_residual_epilogue", x0.data_ptr(), g.data_ptr(), _p(b), sign, want_y.data_ptr(), m, d, p, 4242, sd.data_ptr(), _s())
        x = x0.clone()
        y = None if in_place else _nan((m, d), gpu)
        xn, mean, rstd = _nan((m, d), gpu, torch.bfloat16), _nan((m,), gpu), _nan((m,), gpu)
        _lib.call("rtts_residual_ln", x.data_ptr(), g.data_ptr(), _p(b), sign, gamma.data_ptr(), beta.data_ptr(), xn.data_ptr(),
                  mean.data_ptr(), rstd.data_ptr(), m, d, p, 4242, sd.data_ptr(), _p(y), _s())
        torch.cuda.synchronize()
        got_y = x if in_place else y
        assert _same_bits(got_y, want_y), (sign, with_bias, in_place, p)
        if not in_place:
            assert _same_bits(x, x0)
        y64 = got_y.double()
        mu, rs = _stats64(y64)
        e_mu, e_rs, e_xn = _ln_bounds(y64, gamma.double(), beta.double(), _epl(d))
        _within("residual_ln mean", mean, mu, e_mu)
        _within("residual_ln rstd", rstd, rs, e_rs)
        _check_bf16("residual_ln xn", xn, torch.nn.functional.layer_norm(y64, (d,), gamma.double(), beta.double(), 1e-5), e_xn)


_LN_BWD_ENTRIES = ("rtts_ln_bwd", "rtts_ln_bwd_to", "rtts_ln_bwd_join")


def _ln_bwd_call(entry, dxn, x, mean, rstd, gamma, dx_in, addend, out, dgamma, dbeta, ws, m, d, dyb_next, pn, p, sd):
    from reformer_tts_amd import _lib
    head = (dxn.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr())
    tail = (_p(dgamma), _p(dbeta), ws.data_ptr(), m, d, _p(dyb_next), _p(pn), p, 4242, sd.data_ptr(), _s())
    if entry == "rtts_ln_bwd":
        _lib.call(entry, *head, out.data_ptr(), *tail)
    elif entry == "rtts_ln_bwd_to":
        _lib.call(entry, *head, dx_in.data_ptr(), out.data_ptr(), *tail)
    else:
        _lib.call(entry, *head, dx_in.data_ptr(), addend.data_ptr(), out.data_ptr(), *tail)


def _run_ln_bwd(gpu, entry, dxn, x, mean, rstd, gamma, dx_in, addend, nxt_p, grouped, init_g, init_b, sd):
    """One LayerNorm backward through ``entry``; with ``grouped`` dgamma = dbeta = NULL and the partial rows are finalised by
    rtts_colsum_final_grouped (the engine's deferred form).  ``nxt_p`` None: no dyb_next; else its dropout p.
    -> (dx_out, dgamma, dbeta, dyb_next, column sums of partial_next)."""
    m, d = x.shape
    out = dx_in.clone() if entry == "rtts_ln_bwd" else _nan((m, d), gpu)
    dgamma, dbeta = init_g.clone(), init_b.clone()
    ws = _nan((2 * PARTIAL_CAP * d,), gpu)
    dyb = pn = sn = None
    if nxt_p is not None:
        dyb, pn, sn = _nan((m, d), gpu, torch.bfloat16), _nan((PARTIAL_CAP * d,), gpu), init_b.clone()
    _ln_bwd_call(entry, dxn, x, mean, rstd, gamma, dx_in, addend, out, None if grouped else dgamma, None if grouped else dbeta, ws, m, d,
                 dyb, pn, nxt_p or 0.0, sd)
    rows = _partial_rows(m)
    jobs = [(ws, 0, rows, d, d, dgamma), (ws, PARTIAL_CAP * d, rows, d, d, dbeta)] if grouped else []
    if nxt_p is not None:
        jobs.append((pn, 0, rows, d, d, sn))
    if jobs:
        _finalise(jobs)
    torch.cuda.synchronize()
    return out, dgamma, dbeta, dyb, sn


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_ln_bwd_column_sums_exact(gpu, d, m):
    """rtts_ln_bwd / _to / _join with and without dyb_next (+ dropout p = 0.5, keep-scale 2) and with dgamma = dbeta = NULL
    + grouped finalisation, on exact inputs: mean 0, rstd 1 and x on the 2^-4 grid make xhat = x; gamma = 0 makes
    dx_out = dx_in (+ addend) exactly.  dgamma, dbeta, the partial_next sums (accumulated into non-zero outputs) and dyb_next are
    then exact in fp32 and must match float64 bit for bit on every path."""
    gen = torch.Generator(device=gpu).manual_seed(d * 13 + m)
    x = _grid((m, d), -2, 2, gen, gpu)
    dxn = _grid((m, d), -2, 2, gen, gpu, torch.bfloat16)
    dx_in, addend = _grid((m, d), -4, 4, gen, gpu), _grid((m, d), -4, 4, gen, gpu)
    mean, rstd, gamma = torch.zeros(m, device=gpu), torch.ones(m, device=gpu), torch.zeros(d, device=gpu)
    init_g, init_b = _grid((d,), -8, 8, gen, gpu), _grid((d,), -8, 8, gen, gpu)
    sd = torch.tensor([5], dtype=torch.int32, device=gpu)
    want_g = (init_g.double() + (dxn.double() * x.double()).sum(0)).float()
    want_b = (init_b.double() + dxn.double().sum(0)).float()
    keep = _drop_keep(gpu, m, d, 0.5, 4242, sd)
    for entry in _LN_BWD_ENTRIES:
        want_dx = (dx_in.double() + (addend.double() if entry == "rtts_ln_bwd_join" else 0.0)).float()
        for nxt_p in (None, 0.0, 0.5):
            for grouped in (False, True):
                dx, dg, db, dyb, sn = _run_ln_bwd(gpu, entry, dxn, x, mean, rstd, gamma, dx_in, addend, nxt_p, grouped, init_g, init_b, sd)
                where = (entry, nxt_p, grouped)
                assert _same_bits(dx, want_dx), where
                assert _same_bits(dg, want_g), where
                assert _same_bits(db, want_b), where
                if nxt_p is not None:
                    k = keep.double() if nxt_p else 1.0
                    assert _same_bits(dyb, (want_dx.double() * k).bfloat16()), where
                    assert _same_bits(sn, (init_b.double() + (want_dx.double() * k).sum(0)).float()), where


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_ln_bwd_against_float64(gpu, d, m):
    """rtts_ln_bwd / _to / _join on N(0,1)-style data against the float64 LayerNorm backward at the same mean / rstd inputs:
    dx within its fp32 bound, dgamma / dbeta within the column-sum bound on both the direct and the grouped-finalisation path,
    dyb_next (dropout p = 0.15) = bf16(dx_out * keep-scale) bit for bit and within one bf16 ulp of float64, partial_next within
    the column-sum bound; two launches are bit-identical."""
    gen = torch.Generator(device=gpu).manual_seed(d * 17 + m)
    x = torch.randn(m, d, generator=gen, device=gpu) * 2.0 + 0.3
    gamma = torch.rand(d, generator=gen, device=gpu) + 0.5
    dxn = torch.randn(m, d, generator=gen, device=gpu).bfloat16()
    dx_in, addend = torch.randn(m, d, generator=gen, device=gpu), torch.randn(m, d, generator=gen, device=gpu)
    mu64, rs64 = _stats64(x.double())
    mean, rstd = mu64.float(), rs64.float()
    init_g, init_b = torch.randn(d, generator=gen, device=gpu), torch.randn(d, generator=gen, device=gpu)
    sd = torch.tensor([9], dtype=torch.int32, device=gpu)
    epl = _epl(d)
    # float64 reference at the kernel's own (fp32) mean / rstd
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    gg = dxn.double() * gamma.double()
    s1, s2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    dln = rstd.double()[:, None] * (gg - s1 - xh * s2)
    rs = rstd.double()[:, None]
    # dx: xhat (2 roundings), g = dxn * gamma (1), s1 / s2 (EPL + 6 adds + 1/D, + the errors of their terms), the bracket (3),
    # rstd * bracket (1), the adds of dx_in / addend (2); doubled for the fused multiply-adds
    e_bracket = (4 * gg.abs() + 4 * s1.abs() + (epl + 8) * gg.abs().mean(-1, keepdim=True)
                 + xh.abs() * ((epl + 11) * (gg * xh).abs().mean(-1, keepdim=True) + 6 * s2.abs()))
    depth = _sum_depth(m)
    for entry in _LN_BWD_ENTRIES:
        add = addend.double() if entry == "rtts_ln_bwd_join" else 0.0
        want_dx = dx_in.double() + add + dln
        e_dx = 2 * U * (2 * (dx_in.double().abs() + (addend.double().abs() if entry == "rtts_ln_bwd_join" else 0.0)) + 2 * want_dx.abs()
                        + rs * e_bracket)
        want_g = init_g.double() + (dxn.double() * xh).sum(0)
        want_b = init_b.double() + dxn.double().sum(0)
        e_g = 2 * U * ((depth + 3) * (dxn.double() * xh).abs().sum(0) + init_g.double().abs())
        e_b = 2 * U * (depth * dxn.double().abs().sum(0) + init_b.double().abs())
        keep = _drop_keep(gpu, m, d, 0.15, 4242, sd)
        results = {}
        for nxt_p in (None, 0.15):
            for grouped in (False, True):
                dx, dg, db, dyb, sn = _run_ln_bwd(gpu, entry, dxn, x, mean, rstd, gamma, dx_in, addend, nxt_p, grouped, init_g, init_b, sd)
                results[(nxt_p, grouped)] = (dx, dg, db)
                _within("ln_bwd dx", dx, want_dx, e_dx)
                _within("ln_bwd dgamma", dg, want_g, e_g)
                _within("ln_bwd dbeta", db, want_b, e_b)
                if nxt_p is not None:
                    assert _same_bits(dyb, (dx * keep).bfloat16()), (entry, grouped)
                    k64 = keep.double()
                    _check_bf16("ln_bwd dyb_next", dyb, want_dx * k64, e_dx * k64 + U * (want_dx * k64).abs())
                    e_n = 2 * U * ((depth + 1) * (want_dx * k64).abs().sum(0) + init_b.double().abs()) + (e_dx * k64).sum(0)
                    _within("ln_bwd partial_next", sn, init_b.double() + (want_dx * k64).sum(0), e_n)
        # dx does not depend on the path; the grouped finalisation agrees with the direct one (bound: two column-sum bounds)
        for key, (dx, dg, db) in results.items():
            assert _same_bits(dx, results[(None, False)][0]), (entry, key)
            _within("ln_bwd dgamma grouped vs direct", dg, results[(None, False)][1].double(), 2 * e_g)
            _within("ln_bwd dbeta grouped vs direct", db, results[(None, False)][2].double(), 2 * e_b)
        again = _run_ln_bwd(gpu, entry, dxn, x, mean, rstd, gamma, dx_in, addend, 0.15, True, init_g, init_b, sd)
        first = _run_ln_bwd(gpu, entry, dxn, x, mean, rstd, gamma, dx_in, addend, 0.15, True, init_g, init_b, sd)
        assert all(_same_bits(a, b) for a, b in zip(again, first)), entry


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_cast_colsum_exact(gpu, d, m):
    """rtts_cast_colsum: dyb = bf16(dy [* scale_dev] [* keep-scale]) and dbias += column sums, exact on 2^-4 grid inputs
    (scale 0.75, dropout p = 0.5 with a device seed word); dbias = NULL + grouped finalisation in column blocks of the d-wide
    partial rows (ld = d: engine.cast_colsum(blocks=...)); two launches are bit-identical."""
    from reformer_tts_amd import _lib
    gen = torch.Generator(device=gpu).manual_seed(d * 19 + m)
    dy = _grid((m, d), -4, 4, gen, gpu)
    init = _grid((d,), -8, 8, gen, gpu)
    sd = torch.tensor([3], dtype=torch.int32, device=gpu)
    scale = torch.tensor([0.75], device=gpu)
    keep = _drop_keep(gpu, m, d, 0.5, 777, sd)
    rows = _partial_rows(m)
    cuts = [0, 80, 81, 81 + (d - 81) // 2, d]          # blocks of 80, 1, ... columns (not multiples of 64)
    for p, sc in ((0.0, None), (0.5, scale), (0.0, scale), (0.5, None)):
        v = dy.double() * (0.75 if sc is not None else 1.0) * (keep.double() if p else 1.0)
        want_b = (init.double() + v.sum(0)).float()
        outs = []
        for grouped in (False, True):
            dyb, dbias, ws = _nan((m, d), gpu, torch.bfloat16), init.clone(), _nan((PARTIAL_CAP * d,), gpu)
            _lib.call("rtts_cast_colsum", dy.data_ptr(), dyb.data_ptr(), None if grouped else dbias.data_ptr(), ws.data_ptr(), m, d, p, 777,
                      sd.data_ptr(), _p(sc), _s())
            if grouped:
                _finalise([(ws, c0, rows, c1 - c0, d, dbias[c0:c1]) for c0, c1 in zip(cuts, cuts[1:])])
            torch.cuda.synchronize()
            assert _same_bits(dyb, v.bfloat16()), (p, sc is not None, grouped)
            assert _same_bits(dbias, want_b), (p, sc is not None, grouped)
            outs.append((dyb, dbias))
        dyb2, dbias2, ws2 = _nan((m, d), gpu, torch.bfloat16), init.clone(), _nan((PARTIAL_CAP * d,), gpu)
        _lib.call("rtts_cast_colsum", dy.data_ptr(), dyb2.data_ptr(), dbias2.data_ptr(), ws2.data_ptr(), m, d, p, 777,
                  sd.data_ptr(), _p(sc), _s())
        torch.cuda.synchronize()
        assert _same_bits(dyb2, outs[0][0]) and _same_bits(dbias2, outs[0][1])


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_colsum_bf16_exact(gpu, d, m):
    """rtts_colsum_bf16: dbias += column sums of dh, or of dh * (h > 0) * gate_scale (relu_gate 1, written in place or to
    gated_out), with a row stride ld > d; columns d..ld of every strided buffer are untouched (NaN sentinels), the sums exact."""
    from reformer_tts_amd import _lib
    gen = torch.Generator(device=gpu).manual_seed(d * 23 + m)
    ld = d + 72
    dh0 = _nan((m, ld), gpu, torch.bfloat16)
    dh0[:, :d] = _grid((m, d), -2, 2, gen, gpu, torch.bfloat16)
    h = _nan((m, ld), gpu, torch.bfloat16)
    h[:, :d] = _grid((m, d), -1, 1, gen, gpu, torch.bfloat16)        # zeros among them: h > 0 is strict
    init = _grid((d,), -8, 8, gen, gpu)
    rows = _partial_rows(m)
    for relu, gs, gated_out, stride, grouped in ((0, 1.0, False, ld, False), (0, 1.0, False, d, True), (1, 1.25, False, ld, False),
                                                (1, 1.25, True, ld, True), (1, 1.0, True, d, False), (1, 0.5, False, d, True)):
        if stride == d:
            dh, hh = dh0[:, :d].contiguous(), h[:, :d].contiguous()
        else:
            dh, hh = dh0.clone(), h
        out = _nan(dh.shape, gpu, torch.bfloat16) if gated_out else None
        v = dh[:, :d].double()
        if relu:
            v = torch.where(hh[:, :d].double() > 0, v * gs, torch.zeros_like(v))
        dbias, ws = init.clone(), _nan((PARTIAL_CAP * d,), gpu)
        _lib.call("rtts_colsum_bf16", dh.data_ptr(), _p(hh if relu else None), stride, None if grouped else dbias.data_ptr(), ws.data_ptr(),
                  m, d, relu, gs, _p(out), _s())
        if grouped:
            _finalise([(ws, 0, rows, d, d, dbias)])
        torch.cuda.synchronize()
        where = (relu, gs, gated_out, stride, grouped)
        assert _same_bits(dbias, (init.double() + v.sum(0)).float()), where
        dst = out if gated_out else dh
        src_unchanged = dh0 if stride == ld else dh0[:, :d]
        if relu:
            assert _same_bits(dst[:, :d], v.bfloat16()), where
        if not relu or gated_out:
            assert _same_bits(dh[:, :d], src_unchanged[:, :d]), where     # not gated in place: dh stays as it was
        if stride == ld:
            assert torch.isnan(dh[:, d:].float()).all() and (out is None or torch.isnan(out[:, d:].float()).all()), where


@pytest.mark.parametrize("njobs", [1, 2, 7, 16])
def test_colsum_final_grouped_mixed_jobs(gpu, njobs):
    """rtts_colsum_final_grouped: up to 16 jobs of mixed width n (not multiples of 64), row stride ld >= n (columns n..ld NaN:
    never read) and 1..300 partial rows (past 256: the remainder loop), added into non-zero outputs -- exact."""
    from reformer_tts_amd import _lib
    gen = torch.Generator(device=gpu).manual_seed(njobs)
    cpu = torch.Generator().manual_seed(njobs)
    nrows_set = (1, 3, 16, 63, 255, 256, 257, 300)
    jobs, wants = [], []
    for i in range(njobs):
        n = int(torch.randint(1, 300, (1,), generator=cpu)) | 1
        ld = n + int(torch.randint(0, 40, (1,), generator=cpu))
        nrows = nrows_set[(i + njobs) % len(nrows_set)]
        partial = _nan((nrows, ld), gpu)
        partial[:, :n] = _grid((nrows, n), -16, 16, gen, gpu)
        out = _grid((n,), -8, 8, gen, gpu)
        wants.append((out.double() + partial[:, :n].double().sum(0)).float())
        jobs.append((partial, 0, nrows, n, ld, out))
    _finalise(jobs)
    torch.cuda.synchronize()
    for (partial, _, nrows, n, ld, out), want in zip(jobs, wants):
        assert _same_bits(out, want), (nrows, n, ld)
    # ld = 0 means ld = n
    partial = _grid((300, 77), -16, 16, gen, gpu)
    out = torch.zeros(77, device=gpu)
    arr = (_lib.ColsumJob * 1)()
    arr[0].partial, arr[0].out, arr[0].nrows, arr[0].n, arr[0].ld = partial.data_ptr(), out.data_ptr(), 300, 77, 0
    _lib.call("rtts_colsum_final_grouped", arr, 1, _s())
    torch.cuda.synchronize()
    assert _same_bits(out, partial.double().sum(0).float())


@pytest.mark.parametrize("d", WIDTHS)
def test_dropout_key_is_the_flat_index_at_every_width(gpu, d):
    """The keep decision of residual_ln, cast_colsum and ln_bwd's dyb_next is keyed by row * d + column of the element a lane
    holds (row_col<VEC>, VEC = 2 at d = 128 and 384): it must equal the flat-index mask of rtts_residual_epilogue."""
    from reformer_tts_amd import _lib
    m, p, seed = 37, 0.15, 4242
    sd = torch.tensor([99], dtype=torch.int32, device=gpu)
    keep = _drop_keep(gpu, m, d, p, seed, sd)
    assert abs(float((keep > 0).double().mean()) - (1 - p)) < 0.03
    ones_bf, ones = torch.ones(m, d, dtype=torch.bfloat16, device=gpu), torch.ones(m, d, device=gpu)
    zeros_d, zeros_m = torch.zeros(d, device=gpu), torch.zeros(m, device=gpu)
    x = torch.zeros(m, d, device=gpu)
    xn, mean, rstd = _nan((m, d), gpu, torch.bfloat16), _nan((m,), gpu), _nan((m,), gpu)
    _lib.call("rtts_residual_ln", x.data_ptr(), ones_bf.data_ptr(), None, 1.0, ones.data_ptr(), zeros_d.data_ptr(), xn.data_ptr(),
              mean.data_ptr(), rstd.data_ptr(), m, d, p, seed, sd.data_ptr(), None, _s())
    dyb, ws = _nan((m, d), gpu, torch.bfloat16), _nan((2 * PARTIAL_CAP * d,), gpu)
    _lib.call("rtts_cast_colsum", ones.data_ptr(), dyb.data_ptr(), None, ws.data_ptr(), m, d, p, seed, sd.data_ptr(), None, _s())
    # ln_bwd with gamma = 0 and dxn = 0: dx_out = dx_in = 1 exactly, so dyb_next is the keep-scale itself
    out, nxt, pn = _nan((m, d), gpu), _nan((m, d), gpu, torch.bfloat16), _nan((PARTIAL_CAP * d,), gpu)
    dxn0, rstd1 = torch.zeros(m, d, dtype=torch.bfloat16, device=gpu), torch.ones(m, device=gpu)
    _lib.call("rtts_ln_bwd_to", dxn0.data_ptr(), x.data_ptr(), zeros_m.data_ptr(), rstd1.data_ptr(), zeros_d.data_ptr(), ones.data_ptr(),
              out.data_ptr(), None, None, ws.data_ptr(), m, d, nxt.data_ptr(), pn.data_ptr(), p, seed, sd.data_ptr(), _s())
    torch.cuda.synchronize()
    assert _same_bits(x, keep)
    assert _same_bits(dyb, keep.bfloat16())
    assert _same_bits(out, ones)
    assert _same_bits(nxt, keep.bfloat16())


# fp32 values at the edges of the bf16 cast: ties to even (down and up), fp32 subnormals (bf16 keeps 8 bits of them), values
# that round past the largest finite bf16 (3.3895e38) to inf, +-inf, signed zeros; NaN is compared by NaN-ness
_EDGE_BITS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x00000001, 0x80000001, 0x00008000,
              0x00018000, 0x007FFFFF, 0x807F8000, 0x00400000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0x7F800000,
              0xFF800000, 0x00000000, 0x80000000, 0x7FC00000, 0xFFC00001, 0x7F800001]


def _edge_values(gpu, n):
    bits = torch.tensor(_EDGE_BITS, dtype=torch.int64).to(torch.int32)
    v = bits.view(torch.float32)
    reps = -(-n // v.numel())
    return v.repeat(reps)[:n].to(gpu)


def _same_bf16_up_to_nan(got, want):
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    return torch.equal(gn, wn) and torch.equal(_bits(got)[~gn], _bits(want)[~wn])


@pytest.mark.parametrize("n", [4, 24, 4096 + 24, 1 << 20])
def test_cast_f32_bf16_edges(gpu, n):
    """rtts_cast_f32_bf16 equals torch's .bfloat16() bit for bit on the edge values (NaN: NaN-ness only)."""
    from reformer_tts_amd import _lib
    v = _edge_values(gpu, n)
    if n > 1024:
        v[1024:] = torch.randn(n - 1024, generator=torch.Generator(device=gpu).manual_seed(n), device=gpu) * 1e3
    out = _nan((n,), gpu, torch.bfloat16)
    _lib.call("rtts_cast_f32_bf16", v.data_ptr(), out.data_ptr(), n, _s())
    torch.cuda.synchronize()
    assert _same_bf16_up_to_nan(out, v.bfloat16())


@pytest.mark.parametrize("d", WIDTHS)
def test_cast_colsum_bf16_rows_at_the_edges(gpu, d):
    """The bf16 rows of rtts_cast_colsum equal torch's .bfloat16() on the edge values (NaN: NaN-ness only)."""
    from reformer_tts_amd import _lib
    m = 9
    v = _edge_values(gpu, m * d).view(m, d)
    dyb, ws = _nan((m, d), gpu, torch.bfloat16), _nan((PARTIAL_CAP * d,), gpu)
    _lib.call("rtts_cast_colsum", v.data_ptr(), dyb.data_ptr(), None, ws.data_ptr(), m, d, 0.0, 0, None, None, _s())
    torch.cuda.synchronize()
    assert _same_bf16_up_to_nan(dyb, v.bfloat16())


@pytest.mark.parametrize("m,d", [(1, 8), (3, 136), (1025, 512), (4099, 1024)])
def test_elementwise_row_kernels_exact(gpu, m, d):
    """rtts_residual_epilogue (sign +-1, bias / NULL, no dropout), rtts_bias_act (ReLU on / off), rtts_sum_streams (fp32 and / or
    bf16 twin) on 2^-4 grid inputs: bit for bit against float64 rounded once."""
    from reformer_tts_amd import _lib
    gen = torch.Generator(device=gpu).manual_seed(m * d)
    x = _grid((m, d), -8, 8, gen, gpu)
    g = _grid((m, d), -4, 4, gen, gpu, torch.bfloat16)
    bias = _grid((d,), -4, 4, gen, gpu)
    for sign in (1.0, -1.0):
        for b in (bias, None):
            y = _nan((m, d), gpu)
            _lib.call("rtts_residual_epilogue", x.data_ptr(), g.data_ptr(), _p(b), sign, y.data_ptr(), m, d, 0.0, 0, None, _s())
            torch.cuda.synchronize()
            want = x.double() + sign * (g.double() + (b.double() if b is not None else 0.0))
            assert _same_bits(y, want.float()), (sign, b is None)
    for relu in (0, 1):
        h = g.clone()
        _lib.call("rtts_bias_act", h.data_ptr(), bias.data_ptr(), m, d, relu, _s())
        torch.cuda.synchronize()
        want = g.double() + bias.double()
        assert _same_bits(h, (want.clamp_min(0.0) if relu else want).bfloat16()), relu
    n = m * d
    a, b2 = x.view(-1), _grid((n,), -8, 8, gen, gpu)
    for want_f32, want_bf16 in ((True, True), (True, False), (False, True)):
        o, ob = _nan((n,), gpu), _nan((n,), gpu, torch.bfloat16)
        _lib.call("rtts_sum_streams", a.data_ptr(), b2.data_ptr(), n, o.data_ptr() if want_f32 else None, ob.data_ptr() if want_bf16 else None,
                  _s())
        torch.cuda.synchronize()
        s = (a.double() + b2.double()).float()
        assert _same_bits(o, s) if want_f32 else torch.isnan(o).all()
        assert _same_bits(ob, s.bfloat16()) if want_bf16 else torch.isnan(ob.float()).all()


def test_row_entry_points_reject_and_launch_nothing(gpu):
    """Unsupported widths (64, 640), drop_p = 1, a colsum_bf16 row stride below d or not a multiple of 8, and cast lengths that
    are not multiples of 4 return RttsError -- and the NaN sentinels of every output show that nothing was launched."""
    from reformer_tts_amd import _lib
    m = 8
    for d in (64, 640, 512):
        p = 1.0 if d == 512 else 0.0                 # d = 512 is supported: there drop_p = 1 is the refused argument
        x, xf = torch.randn(m, d, device=gpu), torch.ones(d, device=gpu)
        g = torch.ones(m, d, dtype=torch.bfloat16, device=gpu)
        outs = [_nan((m, d), gpu, torch.bfloat16), _nan((m,), gpu), _nan((m,), gpu), _nan((m, d), gpu), _nan((d,), gpu), _nan((d,), gpu),
                _nan((2 * PARTIAL_CAP * d,), gpu), _nan((m, d), gpu, torch.bfloat16)]
        xn, mean, rstd, dx, dg, db, ws, dyb = outs
        calls = [
            ("rtts_residual_ln", x.data_ptr(), g.data_ptr(), None, 1.0, xf.data_ptr(), xf.data_ptr(), xn.data_ptr(), mean.data_ptr(),
             rstd.data_ptr(), m, d, p, 0, None, dx.data_ptr(), _s()),
            ("rtts_ln_bwd_to", g.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), xf.data_ptr(), x.data_ptr(), dx.data_ptr(),
             dg.data_ptr(), db.data_ptr(), ws.data_ptr(), m, d, dyb.data_ptr(), ws.data_ptr(), p, 0, None, _s()),
            ("rtts_cast_colsum", x.data_ptr(), dyb.data_ptr(), dg.data_ptr(), ws.data_ptr(), m, d, p, 0, None, None, _s()),
        ]
        if d != 512:
            calls += [
                ("rtts_ln_fwd", x.data_ptr(), xf.data_ptr(), xf.data_ptr(), xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), m, d, _s()),
                ("rtts_ln_bwd", g.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), xf.data_ptr(), dx.data_ptr(), dg.data_ptr(),
                 db.data_ptr(), ws.data_ptr(), m, d, None, None, 0.0, 0, None, _s()),
                ("rtts_ln_bwd_join", g.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), xf.data_ptr(), x.data_ptr(), x.data_ptr(),
                 dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), m, d, None, None, 0.0, 0, None, _s()),
                ("rtts_colsum_bf16", dyb.data_ptr(), None, d, dg.data_ptr(), ws.data_ptr(), m, d, 0, 1.0, None, _s()),
            ]
        else:
            calls += [("rtts_residual_epilogue", x.data_ptr(), g.data_ptr(), None, 1.0, dx.data_ptr(), m, d, p, 0, None, _s()),
                      ("rtts_colsum_bf16", dyb.data_ptr(), None, d - 8, dg.data_ptr(), ws.data_ptr(), m, d, 0, 1.0, None, _s()),
                      ("rtts_colsum_bf16", dyb.data_ptr(), None, d + 4, dg.data_ptr(), ws.data_ptr(), m, d, 0, 1.0, None, _s())]
        for name, *args in calls:
            with pytest.raises(_lib.RttsError):
                _lib.call(name, *args)
        torch.cuda.synchronize()
        for o in outs:
            assert torch.isnan(o.float()).all(), d
    src, dst = torch.ones(12, device=gpu), _nan((12,), gpu, torch.bfloat16)
    o32 = _nan((12,), gpu)
    for n in (6, 10, 0):
        with pytest.raises(_lib.RttsError):
            _lib.call("rtts_cast_f32_bf16", src.data_ptr(), dst.data_ptr(), n, _s())
        with pytest.raises(_lib.RttsError):
            _lib.call("rtts_sum_streams", src.data_ptr(), src.data_ptr(), n, o32.data_ptr(), dst.data_ptr(), _s())
    torch.cuda.synchronize()
    assert torch.isnan(dst.float()).all() and torch.isnan(o32).all()

