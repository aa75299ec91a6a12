"""rtts_tts_loss, rtts_heads_grad (csrc/edges.hip) and model.TTSLoss against float64 autograd of the reference loss
(oracle/model_ref.tts_loss: masked MSE | L1 over all elements, BCE-with-logits with pos_weight, weighted total).

The kernel is called through the C-ABI as edges.PostnetLoss and model/loss.py call it, on every path and layout it has: the
vec4 and the scalar path (NM = 79, an odd row stride or a view one float off the 16-byte grid -- never a misaligned pointer on
the vec4 path: the launcher's predicate is restated in ``_vec4`` and each case asserts which path it takes), post given or
built as raw + res with res and d_post in halo rows, a valid length below the padded one on the host and as a device word,
time-sliced target / mask / stop-target views, padding columns up to ld_grad.  Every output starts as NaN: whatever the kernel
leaves unwritten shows up."""
import math
import zlib

import pytest
import torch

from oracle import model_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # fp32 unit roundoff
BLOCKS, THREADS = 512, 256     # the loss kernel's grid: per-thread partial sums, then 512 block partials
_RATIOS = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k in sorted(_RATIOS):
        print(f"error/bound {k}: {_RATIOS[k]:.4f}")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _within(name, got, want, bound):
    err = (got.double() - want.double()).abs()
    assert not torch.isnan(got).any(), name
    ratio = float((err / bound).max())
    _RATIOS[name] = max(_RATIOS.get(name, 0.0), ratio)
    assert ratio <= 1.0, f"{name}: error {float(err.max()):.3e} exceeds its fp32 bound (ratio {ratio:.3f})"


def _vec4(ptrs, nm, ld_mel, ld_grad, ld_res, tgt_bs, mask_bs, rows):
    """The launcher's choice of the four-channel path (rtts_tts_loss in csrc/edges.hip)."""
    bits = 0
    for p in ptrs:
        bits |= p or 0
    return (nm % 4 == 0 and bits & 15 == 0 and ld_mel % 4 == 0 and ld_grad % 4 == 0 and (ld_res is None or ld_res % 4 == 0)
            and tgt_bs % 4 == 0 and mask_bs % 4 == 0 and rows * (nm // 4) < 2 ** 31)


# path -> (NM, row stride of raw / post, one float off the 16-byte grid)
_PATHS = {"vec4": (80, 128, False), "scalar NM=79": (79, 128, False), "scalar odd ld": (80, 81, False), "scalar offset": (80, 128, True)}


class _Case:
    """Inputs of one launch in the layouts the trainer uses: predictions (B*Lp rows of ld_mel), stop logits a column of a
    (B*Lp, 128) array, targets / mask / stop targets time-sliced views of longer arrays (frames [k, k + Lv) of each sample)."""

    def __init__(self, gpu, kind, path, post_mode, ld_grad, b=3, lp=256, lv=256, seed=0):
        nm, ld_mel, offset = _PATHS[path]
        self.kind, self.nm, self.b, self.lp, self.lv, self.post_mode = kind, nm, b, lp, lv, post_mode
        self.ld_grad = max(ld_grad, nm)
        self.rows = rows = b * lp
        gen = torch.Generator(device=gpu).manual_seed(seed)
        g = lambda *shape: torch.randn(*shape, generator=gen, device=gpu)     # noqa: E731
        off = 1 if offset else 0
        self.raw_buf = _nan((rows * ld_mel + 4,), gpu)
        self.raw = self.raw_buf[off:off + rows * ld_mel].view(rows, ld_mel)
        self.raw[:, :nm] = g(rows, nm)
        self.ld_mel = ld_mel
        self.halo = 2 if post_mode == "res" else 0
        self.lead = 8 if post_mode == "res" else 0
        p = lp + 2 * self.halo
        if post_mode == "res":
            self.res = _nan((b * p, 128), gpu)                        # halo rows stay NaN: never read
            self.res.view(b, p, 128)[:, self.halo:self.halo + lp, :nm] = 0.3 * g(b, lp, nm)
            self.post = None
            self.dpost_rows = self.lead + b * p + 24                   # a lead-in and a tail, as edges.Halo allocates
            post = (self.raw[:, :nm].view(b, lp, nm) + self.res.view(b, p, 128)[:, self.halo:self.halo + lp, :nm]).reshape(rows, nm)
        else:
            self.res = None
            self.post_buf = _nan((rows * ld_mel + 4,), gpu)
            self.post = self.post_buf[off:off + rows * ld_mel].view(rows, ld_mel)
            self.post[:, :nm] = self.raw[:, :nm] + 0.3 * g(rows, nm)
            self.dpost_rows = rows
            post = self.post[:, :nm]
        self.post_f32 = post.clone()                                   # the fp32 prediction the kernel forms (raw + res in fp32)
        # targets: frames [1, Lv + 1) of a longer array; mask: frames [2, Lv + 2), fractional with exact 0 and 1; stop targets
        # frames [3, Lv + 3)
        self.tgt_full = g(b, lv + 1, nm)
        self.mask_full = torch.rand(b, lv + 2, nm, generator=gen, device=gpu)
        self.mask_full[self.mask_full < 0.2] = 0.0
        self.mask_full[self.mask_full > 0.8] = 1.0
        self.tstop_full = (torch.rand(b, lv + 3, generator=gen, device=gpu) < 0.3).float()
        tgt, mask = self.tgt_full[:, 1:], self.mask_full[:, 2:]
        if kind == "l1":       # exact ties raw * mask == tgt (and post * mask == tgt): the L1 gradient there is 0
            r3, p3 = self.raw[:, :nm].view(b, lp, nm)[:, :lv], post.view(b, lp, nm)[:, :lv]
            tie_r = torch.rand(b, lv, nm, generator=gen, device=gpu) < 0.05
            tie_p = torch.rand(b, lv, nm, generator=gen, device=gpu) < 0.05
            mask[tie_r | tie_p] = 1.0
            tgt[tie_r] = r3[tie_r]
            tgt[tie_p & ~tie_r] = p3[tie_p & ~tie_r]
            self.n_ties = int(tie_r.sum()) + int((tie_p & ~tie_r).sum())
        self.tgt, self.mask, self.tstop = tgt, mask, self.tstop_full[:, 3:]
        self.heads = _nan((rows, 128), gpu)
        self.heads[:, nm] = 12.0 * g(rows)                             # logits up to ~+-40: the saturated softplus / sigmoid
        self.stop = self.heads[:, nm]

    def vec4(self):
        ptrs = [self.raw.data_ptr(), None if self.post is None else self.post.data_ptr(), None if self.res is None else self.res.data_ptr(),
                self.tgt.data_ptr(), self.mask.data_ptr()]
        return _vec4(ptrs, self.nm, self.ld_mel, self.ld_grad, None if self.res is None else 128, self.tgt.stride(0),
                     self.mask.stride(0), self.rows)

    def launch(self, gpu, weights, pos_weight, lv_dev=None):
        """-> (losses, d_raw, d_post, d_stop) of one launch; outputs start as NaN.  ``lv_dev``: a device word for the valid
        length (the host value stays self.lv, the layout of the target / mask / stop-target views)."""
        from reformer_tts_amd import _lib
        d_raw, d_post, d_stop = _nan((self.rows, self.ld_grad), gpu), _nan((self.dpost_rows, self.ld_grad), gpu), _nan((self.rows,), gpu)
        losses, ws = _nan((4,), gpu), _nan((1536,), gpu)
        dev_word = None if lv_dev is None else torch.tensor([lv_dev], dtype=torch.int32, device=gpu)
        assert d_raw.data_ptr() % 16 == 0 and d_post.data_ptr() % 16 == 0
        _lib.call("rtts_tts_loss", self.raw.data_ptr(), None if self.post is None else self.post.data_ptr(), self.ld_mel, self.tgt.data_ptr(),
                  self.mask.data_ptr(), self.stop.data_ptr(), 128, self.tstop.data_ptr(), self.rows, self.nm, {"mse": 0, "l1": 1}[self.kind],
                  pos_weight, *weights, d_raw.data_ptr(), d_post.data_ptr(), self.ld_grad, d_stop.data_ptr(), losses.data_ptr(), ws.data_ptr(),
                  self.lp, self.lv, None if self.res is None else self.res.data_ptr(), 128, self.halo, self.lead, self.dpost_rows,
                  self.tgt.stride(0), None if dev_word is None else dev_word.data_ptr(), self.mask.stride(0), self.tstop.stride(0), _s())
        torch.cuda.synchronize()
        return losses, d_raw, d_post, d_stop

    def reference(self, lv, weights, pos_weight):
        """float64 autograd of oracle.model_ref.tts_loss on the predictions cropped to lv frames (reformer_tts.py:141-143)."""
        b, lp, nm = self.b, self.lp, self.nm
        dev = self.raw.device
        raw = self.raw[:, :nm].double().cpu().view(b, lp, nm)[:, :lv].clone().requires_grad_()
        post = self.post_f32.double().cpu().view(b, lp, nm)[:, :lv].clone().requires_grad_()
        stop = self.stop.double().cpu().view(b, lp)[:, :lv].clone().requires_grad_()
        tgt, mask, tstop = (t[:, :lv].double().cpu() for t in (self.tgt, self.mask, self.tstop))
        res = model_ref.tts_loss(raw, post, stop, tgt, tstop, mask, pos_weight, weights, self.kind)
        res[0].backward()
        inputs = tuple(t.detach().to(dev) for t in (raw, post, stop, tgt, mask, tstop))
        return [float(r) for r in res], raw.grad.to(dev), post.grad.to(dev), stop.grad.to(dev), inputs

    def halo_rows(self, lv):
        """Row indices (into d_post) of the valid (b, t < lv) entries, in (b, t) order."""
        p = self.lp + 2 * self.halo
        bi = torch.arange(self.b).view(-1, 1)
        t = torch.arange(lv).view(1, -1)
        return (self.lead + bi * p + self.halo + t).reshape(-1)


def _bounds(case, lv, weights, pos_weight, inputs, want):
    """fp32 error bounds of the loss kernel, first order and doubled for the fused multiply-adds -ffp-contract=on may form.
    Per element: r = v * mask - tgt (2 roundings); r^2 or |r|; the gradient's 4 products.  Sums: the elements one thread walks,
    the wave butterfly (6), the block's 4 waves (3), the finaliser's 8 block partials per lane + butterfly (14), * 1/n (2)."""
    raw, post, stop, tgt, mask, tstop = inputs
    n_el = case.b * lv * case.nm
    per_thread = 4 * math.ceil(case.rows * case.nm / (4 * BLOCKS * THREADS))
    depth = per_thread + 6 + 3 + 14 + 2
    inv_el, inv_rows = 1.0 / n_el, 1.0 / (case.b * lv)
    out = {}
    for name, v, w, g in (("raw", raw, weights[0], want[1]), ("post", post, weights[1], want[2])):
        vm = v * mask
        r = vm - tgt
        e_r = 2 * U * (r.abs() + vm.abs())
        if case.kind == "mse":
            e_loss = 2 * (depth * U * (r * r).sum() + (2 * r.abs() * e_r).sum() + U * (r * r).sum()) * inv_el
            e_grad = 2 * (6 * U * g.abs() + abs(w) * 2 * mask * e_r * inv_el)
        else:
            e_loss = 2 * (depth * U * r.abs().sum() + e_r.sum()) * inv_el
            # a sign can only differ where r is within its rounding error of 0 (never at the exact ties: there r = 0 in fp32 too)
            near = (r.abs() <= e_r) & (r != 0)
            e_grad = 2 * (4 * U * g.abs()) + near * 2 * abs(w) * mask * inv_el
        out[name] = (e_loss, e_grad + 1e-300)
    lw = 1.0 + (pos_weight - 1.0) * tstop
    sp = torch.clamp(-stop, min=0.0) + torch.log1p(torch.exp(-stop.abs()))
    comp = ((1 - tstop) * stop).abs() + lw * (stop.abs() + sp)
    term = (1 - tstop) * stop + lw * sp
    e_loss = 2 * (depth * U * term.abs().sum() + 8 * U * comp.sum()) * inv_rows
    e_grad = 2 * abs(weights[2]) * inv_rows * 8 * U * ((1 - tstop).abs() + lw) + 8 * U * want[3].abs() + 1e-300
    out["stop"] = (e_loss, e_grad)
    return out


def _check_launch(case, got, lv, weights, pos_weight, tag):
    losses, d_raw, d_post, d_stop = got
    want_l, g_raw, g_post, g_stop, inputs = case.reference(lv, weights, pos_weight)
    bounds = _bounds(case, lv, weights, pos_weight, inputs, (None, g_raw, g_post, g_stop))
    b, lp, nm = case.b, case.lp, case.nm
    # nothing left NaN; zeros wherever there is no gradient
    for t in got:
        assert not torch.isnan(t).any(), tag
    dr = d_raw.view(b, lp, case.ld_grad)
    assert torch.equal(dr[:, lv:], torch.zeros_like(dr[:, lv:])), tag
    assert torch.equal(dr[..., nm:], torch.zeros_like(dr[..., nm:])), tag
    valid = case.halo_rows(lv).to(d_post.device)
    dp_valid = d_post[valid].view(b, lv, case.ld_grad)
    others = torch.ones(case.dpost_rows, dtype=torch.bool, device=d_post.device)
    others[valid] = False
    assert torch.equal(d_post[others], torch.zeros_like(d_post[others])), tag          # halo rows, lead-in, tail, frames >= lv
    assert torch.equal(dp_valid[..., nm:], torch.zeros_like(dp_valid[..., nm:])), tag
    ds = d_stop.view(b, lp)
    assert torch.equal(ds[:, lv:], torch.zeros_like(ds[:, lv:])), tag
    # gradients and losses against float64
    _within(f"{case.kind} d_raw", dr[:, :lv, :nm], g_raw, bounds["raw"][1])
    _within(f"{case.kind} d_post", dp_valid[..., :nm], g_post, bounds["post"][1])
    _within("d_stop", ds[:, :lv], g_stop, bounds["stop"][1])
    if case.kind == "l1":
        for v, gv in ((inputs[0], dr[:, :lv, :nm]), (inputs[1], dp_valid[..., :nm])):      # sign(0) = 0, as F.l1_loss's backward
            tie = (v * inputs[4] - inputs[3]) == 0
            assert torch.equal(gv[tie], torch.zeros_like(gv[tie])), tag
    e = {k: float(v[0]) for k, v in bounds.items()}
    e_total = abs(weights[0]) * e["raw"] + abs(weights[1]) * e["post"] + abs(weights[2]) * e["stop"] + 4 * U * sum(
        abs(w) * abs(x) for w, x in zip(weights, want_l[1:]))
    for i, (name, bound) in enumerate((("total", e_total), ("raw", e["raw"]), ("post", e["post"]), ("stop", e["stop"]))):
        _within(f"{case.kind} loss {name}", losses[i:i + 1], torch.tensor([want_l[i]], dtype=torch.float64, device=losses.device),
                torch.tensor([bound], dtype=torch.float64, device=losses.device))


_WEIGHTS, _POS_WEIGHT = (0.7, 1.3, 0.4), 5.0


@pytest.mark.parametrize("ld_grad", [0, 128])             # 0: ld_grad = NM
@pytest.mark.parametrize("valid", ["full", "host", "device"])
@pytest.mark.parametrize("post_mode", ["post", "res"])
@pytest.mark.parametrize("path", list(_PATHS))
@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_tts_loss_against_float64(gpu, kind, path, post_mode, valid, ld_grad):
    """rtts_tts_loss: the four losses within their fp32 bounds, d_raw / d_post / d_stop within theirs, every row the loss does
    not cover (frames >= the valid length, halo rows, the lead-in and tail of d_post) and every padding column exactly 0,
    nothing left NaN; two launches are bit-identical.  ``valid``: 'host' = a valid length below the padded one, 'device' = a
    device word below the host value (the buffers keep the host layout)."""
    lv_host = {"full": 256, "host": 200, "device": 200}[valid]
    case = _Case(gpu, kind, path, post_mode, ld_grad, lv=lv_host, seed=zlib.crc32(repr((kind, path, post_mode, valid, ld_grad)).encode()) % 1000)
    assert case.vec4() == (path == "vec4")
    lv_dev = 133 if valid == "device" else None
    got = case.launch(gpu, _WEIGHTS, _POS_WEIGHT, lv_dev=lv_dev)
    _check_launch(case, got, lv_dev or lv_host, _WEIGHTS, _POS_WEIGHT, (kind, path, post_mode, valid, ld_grad))
    if kind == "l1":
        assert case.n_ties > 100
    again = case.launch(gpu, _WEIGHTS, _POS_WEIGHT, lv_dev=lv_dev)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_heads_grad_against_float64(gpu, kind):
    """rtts_heads_grad: dheads = (d_raw + d_post) * up + dx0 in columns < NM, column NM = d_stop * up, the rest (d_raw + d_post) * up
    = 0 -- from the loss kernel's own halo-row outputs (as edges.PostnetLoss.backward), without and with scale_dev."""
    from reformer_tts_amd import _lib
    from reformer_tts_amd.edges import Halo
    case = _Case(gpu, kind, "vec4", "res", 128, lv=256, seed=7)
    h = Halo(case.b, case.lp)
    assert (h.H, h.LEAD) == (case.halo, case.lead)
    # d_post in a buffer laid out as edges.Halo allocates it
    case.dpost_rows = h.alloc
    losses, d_raw, d_post, d_stop = case.launch(gpu, _WEIGHTS, _POS_WEIGHT)
    dx0 = torch.randn(h.mp, 128, device=gpu)
    nm, m = case.nm, case.rows
    rows = torch.arange(m, device=gpu)
    hrow = (rows // case.lp) * h.p + h.H + rows % case.lp
    for up in (None, 0.75):
        up_t = None if up is None else torch.tensor([up], device=gpu)
        out = _nan((m, 128), gpu)
        _lib.call("rtts_heads_grad", d_raw.data_ptr(), d_post.data_ptr(), h.LEAD, dx0.data_ptr(), 128, d_stop.data_ptr(), case.b, case.lp, h.H,
                  nm, 128, out.data_ptr(), None if up_t is None else up_t.data_ptr(), _s())
        torch.cuda.synchronize()
        u = 1.0 if up is None else up
        ab = d_raw.double() + d_post[h.LEAD + hrow].double()
        want = ab * u
        want[:, :nm] += dx0[hrow, :nm].double()
        want[:, nm] = d_stop.double() * u
        # (a + b), * up, + dx0: three roundings, doubled for a fused multiply-add
        bound = 2 * U * (2 * ab.abs() * u + want.abs()) + 1e-300
        _within("heads_grad", out, want, bound)
        assert torch.equal(out[:, nm + 1:], torch.zeros_like(out[:, nm + 1:]))


def test_tts_loss_rejects_bad_layouts(gpu):
    """Argument checks of rtts_tts_loss: loss kind, valid length, halo room, batch strides below the valid rows."""
    from reformer_tts_amd import _lib
    case = _Case(gpu, "mse", "vec4", "res", 128, lv=200, seed=3)
    d = _nan((case.dpost_rows, 128), gpu)
    dr, ds, losses, ws = _nan((case.rows, 128), gpu), _nan((case.rows,), gpu), _nan((4,), gpu), _nan((1536,), gpu)

    def call(kind=0, lv=200, dpost_rows=case.dpost_rows, tgt_bs=case.tgt.stride(0), mask_bs=case.mask.stride(0), tstop_bs=case.tstop.stride(0)):
        _lib.call("rtts_tts_loss", case.raw.data_ptr(), None, case.ld_mel, case.tgt.data_ptr(), case.mask.data_ptr(), case.stop.data_ptr(), 128,
                  case.tstop.data_ptr(), case.rows, case.nm, kind, 5.0, 1.0, 1.0, 1.0, dr.data_ptr(), d.data_ptr(), 128, ds.data_ptr(),
                  losses.data_ptr(), ws.data_ptr(), case.lp, lv, case.res.data_ptr(), 128, case.halo, case.lead, dpost_rows, tgt_bs, None,
                  mask_bs, tstop_bs, _s())
    for kw in (dict(kind=2), dict(lv=0), dict(lv=case.lp + 1), dict(dpost_rows=case.lead + case.b * (case.lp + 4) - 1),
               dict(tgt_bs=199 * case.nm), dict(mask_bs=199 * case.nm), dict(tstop_bs=199)):
        with pytest.raises(_lib.RttsError):
            call(**kw)
    torch.cuda.synchronize()
    assert torch.isnan(d).all() and torch.isnan(dr).all() and torch.isnan(losses).all()


# ------------------------------------------------------------------------------------------------------------------ TTSLoss
@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0), (0.0, 0.5, 2.0), (1.5, 0.0, 0.0), (0.0, 0.0, 0.0)])
def test_ttsloss_module_gradients_of_every_returned_loss(gpu, kind, weights):
    """model.TTSLoss end to end: backpropagating through each of the four returned losses alone, and through weighted
    combinations of them, gives float64 autograd's gradients of the reference -- also for a part whose weight is 0 (the
    kernel's stored gradients are those of the weighted total: a zero weight must not drop that part's own gradient)."""
    from reformer_tts_amd.model import TTSLoss
    gen = torch.Generator(device=gpu).manual_seed(int(sum(weights) * 10) + len(kind))
    b, l, nm = 2, 96, 80
    raw0 = torch.randn(b, l, nm, generator=gen, device=gpu)
    post0 = raw0 + 0.3 * torch.randn(b, l, nm, generator=gen, device=gpu)
    stop0 = 8.0 * torch.randn(b, l, generator=gen, device=gpu)
    tgt = torch.randn(b, l, nm, generator=gen, device=gpu)
    mask = (torch.rand(b, l, nm, generator=gen, device=gpu) > 0.2).float() * torch.rand(b, l, nm, generator=gen, device=gpu).clamp_min(0.5)
    tstop = (torch.rand(b, l, generator=gen, device=gpu) < 0.3).float()
    loss_mod = TTSLoss(torch.tensor(_POS_WEIGHT), *weights, spectrogram_loss=kind)
    mixes = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0.5, 2.0, -1.0, 0.25), (0.0, 1.0, 1.0, 1.0)]
    for mix in mixes:
        raw, post, stop = (t.clone().requires_grad_() for t in (raw0, post0, stop0))
        res = loss_mod(raw, post, stop, tgt, tstop, mask)
        sum(c * r for c, r in zip(mix, res) if c).backward()
        r64, p64, s64 = (t.double().cpu().requires_grad_() for t in (raw0, post0, stop0))
        ref = model_ref.tts_loss(r64, p64, s64, tgt.double().cpu(), tstop.double().cpu(), mask.double().cpu(), _POS_WEIGHT, weights, kind)
        sum(c * r for c, r in zip(mix, ref) if c).backward()
        # a prediction the combination does not reach has no gradient in autograd (None); TTSLoss returns zeros for it
        g_raw, g_post, g_stop = (torch.zeros_like(t).to(gpu) if t.grad is None else t.grad.to(gpu) for t in (r64, p64, s64))
        for i in range(4):      # the losses' own fp32 bounds are test_tts_loss_against_float64's; here: ~170 ulp
            assert abs(float(res[i]) - float(ref[i])) <= 1e-5 * (abs(float(ref[i])) + 1e-3), (mix, i)
        n_el, n_rows = b * l * nm, b * l
        # d(mix . losses)/d(part) = mix_total * weight + mix_part: the scale of each part's own (unweighted) gradient g.  Bound:
        # a few roundings of |g| * scale (the kernel's products, the backward's rescaling) + g's own error from r = v * mask - tgt
        # (MSE) or from the softplus / sigmoid (stop); doubled for fused multiply-adds
        sc = [abs(mix[0] * w) + abs(c) for w, c in zip(weights, mix[1:])]
        lw = 1.0 + (_POS_WEIGHT - 1.0) * tstop.double()
        for got, want, v, scale in ((raw.grad, g_raw, raw0, sc[0]), (post.grad, g_post, post0, sc[1])):
            vm = v.double() * mask.double()
            r = vm - tgt.double()
            if kind == "mse":
                g_mag, e_g = 2 * r.abs() * mask / n_el, 2 * mask * 2 * U * (r.abs() + vm.abs()) / n_el
            else:
                g_mag, e_g = mask.double() / n_el, ((r.abs() <= 2 * U * vm.abs()) & (r != 0)) * 2 * mask / n_el
            _within(f"TTSLoss {kind} spectrogram gradients", got, want, 2 * scale * (8 * U * g_mag + e_g) + 1e-300)
        g_mag = ((1 - tstop.double()).abs() + lw) / n_rows
        _within("TTSLoss stop gradient", stop.grad, g_stop, 2 * sc[2] * 16 * U * g_mag + 1e-300)
