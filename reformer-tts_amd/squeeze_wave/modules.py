"""SqueezeWave vocoder, inference on MI355X.

Module tree, constructor arguments and ``state_dict`` names follow
``/root/reference/reformer_tts/squeeze_wave/modules.py`` (``SqueezeWave`` :238-290, ``WN`` :125-201,
``DepthwiseSeparableConv1d`` :88-122, ``InvertibleConv1d`` :27-85) so that the reference's checkpoints load; the
modules here only HOLD parameters.  ``infer`` (:334-376) runs through an explicit executor:

* activations are channels-last rows ``(B*L, C)``: every 1x1 ``Conv1d`` is one ``rtts_gemm_nt`` launch over rows (the
  hand-written MFMA kernel of csrc/gemm_nt.hip: bf16 operands, fp32 accumulate, bias / fp32 store in its epilogue), the WN
  residual stream and the audio stay fp32;
* weight norm and the eval-mode BatchNorm in front of each depthwise convolution are folded into plain weights once
  per parameter version (what ``remove_norms`` :237-248,378-419 does destructively);
* the mel conditioning of all ``n_layers`` layers of a flow is one GEMM (``cond_layer``), consumed in place by the gate
  kernel with nearest-neighbour upsampling done by indexing;
* depthwise k3 + folded BatchNorm, tanh*sigmoid gate and inverse affine coupling are the kernels of
  ``csrc/squeezewave.hip``; the residual add is the TTS path's ``rtts_residual_epilogue``;
* the inverse of each invertible 1x1 convolution is cached (fp32) like the reference's ``W_inverse`` and applied, with the
  inverse coupling in front of it, by the fp32 kernel ``rtts_sw_coupling_inv1x1``.

The analysis direction, ``forward`` (:294-332) and the likelihood ``nll`` / ``nll_ragged`` / ``capture_nll_ragged``
(``squeeze_wave/loss.py:14-31``), runs the same folded WN blocks in eval mode (running-statistics BatchNorm): per flow one
``rtts_sw_coupling_fwd1x1`` launch (the previous flow's coupling, this flow's early output and 1x1 convolution) in front of
``_FoldedWN.forward``, and one ``rtts_sw_nll_reduce`` launch for the per-utterance sums.  The launch list of a WN block is
written once, ``_FoldedWN.walk``, and so is the walk over the flows of each direction (``_flows``, ``_flows_fwd``); the mel is
cast to bf16 rows once per call (``_MelRows``) and every flow's conditioning GEMM reads those rows.

Training (``LitSqueezeWave``, ``training/wrappers.py:327-418``): ``nll_backward`` runs the same ``_flows_fwd`` over ``_TrainWN``
blocks -- the same ``walk``, given batch-statistics depthwise taps and a stash that keeps every layer's activations -- and walks
it backwards -- ``rtts_sw_boundary_bwd`` per flow boundary, ``rtts_sw_gate_bwd`` and ``rtts_sw_dwbn_bwd_sums`` / ``_apply`` per
layer, ``rtts_gemm_nt`` (input gradients) and ``rtts_gemm_tn`` (weight gradients) for every 1x1 convolution -- adding the loss's
gradient into every parameter's ``.grad``.  With ``logdet="device"`` the inverses and log-determinants of the 1x1 convolutions come
from ``rtts_sw_inv1x1_factor`` (csrc/sw_lu.hip) instead of the host's LAPACK: the step then touches the host nowhere, and
``VocoderTrainer.capture`` replays it as one hipGraph.

There is no CPU fallback: ``infer`` and ``forward`` raise off the GPU."""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import nn

from .. import _lib, ops
from .._graphs import warm_capture
from ..edges import _ws
from ..engine import _WS, _slab_ws, gemm
from .config import WNConfig


def _s() -> int:
    return torch.cuda.current_stream().cuda_stream


class InvertibleConv1d(nn.Module):
    def __init__(self, n_channels: int):
        super().__init__()
        self.conv = nn.Conv1d(n_channels, n_channels, kernel_size=1, bias=False)
        w = torch.linalg.qr(torch.randn(n_channels, n_channels))[0]          # random orthonormal, det +1
        if torch.det(w) < 0:
            w[:, 0] = -w[:, 0]
        self.conv.weight.data = w.reshape(n_channels, n_channels, 1).contiguous()


class DepthwiseSeparableConv1d(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: int):
        super().__init__()
        assert kernel_size % 2 == 1 and in_channels % 2 == 0
        self.layer = nn.Sequential(nn.BatchNorm1d(in_channels),
                                   nn.Conv1d(in_channels, in_channels, kernel_size, padding=(kernel_size - 1) // 2, groups=in_channels),
                                   nn.Conv1d(in_channels, out_channels, 1))


class WN(nn.Module):
    def __init__(self, in_audio_channels: int, in_mel_channels: int, n_layers: int, n_channels: int, conv_kernel_size: int,
                 mel_upsample_scale: int):
        super().__init__()
        assert conv_kernel_size % 2 == 1 and n_channels % 2 == 0
        self.n_layers, self.n_channels, self.kernel_size, self.upsample_scale = n_layers, n_channels, conv_kernel_size, mel_upsample_scale
        wn = torch.nn.utils.weight_norm
        self.cond_layer = wn(nn.Conv1d(in_mel_channels, 2 * n_channels * n_layers, 1), name="weight")
        self.start_conv = wn(nn.Conv1d(in_audio_channels, n_channels, 1), name="weight")
        self.end_conv = nn.Conv1d(n_channels, 2 * in_audio_channels, 1)
        self.end_conv.weight.data.zero_()
        self.end_conv.bias.data.zero_()
        self.in_layers = nn.ModuleList(DepthwiseSeparableConv1d(n_channels, 2 * n_channels, conv_kernel_size) for _ in range(n_layers))
        self.res_skip_layers = nn.ModuleList(wn(nn.Conv1d(n_channels, n_channels, 1), name="weight") for _ in range(n_layers))


def _normed(conv) -> torch.Tensor:
    """(Cout, Cin) fp32 weight of a 1x1 convolution, weight norm applied if it is still attached."""
    if hasattr(conv, "weight_g"):
        v, g = conv.weight_v.detach().float(), conv.weight_g.detach().float()
        w = v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))
    else:
        w = conv.weight.detach().float()
    return w.squeeze(-1)


def _pad(n: int, q: int) -> int:
    return -(-n // q) * q


class _Segments:
    """Which activation rows of a WN block belong to which utterance.  ``b`` x ``length`` audio rows (``b`` x ``mel_len``
    mel rows) are what the row-wise entry points see; ``moff`` is None for a uniform batch (``b`` utterances of ``length``
    rows) or the device int32 table of ``nseg`` + 1 mel-frame offsets of a packed one (``b`` = 1: all rows, capacity
    padding included, are one sequence to the row-wise kernels; the depthwise kernel reads the table)."""

    __slots__ = ("b", "length", "mel_len", "up", "moff", "nseg")

    def __init__(self, b: int, length: int, mel_len: int, up: int, moff: Optional[torch.Tensor] = None, nseg: int = 0):
        self.b, self.length, self.mel_len, self.up, self.moff, self.nseg = b, length, mel_len, up, moff, nseg

    @classmethod
    def uniform(cls, b: int, mel_len: int, up: int) -> "_Segments":
        return cls(b, up * mel_len, mel_len, up)

    @classmethod
    def packed(cls, moff: torch.Tensor, capacity_frames: int, up: int) -> "_Segments":
        return cls(1, up * capacity_frames, capacity_frames, up, moff, moff.numel() - 1)

    @property
    def rows(self) -> int:
        return self.b * self.length


SW_MAX_SEGMENTS = 1024          # utterances of one ragged call: the offset table is staged in LDS (csrc/squeezewave.hip)


def host_lengths(lengths) -> List[int]:
    """Per-utterance mel frame counts as host ints (a list, tuple or CPU tensor; a device tensor would be a hidden sync)."""
    if torch.is_tensor(lengths):
        if lengths.is_cuda:
            raise ValueError("lengths must be host values (a list or a CPU tensor)")
        lengths = lengths.tolist()
    out = [int(n) for n in lengths]
    if any(n < 0 for n in out):
        raise ValueError(f"negative utterance length in {out}")
    return out


def segment_offsets(lengths) -> List[int]:
    """B + 1 non-decreasing mel-frame offsets of utterances laid end to end: [0, l0, l0 + l1, ...]."""
    moff = [0]
    for n in host_lengths(lengths):
        moff.append(moff[-1] + n)
    return moff


def pack_noise(noise, lengths, up: int, capacity_frames: Optional[int] = None) -> List[torch.Tensor]:
    """Per-utterance draws -> packed rows.  ``noise[i]`` is utterance i's list in the layout and order of
    ``noise_shapes(1, lengths[i])``; draw k of all utterances becomes ONE fp32 (up * capacity_frames, C_k) row tensor,
    utterance i in rows [up * moff[i], up * moff[i+1]) -- the rows ``infer`` itself makes of a (1, C_k, L) draw -- and zero
    rows after the total."""
    moff = segment_offsets(lengths)
    cap = moff[-1] if capacity_frames is None else int(capacity_frames)
    if cap < moff[-1] or len(noise) != len(moff) - 1:
        raise ValueError(f"pack_noise: {len(noise)} noise lists for {len(moff) - 1} utterances, {moff[-1]} frames in a capacity of {cap}")
    out = []
    for k in range(len(noise[0]) if noise else 0):
        pieces = [z[k][0].t() for z in noise]
        pad = up * (cap - moff[-1])
        if pad:
            pieces.append(pieces[0].new_zeros(pad, pieces[0].shape[1]))
        out.append(torch.cat(pieces).to(torch.float32))
    return out


def unpack_noise(draws, lengths, up: int) -> List[List[torch.Tensor]]:
    """The inverse of ``pack_noise``: per-utterance views (1, C_k, up * lengths[i]) of packed draws (rows, C_k)."""
    moff = segment_offsets(lengths)
    return [[d[up * moff[i]:up * moff[i + 1]].t().unsqueeze(0) for d in draws] for i in range(len(moff) - 1)]


class _MelRows:
    """The mel of one call: fp32 (B*Lm, n_mel) rows, and the bf16 rows the cond_layer of every flow reads, made ONCE per call
    and layout.  ``in_tree`` is per flow (n_half shrinks at every early return), so a model may mix the two layouts: zero-padded
    to 128 rows and the width of ``w_cond`` for the MFMA GEMM, a plain cast for the library GEMM.  ``wide`` (a training block:
    cond_layer's weight gradient reads the rows again) widens the in-tree rows to ``rtts_gemm_tn``'s 128-column K granule."""

    def __init__(self, rows: torch.Tensor, seg: _Segments):
        self.rows, self.seg, self.cast = rows, seg, {}

    def bf16(self, f: "_FoldedWN", wide: bool) -> torch.Tensor:
        key = (f.in_tree, wide)
        if key not in self.cast:
            self.cast[key] = self._cast(f, wide)
        return self.cast[key]

    def _cast(self, f: "_FoldedWN", wide: bool) -> torch.Tensor:
        rows, seg = self.rows, self.seg
        if not f.in_tree:
            return rows.to(torch.bfloat16)
        mp, kp = _pad(seg.b * seg.mel_len, 128), f.w_cond.shape[1]
        x = torch.empty(mp, kp, dtype=torch.bfloat16, device=rows.device)
        _lib.call("rtts_to_halo", rows.data_ptr(), rows.stride(0), 0, f.n_mel, 1, seg.b, seg.mel_len, 0, kp, x.data_ptr(), 0, mp, _s())
        return _k128(x) if wide else x


def _fold_taps(bn, dw, a: torch.Tensor, mean: torch.Tensor):
    """BatchNorm as x * a + c0, c0 = beta - mean * a, folded into the depthwise convolution behind it:
    dw(bn(x)) = sum_k (w_k * a) x_{l+k-1} + [b + (sum_k w_k) * c0] -> (taps (C, 3), bias, lo, hi), all fp32.  Zero padding pads
    bn(x), i.e. the reference does NOT add the constant c0 at the borders: at l = 0 the tap k = 0 sees the zero padding, not c0,
    and at l = L-1 the tap k = 2 likewise, so the border rows get the exact corrections lo = w_0 * c0 and hi = w_2 * c0 taken
    off by the depthwise kernel.  ``a`` and ``mean`` come from the running statistics (inference, the likelihood) or from the
    batch's (training)."""
    c0 = bn.bias.detach().float() - mean * a
    w = dw.weight.detach().float().squeeze(1)                                  # (C, 3)
    taps, bias = (w * a[:, None]).contiguous(), (dw.bias.detach().float() + w.sum(1) * c0).contiguous()
    return taps, bias, (w[:, 0] * c0).contiguous(), (w[:, 2] * c0).contiguous()


class _FoldedWN:
    """Weights of one WN block and the walk over its launches: bf16 GEMM operands (row-major (Cout, Cin)), fp32 biases, and for
    inference and the likelihood the depthwise taps with the eval-mode BatchNorm folded in (``_fold_taps`` with
    a = gamma / sqrt(var + eps) and the running mean).

    Every 1x1 convolution (``start``, ``cond_layer``, the pointwise half of ``in_layers``, ``res_skip_layers``, ``end``;
    reference ``modules.py:203-235``) is ``rtts_gemm_nt`` (csrc/gemm_nt.hip) over channels-last rows: operands are padded ONCE
    here to the kernel's granules -- input widths to multiples of 64 (audio halves 64, 56, ... and the 80 mel channels: zero
    columns), the ``end`` projection's 2 * n_half outputs to a multiple of 64 (zero rows; its consumer takes a row stride) --
    and the row count of an utterance is rounded up to 128 in the activation buffers (rows are independent: the extra rows
    are never read back).  ``in_tree`` is False for toy widths the MFMA kernel does not tile (n_channels % 64, n_half % 8 or
    n_mel % 8 != 0): those run the same arithmetic through the library GEMM (``gemms``: the one place that choice is made) and
    say so once."""

    def __init__(self, wn: WN, fold_bn: bool = True):
        bf = torch.bfloat16
        self.c, self.nl, self.up = wn.n_channels, wn.n_layers, wn.upsample_scale
        if wn.kernel_size != 3:
            raise NotImplementedError("the HIP depthwise kernel is built for conv_kernel_size == 3")
        w_start, w_cond = _normed(wn.start_conv), _normed(wn.cond_layer)
        w_end = wn.end_conv.weight.detach().float().squeeze(-1)
        self.n_half, self.n_mel = w_start.shape[1], w_cond.shape[1]
        self.in_tree = self.c % 64 == 0 and self.n_half % 8 == 0 and self.n_mel % 8 == 0
        self.gemms = _MfmaGemms if self.in_tree else _LibraryGemms
        dev = w_start.device

        def kpad(w):            # (N, K) -> (N, K rounded up to 64) bf16, zero columns
            if not self.in_tree:
                return w.to(bf).contiguous()
            out = torch.zeros(w.shape[0], _pad(w.shape[1], 64), dtype=bf, device=dev)
            out[:, :w.shape[1]] = w.to(bf)
            return out

        self.w_start, self.b_start = kpad(w_start), wn.start_conv.bias.detach().float().contiguous()
        self.w_cond, self.b_cond = kpad(w_cond), wn.cond_layer.bias.detach().float().contiguous()
        self.n_end = _pad(w_end.shape[0], 64) if self.in_tree else w_end.shape[0]
        self.w_end = torch.zeros(self.n_end, self.c, dtype=bf, device=dev)
        self.w_end[:w_end.shape[0]] = w_end.to(bf)
        self.b_end = torch.zeros(self.n_end, dtype=torch.float32, device=dev)
        self.b_end[:w_end.shape[0]] = wn.end_conv.bias.detach().float()
        self.dw_taps, self.w_pw, self.b_pw, self.w_rs, self.b_rs = [], [], [], [], []
        for i in range(wn.n_layers):
            bn, dw, pw = wn.in_layers[i].layer
            self.w_pw.append(pw.weight.detach().float().squeeze(-1).to(bf).contiguous())
            self.b_pw.append(pw.bias.detach().float().contiguous())
            self.w_rs.append(_normed(wn.res_skip_layers[i]).to(bf).contiguous())
            self.b_rs.append(wn.res_skip_layers[i].bias.detach().float().contiguous())
            if fold_bn:              # a training step folds its own batch statistics (_TrainWN): no depthwise taps here
                a = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
                self.dw_taps.append(_fold_taps(bn, dw, a, bn.running_mean.float()))

    def forward(self, audio: torch.Tensor, mel: _MelRows, seg: _Segments) -> torch.Tensor:
        """The block in eval mode, arguments and result as ``walk``: the taps folded from the running statistics, nothing kept."""
        return self.walk(audio, mel, seg, lambda i, h, seg: self.dw_taps[i])

    def walk(self, audio: torch.Tensor, mel: _MelRows, seg: _Segments, taps_of, stash=None) -> torch.Tensor:
        """The launch list of a WN block (``WN.forward``, reference ``modules.py:203-235``): audio fp32 (seg.rows, n_rem) rows
        (the first n_half channels condition the block), the call's mel rows -> fp32 (rows >= seg.rows,
        n_end >= 2*n_half) = [log_s | b | zero columns].  The conditioning of all layers is one GEMM; only the depthwise
        convolution looks across rows: it is the one launch that differs between a uniform and a packed batch.

        ``taps_of(i, h, seg)`` gives layer i's depthwise (taps, bias, lo, hi) for the residual stream ``h`` in front of it,
        followed by whatever else the stash is to keep with that layer.  ``stash`` (training): the object that gets what the
        backward needs as attributes -- ``xmel`` (widened, like ``a0``, to the weight-gradient GEMM's K granule), ``cond``,
        ``a0``, ``hb``, ``mp`` and ``layers``, per layer ``(h, dwo, pw, acts, *what taps_of added)`` -- so the residual epilogue
        writes a fresh buffer instead of ``h`` in place, and padding rows (the activation buffers are rounded up to 128 rows)
        are zeroed wherever a buffer is written by a kernel that stops at the real rows: the weight-gradient GEMMs and column
        sums run over all rows.  Without it buffers are plain ``torch.empty`` and nothing is zeroed."""
        dev, c, bf, mm = audio.device, self.c, torch.bfloat16, self.gemms.mm
        b, length, mel_len, up, m = seg.b, seg.length, seg.mel_len, seg.up, seg.rows
        keep = stash is not None
        xmel = mel.bf16(self, wide=keep)
        if self.in_tree:
            cond = mm(xmel[:, :self.w_cond.shape[1]], self.w_cond, self.b_cond)  # (rows, 2c * n_layers) bf16
            mp, kp = _pad(m, 128), self.w_start.shape[1]
            a0 = torch.empty(mp, kp, dtype=bf, device=dev)                     # bf16 copy of the conditioning half, zero padded
            _lib.call("rtts_to_halo", audio.data_ptr(), audio.stride(0), 0, self.n_half, 1, b, length, 0, kp, a0.data_ptr(), 0, mp, _s())
            h = mm(a0, self.w_start, self.b_start, True)                       # (mp, c) fp32: the WN residual stream
            a0 = _k128(a0) if keep else a0
        else:                                                                  # the toy path keeps start_conv's input in fp32
            _lib.note_general_path("SqueezeWave WN block", f"widths (n_channels {c}, n_half {self.n_half}, n_mel {self.n_mel}) the MFMA GEMM "
                                   "does not tile (n_channels % 64, n_half % 8, n_mel % 8): library GEMM")
            cond = torch.addmm(self.b_cond.to(bf), xmel, self.w_cond.t())
            mp = m
            a0 = audio[:, :self.n_half].contiguous()
            h = torch.addmm(self.b_start, a0, self.w_start.float().t())

        def rows(width, dtype):
            t = torch.empty(mp, width, dtype=dtype, device=dev)
            return _zero_tail(t, m) if keep else t

        layers = []
        for i in range(self.nl):
            taps, bias, lo, hi, *kept = taps_of(i, h, seg)                     # zero padding pads bn(x): no folded constant there
            dwo = rows(c, bf)
            if seg.moff is None:
                _lib.call("rtts_sw_depthwise_k3", h.data_ptr(), taps.data_ptr(), bias.data_ptr(), b, length, c, dwo.data_ptr(), lo.data_ptr(),
                          hi.data_ptr(), _s())
            else:
                _lib.call("rtts_sw_depthwise_k3_seg", h.data_ptr(), taps.data_ptr(), bias.data_ptr(), seg.moff.data_ptr(), seg.nseg, up, m, c,
                          dwo.data_ptr(), lo.data_ptr(), hi.data_ptr(), _s())
            pw = mm(dwo, self.w_pw[i], self.b_pw[i])                           # (mp, 2c) bf16
            acts = rows(c, bf)
            _lib.call("rtts_sw_gate", pw.data_ptr(), cond.data_ptr(), cond.stride(0), i * 2 * c, up, b, length, mel_len, c, acts.data_ptr(), _s())
            rs = mm(acts, self.w_rs[i])
            nxt = rows(c, torch.float32) if keep else h
            _lib.call("rtts_residual_epilogue", h.data_ptr(), rs.data_ptr(), self.b_rs[i].data_ptr(), 1.0, nxt.data_ptr(), m, c, 0.0, 0, None, _s())
            if keep:
                layers.append((h, dwo, pw, acts, *kept))
            h = nxt
        hb = rows(c, bf)
        _lib.call("rtts_cast_f32_bf16", h.data_ptr(), hb.data_ptr(), m * c, _s())
        if keep:
            stash.xmel, stash.cond, stash.a0, stash.hb, stash.mp, stash.layers = xmel, cond, a0, hb, mp, layers
        return mm(hb, self.w_end, self.b_end, True)


def _zero_tail(t: torch.Tensor, m: int) -> torch.Tensor:
    """Rows from ``m`` on are padding to the GEMMs' 128-row granule: zeroed, so that a reduction over all rows (a weight
    gradient, a bias sum) sees nothing there, whatever the allocator handed out."""
    if t.shape[0] > m:
        t[m:].zero_()
    return t


def _k128(x: torch.Tensor) -> torch.Tensor:
    """bf16 rows with the width rounded up to 128 (zero columns): the K granule of ``rtts_gemm_tn``."""
    if x.shape[1] % 128 == 0:
        return x
    out = torch.zeros(x.shape[0], _pad(x.shape[1], 128), dtype=x.dtype, device=x.device)
    out[:, :x.shape[1]] = x
    return out


TRAIN_WIDTHS = (128, 256, 512, 1024)     # n_channels the in-tree backward tiles: rtts_gemm_tn's 128 granule, the column-sum kernels' widths


class _MfmaGemms:
    """The GEMM forms of a WN block, forward and backward, on the in-tree kernels: bf16 operands, fp32 accumulation."""

    @staticmethod
    def mm(x, w, bias=None, f32=False):
        """y = x @ w^T (+ bias), w (N, K): bf16, or the unrounded fp32 result."""
        return gemm(x, w, bias=bias, out_f32=f32)

    @staticmethod
    def dgrad(dy, w, f32=False):
        """dx = dy @ w, w (N, K) as the forward holds it."""
        return gemm(dy, w, kn=True, out_f32=f32)

    @staticmethod
    def wgrad(dy, x):
        """dW (N, K) fp32 = dy^T @ x over ALL rows (padding rows of dy are zero, of x finite)."""
        n, k = dy.shape[1], x.shape[1]
        out = torch.empty(n, k, dtype=torch.float32, device=dy.device)
        ws = _slab_ws(dy.device)
        _lib.call("rtts_gemm_tn", dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dy.shape[0], n, k, out.data_ptr(), k, 0, ws.data_ptr(),
                  ws.numel(), _s())
        return out

    @staticmethod
    def cast_colsum(d):
        """fp32 (M, d) -> (its bf16 copy, its column sums fp32 (d,))."""
        m, w = d.shape
        db = torch.empty(m, w, dtype=torch.bfloat16, device=d.device)
        out = torch.zeros(w, dtype=torch.float32, device=d.device)
        _lib.call("rtts_cast_colsum", d.data_ptr(), db.data_ptr(), out.data_ptr(), _WS.partial(d.device, w).data_ptr(), m, w, 0.0, 0, None, None, _s())
        return db, out

    @staticmethod
    def colsum(d, col0: int, width: int, out: torch.Tensor):
        """out (width,) fp32 += column sums of columns [col0, col0 + width) of the bf16 rows ``d``."""
        view = d[:, col0:col0 + width]
        _lib.call("rtts_colsum_bf16", view.data_ptr(), None, d.stride(0), out.data_ptr(), _WS.partial(d.device, width).data_ptr(), d.shape[0], width,
                  0, 1.0, None, _s())


class _LibraryGemms:
    """The same forms for toy widths the MFMA kernels do not tile: the same arithmetic (bf16 operands, fp32 accumulation)
    through the library GEMM."""

    @staticmethod
    def mm(x, w, bias=None, f32=False):
        y = torch.mm(x, w.t(), out_dtype=torch.float32)
        y = y if bias is None else y + bias
        return y if f32 else y.to(torch.bfloat16)

    @staticmethod
    def dgrad(dy, w, f32=False):
        dx = torch.mm(dy, w, out_dtype=torch.float32)
        return dx if f32 else dx.to(torch.bfloat16)

    @staticmethod
    def wgrad(dy, x):
        return torch.mm(dy.t(), x, out_dtype=torch.float32)

    @staticmethod
    def cast_colsum(d):
        return d.to(torch.bfloat16), d.sum(0)

    @staticmethod
    def colsum(d, col0: int, width: int, out: torch.Tensor):
        out += d[:, col0:col0 + width].float().sum(0)


class _TrainWN:
    """One WN block of a training step (``WN.forward`` in ``.train()``): ``_FoldedWN.walk`` with its two arguments.  The taps:
    in front of each depthwise convolution the statistics of the fp32 residual stream over the B * L real rows are taken
    (``rtts_bn_moments`` / ``rtts_bn_from_moments``, which also maintain the running statistics) and folded into the depthwise
    taps and edge corrections on the device (C-sized torch ops, no host read).  The stash: this object; every layer's input,
    depthwise output, pointwise output, gate output and statistics are kept for ``backward``.  Toy widths (``in_tree`` False)
    run the same arithmetic through ``torch.mm``, as the forward does."""

    def __init__(self, wn: WN, f: _FoldedWN):
        self.wn, self.f = wn, f                 # widths: SqueezeWave._train_widths has refused what the backward does not tile

    def _batch_taps(self, i: int, h: torch.Tensor, seg: _Segments):
        bn, dwc, _ = self.wn.in_layers[i].layer
        dev, c = h.device, self.f.c
        mom = torch.empty(2 * c + 1, dtype=torch.float32, device=dev)
        mean, rstd = torch.empty(c, dtype=torch.float32, device=dev), torch.empty(c, dtype=torch.float32, device=dev)
        _lib.call("rtts_bn_moments", h.data_ptr(), seg.b, seg.length, 0, c, mom.data_ptr(), _ws(dev, c).data_ptr(), _s())
        _lib.call("rtts_bn_from_moments", mom.data_ptr(), seg.rows, c, mean.data_ptr(), rstd.data_ptr(), bn.running_mean.data_ptr(),
                  bn.running_var.data_ptr(), None, bn.num_batches_tracked.data_ptr(), _s())
        return (*_fold_taps(bn, dwc, bn.weight.detach() * rstd, mean), mean, rstd, dwc.weight.detach().squeeze(1).contiguous())

    def forward(self, audio: torch.Tensor, mel: _MelRows, seg: _Segments) -> torch.Tensor:
        """-> fp32 [log_s | b | zero columns], as ``_FoldedWN.forward``; everything ``backward`` needs stays on ``self``."""
        return self.f.walk(audio, mel, seg, self._batch_taps, stash=self)

    def new_dwn(self, seg: _Segments) -> torch.Tensor:
        """The buffer ``rtts_sw_boundary_bwd`` writes d [log_s | b] into: 128 columns wide and zero outside the real rows and
        columns on the in-tree path (N of the end_conv weight-gradient GEMM)."""
        dev = self.hb.device
        if self.f.in_tree:
            return torch.zeros(self.mp, 128, dtype=torch.float32, device=dev)
        return torch.empty(seg.rows, 2 * self.f.n_half, dtype=torch.float32, device=dev)

    @staticmethod
    def _weight_norm_grads(conv, dw: torch.Tensor, grads: list):
        """dw (Cout, Cin) fp32 = the gradient of the effective weight w = g * v / ||v|| -> the gradients of g and v."""
        dw = dw.unsqueeze(-1)
        if not hasattr(conv, "weight_g"):
            grads.append((conv.weight, dw))
            return
        v, g = conv.weight_v.detach(), conv.weight_g.detach()
        nrm = v.flatten(1).norm(dim=1).view(-1, 1, 1)
        vh = v / nrm
        dg = (dw * vh).flatten(1).sum(1).view(-1, 1, 1)
        grads.append((conv.weight_g, dg))
        grads.append((conv.weight_v, (g / nrm) * (dw - dg * vh)))

    def backward(self, dwn: torch.Tensor, seg: _Segments, grads: list) -> torch.Tensor:
        """dwn = d loss / d [log_s | b] (``new_dwn``) -> d loss / d (the conditioning half of the block's input) fp32 (seg.rows,
        n_half); appends (parameter, gradient) for every parameter of the block to ``grads``."""
        f, wn, g = self.f, self.wn, self.f.gemms
        dev, c, nh, bf = dwn.device, f.c, f.n_half, torch.bfloat16
        b, length, mel_len, m, mp = seg.b, seg.length, seg.mel_len, seg.rows, self.mp
        dwn_b, db_end = g.cast_colsum(dwn)
        dw_end = g.wgrad(dwn_b, self.hb)
        grads.append((wn.end_conv.weight, dw_end[:2 * nh].unsqueeze(-1)))
        grads.append((wn.end_conv.bias, db_end[:2 * nh]))
        dh = g.dgrad(dwn_b[:, :f.w_end.shape[0]], f.w_end, True)              # (mp, c) fp32, zero in the padding rows
        dcond = _zero_tail(torch.empty(self.cond.shape, dtype=bf, device=dev), b * mel_len)
        db_cond = torch.zeros(self.cond.shape[1], dtype=torch.float32, device=dev)
        n_part = _lib.load().rtts_sw_dwbn_bwd_partial_floats(m, c)
        part = torch.empty(n_part, dtype=torch.float32, device=dev)
        for i in reversed(range(f.nl)):
            h_in, dwo, pw, acts, mean, rstd, w = self.layers[i]
            bn, dwc, pwc = wn.in_layers[i].layer
            drs, db_rs = g.cast_colsum(dh)
            self._weight_norm_grads(wn.res_skip_layers[i], g.wgrad(drs, acts), grads)
            grads.append((wn.res_skip_layers[i].bias, db_rs))
            dacts = g.dgrad(drs, f.w_rs[i])
            dpw = _zero_tail(torch.empty(mp, 2 * c, dtype=bf, device=dev), m)
            _lib.call("rtts_sw_gate_bwd", pw.data_ptr(), self.cond.data_ptr(), self.cond.stride(0), i * 2 * c, seg.up, b, length, mel_len, c,
                      dacts.data_ptr(), dpw.data_ptr(), dcond.data_ptr(), dcond.stride(0), _s())
            g.colsum(dcond, i * 2 * c, 2 * c, db_cond[i * 2 * c:(i + 1) * 2 * c])
            db_pw = torch.zeros(2 * c, dtype=torch.float32, device=dev)
            g.colsum(dpw, 0, 2 * c, db_pw)
            grads.append((pwc.weight, g.wgrad(dpw, dwo).unsqueeze(-1)))
            grads.append((pwc.bias, db_pw))
            ddw = g.dgrad(dpw, f.w_pw[i])                                      # (mp, c) bf16
            sums = torch.empty(6, c, dtype=torch.float32, device=dev)
            stats = (mean.data_ptr(), rstd.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), w.data_ptr())
            _lib.call("rtts_sw_dwbn_bwd_sums", h_in.data_ptr(), ddw.data_ptr(), *stats, b, length, c, sums.data_ptr(), part.data_ptr(), _s())
            _lib.call("rtts_sw_dwbn_bwd_apply", h_in.data_ptr(), ddw.data_ptr(), *stats, sums.data_ptr(), b, length, c, dh.data_ptr(), _s())
            grads.append((dwc.weight, sums[0:3].t().unsqueeze(1)))
            grads.append((dwc.bias, sums[3]))
            grads.append((bn.weight, sums[4]))
            grads.append((bn.bias, sums[5]))
        self._weight_norm_grads(wn.cond_layer, g.wgrad(dcond, self.xmel)[:, :f.n_mel], grads)
        grads.append((wn.cond_layer.bias, db_cond))
        if f.in_tree:
            dhs, db_start = g.cast_colsum(dh)
            dw_start = g.wgrad(dhs, self.a0)[:, :nh]
            da0 = g.dgrad(dhs, f.w_start, True)[:m, :nh]
        else:                                                                      # the toy path keeps start_conv's input in fp32
            db_start, dw_start, da0 = dh.sum(0), torch.mm(dh.t(), self.a0), torch.mm(dh, f.w_start.float())
        self._weight_norm_grads(wn.start_conv, dw_start, grads)
        grads.append((wn.start_conv.bias, db_start))
        return da0


class SqueezeWave(nn.Module):
    def __init__(self, n_flows: int, n_audio_channels: int, n_mel_channels: int, early_return_interval: int, early_return_size: int,
                 wn_config: WNConfig):
        super().__init__()
        assert n_audio_channels % 2 == 0, "n_audio_channels must be divisible by 2"
        assert early_return_size % 2 == 0, "early_return_size must be divisible by 2"
        self.n_flows, self.n_audio_channels, self.early_return_size = n_flows, n_audio_channels, early_return_size
        self.early_return_interval = early_return_interval
        self.wn_layers, self.inv_conv_layers = nn.ModuleList(), nn.ModuleList()
        n_half, n_rem = n_audio_channels // 2, n_audio_channels
        for k in range(n_flows):
            if self.return_early(k):
                n_half -= early_return_size // 2
                n_rem -= early_return_size
            self.inv_conv_layers.append(InvertibleConv1d(n_rem))
            self.wn_layers.append(WN(n_half, n_mel_channels, wn_config.n_layers, wn_config.n_channels, wn_config.conv_kernel_size,
                                     wn_config.mel_upsample_scale))
        self.n_remaining_channels = n_rem
        self._folded: Optional[List[_FoldedWN]] = None
        self._folded_key = None

    def return_early(self, flow: int) -> bool:
        return flow % self.early_return_interval == 0 and flow > 0

    def _fold(self, fold_bn: bool = True, logdet: str = "host"):
        """``fold_bn=False`` (a training step): the GEMM operands only, built anew and not kept as the inference fold -- the step
        changes the parameters and the running statistics anyway.  ``logdet="device"`` (training folds only): the inverses and
        log-determinants of the 1x1 convolutions come from ``rtts_sw_inv1x1_factor`` -- ``_winv`` and ``_slogdet_dev`` (n_flows, 2)
        float64 = {sign, log|det|}, both on the device, no host read and no synchronisation; the host values (``_slogdet``) are
        dropped, whoever needs them folds on the host again."""
        if logdet not in ("host", "device"):
            raise ValueError(f"logdet must be 'host' or 'device' (got {logdet!r})")
        if logdet == "device" and fold_bn:
            raise ValueError("logdet='device' is the training fold's (fold_bn=False); inference and the eval likelihood factor on the host")
        key = tuple((p.data_ptr(), p._version) for p in self.parameters()) + tuple((b.data_ptr(), b._version) for b in self.buffers())
        if self._folded is None or self._folded_key != key or not fold_bn:
            with torch.no_grad():
                self._folded = [_FoldedWN(wn, fold_bn) for wn in self.wn_layers]
                # the forward direction: W itself (fp32, as the reference's conv applies it)
                self._wfwd = [conv.conv.weight.detach().squeeze(-1).float().contiguous() for conv in self.inv_conv_layers]
                if logdet == "device":
                    # one launch, float64 Gauss-Jordan in LDS (csrc/sw_lu.hip); the signs are judged by check_determinants()
                    self._winv, self._slogdet_dev = ops.sw_inv1x1_factor(self._wfwd)
                    self._slogdet = None
                else:
                    # twelve matrices of at most 128 x 128, once per parameter version: inverted on the host in float64 (LAPACK) -- no
                    # device library (rocSOLVER / hipBLAS) call anywhere in the vocoder
                    dev = self.inv_conv_layers[0].conv.weight.device
                    w64 = [conv.conv.weight.detach().squeeze(-1).double().cpu() for conv in self.inv_conv_layers]
                    self._winv = [w.inverse().float().contiguous().to(dev) for w in w64]
                    # log det W in float64 on the host (modules.py:63 computes it per call in fp32); (sign, log|det|) per flow,
                    # judged where it is used
                    self._slogdet = [tuple(float(v) for v in torch.linalg.slogdet(w)) for w in w64]
            self._folded_key = key if fold_bn else None
        return self._folded

    def noise_shapes(self, batch: int, mel_len: int):
        """Shapes (reference layout (B, C, L)) of the Gaussian draws of one ``infer`` call, in the order they are consumed."""
        length = mel_len * (256 // self.n_audio_channels)
        shapes = [(batch, self.n_remaining_channels, length)]
        shapes += [(batch, self.early_return_size, length) for k in reversed(range(self.n_flows)) if self.return_early(k)]
        return shapes

    def _device(self, what: str) -> torch.device:
        dev = self.inv_conv_layers[0].conv.weight.device
        if dev.type != "cuda":
            raise _lib.RttsError(f"SqueezeWave.{what} runs on the GPU only (no CPU fallback for the HIP path)")
        return dev

    def _n_mel(self) -> int:
        cond = self.wn_layers[0].cond_layer
        return (cond.weight_v if hasattr(cond, "weight_v") else cond.weight).shape[1]

    def _up(self) -> int:
        up = self.wn_layers[0].upsample_scale
        if up * self.n_audio_channels != 256:
            raise ValueError("mel_upsample_scale must equal 256 // n_audio_channels")
        return up

    def _flows(self, folded: List[_FoldedWN], mel_rows: torch.Tensor, seg: _Segments, draws, sigma: float) -> torch.Tensor:
        """The executor of ``infer`` (modules.py:340-376) over rows: ``draws`` yields the Gaussian draws as fp32
        (seg.rows, C) rows in the order they are consumed -> clamped audio rows (seg.rows, n_audio_channels).  The bf16 mel
        rows are made once (``_MelRows``); every flow's conditioning GEMM reads them."""
        mel = _MelRows(mel_rows, seg)
        audio = next(draws)                                                        # (rows, n_remaining) fp32
        for k in reversed(range(self.n_flows)):
            n = audio.shape[1]
            wn_out = folded[k].forward(audio, mel, seg)                            # [s | b | padding], row stride n_end
            nxt = torch.empty_like(audio)
            # inverse coupling + inverse 1x1 convolution in one fp32 launch (modules.py:353-361)
            _lib.call("rtts_sw_coupling_inv1x1", audio.data_ptr(), audio.stride(0), wn_out.data_ptr(), wn_out.stride(0),
                      self._winv[k].data_ptr(), n, audio.shape[0], nxt.data_ptr(), nxt.stride(0), _s())
            audio = nxt
            if self.return_early(k):
                audio = torch.cat((sigma * next(draws), audio), dim=1)
        return torch.clamp(audio, -1, 1)

    @torch.no_grad()
    def infer(self, mel_spectrogram: torch.Tensor, sigma: float = 0.6, noise: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """``modules.py:334-376``: mel (B, n_mel, Lm) -> audio (B, 256 * Lm) in [-1, 1].  ``noise``: the Gaussian draws in
        the reference's (B, C, L) layout and order (see ``noise_shapes``); drawn on the device when omitted."""
        dev = self._device("infer")
        folded = self._fold()
        mel = mel_spectrogram.to(dev)
        b, n_mel, mel_len = mel.shape
        up = self._up()
        length = up * mel_len
        shapes = self.noise_shapes(b, mel_len)
        if noise is None:
            noise = [torch.randn(s, device=dev) for s in shapes]
        assert [tuple(z.shape) for z in noise] == shapes, "noise tensors do not match noise_shapes()"
        rows = lambda z: z.to(dev, torch.float32).permute(0, 2, 1).reshape(b * length, -1).contiguous()    # noqa: E731
        mel_rows = mel.to(torch.float32).permute(0, 2, 1).reshape(b * mel_len, n_mel).contiguous()
        audio = self._flows(folded, mel_rows, _Segments.uniform(b, mel_len, up), (rows(z) for z in noise), sigma)
        return audio.view(b, length * audio.shape[1])

    def _pack_mel(self, mel: torch.Tensor, lens: List[int], moff: torch.Tensor, capacity_frames: int, out: Optional[torch.Tensor] = None):
        """mel (B, n_mel, >= max(lens)) fp32, any strides -> packed fp32 rows (capacity_frames, n_mel), one launch."""
        b, n_mel, lmax = mel.shape
        if n_mel != self._n_mel() or len(lens) != b or (lens and max(lens) > lmax):
            raise ValueError(f"mel {tuple(mel.shape)} does not hold {b} utterances of {lens} frames and {self._n_mel()} channels")
        if not 1 <= b <= SW_MAX_SEGMENTS:
            raise ValueError(f"a ragged vocoder call takes 1..{SW_MAX_SEGMENTS} utterances (got {b})")
        if mel.dtype != torch.float32:
            mel = mel.float()
        if out is None:
            out = torch.empty(capacity_frames, n_mel, dtype=torch.float32, device=mel.device)
        _lib.call("rtts_sw_pack_mel", mel.data_ptr(), mel.stride(0), mel.stride(1), mel.stride(2), lmax, n_mel, moff.data_ptr(), b,
                  capacity_frames, out.data_ptr(), out.stride(0), _s())
        return out

    def _offsets_to(self, moff_host: List[int], dev, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The offset table on the device: a pinned host copy, enqueued without waiting for the device."""
        host = torch.tensor(moff_host, dtype=torch.int32).pin_memory()
        if out is None:
            return host.to(dev, non_blocking=True)
        return out.copy_(host, non_blocking=True)

    @staticmethod
    def split_packed(audio: torch.Tensor, moff_host: List[int]) -> List[torch.Tensor]:
        """Packed audio -> the per-utterance views (256 samples per mel frame) of the offsets ``moff_host``."""
        flat = audio.view(-1)
        return [flat[256 * moff_host[i]:256 * moff_host[i + 1]] for i in range(len(moff_host) - 1)]

    def pack_noise(self, noise, lengths, capacity_frames: Optional[int] = None) -> List[torch.Tensor]:
        """Per-utterance draws (``noise_shapes(1, lengths[i])`` each) -> the packed rows ``infer_ragged`` consumes."""
        lens = host_lengths(lengths)
        for i, (z, n) in enumerate(zip(noise, lens)):
            if [tuple(t.shape) for t in z] != self.noise_shapes(1, n):
                raise ValueError(f"noise of utterance {i} does not match noise_shapes(1, {n})")
        return pack_noise(noise, lens, self._up(), capacity_frames)

    def unpack_noise(self, draws, lengths) -> List[List[torch.Tensor]]:
        """Packed draws (e.g. what a ``capture_ragged`` replay drew: ``run.noise``) -> per-utterance ``noise_shapes(1, n)`` views."""
        return unpack_noise(draws, lengths, self._up())

    @torch.no_grad()
    def infer_ragged(self, mel: torch.Tensor, lengths, sigma: float = 0.6, noise=None):
        """A batch of utterances of different lengths, each vocoded as ``infer(mel[i:i+1, :, :lengths[i]])`` would vocode it:
        mel (B, n_mel, Lmax) (any strides), ``lengths`` (B,) host ints -> (packed audio (256 * sum(lengths),), list of B
        views of 256 * lengths[i] samples).  The utterances are laid end to end as rows; only the depthwise convolution
        looks across rows, and it stops at each utterance's edges (``rtts_sw_depthwise_k3_seg``).  ``noise``: one list per
        utterance in the shapes and order of ``noise_shapes(1, lengths[i])``; drawn on the device when omitted."""
        dev = self._device("infer_ragged")
        folded = self._fold()
        up = self._up()
        lens = host_lengths(lengths)
        moff_h = segment_offsets(lens)
        total = moff_h[-1]
        if total == 0:
            empty = torch.empty(0, device=dev)
            return empty, [empty] * len(lens)
        mel = mel.to(dev)
        moff = self._offsets_to(moff_h, dev)
        mel_rows = self._pack_mel(mel, lens, moff, total)
        if noise is None:
            draws = (torch.randn(up * total, s[1], device=dev) for s in self.noise_shapes(1, 1))
        else:
            draws = iter([z.to(dev) for z in self.pack_noise(noise, lens)])
        audio = self._flows(folded, mel_rows, _Segments.packed(moff, total, up), draws, sigma).view(-1)
        return audio, self.split_packed(audio, moff_h)

    def capture(self, batch: int, mel_len: int, sigma: float = 0.6):
        """-> ``run(mel) -> audio``: the whole ``infer`` for one (batch, mel_len) shape as ONE hipGraph (~1000 launches
        replayed without host work; eager inference is launch-bound: 14 ms whether B is 1 or 8).  Per call the mel is
        copied into the graph's input buffer and fresh Gaussian noise is drawn inside the graph (the default CUDA
        generator is graph-safe).  The returned audio tensor is the graph's output buffer: copy it before the next call."""
        dev = self._device("capture")
        mel_buf = torch.zeros(batch, self._n_mel(), mel_len, device=dev)
        graph, out = warm_capture(lambda: self.infer(mel_buf, sigma))          # infer draws its noise on the device

        def run(mel: torch.Tensor) -> torch.Tensor:
            mel_buf.copy_(mel, non_blocking=True)
            graph.replay()
            return out
        return run

    def capture_ragged(self, batch: int, capacity_frames: int, sigma: float = 0.6):
        """-> ``run(mel, lengths) -> (packed audio, per-utterance views)``: ``infer_ragged`` for up to ``batch`` utterances
        of at most ``capacity_frames`` mel frames in total, as ONE hipGraph that any set of lengths replays.  Per call the
        offset table is copied in and the mel packed into the graph's input rows (one kernel, outside the graph); the
        Gaussian draws are made inside the graph over all capacity rows, into ``run.noise`` (packed rows, readable after
        the replay: ``unpack_noise(run.noise, lengths)`` gives each utterance's draws).  A total above the capacity raises
        before anything is launched.  Graphs are kept per (batch, capacity, sigma).  The returned audio is the graph's
        output buffer: copy it before the next call."""
        dev = self._device("capture_ragged")
        batch, cap = int(batch), int(capacity_frames)
        if not 1 <= batch <= SW_MAX_SEGMENTS or cap < 1:
            raise ValueError(f"capture_ragged: 1..{SW_MAX_SEGMENTS} utterances and a positive capacity (got {batch}, {cap})")
        cache = self.__dict__.setdefault("_ragged_graphs", {})
        key = (batch, cap, float(sigma))
        if key in cache and cache[key].folded is self._fold():
            return cache[key]
        folded = self._fold()
        up = self._up()
        widths = [s[1] for s in self.noise_shapes(1, 1)]
        mel_rows = torch.zeros(cap, self._n_mel(), device=dev)
        moff = torch.zeros(batch + 1, dtype=torch.int32, device=dev)        # every row padding until a call sets the table
        seg = _Segments.packed(moff, cap, up)

        def flows():
            draws = [torch.randn(up * cap, w, device=dev) for w in widths]
            return draws, self._flows(folded, mel_rows, seg, iter(draws), sigma).view(-1)

        graph, (draws, out) = warm_capture(flows)

        def run(mel: torch.Tensor, lengths):
            lens = host_lengths(lengths)
            moff_h = segment_offsets(lens)
            if len(lens) != batch or moff_h[-1] > cap:
                raise ValueError(f"capture_ragged graph for {batch} utterances of {cap} frames in total: got {len(lens)} utterances, "
                                 f"{moff_h[-1]} frames")
            mel = mel.to(dev)
            self._offsets_to(moff_h, dev, out=moff)
            self._pack_mel(mel, lens, moff, cap, out=mel_rows)
            graph.replay()
            return out, self.split_packed(out, moff_h)
        run.noise, run.batch, run.capacity, run.folded, run.graph = draws, batch, cap, folded, graph
        cache[key] = run
        return run


    # ------------------------------------------------------------------ the analysis direction: audio -> z, likelihood
    def _logdets(self) -> List[float]:
        """log det W of every flow (float64, cached by ``_fold``).  The reference's ``torch.logdet`` (modules.py:63) returns
        NaN for a negative determinant and -inf for a singular W; here that is an error that names the flow."""
        self._fold()
        return self._checked_logdets()

    def _checked_logdets(self) -> List[float]:
        for k, (sign, _) in enumerate(self._slogdet):
            if sign <= 0:
                raise ValueError(f"inv_conv_layers.{k}: det W is {'zero' if sign == 0 else 'negative'}: log det W is undefined, the flow "
                                 "has no likelihood (the reference's torch.logdet would return NaN or -inf)")
        return [v for _, v in self._slogdet]

    def _logdet_dev(self) -> torch.Tensor:
        """sum_k log det W_k of the last device fold as a device float64 scalar, after ``torch.logdet`` (modules.py:63): NaN for a
        negative determinant, -inf for a singular W (the kernel's log|det|).  No host value goes in or comes out."""
        sign, logabs = self._slogdet_dev[:, 0], self._slogdet_dev[:, 1]
        return torch.where(sign < 0, float("nan"), logabs).sum()

    def check_determinants(self) -> None:
        """Judge the determinants of the last device-mode fold (``nll_backward(logdet="device")``, a replay of
        ``VocoderTrainer.capture``): ONE device -> host read of n_flows x 2 doubles, at a time the caller chooses -- the step
        itself raises nothing and returns a non-finite loss.  Raises what the host path raises at fold time."""
        sd = getattr(self, "_slogdet_dev", None)
        if sd is None:
            raise _lib.RttsError("SqueezeWave.check_determinants: no device-mode fold yet (run nll_backward(logdet='device') first)")
        for k, sign in enumerate(sd[:, 0].cpu().tolist()):
            if sign <= 0:
                raise ValueError(f"inv_conv_layers.{k}: det W is {'zero' if sign == 0 else 'negative'}: log det W is undefined, the flow "
                                 "has no likelihood (the reference's torch.logdet would return NaN or -inf)")

    def _likelihood_device(self, what: str) -> torch.device:
        dev = self._device(what)
        if self.training:
            raise _lib.RttsError(f"SqueezeWave.{what} needs eval mode: batch-statistics (training-mode) BatchNorm is not on the HIP path, "
                                 "the likelihood is computed with the running statistics (call .eval())")
        return dev

    @staticmethod
    def _on_device(t: torch.Tensor, dev, what: str, name: str) -> torch.Tensor:
        if not torch.is_tensor(t) or t.device != dev:
            raise _lib.RttsError(f"SqueezeWave.{what} runs on the GPU only: {name} is on {getattr(t, 'device', type(t).__name__)}, the model on {dev}")
        return t

    def _flows_fwd(self, blocks, mel_rows: torch.Tensor, seg: _Segments, audio_rows: torch.Tensor, keep: bool, bnd: Optional[list] = None):
        """The executor of ``forward`` (modules.py:308-331) over rows, in eval mode (``blocks``: the ``_FoldedWN`` of every flow)
        and in a training step (the ``_TrainWN``): mel rows fp32 (B*Lm, n_mel), audio rows fp32 (seg.rows, n_audio_channels) ->
        (z rows (seg.rows, n_audio_channels): the early blocks in flow order, then the remainder; ls_row (seg.rows,): every
        row's sum of log_s over all flows; the WN outputs [log_s | b | padding] per flow if ``keep``).  The bf16 mel rows
        are made once (``_MelRows``); then per flow one boundary launch (the previous flow's coupling, this flow's early split and 1x1
        convolution) and the WN block; a last launch applies the final coupling.  ``bnd`` (training): every boundary's
        (x, wn_prev, zcol, n_early, w) is appended to it for the backward walk."""
        rows, dev = seg.rows, audio_rows.device
        mel = _MelRows(mel_rows, seg)
        z = torch.empty(rows, self.n_audio_channels, dtype=torch.float32, device=dev)
        ls_row = torch.zeros(rows, dtype=torch.float32, device=dev)
        x, wn_prev, zcol, kept = audio_rows, None, 0, []

        def boundary(w, n_early, out):
            _lib.call("rtts_sw_coupling_fwd1x1", x.data_ptr(), x.stride(0), None if wn_prev is None else wn_prev.data_ptr(),
                      0 if wn_prev is None else wn_prev.stride(0), None if w is None else w.data_ptr(), x.shape[1], n_early, rows,
                      None if out is None else out.data_ptr(), 0 if out is None else out.stride(0), z.data_ptr(), z.stride(0), zcol,
                      ls_row.data_ptr(), _s())
            if bnd is not None:
                bnd.append((x, wn_prev, zcol, n_early, w))

        for k in range(self.n_flows):
            n_early = self.early_return_size if self.return_early(k) else 0
            out = torch.empty(rows, x.shape[1] - n_early, dtype=torch.float32, device=dev)
            boundary(self._wfwd[k], n_early, out)
            zcol += n_early
            x = out
            wn_prev = blocks[k].forward(x, mel, seg)                               # [log_s | b | padding], row stride n_end
            if keep:
                kept.append(wn_prev)
        boundary(None, x.shape[1], None)
        return z, ls_row, kept

    def _uniform_rows(self, mel: torch.Tensor, audio: torch.Tensor, dev, what: str):
        """(mel (B, n_mel, Lm), audio (B, 256 * Lm)) on the device -> (mel rows, audio rows, segments, B, L)."""
        self._on_device(mel, dev, what, "mel")
        self._on_device(audio, dev, what, "audio")
        up, c = self._up(), self.n_audio_channels
        if mel.dim() != 3 or mel.shape[1] != self._n_mel() or mel.shape[0] < 1 or mel.shape[2] < 1:
            raise ValueError(f"SqueezeWave.{what}: mel {tuple(mel.shape)} is not (B, {self._n_mel()}, Lm)")
        b, n_mel, mel_len = mel.shape
        if tuple(audio.shape) != (b, up * c * mel_len):
            raise ValueError(f"SqueezeWave.{what}: audio {tuple(audio.shape)} is not (B, {up * c} * Lm) = ({b}, {up * c * mel_len}) for mel "
                             f"{tuple(mel.shape)}")
        mel_rows = mel.to(torch.float32).permute(0, 2, 1).reshape(b * mel_len, n_mel).contiguous()
        audio_rows = audio.to(torch.float32).reshape(b * up * mel_len, c).contiguous()      # unfold(1, C, C): row l = samples [l*C, (l+1)*C)
        return mel_rows, audio_rows, _Segments.uniform(b, mel_len, up), b, up * mel_len

    @torch.no_grad()
    def forward(self, forward_input):
        """``modules.py:294-332`` in eval mode: (mel (B, n_mel, Lm), audio (B, 256 * Lm)) -> (z (B, n_audio_channels, L),
        log_s_list, log_det_W_list) with L = 256 * Lm / n_audio_channels; z = the early outputs in flow order, then the
        remainder.  ``log_s_list[k]`` (B, n_half_k, L) is a view of flow k's WN output; ``log_det_W_list[k]`` = B * L * log det
        W_k (fp32, 0-dim), log det taken in float64 at fold time.  ``SqueezeWaveLoss(sigma)`` of this tuple is ``nll``."""
        mel, audio = forward_input
        dev = self._likelihood_device("forward")
        folded, logdet = self._fold(), self._logdets()
        mel_rows, audio_rows, seg, b, length = self._uniform_rows(mel, audio, dev, "forward")
        z, _, kept = self._flows_fwd(folded, mel_rows, seg, audio_rows, True)
        log_s = [w[:seg.rows, :f.n_half].unflatten(0, (b, length)).permute(0, 2, 1) for w, f in zip(kept, folded)]
        ld = torch.tensor([b * length * v for v in logdet], dtype=torch.float64).to(torch.float32).to(dev)
        return z.view(b, length, -1).permute(0, 2, 1), log_s, list(ld.unbind(0))

    def _nll_from_sums(self, sums: torch.Tensor, nrows: torch.Tensor, sigma: float, logdet):
        """``loss.py:21-31`` from the per-utterance sums: sums (n, 2) float64 = {sum z^2, sum log_s}, nrows (n,) float64 = audio
        rows per utterance, ``logdet`` = log det W of every flow as host floats, or their sum as a device float64 scalar
        (``_logdet_dev``) -> (per-utterance loss (n,) fp32: 0 / 0 = NaN for an empty one, loss of the whole batch 0-dim fp32)."""
        c = self.n_audio_channels
        num = sums[:, 0] / (2.0 * float(sigma) ** 2) - sums[:, 1] - nrows * (logdet if torch.is_tensor(logdet) else sum(logdet))
        return (num / (nrows * c)).float(), (num.sum() / (nrows.sum() * c)).float()

    def _reduce(self, z: torch.Tensor, ls_row: torch.Tensor, seg: _Segments) -> torch.Tensor:
        n = seg.b if seg.moff is None else seg.nseg
        sums = torch.empty(n, 2, dtype=torch.float64, device=z.device)
        _lib.call("rtts_sw_nll_reduce", z.data_ptr(), z.stride(0), z.shape[1], ls_row.data_ptr(), None if seg.moff is None else seg.moff.data_ptr(),
                  n, seg.up, seg.length, seg.rows, sums.data_ptr(), _s())
        return sums

    @torch.no_grad()
    def nll(self, mel: torch.Tensor, audio: torch.Tensor, sigma: float = 1.0) -> torch.Tensor:
        """The negative log-likelihood per element of ``audio`` under the flow, ``SqueezeWaveLoss(sigma)(self((mel, audio)))``
        (``loss.py:14-31``; what ``LitSqueezeWave.validation_step`` logs, ``training/wrappers.py:361-368``), without the
        ``log_s`` list: every flow boundary adds its rows' sums of log_s into one fp32 vector, and one launch reduces z^2 and
        that vector per utterance in float64 -> 0-dim fp32 on the device."""
        dev = self._likelihood_device("nll")
        folded, logdet = self._fold(), self._logdets()
        mel_rows, audio_rows, seg, b, length = self._uniform_rows(mel, audio, dev, "nll")
        z, ls_row, _ = self._flows_fwd(folded, mel_rows, seg, audio_rows, False)
        nrows = torch.full((b,), float(length), dtype=torch.float64, device=dev)
        return self._nll_from_sums(self._reduce(z, ls_row, seg), nrows, sigma, logdet)[1]

    # ------------------------------------------------------------------ training: the likelihood's gradient
    def _train_widths(self):
        """Widths the forward runs on the MFMA GEMMs (``_FoldedWN.in_tree``) but the backward does not tile are refused by name:
        ``rtts_gemm_tn`` needs N, K % 128 and the column-sum kernels take 128, 256, 512, 1024 or 2048 columns."""
        n_mel = self._n_mel()
        for wn in self.wn_layers:
            c = wn.n_channels
            n_half = (wn.start_conv.weight_v if hasattr(wn.start_conv, "weight_v") else wn.start_conv.weight).shape[1]
            if c % 64 == 0 and n_half % 8 == 0 and n_mel % 8 == 0 and c not in TRAIN_WIDTHS:
                raise _lib.RttsError(f"SqueezeWave.nll_backward: n_channels {c} is not one of {TRAIN_WIDTHS}, the widths the HIP backward "
                                     "tiles (weight-gradient GEMM and column sums); inference and the likelihood take it")

    @torch.no_grad()
    def nll_backward(self, mel: torch.Tensor, audio: torch.Tensor, sigma: float = 1.0, logdet: str = "host",
                     _after_forward=None) -> torch.Tensor:
        """One forward + backward of the reference's training step (``training/wrappers.py:350-359``): the loss
        ``SqueezeWaveLoss(sigma)(self((mel, audio)))`` with the BatchNorms in training mode (``modules.py:100-117``: batch
        statistics over the B * L rows), mel (B, n_mel, Lm) and audio (B, 256 * Lm) on the device -> the loss (0-dim fp32 on the
        device).  d loss / d p is ADDED into ``p.grad`` of every parameter (created where it is None) and every BatchNorm's
        ``running_mean`` / ``running_var`` / ``num_batches_tracked`` is updated as ``nn.BatchNorm1d`` updates them (momentum 0.1,
        unbiased variance).  Uniform batches only; the model must be in ``.train()``.

        Every layer's activations are kept for the backward (no recomputation through the inverse flow).  ``log det W_k`` and
        ``W_k^-T`` come from ``_fold``: with ``logdet="host"`` from float64 LAPACK on the host (one small device -> host copy per
        parameter version, i.e. per step; a determinant that is not positive raises before anything is launched); with
        ``logdet="device"`` from ``rtts_sw_inv1x1_factor`` -- the step then reads nothing back, copies no computed value to the
        device and can be captured into a graph.  There log det W follows ``torch.logdet`` (NaN for a negative determinant, -inf
        for a singular W): the loss of such a step is not finite, nothing is raised, ``check_determinants()`` tells which flow.
        ``n_channels`` that the MFMA forward takes but the backward does not tile (64, 192, 320, ...: anything outside
        ``TRAIN_WIDTHS``) are refused.  ``_after_forward`` (measurement only): called once between the forward and the backward."""
        return self._nll_backward(lambda dev: self._uniform_rows(mel, audio, dev, "nll_backward")[:3], sigma, logdet, _after_forward)

    @torch.no_grad()
    def nll_backward_rows(self, mel_rows: torch.Tensor, audio_rows: torch.Tensor, batch: int, mel_len: int, sigma: float = 1.0,
                          logdet: str = "host", _after_forward=None) -> torch.Tensor:
        """``nll_backward`` for a batch that already is in the step's row layout: mel_rows fp32 (batch * mel_len, n_mel)
        channels-last and audio_rows fp32 (batch * 256 * mel_len / n_audio_channels, n_audio_channels), both contiguous on the
        device -- what ``nll_backward`` makes of (mel, audio) with a permute and a copy, and what ``rtts_sw_draw_segments`` writes
        directly.  Everything else is ``nll_backward``: same launches, same gradients bit for bit for the same rows."""
        batch, mel_len = int(batch), int(mel_len)

        def rows_of(dev):
            up, c = self._up(), self.n_audio_channels
            for name, t, shape in (("mel_rows", mel_rows, (batch * mel_len, self._n_mel())), ("audio_rows", audio_rows, (batch * up * mel_len, c))):
                self._on_device(t, dev, "nll_backward_rows", name)
                if batch < 1 or mel_len < 1 or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError(f"SqueezeWave.nll_backward_rows: {name} must be contiguous fp32 {shape} for batch {batch}, mel_len {mel_len} "
                                     f"(got {t.dtype} {tuple(t.shape)})")
            return mel_rows, audio_rows, _Segments.uniform(batch, mel_len, up)
        return self._nll_backward(rows_of, sigma, logdet, _after_forward)

    def _nll_backward(self, rows_of, sigma: float, logdet: str, after_forward) -> torch.Tensor:
        """The body of ``nll_backward``: ``rows_of(dev)`` -> (mel rows, audio rows, segments), called once the model has been checked and
        folded."""
        self._train_widths()
        dev = self._device("nll_backward")
        if not self.training:
            raise _lib.RttsError("SqueezeWave.nll_backward needs training mode (call .train()): it differentiates the loss with "
                                 "batch-statistics BatchNorm; nll scores in eval mode")
        if any(p.dtype != torch.float32 for p in self.parameters()):
            raise _lib.RttsError("SqueezeWave.nll_backward: the parameters must be fp32 (they are the optimiser's master weights)")
        folded = self._fold(fold_bn=False, logdet=logdet)
        logdet = self._logdet_dev() if logdet == "device" else self._checked_logdets()
        mel_rows, audio_rows, seg = rows_of(dev)
        try:
            return self._train_step(folded, logdet, mel_rows, audio_rows, seg, float(sigma), after_forward)
        finally:
            self._folded, self._folded_key = None, None      # not an inference fold, and the running statistics changed in place

    def _train_step(self, folded, logdet, mel_rows, audio_rows, seg: _Segments, sigma: float, after_forward=None) -> torch.Tensor:
        rows, dev, c = seg.rows, audio_rows.device, self.n_audio_channels
        f32 = torch.float32
        blocks = [_TrainWN(wn, f) for wn, f in zip(self.wn_layers, folded)]
        bnd = []                               # the forward: the likelihood's walk over training blocks, every boundary recorded
        z, ls_row, _ = self._flows_fwd(blocks, mel_rows, seg, audio_rows, False, bnd)
        nrows = torch.full((seg.b,), float(seg.length), dtype=torch.float64, device=dev)
        loss = self._nll_from_sums(self._reduce(z, ls_row, seg), nrows, sigma, logdet)[1]
        if after_forward is not None:
            after_forward()

        # backward: the boundaries from the tail to the first flow, each WN block between two of them
        n_all = float(rows) * c
        z_scale, inv_n = 1.0 / (sigma * sigma * n_all), 1.0 / n_all
        nblk = _lib.load().rtts_sw_boundary_bwd_blocks(rows)
        grads, dout = [], None
        for j in reversed(range(self.n_flows + 1)):
            x_in, wn_in, zc, n_early, w = bnd[j]
            n_in = x_in.shape[1]
            n = n_in - n_early
            dx = dwn = dw = part = None
            if wn_in is not None:
                dx = torch.empty(rows, n_in, dtype=f32, device=dev)
                dwn = blocks[j - 1].new_dwn(seg)
            if w is not None:
                dw = torch.empty(n, n, dtype=f32, device=dev)
                part = torch.empty(nblk * n * n, dtype=f32, device=dev)
            ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
            ld = lambda t: 0 if t is None else t.stride(0)          # noqa: E731
            _lib.call("rtts_sw_boundary_bwd", x_in.data_ptr(), x_in.stride(0), ptr(wn_in), ld(wn_in), ptr(w), n_in, n_early, rows, ptr(dout),
                      ld(dout), z.data_ptr(), z.stride(0), zc, z_scale, inv_n, ptr(dx), ld(dx), ptr(dwn), ld(dwn), ptr(dw), ptr(part), _s())
            if w is not None:                                                      # - (B L / N) W^-T from the log-determinant
                grads.append((self.inv_conv_layers[j].conv.weight, (dw - self._winv[j].t() / c).unsqueeze(-1)))
            if wn_in is not None:
                da0 = blocks[j - 1].backward(dwn, seg, grads)
                dx[:, :da0.shape[1]] += da0
                dout = dx
        params = {id(p) for p in self.parameters()}
        assert len(grads) == len(params) and {id(p) for p, _ in grads} == params, "nll_backward: a parameter was left without a gradient"
        for p, g in grads:                     # one addition per parameter: two calls give exactly twice the gradient
            g = g.reshape(p.shape)
            if p.grad is None:
                p.grad = g.contiguous().clone()
            else:
                p.grad.add_(g)
        return loss

    def samples_per_frame(self) -> int:
        """Audio samples per mel frame: mel_upsample_scale * n_audio_channels (256, ``modules.py:341``)."""
        return self._up() * self.n_audio_channels

    def _audio_starts(self, audio: torch.Tensor, lens: List[int], sample_offsets, dev, what: str):
        """-> (flat fp32 device buffer, host list of every utterance's first sample in it).  ``audio``: (B, N) padded rows
        (utterance i = the first 256 * lens[i] samples of row i) or a flat buffer with ``sample_offsets`` (B or B + 1 host
        ints; default: the utterances end to end, 256 * lens[i] samples each)."""
        self._on_device(audio, dev, what, "audio")
        spf = self.samples_per_frame()
        if audio.dim() == 2:
            if sample_offsets is not None or audio.shape[0] != len(lens):
                raise ValueError(f"SqueezeWave.{what}: audio {tuple(audio.shape)} for {len(lens)} utterances (sample_offsets go with a flat buffer)")
            starts = [i * audio.shape[1] for i in range(len(lens))]
            ends = [(i + 1) * audio.shape[1] for i in range(len(lens))]
        elif audio.dim() == 1:
            if sample_offsets is None:
                starts = [spf * m for m in segment_offsets(lens)[:-1]]
            else:
                starts = host_lengths(sample_offsets)[:len(lens)]
                if len(starts) != len(lens):
                    raise ValueError(f"SqueezeWave.{what}: {len(starts)} sample offsets for {len(lens)} utterances")
            ends = [audio.numel()] * len(lens)
        else:
            raise ValueError(f"SqueezeWave.{what}: audio is (B, N) or a flat buffer (got {tuple(audio.shape)})")
        for i, (a, e, n) in enumerate(zip(starts, ends, lens)):
            if a + spf * n > e:
                raise ValueError(f"SqueezeWave.{what}: utterance {i} has {n} frames = {spf * n} samples, its audio holds {max(e - a, 0)} "
                                 f"(the audio length must be {spf} * frames)")
        flat = audio.to(torch.float32).contiguous().view(-1)
        return flat, starts

    def _pack_audio(self, flat: torch.Tensor, starts: List[int], moff: torch.Tensor, nseg: int, capacity_frames: int,
                    start_table: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """flat fp32 audio + per-utterance first samples -> packed rows (up * capacity_frames, n_audio_channels), one launch."""
        up, c = self._up(), self.n_audio_channels
        host = torch.tensor(starts, dtype=torch.int64).pin_memory()
        start_table = host.to(flat.device, non_blocking=True) if start_table is None else start_table.copy_(host, non_blocking=True)
        if out is None:
            out = torch.empty(up * capacity_frames, c, dtype=torch.float32, device=flat.device)
        _lib.call("rtts_sw_pack_audio", flat.data_ptr(), max(flat.numel(), 1), start_table.data_ptr(), moff.data_ptr(), nseg, up, c,
                  up * capacity_frames, out.data_ptr(), _s())
        return out

    def _ragged_lengths(self, frames, what: str):
        lens = host_lengths(frames)
        if not 1 <= len(lens) <= SW_MAX_SEGMENTS:
            raise ValueError(f"SqueezeWave.{what}: a ragged vocoder call takes 1..{SW_MAX_SEGMENTS} utterances (got {len(lens)})")
        return lens, segment_offsets(lens)

    @torch.no_grad()
    def nll_ragged(self, mel: torch.Tensor, frames, audio: torch.Tensor, sample_offsets=None, sigma: float = 1.0):
        """B utterances of different lengths, each scored as ``nll(mel[i:i+1, :, :frames[i]], its 256 * frames[i] samples)``
        would score it: mel (B, n_mel, Lmax) (any strides), ``frames`` (B,) host ints, ``audio`` (B, N) padded rows or a flat
        buffer (``sample_offsets``: every utterance's first sample, host ints; default end to end) -> (per-utterance NLL
        (B,) fp32, the loss of the whole batch 0-dim fp32: all sums over all utterances divided by the total element count,
        ``SqueezeWaveLoss`` of the concatenation).  The utterances are laid end to end as rows, as in ``infer_ragged``.  An
        utterance of zero frames scores NaN and adds nothing to the batch loss."""
        dev = self._likelihood_device("nll_ragged")
        folded, logdet = self._fold(), self._logdets()
        lens, moff_h = self._ragged_lengths(frames, "nll_ragged")
        self._on_device(mel, dev, "nll_ragged", "mel")
        flat, starts = self._audio_starts(audio, lens, sample_offsets, dev, "nll_ragged")
        total = moff_h[-1]
        if total == 0:
            nan = torch.full((len(lens),), float("nan"), device=dev)
            return nan, nan[0].clone()
        up = self._up()
        moff = self._offsets_to(moff_h, dev)
        mel_rows = self._pack_mel(mel, lens, moff, total)
        audio_rows = self._pack_audio(flat, starts, moff, len(lens), total)
        seg = _Segments.packed(moff, total, up)
        z, ls_row, _ = self._flows_fwd(folded, mel_rows, seg, audio_rows, False)
        nrows = (moff[1:] - moff[:-1]).to(torch.float64) * up
        return self._nll_from_sums(self._reduce(z, ls_row, seg), nrows, sigma, logdet)

    def capture_nll_ragged(self, batch: int, capacity_frames: int, sigma: float = 1.0):
        """-> ``run(mel, frames, audio, sample_offsets=None) -> (per-utterance NLL (B,), batch NLL)``: ``nll_ragged`` for
        ``batch`` utterances of at most ``capacity_frames`` mel frames in total, as ONE hipGraph that any set of lengths
        replays (the contract and cache of ``capture_ragged``).  Per call the offset tables are copied in and the mel and the
        audio packed into the graph's input rows (two kernels, outside the graph).  A total above the capacity raises before
        anything is launched.  The returned tensors are the graph's output buffers: copy them before the next call."""
        dev = self._likelihood_device("capture_nll_ragged")
        batch, cap = int(batch), int(capacity_frames)
        if not 1 <= batch <= SW_MAX_SEGMENTS or cap < 1:
            raise ValueError(f"capture_nll_ragged: 1..{SW_MAX_SEGMENTS} utterances and a positive capacity (got {batch}, {cap})")
        cache = self.__dict__.setdefault("_nll_graphs", {})
        key = (batch, cap, float(sigma))
        if key in cache and cache[key].folded is self._fold():
            return cache[key]
        folded, logdet = self._fold(), self._logdets()
        up, c = self._up(), self.n_audio_channels
        mel_rows = torch.zeros(cap, self._n_mel(), device=dev)
        audio_rows = torch.zeros(up * cap, c, device=dev)
        moff = torch.zeros(batch + 1, dtype=torch.int32, device=dev)        # every row padding until a call sets the table
        start_table = torch.zeros(batch, dtype=torch.int64, device=dev)
        seg = _Segments.packed(moff, cap, up)

        def score():
            z, ls_row, _ = self._flows_fwd(folded, mel_rows, seg, audio_rows, False)
            nrows = (moff[1:] - moff[:-1]).to(torch.float64) * up
            return self._nll_from_sums(self._reduce(z, ls_row, seg), nrows, sigma, logdet)

        graph, (per, total_loss) = warm_capture(score)

        def run(mel: torch.Tensor, frames, audio: torch.Tensor, sample_offsets=None):
            if self.training:
                raise _lib.RttsError("capture_nll_ragged: the graph was captured in eval mode (running-statistics BatchNorm); call .eval()")
            lens, moff_h = self._ragged_lengths(frames, "capture_nll_ragged")
            if len(lens) != batch or moff_h[-1] > cap:
                raise ValueError(f"capture_nll_ragged graph for {batch} utterances of {cap} frames in total: got {len(lens)} utterances, "
                                 f"{moff_h[-1]} frames")
            self._on_device(mel, dev, "capture_nll_ragged", "mel")
            flat, starts = self._audio_starts(audio, lens, sample_offsets, dev, "capture_nll_ragged")
            self._offsets_to(moff_h, dev, out=moff)
            self._pack_mel(mel, lens, moff, cap, out=mel_rows)
            self._pack_audio(flat, starts, moff, batch, cap, start_table=start_table, out=audio_rows)
            graph.replay()
            return per, total_loss
        run.batch, run.capacity, run.folded, run.graph = batch, cap, folded, graph
        cache[key] = run
        return run
