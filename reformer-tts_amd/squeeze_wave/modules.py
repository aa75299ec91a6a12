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

There is no CPU fallback: ``infer`` raises off the GPU."""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import nn

from .. import _lib
from .._graphs import capturing
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


class _FoldedWN:
    """Inference weights of one WN block: bf16 GEMM operands (row-major (Cout, Cin)), fp32 biases, depthwise taps with
    the eval-mode BatchNorm folded in:  dw(bn(x)) = sum_k (w_k * a) x_{l+k-1} + [b + (sum_k w_k) * c],
    a = gamma / sqrt(var + eps), c = beta - mean * a.  (Zero padding pads bn(x), i.e. the constant c is NOT added at the
    borders by the reference; the border rows get the exact correction below.)

    Every 1x1 convolution (``start``, ``cond_layer``, the pointwise half of ``in_layers``, ``res_skip_layers``, ``end``;
    reference ``modules.py:203-235``) is ``rtts_gemm_nt`` (csrc/gemm_nt.hip) over channels-last rows: operands are padded ONCE
    here to the kernel's granules -- input widths to multiples of 64 (audio halves 64, 56, ... and the 80 mel channels: zero
    columns), the ``end`` projection's 2 * n_half outputs to a multiple of 64 (zero rows; its consumer takes a row stride) --
    and the row count of an utterance is rounded up to 128 in the activation buffers (rows are independent: the extra rows
    are never read back).  ``in_tree`` is False for toy widths the MFMA kernel does not tile (n_channels % 64, n_half % 8 or
    n_mel % 8 != 0): those run the same arithmetic through the library GEMM and say so once."""

    def __init__(self, wn: WN):
        bf = torch.bfloat16
        self.c, self.nl, self.up = wn.n_channels, wn.n_layers, wn.upsample_scale
        if wn.kernel_size != 3:
            raise NotImplementedError("the HIP depthwise kernel is built for conv_kernel_size == 3")
        w_start, w_cond = _normed(wn.start_conv), _normed(wn.cond_layer)
        w_end = wn.end_conv.weight.detach().float().squeeze(-1)
        self.n_half, self.n_mel = w_start.shape[1], w_cond.shape[1]
        self.in_tree = self.c % 64 == 0 and self.n_half % 8 == 0 and self.n_mel % 8 == 0
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
        self.dw_w, self.dw_b, self.dw_edge, self.w_pw, self.b_pw, self.w_rs, self.b_rs = [], [], [], [], [], [], []
        for i in range(wn.n_layers):
            bn, dw, pw = wn.in_layers[i].layer
            a = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
            cst = bn.bias.detach().float() - bn.running_mean.float() * a
            w = dw.weight.detach().float().squeeze(1)                          # (C, 3)
            self.dw_w.append((w * a[:, None]).contiguous())
            self.dw_b.append((dw.bias.detach().float() + w.sum(1) * cst).contiguous())
            # at l = 0 the tap k = 0 sees the zero padding of bn(x), not c; at l = L-1 the tap k = 2 likewise
            self.dw_edge.append(((w[:, 0] * cst).contiguous(), (w[:, 2] * cst).contiguous()))
            self.w_pw.append(pw.weight.detach().float().squeeze(-1).to(bf).contiguous())
            self.b_pw.append(pw.bias.detach().float().contiguous())
            self.w_rs.append(_normed(wn.res_skip_layers[i]).to(bf).contiguous())
            self.b_rs.append(wn.res_skip_layers[i].bias.detach().float().contiguous())

    def condition(self, mel: torch.Tensor, seg: _Segments) -> torch.Tensor:
        """mel fp32 (B*Lm, n_mel) rows -> (rows, 2c * n_layers) bf16: the conditioning of all layers in one GEMM."""
        if not self.in_tree:
            return torch.addmm(self.b_cond.to(torch.bfloat16), mel.to(torch.bfloat16), self.w_cond.t())
        from ..engine import gemm
        mp, kp = _pad(seg.b * seg.mel_len, 128), self.w_cond.shape[1]
        x = torch.empty(mp, kp, dtype=torch.bfloat16, device=mel.device)
        _lib.call("rtts_to_halo", mel.data_ptr(), mel.stride(0), 0, self.n_mel, 1, seg.b, seg.mel_len, 0, kp, x.data_ptr(), 0, mp, _s())
        return gemm(x, self.w_cond, bias=self.b_cond)

    def forward(self, audio: torch.Tensor, mel: torch.Tensor, seg: _Segments) -> torch.Tensor:
        """audio fp32 (seg.rows, n_rem) rows (the first n_half channels condition the block), mel fp32 (B*Lm, n_mel) rows
        -> fp32 (rows >= seg.rows, n_end >= 2*n_half) = [s | b | zero columns].  Only the depthwise convolution looks
        across rows: it is the one launch that differs between a uniform and a packed batch."""
        dev, c = audio.device, self.c
        b, length, mel_len, up = seg.b, seg.length, seg.mel_len, seg.up
        m = seg.rows
        cond = self.condition(mel, seg)
        if self.in_tree:
            from ..engine import gemm
            mp, kp = _pad(m, 128), self.w_start.shape[1]
            a0 = torch.empty(mp, kp, dtype=torch.bfloat16, device=dev)        # bf16 copy of the conditioning half, zero padded
            _lib.call("rtts_to_halo", audio.data_ptr(), audio.stride(0), 0, self.n_half, 1, b, length, 0, kp, a0.data_ptr(), 0, mp, _s())
            h = gemm(a0, self.w_start, bias=self.b_start, out_f32=True)        # (mp, c) fp32: the WN residual stream
            mm = lambda x, w, bias=None, f32=False: gemm(x, w, bias=bias, out_f32=f32)     # noqa: E731
        else:
            _lib.note_general_path("SqueezeWave WN block", f"widths (n_channels {c}, n_half {self.n_half}, n_mel {self.n_mel}) the MFMA GEMM "
                                   "does not tile (n_channels % 64, n_half % 8, n_mel % 8): library GEMM")
            mp = m
            a0 = audio[:, :self.n_half].contiguous()
            h = torch.addmm(self.b_start, a0, self.w_start.float().t())

            def mm(x, w, bias=None, f32=False):
                y = torch.mm(x, w.t(), out_dtype=torch.float32)
                y = y if bias is None else y + bias
                return y if f32 else y.to(torch.bfloat16)
        for i in range(self.nl):
            dw = torch.empty(mp, c, dtype=torch.bfloat16, device=dev)
            lo, hi = self.dw_edge[i]                                             # zero padding pads bn(x): no folded constant there
            if seg.moff is None:
                _lib.call("rtts_sw_depthwise_k3", h.data_ptr(), self.dw_w[i].data_ptr(), self.dw_b[i].data_ptr(), b, length, c, dw.data_ptr(),
                          lo.data_ptr(), hi.data_ptr(), _s())
            else:
                _lib.call("rtts_sw_depthwise_k3_seg", h.data_ptr(), self.dw_w[i].data_ptr(), self.dw_b[i].data_ptr(), seg.moff.data_ptr(),
                          seg.nseg, up, m, c, dw.data_ptr(), lo.data_ptr(), hi.data_ptr(), _s())
            pw = mm(dw, self.w_pw[i], self.b_pw[i])                                # (mp, 2c) bf16
            acts = torch.empty(mp, c, dtype=torch.bfloat16, device=dev)
            _lib.call("rtts_sw_gate", pw.data_ptr(), cond.data_ptr(), cond.stride(0), i * 2 * c, up, b, length, mel_len, c, acts.data_ptr(), _s())
            rs = mm(acts, self.w_rs[i])
            _lib.call("rtts_residual_epilogue", h.data_ptr(), rs.data_ptr(), self.b_rs[i].data_ptr(), 1.0, h.data_ptr(), m, c, 0.0, 0, None, _s())
        hb = torch.empty(mp, c, dtype=torch.bfloat16, device=dev)
        _lib.call("rtts_cast_f32_bf16", h.data_ptr(), hb.data_ptr(), m * c, _s())
        return mm(hb, self.w_end, self.b_end, True)


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

    def _fold(self):
        key = tuple((p.data_ptr(), p._version) for p in self.parameters()) + tuple((b.data_ptr(), b._version) for b in self.buffers())
        if self._folded is None or self._folded_key != key:
            with torch.no_grad():
                self._folded = [_FoldedWN(wn) for wn in self.wn_layers]
                # twelve matrices of at most 128 x 128, once per parameter version: inverted on the host in float64 (LAPACK) -- no
                # device library (rocSOLVER / hipBLAS) call anywhere in the vocoder
                dev = self.inv_conv_layers[0].conv.weight.device
                self._winv = [conv.conv.weight.detach().squeeze(-1).double().cpu().inverse().float().contiguous().to(dev)
                              for conv in self.inv_conv_layers]
            self._folded_key = key
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
        (seg.rows, C) rows in the order they are consumed -> clamped audio rows (seg.rows, n_audio_channels)."""
        audio = next(draws)                                                        # (rows, n_remaining) fp32
        for k in reversed(range(self.n_flows)):
            n = audio.shape[1]
            wn_out = folded[k].forward(audio, mel_rows, seg)                       # [s | b | padding], row stride n_end
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
        length = mel_len * (256 // self.n_audio_channels)
        if folded[0].up * mel_len != length:
            raise ValueError("mel_upsample_scale must equal 256 // n_audio_channels")
        shapes = self.noise_shapes(b, mel_len)
        if noise is None:
            noise = [torch.randn(s, device=dev) for s in shapes]
        assert [tuple(z.shape) for z in noise] == shapes, "noise tensors do not match noise_shapes()"
        rows = lambda z: z.to(dev, torch.float32).permute(0, 2, 1).reshape(b * length, -1).contiguous()    # noqa: E731
        mel_rows = mel.to(torch.float32).permute(0, 2, 1).reshape(b * mel_len, n_mel).contiguous()
        audio = self._flows(folded, mel_rows, _Segments.uniform(b, mel_len, folded[0].up), (rows(z) for z in noise), sigma)
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
        dev = self.inv_conv_layers[0].conv.weight.device
        mel_buf = torch.zeros(batch, self.wn_layers[0].cond_layer.weight_v.shape[1] if hasattr(self.wn_layers[0].cond_layer, "weight_v")
                              else self.wn_layers[0].cond_layer.weight.shape[1], mel_len, device=dev)
        shapes = self.noise_shapes(batch, mel_len)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.infer(mel_buf, sigma)                         # warm-up: folding, allocator, lazy attributes
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with capturing(graph):
            out = self.infer(mel_buf, sigma, noise=[torch.randn(s, device=dev) for s in shapes])

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
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # warm-up: allocator, lazy attributes
            self._flows(folded, mel_rows, seg, iter([torch.randn(up * cap, w, device=dev) for w in widths]), sigma)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with capturing(graph):
            draws = [torch.randn(up * cap, w, device=dev) for w in widths]
            out = self._flows(folded, mel_rows, seg, iter(draws), sigma).view(-1)

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

