"""Incremental generation for an all-dense decoder: one new frame = ONE row per utterance through the decoder, against a cache.

Dense shared-QK attention (``use_full_attn``, csrc/full_attn.hip) is exact, deterministic and causal: a decoder row at a valid
position depends only on the valid rows at or before it, and all that has to be kept from earlier frames is one ``[qk | v]`` row
per layer.  ``IncrementalDecoder`` runs, for position p, what ``ReformerTTS.forward`` computes at row p when the decoder input
is the p + 1 frames generated so far and NO padding rows are appended behind them:

  * the encoder once per utterance, and every decoder layer's cross-attention ``k | v`` projection of its output once;
  * prenet -> alpha * PE(p) -> the decoder stack's program (``engine.build_program``) -> mel / stop heads on rows padded to 128,
    through the GEMM / LayerNorm / residual kernels the full-window executor uses in eval mode, with the two attention cores
    replaced by the single-query kernels of csrc/decode.hip (``ops.decode_self_attn``, ``ops.decode_cross_attn``);
  * the postnet on its TAIL: the last output row of n = depth + 1 convolutions (k = 5) needs the last 2 n + 1 mel rows only.

The position lives in a device int32 that every kernel reads when it runs, so the step is captured into one hipGraph ONCE and
that graph is replayed for every frame of every length (the windowed path needs a graph per padded window).

The one visible difference to the windowed ``infer``: there the postnet runs over the PADDED window, so row p also sees up to
10 rows of decoder output at padding positions, which in "concat" mode feeds back into the autoregression.  Here the sequence
ends at p -- ``mel_post[p] = mel[p] + postnet(mel[0..p])[p]``, zero padding on the right -- so incremental generation is not
frame-for-frame equal to windowed generation of the same model.

A checkpoint trained with LSH layers loads into a ``use_full_attn: true`` decoder config unchanged (same ``toqk`` / ``tov`` /
``to_out`` names); the generator itself never switches a layer's branch and refuses a decoder that is not dense."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

ROWS = 128                # the row tile of rtts_gemm_nt: the B <= 128 new rows ride in one tile
MAX_BATCH = 128
MAX_CAPACITY = 4096


def _ceil(n: int, base: int) -> int:
    return -(-n // base) * base


def generation_plan(batch: int, n_mels: int, max_len: int) -> Tuple[int, int]:
    """(frames generated when no sample stops, cache capacity) for ``infer``'s loop: it runs while ``max(batch, cur, n_mels) <=
    max_len`` with ``cur`` = frames in the buffer (start frame included), so at least once."""
    steps = max_len if max(batch, n_mels) <= max_len else 1          # cur counts 2, 3, ... and the first cur > max_len ends the loop
    return steps, _ceil(steps, 64)


def _decoder_sublayers(model):
    """[(block, inner WithNorm)] of the decoder's ReversibleHalfResidual blocks, in order."""
    from .reformer import Chunk
    from .reversible import ReversibleHalfResidual
    out = []
    for blk in model.dec.reformer.layers.blocks:
        if isinstance(blk, ReversibleHalfResidual):
            net = blk.f.net
            out.append(net.fn if isinstance(net, Chunk) else net)
    return out


def check_supported(model, batch: int, capacity: int, text_len: Optional[int] = None) -> None:
    """Raise NotImplementedError, naming what is missing, unless ``IncrementalDecoder`` can run ``model`` (host logic only)."""
    from ..engine import FFNExec, XAttnExec, build_program
    from .reformer import LSHSelfAttentionWrapper, MultiheadAttentionWrapper
    for wn in _decoder_sublayers(model):
        fn = wn.fn
        if isinstance(fn, LSHSelfAttentionWrapper):
            if fn.implementation != "hip":
                raise NotImplementedError(f"incremental generation needs decoder self-attention with implementation='hip', got {fn.implementation!r}")
            if not fn.layer.use_full_attn:
                raise NotImplementedError("incremental generation needs dense decoder self-attention (self_attn_kwargs.use_full_attn: true): "
                                          "LSH attention draws fresh rotations per call and sorts padding positions, a different function per draw")
            if fn.layer.dim // fn.layer.heads != 64:
                raise NotImplementedError(f"incremental generation: self-attention heads of {fn.layer.dim // fn.layer.heads} (the kernels take 64)")
        elif isinstance(fn, MultiheadAttentionWrapper):
            if not XAttnExec.supported(wn):
                raise NotImplementedError("incremental generation: the cross-attention is outside XAttnExec.supported (heads of 64 or 128, no bias_k, "
                                          "no add_zero_attn, one embedding width)")
        elif hasattr(fn, "net"):
            if not FFNExec.supported(wn):
                raise NotImplementedError("incremental generation: the feed-forward is outside the executors' envelope (dropout 0, widths % 64 == 0)")
    if build_program(model.dec.reformer.layers) is None:
        raise NotImplementedError("incremental generation: a decoder block is outside the explicit executors' envelope")
    d, nm = model.dec.prenet.output_size, model.num_mel_coeffs
    if d % 128 != 0:
        raise NotImplementedError(f"incremental generation: model width {d} is not a multiple of 128 (the executors' envelope)")
    if nm % 8 != 0 or nm > 128:
        raise NotImplementedError(f"incremental generation: n_mels {nm} is outside the executors' envelope (a multiple of 8 up to 128)")
    if not 1 <= batch <= MAX_BATCH:
        raise NotImplementedError(f"incremental generation: batch {batch} > {MAX_BATCH} (the new rows ride in one 128-row GEMM tile)")
    if not 1 <= capacity or _ceil(capacity, 64) > MAX_CAPACITY:
        raise NotImplementedError(f"incremental generation: capacity {capacity} > {MAX_CAPACITY} frames")
    if text_len is not None and (text_len % 128 != 0 or not 128 <= text_len <= 2048):
        raise NotImplementedError(f"incremental generation: {text_len} encoder keys (the cross-attention kernels take multiples of 128 up to 2048)")


def postnet_convs(postnet) -> List[tuple]:
    """[(conv, bn | None)] of a PostConvNet: depth x (Conv1d, BatchNorm1d) + the bare last convolution."""
    depth = (len(postnet.layers) - 1) // 4
    return [(getattr(postnet.layers, f"conv{i}"), getattr(postnet.layers, f"bn{i}")) for i in range(depth)] + [(postnet.layers.convend, None)]


def postnet_tail_reference(postnet, mel: torch.Tensor, p: int) -> torch.Tensor:
    """``postnet(mel[:, :p + 1])[:, p]`` (eval mode) from the last 2 n + 1 rows only, with the row bookkeeping of the device path:
    window row w <-> position a = p - 2 n + w; layer k reads window rows >= 2 k, writes rows >= 2 k + 2; a row is absent (zero) at
    EVERY layer's input when its position is in front of frame 0 or behind p.  Plain torch in ``mel``'s dtype (float64 on the CPU
    in the tests); mel (B, >= p + 1, n_mels) -> (B, n_mels)."""
    convs = postnet_convs(postnet)
    n = len(convs)
    r = 2 * n + 1
    b = mel.shape[0]
    pos = torch.arange(r) + (p - (r - 1))
    x = torch.zeros(b, r, mel.shape[2], dtype=mel.dtype)
    ok = pos >= 0
    x[:, ok] = mel[:, pos[ok]]
    src_r0 = 0
    for k, (conv, bn) in enumerate(convs):
        r0 = 2 * (k + 1)
        w = conv.weight.to(mel.dtype)                                        # (Co, Ci, 5)
        rows = []
        for row in range(r0, r):
            acc = conv.bias.to(mel.dtype).expand(b, -1).clone()
            for tap in range(5):
                wi = row + tap - 2
                if 0 <= wi < r and pos[wi] >= 0 and wi >= src_r0:
                    acc = acc + x[:, wi - src_r0] @ w[:, :, tap].t()
            rows.append(acc)
        y = torch.stack(rows, dim=1)
        if bn is not None:
            y = (y - bn.running_mean.to(mel.dtype)) * torch.rsqrt(bn.running_var.to(mel.dtype) + bn.eps) * bn.weight.to(mel.dtype) + bn.bias.to(mel.dtype)
            y = torch.tanh(y)
        x, src_r0 = y, r0
    return x[:, -1]


class IncrementalDecoder:
    """State of one batch of utterances being generated frame by frame (see the module docstring).

    ``step(frame)``: frame (B, n_mels) = the decoder input at position ``pos`` (the zero start frame at 0) -> (mel, mel_post,
    stop_logit) of that position; ``pos`` advances on the device, nothing is read back.  ``generate_step()`` is ``step`` on the
    frame the previous step produced plus ``infer``'s bookkeeping (output buffer, stop indices); ``capture()`` records it once."""

    def __init__(self, model, phonemes: torch.Tensor, capacity: int, stop_threshold: float = 0.25, track_stops: bool = True):
        from ..engine import LSHExec, XAttnExec, build_program
        self.b = b = phonemes.shape[0]
        self.tk = _ceil(phonemes.shape[1], model.pad_base)
        check_supported(model, b, capacity, self.tk)
        model._require_gpu()
        self.model = model
        self.dev = dev = model.dec.mel_linear.weight.device
        self.cap = cap = _ceil(capacity, 64)
        self.nm = nm = model.num_mel_coeffs
        self.d = d = model.dec.prenet.output_size
        self.thr, self.track_stops = float(stop_threshold), bool(track_stops)
        self.program = [(kind, f) for kind, f, _ in build_program(model.dec.reformer.layers)]
        if any(kind == "block" for kind, _ in self.program):
            raise NotImplementedError("incremental generation: the decoder stack is expected to be half-residual blocks and swaps")
        self.execs = [f for kind, f in self.program if kind == "half"]
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)       # noqa: E731
        self.frame = z(ROWS, nm)                                   # the decoder input rows; rows >= B stay zero (finite filler)
        self.pos = z(1, dt=torch.int32)
        self.pos64 = z(1, dt=torch.long)                           # the same position for torch's index kernels
        self.mel_hist = z(b, cap, nm)
        self.spec = z(b, cap + 1, nm)                              # frame 0 = the zero start frame
        self.stop = z(b, dt=torch.long)
        self.pad_ph = z(b, self.tk, dt=torch.long)
        self.kvalid = z(b, self.tk, dt=torch.uint8)
        self.keys_bf16 = z(b * self.tk, d, dt=torch.bfloat16)
        self.state = {}                                            # id(executor) -> its persistent buffers
        for ex in self.execs:
            st = self.state[id(ex)] = {}
            if isinstance(ex, LSHExec):
                h = ex.layer.heads
                st.update(cache=z(b, cap, 2 * d, dt=torch.bfloat16), o=z(ROWS, d, dt=torch.bfloat16), wqkv=z(2 * d, d, dt=torch.bfloat16),
                          wo=z(d, d, dt=torch.bfloat16), heads=h)
                self._workspace(st, b * h, cap, 64)
            elif isinstance(ex, XAttnExec):
                h = ex.mha.num_heads
                st.update(kv=z(b, self.tk, 2 * d, dt=torch.bfloat16), o=z(ROWS, d, dt=torch.bfloat16), win=z(3 * d, d, dt=torch.bfloat16),
                          wo=z(d, d, dt=torch.bfloat16), heads=h)
                self._workspace(st, b * h, self.tk, d // h)
            else:
                ff = ex.l1.weight.shape[0]
                st.update(w1=z(ff, d, dt=torch.bfloat16), w2=z(d, ff, dt=torch.bfloat16))
        # postnet tail: window of R = 2 n + 1 positions; layer k writes window rows 2 k + 2 ... R - 1
        from ..edges import _conv_exec
        self.convs = postnet_convs(model.postnet)
        self.R = 2 * len(self.convs) + 1
        self.tail = []
        for k, (conv, bn) in enumerate(self.convs):
            ex = _conv_exec(conv)
            nr = self.R - 2 * (k + 1)
            t = dict(ex=ex, nr=nr, a=z(_ceil(b * nr, ROWS), 5 * ex.cp, dt=torch.bfloat16))
            if bn is not None:
                t.update(mean=z(ex.cop), rstd=z(ex.cop), gamma=z(ex.cop), beta=z(ex.cop))
            else:
                t.update(bias=z(ex.cop))
            self.tail.append(t)
        self.pe_table = model.dec.positional_encoding.table(cap, dev)
        self.graph = None
        self.graphs_captured = 0
        self.params = tuple(p_.data_ptr() for p_ in model.parameters())
        self.begin(phonemes)

    def _workspace(self, st, bh, t, dh):
        from .. import _lib, ops
        st["splits"] = ops.decode_attn_splits(bh, t)
        if st["splits"] < 1:
            raise _lib.RttsError(f"single-query attention: no split count for B*H={bh}, T={t}")
        nbytes = int(_lib.load().rtts_decode_attn_workspace(bh, st["splits"], dh))
        st["ws"] = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=self.dev)

    # ------------------------------------------------------------------------------------------------ per utterance
    @torch.no_grad()
    def begin(self, phonemes: torch.Tensor) -> None:
        """A new batch of utterances of the shape this state was built for: refresh the bf16 weight copies and the postnet's
        folded BatchNorm vectors IN PLACE (a captured graph holds their addresses), run the encoder once, project its output to
        every layer's cross-attention ``k | v``, and rewind the position."""
        from ..engine import LSHExec, XAttnExec, _bf16, bf16_twin, gemm
        from .reformer_tts import pad_to_multiple
        model, b, d = self.model, self.b, self.d
        pad_ph = pad_to_multiple(phonemes.to(self.dev).unsqueeze(-1), model.pad_base).squeeze(-1)
        if tuple(pad_ph.shape) != (b, self.tk):
            raise ValueError(f"IncrementalDecoder.begin: phonemes pad to {tuple(pad_ph.shape)}, this state was built for {(b, self.tk)}")
        was_training = model.training
        model.eval()
        enc_stack = model.enc.reformer.layers
        was_fused = enc_stack.fused_in_eval
        enc_stack.fused_in_eval = True                      # the encoder through the explicit executor: no library GEMM
        try:
            self.pad_ph.copy_(pad_ph)
            ph_mask = self.pad_ph != 0
            self.kvalid.copy_(ph_mask)
            keys = model.enc(self.pad_ph, input_mask=ph_mask)
            twin = bf16_twin(keys)
            self.keys_bf16.copy_(keys.reshape(-1, d) if twin is None else twin.view(-1, d))
        finally:
            enc_stack.fused_in_eval = was_fused
            model.train(was_training)
        for ex in self.execs:
            st = self.state[id(ex)]
            if isinstance(ex, LSHExec):
                st["wqkv"].copy_(ex._wqkv())
                st["wo"].copy_(_bf16(ex.layer.to_out.weight))
            elif isinstance(ex, XAttnExec):
                st["win"].copy_(_bf16(ex.mha.in_proj_weight))
                st["wo"].copy_(_bf16(ex.mha.out_proj.weight))
                # the k | v projection of the keys, once per utterance: the existing GEMM on B * T_k rows
                st["kv"].view(-1, 2 * d).copy_(gemm(self.keys_bf16, st["win"][d:], bias=ex.mha.in_proj_bias[d:]))
            else:
                st["w1"].copy_(_bf16(ex.l1.weight))
                st["w2"].copy_(_bf16(ex.l2.weight))
        for (conv, bn), t in zip(self.convs, self.tail):
            ex = t["ex"]
            ex.weight_perm()
            if bn is not None:                              # eval BatchNorm: the kernel's "mean" is running_mean - conv bias
                t["mean"][:ex.co].copy_(bn.running_mean - conv.bias.detach())
                t["rstd"][:ex.co].copy_(torch.rsqrt(bn.running_var + bn.eps))
                t["gamma"][:ex.co].copy_(bn.weight.detach())
                t["beta"][:ex.co].copy_(bn.bias.detach())
            else:
                t["bias"][:ex.co].copy_(conv.bias.detach())
        self.rewind()

    def rewind(self) -> None:
        """Back to position 0 with the zero start frame.  The caches need no clearing: rows at or beyond ``pos`` are never read."""
        for t_ in (self.pos, self.pos64, self.stop, self.frame, self.spec):
            t_.zero_()

    # ------------------------------------------------------------------------------------------------ one position
    def _sublayer(self, ex, xn):
        """f(LN(inp)) in front of its output bias: -> (g (ROWS, d) bf16, bias)."""
        from .. import ops
        from ..engine import LSHExec, XAttnExec, gemm
        st, b, d = self.state[id(ex)], self.b, self.d
        if isinstance(ex, LSHExec):
            row = gemm(xn, st["wqkv"])                                                       # (ROWS, 2d) = [qk | v] of the new position
            ops.decode_self_attn(row, st["cache"], self.pos, st["heads"], splits=st["splits"], out=st["o"], workspace=st["ws"], batch=b)
            return gemm(st["o"], st["wo"]), ex.layer.to_out.bias
        if isinstance(ex, XAttnExec):
            q = gemm(xn, st["win"][:d], bias=ex.mha.in_proj_bias[:d])
            ops.decode_cross_attn(q, st["kv"], st["heads"], self.kvalid, splits=st["splits"], out=st["o"], workspace=st["ws"], batch=b)
            return gemm(st["o"], st["wo"]), ex.mha.out_proj.bias
        h = gemm(xn, st["w1"], bias=ex.l1.bias, relu=True)
        return gemm(h, st["w2"]), ex.l2.bias

    def _postnet_tail(self, mel):
        """postnet(mel[0..p])[p] for every utterance: (B, n_mels) fp32.  ``mel_hist`` already holds row p."""
        from .. import _lib
        from .._seeds import seed_base
        from ..engine import _s, gemm
        b, dev = self.b, self.dev
        src, src_abs, ld, stride, src_r0, c = self.mel_hist, 1, self.nm, self.cap * self.nm, 0, self.nm
        y = None
        for k, t in enumerate(self.tail):
            ex, nr, a = t["ex"], t["nr"], t["a"]
            _lib.call("rtts_decode_tail_im2col", src.data_ptr(), src_abs, ld, stride, src_r0, c, self.pos.data_ptr(), self.cap, b, self.R,
                      self.R - nr, nr, ex.cp, a.data_ptr(), _s())
            if "bias" in t:
                y = gemm(a, ex.weight_perm(), bias=t["bias"], out_f32=True)
                break
            y = gemm(a, ex.weight_perm(), out_f32=True)
            rows = a.shape[0]
            zb = torch.empty(rows, ex.cop, dtype=torch.bfloat16, device=dev)
            _lib.call("rtts_bn_act_fwd", y.data_ptr(), t["mean"].data_ptr(), t["rstd"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), 2,
                      0.0, 0, seed_base(dev).data_ptr(), 1, rows, 0, ex.cop, zb.data_ptr(), 0, 0, rows, _s())
            src, src_abs, ld, stride, src_r0, c = zb, 0, ex.cop, nr * ex.cop, self.R - nr, ex.cop
        return y[:b, :self.nm]

    @torch.no_grad()
    def step(self, frame: Optional[torch.Tensor] = None):
        """One position for every utterance.  ``frame`` (B, n_mels) or None (the frame buffer as it stands).  The model must be
        in eval mode (``infer`` sees to it)."""
        from .. import _lib
        from ..edges import linear_nograd
        from ..engine import _s, ln_fwd, residual
        dec, b, d = self.model.dec, self.b, self.d
        if dec.training:
            raise RuntimeError("IncrementalDecoder.step runs the eval-mode kernels: call model.eval() first")
        if frame is not None:
            self.frame[:b].copy_(frame)
        x = dec.prenet(self.frame)                                                            # (ROWS, d) fp32, dropouts off
        pe = dec.positional_encoding
        x = x + pe.alpha * self.pe_table.index_select(0, self.pos64)                          # alpha * PE(p), p read on the device
        s1 = s2 = x.contiguous()
        pre, pre_ptr = None, None
        halves = [i for i, (kind, _) in enumerate(self.program) if kind == "half"]
        for i, (kind, ex) in enumerate(self.program):
            if kind == "swap":
                s1, s2 = s2, s1
                continue
            xn = pre[0] if (pre is not None and pre_ptr == s2.data_ptr()) else ln_fwd(s2, ex.norm)[0]
            g, bias = self._sublayer(ex, xn)
            later = [j for j in halves if j > i]
            nxt = self.program[later[0]][1].norm if later else None
            out = torch.empty_like(s1)
            pre = residual(s1, g, bias, 1.0, nxt, None, out=out)      # + the next sublayer's LayerNorm in the same launch
            s1, pre_ptr = out, out.data_ptr()
        hid = torch.empty(ROWS, d, dtype=torch.float32, device=self.dev)
        twin = torch.empty(ROWS, d, dtype=torch.bfloat16, device=self.dev)
        _lib.call("rtts_sum_streams", s1.data_ptr(), s2.data_ptr(), ROWS * d, hid.data_ptr(), twin.data_ptr(), _s())
        mel = linear_nograd(twin, dec.mel_linear, out_f32=True)[:b]
        stop_logit = linear_nograd(twin, dec.stop_linear, out_f32=True)[:b]
        self.mel_hist.index_copy_(1, self.pos64, mel.unsqueeze(1))
        mel_post = mel + self._postnet_tail(mel)
        self.pos.add_(1)
        self.pos64.add_(1)
        return mel, mel_post, stop_logit

    @torch.no_grad()
    def generate_step(self) -> None:
        """``step`` on the frame the previous step produced, plus the bookkeeping of ``ReformerTTS._infer_graphed``: the new frame
        goes behind the newest one in the output buffer and becomes the next input; a sample's stop index is set the first
        time its stop probability exceeds the threshold."""
        _, mel_post, stop_logit = self.step(None)
        if self.track_stops:
            stops_now = torch.sigmoid(stop_logit.reshape(self.b)) > self.thr
            self.stop.copy_(torch.where((self.stop == 0) & stops_now, stops_now.long() * self.pos64 + 1, self.stop))
        self.spec.index_copy_(1, self.pos64, mel_post.unsqueeze(1))
        self.frame[:self.b].copy_(mel_post)

    def capture(self) -> None:
        """Record ``generate_step`` into ONE hipGraph (after a warm-up on a side stream).  The step runs on one stream with no
        fork, so the graph has no parallel branches; the position is a device value, so the graph serves every frame."""
        from .._graphs import capturing
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.generate_step()
        torch.cuda.current_stream().wait_stream(side)
        self.rewind()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with capturing(self.graph):
            self.generate_step()
        self.graphs_captured += 1

    # ------------------------------------------------------------------------------------------------ the loop
    @torch.no_grad()
    def generate(self, max_len: int, stop_at_stop_token: bool, check_every: int, use_graph: bool):
        """The loop of ``ReformerTTS._infer_graphed`` over ``generate_step``: same guard, same stop bookkeeping, same shapes."""
        b, nm = self.b, self.nm
        if use_graph and self.graph is None:
            self.capture()
        cur, it = 1, 0
        every = max(1, int(check_every))
        while True:
            if stop_at_stop_token and it % every == 0 and bool(torch.all(self.stop > 0)):
                break
            it += 1
            if cur > self.cap:
                raise RuntimeError(f"IncrementalDecoder: capacity {self.cap} exhausted")
            if use_graph:
                self.graph.replay()
            else:
                self.generate_step()
            cur += 1
            if max(b, cur, nm) > max_len:
                break
        if stop_at_stop_token and bool(torch.all(self.stop > 0)):
            cur = min(cur, int(self.stop.max()))
        stop_out = torch.where(self.stop == 0, torch.full_like(self.stop, max_len), self.stop)
        return self.spec[:, 1:cur].transpose(1, 2).contiguous(), stop_out
