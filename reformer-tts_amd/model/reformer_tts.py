"""Top-level module (``/root/reference/reformer_tts/model/reformer_tts.py``)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import nn
import torch.nn.functional as F

from .modules import DecoderPreNet, EncoderPreNet, PostConvNet, ScaledPositionalEncoding
from .reformer import ReformerDec, ReformerEnc


class Encoder(nn.Module):
    def __init__(self, dict_size: int, embedding_dim: int, scp_encoding_dropout: float, reformer_kwargs: Dict, prenet_kwargs: Dict):
        super().__init__()
        self.prenet = EncoderPreNet(num_embeddings=dict_size + 1, embedding_dim=embedding_dim, **prenet_kwargs)
        self.positional_encoding = ScaledPositionalEncoding(embedding_dim, scp_encoding_dropout)
        self.reformer = ReformerEnc(embedding_dim, **reformer_kwargs)

    def forward(self, input_, input_mask=None, stack_hook=None):
        x = self.prenet(input_, pe=self.positional_encoding)
        if stack_hook is not None:                    # data-parallel trainer: cut between prenet and reversible stack
            x = stack_hook(x)
        return self.reformer(x, input_mask=input_mask)


class Decoder(nn.Module):
    def __init__(self, num_mel_coeffs: int, embedding_dim: int, scp_encoding_dropout: float, prenet_kwargs: Dict, reformer_kwargs: Dict):
        super().__init__()
        self.prenet = DecoderPreNet(input_size=num_mel_coeffs, output_size=embedding_dim, **prenet_kwargs)
        self.positional_encoding = ScaledPositionalEncoding(embedding_dim, scp_encoding_dropout)
        self.reformer = ReformerDec(embedding_dim, **reformer_kwargs)
        self.mel_linear = nn.Linear(embedding_dim, num_mel_coeffs)
        self.stop_linear = nn.Linear(embedding_dim, 1)

    use_fused = True

    def hidden(self, input_, keys, key_padding_mask=None, input_mask=None):
        d = self.prenet.output_size
        if (self.use_fused and self.training and input_.is_cuda and d % 128 == 0 and self.prenet.hidden_size % 128 == 0
                and (input_.shape[0] * input_.shape[1]) % 64 == 0):
            from ..edges import decoder_prenet_pe
            x = decoder_prenet_pe(self.prenet, self.positional_encoding, input_)
        else:
            x = self.positional_encoding(self.prenet(input_))
        return self.reformer(x, keys=keys, key_padding_mask=key_padding_mask, input_mask=input_mask)

    def forward(self, input_, keys, key_padding_mask=None, input_mask=None):
        x, attention_matrices = self.hidden(input_, keys, key_padding_mask=key_padding_mask, input_mask=input_mask)
        if not self.training and x.is_cuda and not torch.is_grad_enabled():
            from ..edges import linear_nograd            # inference: the heads on rtts_gemm_nt (fp32 epilogue), as in the training step
            return linear_nograd(x, self.mel_linear, out_f32=True), linear_nograd(x, self.stop_linear, out_f32=True), attention_matrices
        return self.mel_linear(x), self.stop_linear(x), attention_matrices


def _pad_len(n: int, base: int) -> int:
    return ((n - 1) // base + 1) * base


def pad_to_multiple(tensor, pad_base):
    """Right zero-pad (batch, seq_len, channels) to a multiple of ``pad_base`` on the tensor's own
    device (``reformer_tts.py:224-232`` relies on a process-wide default CUDA tensor type)."""
    new_len = ((tensor.shape[1] - 1) // pad_base + 1) * pad_base
    if new_len == tensor.shape[1]:
        return tensor          # already a multiple (every synthetic batch; most LJSpeech batches are not): no copy
    return F.pad(tensor, (0, 0, 0, new_len - tensor.shape[1]))


class ReformerTTS(nn.Module):
    def __init__(self, num_mel_coeffs: int, dict_size: int, pad_base: int, embedding_dim: int, scp_encoding_dropout: float,
                 enc_reformer_kwargs: Dict, enc_prenet_kwargs: Dict, dec_prenet_kwargs: Dict, dec_reformer_kwargs: Dict,
                 postnet_kwargs: Dict):
        super().__init__()
        self.num_mel_coeffs = num_mel_coeffs
        self.enc = Encoder(dict_size=dict_size, embedding_dim=embedding_dim, scp_encoding_dropout=scp_encoding_dropout,
                           reformer_kwargs=enc_reformer_kwargs, prenet_kwargs=enc_prenet_kwargs)
        self.dec = Decoder(num_mel_coeffs=num_mel_coeffs, embedding_dim=embedding_dim, scp_encoding_dropout=scp_encoding_dropout,
                           prenet_kwargs=dec_prenet_kwargs, reformer_kwargs=dec_reformer_kwargs)
        self.pad_base = pad_base
        self.postnet = PostConvNet(mel_size=num_mel_coeffs, num_hidden=embedding_dim, **postnet_kwargs)

    def _require_gpu(self):
        """The product path is the HIP path: refuse to run anywhere else instead of limping along on ATen CPU kernels."""
        dev = self.dec.mel_linear.weight.device
        if dev.type != "cuda":
            from .._lib import RttsError
            raise RttsError(f"ReformerTTS runs on the GPU only (model is on {dev}); there is no CPU fallback for the HIP path")

    def _encode_inputs(self, phonemes, spectrogram, spectrogram_mask):
        self._require_gpu()
        dev = spectrogram.device
        pad_phonemes = pad_to_multiple(phonemes.unsqueeze(-1), self.pad_base).squeeze(-1).to(dev)
        phoneme_mask = pad_phonemes != 0
        if spectrogram_mask is None:
            spectrogram_mask = torch.ones(spectrogram.shape[:2], device=dev)
        spectrogram_mask = pad_to_multiple(spectrogram_mask.unsqueeze(-1).to(dev), self.pad_base).squeeze(-1).to(torch.bool)
        return pad_phonemes, phoneme_mask, spectrogram_mask, pad_to_multiple(spectrogram, self.pad_base)

    def _encode_inputs_fused(self, phonemes, spectrogram, loss_mask):
        """``_encode_inputs`` for the training step, where the frame mask is ``loss_mask.mean(-1)`` (``wrappers.py:60``): one launch
        (``rtts_batch_masks``) writes the padded phonemes, both phoneme masks and the padded frame mask.  -> the tuple of
        ``_encode_inputs`` with the inverted phoneme mask attached to the phoneme mask as ``_rtts_not``."""
        from .. import _lib
        self._require_gpu()
        dev = spectrogram.device
        b, lp = phonemes.shape
        lm, n_mels = loss_mask.shape[1], loss_mask.shape[2]
        lpp, lmp = _pad_len(lp, self.pad_base), _pad_len(lm, self.pad_base)
        pad_ph = torch.empty(b, lpp, dtype=torch.long, device=dev)
        ph_mask = torch.empty(b, lpp, dtype=torch.bool, device=dev)
        ph_not = torch.empty(b, lpp, dtype=torch.bool, device=dev)
        sp_mask = torch.empty(b, lmp, dtype=torch.bool, device=dev)
        _lib.call("rtts_batch_masks", phonemes.data_ptr(), phonemes.stride(0), b, lp, lpp, loss_mask.data_ptr(), loss_mask.stride(0),
                  loss_mask.stride(1), lm, lmp, n_mels, pad_ph.data_ptr(), ph_mask.data_ptr(), ph_not.data_ptr(), sp_mask.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream)
        ph_mask._rtts_not = ph_not
        return pad_ph, ph_mask, sp_mask, pad_to_multiple(spectrogram, self.pad_base)

    def decoder_hidden(self, phonemes, spectrogram, spectrogram_mask=None, keys_hook=None, enc_stack_hook=None, enc_stream=None,
                       loss_mask=None):
        """Decoder output (B, T_padded, d) in front of the mel/stop heads: the training step feeds it to the
        fused heads + postnet + loss executor (``edges.PostnetLoss``).  ``keys_hook`` (encoder output -> tensor the
        decoder reads) lets the data-parallel trainer cut the autograd graph between encoder and decoder so that the
        two halves of the backward are separate launches with a gradient all-reduce in between."""
        fused_inputs = (loss_mask is not None and spectrogram_mask is None and phonemes.is_cuda and phonemes.dtype == torch.long
                        and phonemes.dim() == 2 and phonemes.stride(1) == 1 and loss_mask.dtype == torch.float32 and loss_mask.dim() == 3
                        and loss_mask.stride(2) == 1 and loss_mask.shape[1] == spectrogram.shape[1])
        if fused_inputs:
            pad_phonemes, phoneme_mask, spectrogram_mask, pad_spec = self._encode_inputs_fused(phonemes, spectrogram, loss_mask)
        else:
            if spectrogram_mask is None and loss_mask is not None:
                spectrogram_mask = loss_mask.mean(dim=-1)
            pad_phonemes, phoneme_mask, spectrogram_mask, pad_spec = self._encode_inputs(phonemes, spectrogram, spectrogram_mask)
        if enc_stream is not None:
            # the encoder (3,072 rows at the baseline shape: launch- and latency-bound kernels on three quarters of the chip) runs
            # on a stream of its own BESIDE the decoder prenet and the first decoder block, which do not read its output; the
            # decoder's first cross-attention waits for the event left on the keys (engine.FusedStackFn.forward)
            from ..engine import stamp
            main = torch.cuda.current_stream()
            stamp("fork (main stream)")
            enc_stream.wait_stream(main)
            for t_ in (pad_phonemes, phoneme_mask):
                t_.record_stream(enc_stream)
            with torch.cuda.stream(enc_stream):
                stamp("encoder branch: first kernel")
                keys = self.enc(pad_phonemes, input_mask=phoneme_mask, stack_hook=enc_stack_hook)
                stamp("encoder branch: forward done")
                ready = torch.cuda.Event()
                ready.record(enc_stream)
            stamp("decoder branch: first kernel after the fork")
            keys.record_stream(main)
            twin = getattr(keys, "_rtts_bf16", None)
            if twin is not None:
                twin[0].record_stream(main)               # the stack's bf16 copy of the keys: the cross-attention's k|v projection reads it
            keys._rtts_ready = ready
        else:
            keys = self.enc(pad_phonemes, input_mask=phoneme_mask, stack_hook=enc_stack_hook)
        if keys_hook is not None:
            keys = keys_hook(keys)
        kpm = getattr(phoneme_mask, "_rtts_not", None)
        if kpm is None:
            kpm = ~phoneme_mask
        kpm._rtts_not = phoneme_mask          # the stack executor wants the validity mask back: spares it the second inversion
        return self.dec.hidden(pad_spec, keys=keys, key_padding_mask=kpm, input_mask=spectrogram_mask)[0]

    def forward(self, phonemes: torch.LongTensor, spectrogram: torch.Tensor,
                spectrogram_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, list]:
        """``reformer_tts.py:103-143``: returns (mel, mel_postnet, stop, attention_matrices), all cropped
        to the input spectrogram length."""
        self._require_gpu()
        dev = spectrogram.device
        pad_phonemes = pad_to_multiple(phonemes.unsqueeze(-1), self.pad_base).squeeze(-1).to(dev)
        phoneme_mask = pad_phonemes != 0
        if spectrogram_mask is None:
            spectrogram_mask = torch.ones(spectrogram.shape[:2], device=dev)
        spectrogram_mask = pad_to_multiple(spectrogram_mask.unsqueeze(-1).to(dev), self.pad_base).squeeze(-1).to(torch.bool)
        pad_spec = pad_to_multiple(spectrogram, self.pad_base)
        keys = self.enc(pad_phonemes, input_mask=phoneme_mask)
        mel, stop, attention_matrices = self.dec(pad_spec, keys=keys, key_padding_mask=~phoneme_mask, input_mask=spectrogram_mask)
        mel_postnet = mel + self.postnet(mel)
        cutoff = spectrogram.shape[1]
        return mel[:, :cutoff], mel_postnet[:, :cutoff], stop[:, :cutoff], attention_matrices

    # ------------------------------------------------------------------ generation
    @torch.no_grad()
    def infer(self, phonemes: torch.LongTensor, combine_strategy: str = "concat", max_len: int = 1024,
              stop_threshold: float = 0.25, verbose: bool = False, stop_at_stop_token: bool = True,
              cache_encoder: bool = False, check_every: int = 8, use_graph: bool = False,
              incremental: bool = False) -> Tuple[torch.Tensor, torch.LongTensor]:
        """``reformer_tts.py:145-221``: autoregressive generation by repeated full forwards over the spectrogram
        generated so far.  Same arguments, same results -- (spectrogram (B, n_mels, L), stop_idx (B,)) -- including the
        loop guard ``max(spectrogram.shape) > max_len`` (the shape includes the mel axis: ``max_len < n_mels`` ends
        after one forward) and ``stop == max_len`` for samples that never stopped.

        MI355X-first differences, none of them visible in the result:
        * the spectrogram lives in ONE preallocated device buffer (no ``torch.cat`` of a growing tensor per frame);
        * the stop bookkeeping stays on the device; the host looks at it every ``check_every`` iterations only
          ("concat": frames generated after every sample has stopped cannot change earlier frames, so the result is cut
          back to where the reference's loop would have ended; "replace" rewrites every frame and checks every time);
        * ``cache_encoder=True`` runs the encoder once instead of once per frame.  That IS visible -- the reference
          re-draws the LSH rotations of the encoder in every forward -- hence off by default;
        * ``use_graph=True`` ("concat" only): one frame = one hipGraph replay (see ``_infer_graphed``);
        * ``incremental=True`` ("concat" only, an all-dense decoder -- ``use_full_attn`` -- only): one frame = ONE decoder row
          per utterance against a per-layer cache instead of a forward over the whole window (``model/incremental.py``).  It
          implies the cached encoder, and it IS visible: the postnet sees the sequence end at the newest frame, where the
          windowed paths run it over the padded window, so the frames differ from theirs.  ``use_graph=True`` replays one
          captured step for every frame of every length; ``use_graph=False`` runs the same step eagerly."""
        assert combine_strategy in {"concat", "replace"}
        assert -1. < stop_threshold < 1.
        if incremental and combine_strategy != "concat":
            raise ValueError("infer(incremental=True) generates frame by frame: combine_strategy must be 'concat'")
        if self.dec.mel_linear.weight.is_cuda:
            from ..edges import refresh_eval_operands
            refresh_eval_operands(self)               # cached padded / re-laid-out weights follow the parameters (graphs hold addresses)
        if incremental:
            return self._infer_incremental(phonemes, max_len, stop_threshold, stop_at_stop_token, check_every, use_graph)
        if use_graph and combine_strategy == "concat":
            return self._infer_graphed(phonemes, max_len, stop_threshold, stop_at_stop_token, cache_encoder, check_every)
        was_training = self.training
        self.eval()
        stacks = (self.enc.reformer.layers, self.dec.reformer.layers)
        was_fused = [st_.fused_in_eval for st_ in stacks]
        for st_ in stacks:
            st_.fused_in_eval = True         # the stacks' forward through the explicit executor: with the no-grad edges
            #                                  (edges.py) a generation step runs no library GEMM at all
        was_collect = self.dec.reformer.collect_attention
        self.dec.reformer.collect_attention = False          # the alignments of a frame are discarded: no launch for them
        try:
            dev = self.dec.mel_linear.weight.device
            phonemes = phonemes.to(dev)
            b, nm = phonemes.shape[0], self.num_mel_coeffs
            cap = max(max_len, nm, b) + 2                       # the guard below cannot let the buffer grow past this
            buf = torch.zeros(b, cap + 1, nm, device=dev)       # frame 0 = the zero start frame
            cur = 1                                             # frames in the buffer, start frame included
            stop = torch.zeros(b, dtype=torch.long, device=dev)
            keys_cache = None
            if cache_encoder:
                pad_ph = pad_to_multiple(phonemes.unsqueeze(-1), self.pad_base).squeeze(-1)
                ph_mask = pad_ph != 0
                keys_cache = (self.enc(pad_ph, input_mask=ph_mask), ph_mask)
            every = 1 if combine_strategy == "replace" else max(1, int(check_every))
            it = 0
            while True:
                if stop_at_stop_token and it % every == 0 and bool(torch.all(stop > 0)):
                    break
                it += 1
                iteration = cur
                still_running = stop == 0
                if verbose and iteration % 10 == 0:
                    print(f"reached {iteration=}, number_of_running_samples={int(still_running.sum())}...")
                spec = buf[:, :cur]
                if keys_cache is None:
                    _, generated, stop_pred, _ = self.forward(phonemes, spec)
                else:
                    keys, ph_mask = keys_cache
                    pad_spec = pad_to_multiple(spec, self.pad_base)
                    sp_mask = pad_to_multiple(torch.ones(b, cur, 1, device=dev), self.pad_base).squeeze(-1).to(torch.bool)
                    mel, stop_pred, _ = self.dec(pad_spec, keys=keys, key_padding_mask=~ph_mask, input_mask=sp_mask)
                    generated, stop_pred = (mel + self.postnet(mel))[:, :cur], stop_pred[:, :cur]
                stop_pred = stop_pred.reshape(b, -1)
                if combine_strategy == "concat":
                    buf[:, cur] = generated[:, -1, :]
                    cur += 1
                    if stop_at_stop_token:
                        stops_now = torch.sigmoid(stop_pred[:, -1]) > stop_threshold
                        stop = torch.where(still_running & stops_now, stops_now.long() * iteration + 1, stop)
                else:
                    buf[:, 1:1 + generated.shape[1]] = generated
                    cur = 1 + generated.shape[1]
                    if stop_at_stop_token:
                        stops_now = torch.any(torch.sigmoid(stop_pred) > stop_threshold, dim=1)
                        stop = torch.where(stops_now & still_running, torch.argmax(stop_pred, dim=1) + 1, stop)
                if max(b, cur, nm) > max_len:
                    if verbose:
                        print(f"stopped at {max_len=}")
                    break
            if combine_strategy == "concat" and stop_at_stop_token and bool(torch.all(stop > 0)):
                cur = min(cur, int(stop.max()))                 # where the reference's per-iteration check ends the loop
            stop = torch.where(stop == 0, torch.full_like(stop, max_len), stop)
            return buf[:, 1:cur].transpose(1, 2).contiguous(), stop
        finally:
            for st_, f in zip(stacks, was_fused):
                st_.fused_in_eval = f
            self.dec.reformer.collect_attention = was_collect
            self.train(was_training)

    @torch.no_grad()
    def _infer_incremental(self, phonemes, max_len, stop_threshold, stop_at_stop_token, check_every, use_graph):
        """"concat" generation one decoder row at a time (``model/incremental.py``).  State and graph are kept per (batch, padded
        text length, capacity, options) and reused by later calls, as ``_infer_graphed`` keeps its windows' graphs."""
        from .incremental import IncrementalDecoder, check_supported, generation_plan
        b = phonemes.shape[0]
        _, capacity = generation_plan(b, self.num_mel_coeffs, max_len)
        tk = _pad_len(phonemes.shape[1], self.pad_base)
        check_supported(self, b, capacity, tk)
        self._require_gpu()
        dev = self.dec.mel_linear.weight.device
        was_training = self.training
        self.eval()
        try:
            params = tuple(p_.data_ptr() for p_ in self.parameters())
            key = (b, tk, capacity, bool(stop_at_stop_token), float(stop_threshold), str(dev))
            cache = self.__dict__.setdefault("_inc_cache", {})
            gen = cache.get(key)
            if gen is None or gen.params != params:              # new shape, or the weights moved (other device / storage)
                cache.clear()                                    # one generator state at a time (each pins HBM for its caches)
                gen = cache[key] = IncrementalDecoder(self, phonemes, capacity, stop_threshold, stop_at_stop_token)
            else:
                gen.begin(phonemes)
            return gen.generate(max_len, stop_at_stop_token, check_every, use_graph)
        finally:
            self.train(was_training)

    @torch.no_grad()
    def _infer_graphed(self, phonemes, max_len, stop_threshold, stop_at_stop_token, cache_encoder, check_every):
        """"concat" generation with ONE hipGraph replay per frame.  The padded input window, its validity mask, the index
        of the newest frame and the stop bookkeeping are device buffers; the graph runs the decoder (and the encoder
        unless cached) over the window through the explicit executor, picks the output at the newest position with a
        device index, appends it to the window and advances the index -- the host only replays, looks at the stop flags
        every ``check_every`` frames and moves to the next window's graph when the padded length grows by ``pad_base``.
        Buffers and graphs are kept per (batch, padded text length, capacity, options) and reused by later calls, so
        only the first utterance of a shape pays for the captures.  Same results as the eager loop up to the LSH
        rotations, which are redrawn per forward in both."""
        from .._graphs import capturing
        from .lsh_attention import LSHSelfAttention
        was_training = self.training
        self.eval()
        for m in self.modules():
            if isinstance(m, LSHSelfAttention):
                m.use_default_generator = True                       # the per-layer generators are not capturable
        stacks = (self.enc.reformer.layers, self.dec.reformer.layers)
        for st_ in stacks:
            st_.fused_in_eval = True                                 # executor forward: ~half the launches per frame
        was_collect = self.dec.reformer.collect_attention
        self.dec.reformer.collect_attention = False                  # nothing of the alignments is captured into the graphs
        try:
            dev = self.dec.mel_linear.weight.device
            phonemes = phonemes.to(dev)
            b, nm = phonemes.shape[0], self.num_mel_coeffs
            pad_ph_new = pad_to_multiple(phonemes.unsqueeze(-1), self.pad_base).squeeze(-1)
            cap = max(max_len, nm, b) + 2
            total = _pad_len(cap + 1, self.pad_base)
            thr = float(stop_threshold)
            params = tuple(p_.data_ptr() for p_ in self.parameters())   # the graphs read the weights in place: new VALUES are fine
            key = (b, pad_ph_new.shape[1], total, bool(cache_encoder), bool(stop_at_stop_token), thr, str(dev))
            cache = self.__dict__.setdefault("_gen_cache", {})
            g = cache.get(key)
            if g is None or g["params"] != params:                   # new shape, or the weights moved (other device / storage)
                g = dict(params=params, graphs={}, pad_ph=torch.zeros_like(pad_ph_new),
                         spec=torch.zeros(b, total, nm, device=dev),                       # frame 0 = the zero start frame
                         mask=torch.zeros(b, total, dtype=torch.bool, device=dev),
                         pos=torch.zeros(1, dtype=torch.long, device=dev),                 # index of the newest frame = cur - 1
                         stop=torch.zeros(b, dtype=torch.long, device=dev),
                         keys=None)
                cache.clear()                                        # one generator state at a time (each pins HBM for its graphs)
                cache[key] = g
            spec, mask, pos, stop, pad_ph = g["spec"], g["mask"], g["pos"], g["stop"], g["pad_ph"]
            pad_ph.copy_(pad_ph_new)
            ph_mask = g.setdefault("ph_mask", torch.zeros_like(pad_ph, dtype=torch.bool))
            ph_mask.copy_(pad_ph != 0)
            spec.zero_()
            mask.zero_()
            mask[:, 0] = True
            pos.zero_()
            stop.zero_()
            if cache_encoder:
                keys_new = self.enc(pad_ph, input_mask=ph_mask)
                if g["keys"] is None:
                    g["keys"] = torch.empty_like(keys_new)
                g["keys"].copy_(keys_new)
            keys_c = g["keys"] if cache_encoder else None
            nph_mask = g.setdefault("nph_mask", torch.zeros_like(ph_mask))
            nph_mask.copy_(~ph_mask)

            def step(t_pad):
                keys = keys_c if keys_c is not None else self.enc(pad_ph, input_mask=ph_mask)
                mel, stop_pred, _ = self.dec(spec[:, :t_pad], keys=keys, key_padding_mask=nph_mask, input_mask=mask[:, :t_pad])
                gen = (mel + self.postnet(mel)).index_select(1, pos)                    # (B, 1, n_mels) at the newest position
                if stop_at_stop_token:
                    stops_now = torch.sigmoid(stop_pred.reshape(b, -1).index_select(1, pos).reshape(b)) > thr
                    stop.copy_(torch.where((stop == 0) & stops_now, stops_now.long() * (pos + 1) + 1, stop))
                pos.add_(1)
                spec.index_copy_(1, pos, gen)
                mask.index_fill_(1, pos, True)

            graphs = g["graphs"]
            cur, it = 1, 0
            every = max(1, int(check_every))
            while True:
                if stop_at_stop_token and it % every == 0 and bool(torch.all(stop > 0)):
                    break
                it += 1
                t_pad = _pad_len(cur, self.pad_base)
                if t_pad not in graphs:
                    # warm-up on a side stream (lazy tables, allocator), with the bookkeeping restored afterwards
                    saved = (spec.clone(), mask.clone(), pos.clone(), stop.clone())
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        step(t_pad)
                    torch.cuda.current_stream().wait_stream(side)
                    for dst, src in zip((spec, mask, pos, stop), saved):
                        dst.copy_(src)
                    torch.cuda.synchronize()
                    graphs[t_pad] = torch.cuda.CUDAGraph()
                    with capturing(graphs[t_pad]):
                        step(t_pad)
                graphs[t_pad].replay()
                cur += 1
                if max(b, cur, nm) > max_len:
                    break
            if stop_at_stop_token and bool(torch.all(stop > 0)):
                cur = min(cur, int(stop.max()))
            stop_out = torch.where(stop == 0, torch.full_like(stop, max_len), stop)
            return spec[:, 1:cur].transpose(1, 2).contiguous(), stop_out
        finally:
            for st_ in stacks:
                st_.fused_in_eval = False
            self.dec.reformer.collect_attention = was_collect
            self.train(was_training)
