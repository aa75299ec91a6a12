/*
 * rtts.h -- C ABI of librtts_hip.so, the MI355X (gfx950) implementation of the
 * Reformer-TTS training hot path.
 *
 * The reference (kowaalczyk/reformer-tts) is pure Python: it has no FFI of its
 * own.  The seam this library plugs into is the `implementation` switch of
 * LSHSelfAttentionWrapper (reference reformer_tts/model/reformer.py:189-220)
 * and the reversible-block protocol (reformer_tts/model/reversible.py:46-98,
 * 134-203); each entry point below names the reference lines whose arithmetic
 * it replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - the library never allocates, frees or synchronises: outputs and
 *     workspaces are caller-owned, launches go to the `stream` argument
 *     (a hipStream_t passed as void*), so calls are graph-capturable;
 *   - DEVICE of a call: the stream's.  A forward is called from the Python main
 *     thread, a backward from PyTorch's autograd worker thread for the device
 *     (nested inside the reversible function's backward), and HIP's current
 *     device is per thread -- so every launching entry point first binds the
 *     calling thread to the device its `stream` belongs to (hipStreamGetDevice +
 *     hipSetDevice when it differs): the explicit device ordinal SURVEY.md 8(b)
 *     asks for travels inside the stream handle and cannot disagree with it.
 *     A NULL stream (the legacy default stream) means the thread's current
 *     device.  Every pointer of a call must belong to that device; return -3 =
 *     the stream handle is not a stream of this process;
 *   - `bf16` buffers hold IEEE bfloat16 (uint16_t storage);
 *   - activations of width d = H*dh are row-major with an explicit row stride
 *     `ld` in ELEMENTS (so qk and v may be the two halves of one (B*T, 2d) GEMM
 *     output); head h of token (b,t) starts at element (b*T+t)*ld + h*dh;
 *   - return value 0 = launched, <0 = rejected before any launch
 *     (rtts_last_error() gives the reason, thread-local);
 *   - shapes supported by this build: dh == 64, bucket_size in {64,128},
 *     T % (2*bucket_size) == 0, T <= 8192, n_hashes <= 16.
 */
#ifndef RTTS_H
#define RTTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTTS_VERSION 1

int rtts_version(void);
const char* rtts_last_error(void);

/* ---- LSH attention: integer stages -------------------------------------------------
 * Replaces hash_vectors + sort of reformer_pytorch.LSHAttention as called from
 * reformer_tts/model/reformer.py:217.
 *   qk        bf16 (B,T,H*dh) with row stride ld_qk
 *   rotations f32  (rot_rows, dh, n_hashes, n_buckets/2), rot_rows = 1 (shared) or B*H
 *   buckets   i32  (B*H, n_hashes, T)  optional (NULL to skip): bucket id incl. round offset
 *   st        i32  (B*H, n_hashes, T)  sorted slot -> token position ("sticker % T")
 *   undo      i32  (B*H, n_hashes, T)  optional: token -> sorted slot within its round
 * Projection is a k-ordered fp32 fmaf chain (bit-reproducible, see oracle/lsh_int.c). */
int rtts_lsh_hash_sort(const void* qk, int64_t ld_qk, const float* rotations, int rot_rows,
                       int B, int H, int T, int dh, int n_hashes, int bucket_size,
                       int32_t* buckets, int32_t* st, int32_t* undo, void* stream);
/* how the call is worked: 2 = lsh_hash_rounds_kernel (the projections of ALL rounds through the f32 MFMA, every row staged
 * once; bucket ids pass through `st`) + lsh_sort_ids_kernel, from T = 1024 on; 1 = lsh_hash_sort_kernel (one launch, a
 * workgroup per (head, round)) for short sequences.  Same results bit for bit. */
int rtts_lsh_hash_sort_launches(int T);

/* The same stages of HuggingFace's LSHSelfAttention (implementation="huggingface_transformers"): replaces
 * `buckets = self._hash_vectors(...)` and `self._get_sorted_bucket_idx_and_undo_sorted_bucket_idx(...)` of transformers'
 * models/reformer/modeling_reformer.py (LSHSelfAttention.forward), the layer built at reformer_tts/model/reformer.py:202-213
 * and called at :219.
 *   rotations f32 (H, dh, n_hashes, n_buckets/2): per head, shared over the batch (row = bh % H)
 *   mask      u8 (B,T) 1 = valid, or NULL.  With a mask, masked tokens take the extra bucket n_buckets and round r is
 *             offset by r * (n_buckets + 1) (the stride does not change the sorted order, so it is used whenever a mask is
 *             given, whether it hides a token or not); without one the offset is r * n_buckets
 *   n_buckets even, 2 .. 256, independent of T / chunk; T % chunk == 0, T % 128 == 0, dh == 64
 *   buckets / st / undo as above.  Same k-ordered fp32 fmaf chain: tests/hf_lsh_ref.py reproduces the buckets bit for bit. */
int rtts_lsh_hash_sort_hf(const void* qk, int64_t ld_qk, const float* rotations, const uint8_t* mask,
                          int B, int H, int T, int dh, int n_hashes, int chunk, int n_buckets,
                          int32_t* buckets, int32_t* st, int32_t* undo, void* stream);

/* ---- LSH attention: chunked attention forward (Appendix B steps 4-10) ----------------
 *   qk, v  bf16 rows as above (common stride ld)
 *   mask   u8 (B,T) 1 = valid token, or NULL
 *   o      bf16 (B*H, n_hashes, T, dh)  per-round output, already at UNSORTED positions
 *   lse    f32  (B*H, n_hashes, T)      per-round logsumexp of the masked logits */
int rtts_lsh_attn_fwd(const void* qk, const void* v, int64_t ld, const int32_t* st, const uint8_t* mask,
                      int B, int H, int T, int dh, int n_hashes, int bucket_size, int causal,
                      void* o, float* lse, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream);
/* drop_p > 0: dropout on the attention probabilities (the layer's `dropout` knob, reference reformer_tts/model/config.py:27):
 * the chunk's softmax output is multiplied by keep = 0 | 1/(1-p) before it meets the values; lse is that of the undropped
 * probabilities.  keep is a counter hash of (drop_seed + *seed_dev, pair), pair = ((head * chunks + chunk) * bucket_size +
 * query row of the chunk) * 2*bucket_size + key row (own chunk's keys first): no mask is stored, rtts_lsh_attn_bwd called with
 * the same (drop_p, drop_seed, seed_dev) -- and the reversible recompute's forward -- redraw the same one.  seed_dev may be NULL. */
/* how rtts_lsh_attn_fwd works a shape: 0 = one workgroup per chunk (lsh_attn_fwd_kernel; small grids), R > 0 = workgroups
 * that walk runs of R consecutive chunks of a (batch, head) ring (lsh_attn_fwd_walk_kernel: every K / V row gathered once,
 * the next chunk's rows fetched while the current one is merged and stored; same results bit for bit).  -1: bad arguments.
 * rtts_debug_set_walk() below forces a run length for tests and A/B runs; the launch path reads no environment. */
int rtts_lsh_attn_fwd_run_length(int B, int H, int T, int n_hashes, int bucket_size);
/* TEST-ONLY, process-wide (two atomic words): run length of the walking forward / backward kernels.  -1 = the library's own
 * pick (the default: what every product call gets), 0 = the one-chunk kernel, n >= 1 = runs of n where n divides the ring
 * (else the one-chunk kernel).  Replaces the RTTS_LSH_{FWD,BWD}_WALK environment variables the launch path used to read on
 * every call; the Python binding reads those variables ONCE, when it loads the library, and calls this. */
int rtts_debug_set_walk(int fwd_run, int bwd_run);

/* ---- combine the hash rounds (step 11) and merge heads (first half of step 12) -------
 *   out     bf16 (B,T,H*dh) row stride ld_out
 *   lse_tot f32  (B*H, T)  logsumexp over rounds (kept for the backward) */
int rtts_lsh_combine_fwd(const void* o, const float* lse, int B, int H, int T, int dh, int n_hashes,
                         void* out, int64_t ld_out, float* lse_tot, void* stream);

/* ---- backward of steps 4-11 ------------------------------------------------------------
 * The rounds form ONE softmax over the multiset of (round, key) pairs, so the
 * backward needs only lse_tot and delta = rowsum(out * dout) per (token, head):
 *   rtts_lsh_bwd_delta : delta f32 (B*H,T) from out, dout (bf16, strides ld_out, ld_dout)
 *   rtts_lsh_attn_bwd  : per chunk, writes bf16 partial gradients at unsorted positions
 *        dqk_part : (rtts_lsh_bwd_qk_slots() = 2, B*H, n_hashes, T, dh)  slot 0 = the token as a row of its own
 *                   chunk (query role + key role, added on chip), slot 1 = key role as the looked-back chunk
 *        dv_part  : (2, B*H, n_hashes, T, dh)  slot 0 = own chunk, slot 1 = looked-back chunk
 *        every (slot, head, round, token) row is written exactly once: no zero-fill needed
 *        row_flags : u8 (B*H, n_hashes, T), required where rtts_lsh_attn_bwd_run_length() > 0 (else it may be NULL and is
 *                   not written): the walking kernel carries a chunk's dK/dV accumulators through the two steps that work
 *                   its keys and writes each key row ONCE into slot 0; only the ends of a run leave a slot-1 partner, and
 *                   row_flags[row] = 1 marks the slot-0 rows that have one (slot-1 rows without a flag are never written)
 *   rtts_lsh_bwd_reduce: dqk, dv bf16 (B,T,H*dh) stride ld_d = sum over slots and rounds; row_flags as written by the
 *        backward, or NULL = every row has both slots */
int rtts_lsh_bwd_qk_slots(void);
/* how rtts_lsh_attn_bwd works a shape: 0 = one workgroup per chunk (lsh_attn_bwd_kernel), R > 0 = workgroups that walk R
 * consecutive chunks of a ring with the next chunk's rows prefetched (lsh_attn_bwd_walk_kernel); same results bit for bit */
int rtts_lsh_attn_bwd_run_length(int B, int H, int T, int n_hashes, int bucket_size);
int rtts_lsh_bwd_delta(const void* out, int64_t ld_out, const void* dout, int64_t ld_dout,
                       int B, int H, int T, int dh, float* delta, void* stream);
int rtts_lsh_attn_bwd(const void* qk, const void* v, int64_t ld, const int32_t* st, const uint8_t* mask,
                      const void* dout, int64_t ld_dout, const float* lse_tot, const float* delta,
                      int B, int H, int T, int dh, int n_hashes, int bucket_size, int causal,
                      void* dqk_part, void* dv_part, uint8_t* row_flags, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev,
                      void* stream);
int rtts_lsh_bwd_reduce(const void* dqk_part, const void* dv_part, int B, int H, int T, int dh, int n_hashes,
                        void* dqk, void* dv, int64_t ld_d, const uint8_t* row_flags, void* stream);

/* ---- optimizer step over the flat parameter buffer --------------------------------------
 * Replaces clip_grad_norm_ (pytorch-lightning gradient_clip_val, reference
 * reformer_tts/training/train.py:77-89) and transformers.optimization.AdamW.step as configured
 * at reformer_tts/training/wrappers.py:240-256,284-297 (beta 0.9/0.999, eps 1e-6, bias-corrected,
 * decoupled decay applied after the update to parameters whose decay_mask byte is 1).
 *   rtts_grad_clip_scale: scale_out[0] = grad_mult * min(1, max_norm / (grad_mult*|g| + 1e-6)),
 *        scale_out[1] = grad_mult*|g|;  partial_ws: >= 2048 floats.  grad_mult = 1/world_size
 *        after a sum all-reduce.  max_norm <= 0 disables clipping.
 *   rtts_adamw_step: grads are multiplied by scale[0] on the fly (scale may be NULL = 1);
 *        hyper (device) = {lr, lr*sqrt(1-beta2^t)/(1-beta1^t)} for the current step t, read by the kernel so that
 *        a captured hipGraph replays with the values the host wrote before the replay.  n % 4 == 0 (pad the flat
 *        buffers); bf16_mirror (may be NULL): the updated parameters rounded to bf16, written in the same pass. */
int rtts_grad_clip_scale(const float* grads, int64_t n, float grad_mult, float max_norm, float* partial_ws,
                         float* scale_out, void* stream);
int rtts_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                    int64_t n, const float* scale, const float* hyper, float beta1, float beta2, float eps,
                    float weight_decay, void* bf16_mirror, void* stream);

/* ---- row-wise fused kernels around the GEMMs of a reversible block --------------------------
 * Replace the ATen chains of WithNorm / FeedForward / residual adds (reference
 * reformer_tts/model/reformer.py:25-45, modules.py:195-207, reversible.py:56-98) and their
 * autograd backward.  Rows are contiguous (stride d); d in {128,256,384,512,768,1024,2048}.
 * Column sums (bias / LayerNorm-affine gradients) are ACCUMULATED into their outputs through
 * `partial_ws` (>= 2*256*d floats), deterministically.
 *   rtts_ln_fwd            xn(bf16) = LayerNorm(x; eps 1e-5) * gamma + beta; keeps mean, rstd (M)
 *   rtts_ln_bwd            dx_io += dLN(dxn); dgamma += ..., dbeta += ...
 *   rtts_cast_colsum       dyb(bf16) = dy(fp32); dbias += colsum(dy)   (dbias may be NULL); drop_p > 0: dy is first
 *                          multiplied by the keep-scale of the dropout that sat on the block's output
 *   rtts_colsum_bf16       dbias += colsum(dh); relu_gate: dh *= (h > 0) * gate_scale in place first (gate_scale = 1/(1-p)
 *                          when h went through dropout_p after the ReLU)
 *   rtts_residual_epilogue y = x + sign * dropout_p(g(bf16) + bias)    (bias may be NULL; drop_p = post_attn_dropout of
 *                          the LSH layer, reformer.py:198-200 knob list; mask = hash(seed + *seed_dev, element), the same
 *                          in the forward, the reconstruction and the backward)
 *   rtts_bias_act          h(bf16) = [relu](h + bias) in place
 *   rtts_cast_f32_bf16     flat cast (n % 4 == 0): the per-step bf16 mirror of all parameters */
int rtts_ln_fwd(const float* x, const float* gamma, const float* beta, void* xn, float* mean, float* rstd,
                int M, int d, void* stream);
int rtts_ln_bwd(const void* dxn, const float* x, const float* mean, const float* rstd, const float* gamma,
                float* dx_io, float* dgamma, float* dbeta, float* partial_ws, int M, int d,
                void* dyb_next, float* partial_next, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);
/* out-of-place form: dx_out = dx_in + dLN(dxn) (dx_in == dx_out is rtts_ln_bwd).  The stack executor uses it for the first update
 * of each of the two gradient streams of a reversible stack's backward (reference: reversible.py:114-129,155-158 start from two
 * chunks of one dy), which start as the caller's dout itself instead of a copy of it. */
int rtts_ln_bwd_to(const void* dxn, const float* x, const float* mean, const float* rstd, const float* gamma, const float* dx_in,
                   float* dx_out, float* dgamma, float* dbeta, float* partial_ws, int M, int d,
                   void* dyb_next, float* partial_next, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);
/* the joining form: dx_out = dx_in + addend + dLN(dxn) (addend NULL: rtts_ln_bwd_to; must not alias dx_out).  The stack executor's LAST
 * LayerNorm backward: both streams of a reversible stack start as its input (reference reformer.py:85-93, x = cat([x, x])), so
 * d(input) = g1 + g2 -- the other stream joins in the pass that completes this one. */
int rtts_ln_bwd_join(const void* dxn, const float* x, const float* mean, const float* rstd, const float* gamma, const float* dx_in,
                     const float* addend, float* dx_out, float* dgamma, float* dbeta, float* partial_ws, int M, int d,
                     void* dyb_next, float* partial_next, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);
/* dyb_next (may be NULL): bf16 copy of the completed dx_io, times the keep-scale of (drop_p, seed) -- the next block's
 * rtts_cast_colsum folded in; partial_next then receives that copy's partial column sums (same layout as partial_ws). */
int rtts_cast_colsum(const float* dy, void* dyb, float* dbias, float* partial_ws, int M, int d, float drop_p, uint32_t seed,
                     const uint32_t* seed_dev, const float* scale_dev, void* stream);
/* scale_dev (may be NULL): one device float multiplied into dy first -- the upstream gradient of a scalar loss, so that the
 * root of a backward needs no separate scaling pass.  gated_out (may be NULL = in place): where the gated dh goes. */
int rtts_colsum_bf16(void* dh, const void* h, int64_t ld, float* dbias, float* partial_ws, int M, int d,
                     int relu_gate, float gate_scale, void* gated_out, void* stream);
/* Deferred finalisation of the column sums: rtts_ln_bwd (dgamma = dbeta = NULL), rtts_cast_colsum / rtts_colsum_bf16
 * (dbias = NULL) then only write their partial rows -- rtts_colsum_partial_rows(M) rows of d floats; rtts_ln_bwd writes two
 * such blocks, the second 256*d floats after the first -- and ONE grouped launch adds the sums of up to
 * RTTS_COLSUM_MAX_GROUP partial buffers into their outputs (same fixed summation order: deterministic).  The outputs of one
 * call must not overlap (refused: two jobs adding into one element would race). */
#define RTTS_COLSUM_MAX_GROUP 48
typedef struct {
    const float* partial;   /* (nrows, n) fp32, row stride ld */
    float* out;             /* (n): += column sums */
    int32_t nrows, n;
    int32_t ld, reserved;   /* ld = 0: n (a block of columns of a wider partial buffer: ld = its width) */
} rtts_colsum_job;
int rtts_colsum_partial_rows(int M);
int rtts_colsum_final_grouped(const rtts_colsum_job* jobs, int n, void* stream);
int rtts_residual_epilogue(const float* x, const void* g, const float* bias, float sign, float* y,
                           int64_t M, int d, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);
/* The same epilogue fused with the NEXT block's LayerNorm: y = x + sign*(g + bias) (y = NULL: in place), then
 * xn(bf16) = LayerNorm(y)*gamma + beta with mean/rstd per row (reformer.py:25-33 applied to the stream a
 * reversible block has just updated or reconstructed, reversible.py:56-98). */
int rtts_residual_ln(float* x, const void* g, const float* bias, float sign, const float* gamma, const float* beta,
                     void* xn, float* mean, float* rstd, int M, int d, float drop_p, uint32_t seed, const uint32_t* seed_dev,
                     float* y, void* stream);
/* out = a + b (the two streams of a reversible stack); out (fp32) and / or out_bf16 may be NULL; n % 4 == 0 */
int rtts_sum_streams(const float* a, const float* b, int64_t n, float* out, void* out_bf16, void* stream);
int rtts_bias_act(void* h, const float* bias, int64_t M, int d, int relu, void* stream);
int rtts_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);

/* ---- dense encoder-decoder attention (T_k a multiple of 128, 128 or 256 keys on chip at a time) ----
 * Replaces the attention core of nn.MultiheadAttention inside MultiheadAttentionWrapper
 * (reference reformer_tts/model/reformer.py:161-186); projections stay GEMMs outside.
 *   q   bf16 (B,Tq,H*dh) stride ld_q;  kv bf16 (B,Tk,2*H*dh) = [k | v] stride ld_kv
 *   kvalid u8 (B,Tk) 1 = attend (i.e. NOT key_padding_mask), or NULL
 *   o   bf16 (B,Tq,H*dh) stride ld_o;  lse f32 (B*H,Tq)
 *   backward: delta f32 (B*H,Tq) = rowsum(o*do) (rtts_lsh_bwd_delta), dq bf16 like q,
 *   dkv_part bf16 (Tq/128, B, Tk, 2*H*dh) partial slabs -> rtts_sum_slabs -> dkv (B,Tk,2*H*dh)
 *   T_k > 256 (or 384, 640, ...): the forward walks the keys in rtts_xattn_key_chunks(T_k) chunks with a running maximum and
 *   normaliser; the backward gives every chunk its own workgroups (P = exp(s - lse) needs only the forward's lse), which
 *   write their shares of dQ to dq_chunks (chunks, B*Tq, H*dh) bf16 -- summed into dq (ld_dq == H*dh) by the same call;
 *   one chunk: dq_chunks may be NULL
 *   dh = 64 or 128 (nn.MultiheadAttention num_heads 8 or 4 at embedding_dim 512; the reference's
 *   config/legacy/attention-depth-3-heads-4.yml and attention-depth-3-heads-3.yml set num_heads 4); the score scale is
 *   1 / sqrt(dh).  At dh = 128 the backward holds 128 keys at a time, so the number of chunks its dq_chunks needs is
 *   rtts_xattn_bwd_key_chunks(T_k, dh) = T_k / 128 (dh = 64: rtts_xattn_key_chunks(T_k)); -1 outside the envelope (T_k a
 *   multiple of 128 up to 2048, dh 64 or 128).  rtts_lsh_bwd_delta takes dh = 128 for this delta.
 *   A sample WITHOUT ANY valid key (kvalid all 0): its normaliser is 0, so rtts_xattn_fwd writes o = NaN (0 * inf) and
 *   lse = -inf for its rows, as nn.MultiheadAttention does; rtts_lsh_bwd_delta then gives delta = NaN and rtts_xattn_bwd
 *   dq = NaN and dk = NaN (dS = P * (dP - delta) with P = 0, delta = NaN), while dv is exactly 0 (P is taken as 0 where
 *   kvalid is 0; nn.MultiheadAttention's dv is NaN there).  This is NaN in data, never a fault, and the other samples of the
 *   batch are bit-identical to a call in which that sample has valid keys (tests/test_xattn_hip.py).  A padded key of a
 *   sample that has valid keys gets dk = dv = 0 exactly. */
int rtts_xattn_key_chunks(int Tk);
int rtts_xattn_bwd_key_chunks(int Tk, int dh);
int rtts_xattn_fwd(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid,
                   int B, int H, int Tq, int Tk, int dh, void* o, int64_t ld_o, float* lse,
                   float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);
int rtts_xattn_bwd(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid,
                   const void* dout, int64_t ld_dout, const float* lse, const float* delta,
                   int B, int H, int Tq, int Tk, int dh, void* dq, int64_t ld_dq, void* dkv_part,
                   float drop_p, uint32_t seed, const uint32_t* seed_dev, void* dq_chunks, void* stream);
/* drop_p = nn.MultiheadAttention's dropout on the normalised attention probabilities (config #4: 0.15); the keep
 * decision of (head, query, key) is hash(seed + *seed_dev, index), identical in the forward and the backward. */
int rtts_sum_slabs(const void* part, int nslabs, int64_t n, void* out, void* stream);
/* Head-averaged attention probabilities of the same call (eval mode): a[b, i, j] = (1/H) sum_h exp(s_h(i, j) - lse_h(i)),
 * s_h = q_h . k_h / sqrt(dh), exactly 0 where kvalid == 0; a f32 (B,Tq,Tk) row stride ld_a (>= Tk, % 4 == 0, 16-byte
 * aligned).  lse = what rtts_xattn_fwd wrote for the same q / kv / kvalid, so every head's row sums to 1 as in its o.
 * The weights nn.MultiheadAttention returns and MultiheadAttentionWrapper appends to the decoder's attention_matrices_
 * in eval mode (reference reformer_tts/model/reformer.py:161-186, returned by ReformerDec.forward :139-158 and
 * ReformerTTS.forward reformer_tts.py:103-143).  Envelope of rtts_xattn_fwd. */
int rtts_xattn_probs_mean(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid,
                          const float* lse, int B, int H, int Tq, int Tk, int dh, float* a, int64_t ld_a, void* stream);
/* Guided attention loss as a term of the TRAINING loss (Tachibana et al.; DC-TTS, ESPnet).  Not in the reference: it adds to
 * the cross-attention of reference reformer_tts/model/reformer.py:161-186, which only collects the matrices in eval mode.
 *   P = the probabilities of rtts_xattn_fwd before their dropout;  W[b,t,k] = 1 - exp(-(k / K_b - t / T_b)^2 / (2 sigma^2)) for
 *   t < T_b and k < K_b, else 0 (the w of rtts_align_stats, table column [5]);  rows[b,h,t] = sum_k P W (0 for t >= T_b);
 *   loss = sum_{b,h,t} rows / (H sum_b T_b): the mean off-diagonal mass per valid frame, in [0, 1].
 *   n_frames, n_keys i32 (B) on the device: T_b, K_b.  A slot with T_b outside 1..Tq or K_b outside 1..Tk counts in neither
 *   sum; if none counts, the loss and c are 0.
 * rtts_xattn_guide_rows: rows f32 (B*H, Tq) from q, kv, kvalid and the lse of rtts_xattn_fwd; one fixed summation order.
 * rtts_xattn_guide_fold: out f64 (B+1): out[b] = sum_{h,t} rows / (H T_b) (0 for a slot that does not count), out[B] = the loss;
 *   c_dev f32 (1) = c = coef / (H sum_b T_b), coef = the weight the loss term carries into the backward.  f64 sums in a fixed
 *   order, one launch: a second call gives the same bits.
 * rtts_xattn_bwd_guided: rtts_xattn_bwd with dS = P o (keep o dP + c W - (delta + c rows)) / sqrt(dh): the gradient of
 *   sum(o . dout) + coef * loss.  dv is that of rtts_xattn_bwd; the guided term is not multiplied by the dropout keep-scale.
 * Envelope of rtts_xattn_fwd.  A null pointer (kvalid, seed_dev and dq_chunks aside), a bad stride or sigma <= 0 is rejected
 * by the argument's name before any launch; nothing is read by the host, so all three can be captured. */
int rtts_xattn_guide_rows(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid, const float* lse,
                          const int32_t* n_frames, const int32_t* n_keys, int B, int H, int Tq, int Tk, int dh, double sigma,
                          float* rows, void* stream);
int rtts_xattn_guide_fold(const float* rows, const int32_t* n_frames, const int32_t* n_keys, int B, int H, int Tq, int Tk,
                          double coef, double* out, float* c_dev, void* stream);
int rtts_xattn_bwd_guided(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid,
                          const void* dout, int64_t ld_dout, const float* lse, const float* delta,
                          int B, int H, int Tq, int Tk, int dh, void* dq, int64_t ld_dq, void* dkv_part,
                          float drop_p, uint32_t seed, const uint32_t* seed_dev, void* dq_chunks, const float* guide_rows,
                          const float* c_dev, const int32_t* n_frames, const int32_t* n_keys, double sigma, void* stream);

/* ---- dense shared-QK attention (use_full_attn / T <= full_attn_thres of the LSH layer) -------------------
 * What reformer_pytorch's LSHSelfAttention computes on its FullQKAttention branch; the layer is built at reference
 * reformer_tts/model/reformer.py:198-217.  Per (batch, head), rows of dh = 64 bf16 in the [qk | v] layout (common stride ld):
 *   s_ij = (qk_i . qk_j) / (sqrt(dh) max(|qk_j|, 1e-12)); then, each overwriting the last: s_ii = -5e4; s_ij = -FLT_MAX unless
 *   mask_i and mask_j; causal: s_ij = -FLT_MAX for j > i.  P = softmax_j s, o_i = sum_j P_ij keep_ij v_j.
 *   A query with mask_i = 0 therefore has P_ij = 1/T over ALL T keys: o_i = mean(v) and lse_i = -FLT_MAX exactly (the LSH
 *   kernels give v_i there); the backward takes P = 1/T, dS = 0 for such rows and still adds their dout to dv of every key.
 *   mask u8 (B,T) 1 = valid token, or NULL;  out bf16 (B,T,H*dh) stride ld_out;  lse f32 (B*H,T)
 *   keep = 0 | 1/(1-p) by the counter hash of (drop_seed + *seed_dev, (head*T + i)*T + j), head = b*H + h, in wrapping uint32
 *   T a multiple of 64, 64 <= T <= rtts_full_attn_max_t(dh) (4096 at dh = 64; -1 for any other dh): key tiles are streamed
 *   backward: delta f32 (B*H,T) = rowsum(out*dout) (rtts_lsh_bwd_delta or the to_out dgrad epilogue); dqk, dv bf16 (B,T,H*dh)
 *   stride ld_d; workspace of rtts_full_attn_bwd_workspace() bytes (fp32 key-role rows), 16-byte aligned.  Two passes (owner =
 *   key: dv and the key-role rows; owner = query: query role + key role -> dqk), no atomics: every output row is written once
 *   and two runs are bit-identical.  Bad arguments return an error (rtts_last_error) and launch nothing. */
int rtts_full_attn_max_t(int dh);
int rtts_full_attn_fwd(const void* qk, const void* v, int64_t ld, const uint8_t* mask, int B, int H, int T, int dh, int causal,
                       void* out, int64_t ld_out, float* lse, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev,
                       void* stream);
int64_t rtts_full_attn_bwd_workspace(int B, int H, int T, int dh);
int rtts_full_attn_bwd(const void* qk, const void* v, int64_t ld, const uint8_t* mask, const void* dout, int64_t ld_dout,
                       const float* lse, const float* delta, int B, int H, int T, int dh, int causal, void* dqk, void* dv,
                       int64_t ld_d, void* workspace, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream);

/* ---- single-query attention over a frame cache (incremental generation, csrc/decode.hip) -----------------
 * One new decoder position per utterance.  VALU kernels (M = 1), bounded by the read of the keys and values.
 *   rtts_decode_self_attn   row bf16 (B, 2*H*64) = [qk | v] of the new position (stride ld_row); cache bf16 (B, cap, 2*H*64), row
 *                           stride ld_cache, cache_batch_stride elements between two utterances; pos: a DEVICE int32 p = rows
 *                           already cached, shared by the batch and read when the kernel runs (one captured launch serves every
 *                           frame).  The call writes `row` into cache[b, p] exactly once, touches no other cache row, and takes key
 *                           and value of position p from `row`.  Per (b, h): s_j = (q . k_j) / (8 max(|k_j|, 1e-12)) for j < p,
 *                           s_p = -5e4, P = softmax over j <= p, o = sum_j P_j v_j as bf16 (B, H*64) stride ld_o: row p of
 *                           rtts_full_attn_fwd (causal, every position valid) with P and the P V sum kept in fp32.  p = 0: o = v_0.
 *                           cap a multiple of 64, 64 <= cap <= rtts_full_attn_max_t(64).  p outside [0, cap): nothing is written to
 *                           the cache and every o is NaN -- never an out-of-range access.  Cache rows >= p are not read.
 *   rtts_decode_cross_attn  q bf16 (B, H*dh) stride ld_q; kv, kvalid as rtts_xattn_fwd (dh 64 or 128, T_k a multiple of 128 up to
 *                           2048); s_j = q . k_j / sqrt(dh); keys with kvalid = 0 have P exactly 0; a sample without any valid key
 *                           gets o = NaN and leaves the other samples' bits alone.  o bf16 (B, H*dh) stride ld_o.
 *   splits                  a (b, h) is worked by `splits` workgroups (1 ... 64); key tiles of 64 are dealt round-robin (split s takes
 *                           tiles s, s + S, ...), each split leaves an fp32 partial (running maximum, normaliser, dh accumulators)
 *                           in `workspace` (rtts_decode_attn_workspace bytes, 16-byte aligned) and a second launch folds them in
 *                           split order; a split without keys contributes exactly nothing.  splits = 1: no second launch,
 *                           workspace may be NULL.  splits = 0: rtts_decode_attn_splits(B*H, cap or T_k), a host function of its
 *                           arguments only (-1 for sizes the calls reject; the workspace function likewise).  No atomics: two calls
 *                           give the same bits; two split counts differ by fp32 summation order only.
 *   rtts_decode_tail_im2col the postnet tail: im2col rows [tap][channel] (bf16, 5*CP wide) of window rows r0 ... R - 1 of the
 *                           R = 2 n + 1 positions that end at p = *pos (window row w <-> position p - (R - 1) + w).  src_abs = 1: src
 *                           fp32 (B, cap, C) indexed by position; 0: bf16 plain rows of window rows src_r0 ... R - 1 per utterance
 *                           (src_batch_stride elements apart).  Rows in front of position 0 or behind p, channels >= C and a p
 *                           outside [0, cap) give zeros.  dst row b * (R - r0) + (r - r0).
 * Bad arguments return an error naming the argument (rtts_last_error) and launch nothing. */
int rtts_decode_attn_splits(int BH, int T);
int64_t rtts_decode_attn_workspace(int BH, int splits, int dh);
int rtts_decode_self_attn(const void* row, int64_t ld_row, void* cache, int64_t ld_cache, int64_t cache_batch_stride,
                          const int32_t* pos, int B, int H, int cap, int dh, void* o, int64_t ld_o,
                          int splits, void* workspace, void* stream);
int rtts_decode_cross_attn(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid,
                           int B, int H, int Tk, int dh, void* o, int64_t ld_o, int splits, void* workspace, void* stream);
int rtts_decode_tail_im2col(const void* src, int src_abs, int64_t ld_src, int64_t src_batch_stride, int src_r0, int C,
                            const int32_t* pos, int cap, int B, int R, int r0, int nr, int CP, void* dst, void* stream);

/* ---- convolutional edges (prenet / postnet) and the loss ------------------------------------------
 * Reference reformer_tts/model/modules.py:8-61 (EncoderPreNet), :103-169 (PostConvNet); loss.py:28-53.
 * HALO ROWS.  The activations of a convolution stack are channels-last rows (B, L + 2*halo, C), halo = 2, with `halo` zero
 * rows in front of and behind every sequence; a halo array may have a lead-in of `lead` rows before halo row 0 and any
 * number of rows behind row B*(L+2*halo) - 1 -- all zero.  Row m (counted from halo row 0) belongs to sequence m / (L+4)
 * at position m % (L+4) - 2.  A Conv1d(k=5, pad=2) is then the IMPLICIT GEMM rtts_conv1d_k5: tap k reads the same rows
 * shifted by k - 2, the halo supplies the zero padding, nothing like an im2col matrix is written; the transposed product
 * (input gradient) reads the output gradient shifted by 2 - k, and the weight gradient is five rtts_gemm_tn problems on
 * row-shifted views.  halo = 0 everywhere below means plain (B*L) rows.
 *   rtts_conv1d_k5      y (M, C_out) = conv(x) on halo rows: M rows starting at halo row 0 (any multiple of the GEMM's row
 *                       tile; x must be readable 2 rows before and after).  transposed = 0: wp (C_out, 5*C_in) bf16 from
 *                       rtts_conv_w_perm; transposed = 1: dx = conv^T(dy), wp (C_in, 5*C_out) is the SAME array seen as
 *                       [channel of dy][tap][channel of dx].  out_f32: unrounded fp32 result (+ optional bias), else bf16.
 *                       C_in % 64 == 0, (M, C_out) must tile like rtts_gemm_nt.
 *   rtts_to_halo        dst (bf16, `rows` rows of C channels, halo row 0 at row `lead`) = the first C_src channels of src
 *                       (plain (B*L, ld_src) rows, fp32 or bf16); zero in channels >= C_src and everywhere outside the valid
 *                       set (halo = 0: a cast of plain rows with the channels zero-padded to the GEMM's K granule)
 *   rtts_conv_w_perm    wp[co][k][ci] (bf16, ci < CP zero padded) = w[co][ci][k] (fp32 master layout of nn.Conv1d)
 *   rtts_conv_dw_unperm dw[co][ci][k] += dwp[co][k][ci]
 *   rtts_bn_stats       per-channel batch mean / rstd (eps 1e-5) over the B*L valid rows of y (fp32; halo or plain rows);
 *                       optional running-stat update (momentum 0.1, unbiased variance; mean_shift = the conv bias that was
 *                       left out of y)
 *   rtts_bn_act_fwd     z(bf16) = dropout_p(act(gamma*(y-mean)*rstd + beta)); act 1 = ReLU, 2 = tanh; z_halo = 1: z is a halo
 *                       array (z_rows rows, lead-in z_lead), zero outside the valid set; z_halo = 0: B*L plain rows
 *   rtts_bn_act_bwd     dy(bf16, y's layout: dy_rows rows, lead-in dy_lead, zero outside the valid set) = BatchNorm(train)
 *                       backward through act and dropout; dz in halo rows (dz_halo = 1, no lead-in) or plain rows;
 *                       dgamma, dbeta accumulate
 *   rtts_tts_loss       losses[4] = {total, raw, post, stop} and d_raw, d_post (rows, NM; row stride ld_grad >= NM,
 *                       the pad columns are written as zero), d_stop (rows):
 *                       masked MSE (kind 0) / L1 (kind 1) means over ALL elements + BCE-with-logits(pos_weight);
 *                       predictions / gradients have rows = batch * padded_len (the decoder's length, a multiple of
 *                       pad_base), targets batch * valid_len rows (reformer_tts.py:141-143 crops the predictions): rows
 *                       t >= valid_len get zero gradient and do not count.  res != NULL: the postnet prediction is
 *                       raw + res (reformer_tts.py:139-140) with res fp32 in halo rows (no lead-in, stride ld_res), `post`
 *                       is ignored and d_post is written in halo rows (dpost_rows rows, lead-in dpost_lead, zero outside
 *                       the valid set); res == NULL: halo = dpost_lead = 0, d_post in plain rows
 *   rtts_heads_grad     dheads (B*L, width) fp32 = d_raw + d_post (halo rows, lead-in dpost_lead) + dx0 (halo rows, no
 *                       lead-in; columns < n_mels), column n_mels = d_stop: the gradient of the [mel | stop] heads
 * partial_ws: >= (2*256 + 2)*C floats (bn) / 1536 floats (loss). */
int rtts_conv1d_k5(const void* x, int64_t ldx, const void* wp, int64_t ldw, int transposed, int M, int C_out, int C_in,
                   void* y, int64_t ldy, const float* bias, int out_f32, void* stream);
int rtts_to_halo(const void* src, int64_t ld_src, int64_t src_batch_stride, int C_src, int src_f32, int B, int L, int halo, int C,
                 void* dst, int lead, int64_t rows, void* stream);
/* src_batch_stride: elements between two samples of src (0 = L * ld_src; larger for a time-sliced view such as frames [0, L-1)) */
int rtts_conv_w_perm(const float* w, int Co, int Ci, int CP, void* wp, void* stream);
int rtts_conv_dw_unperm(const float* dwp, int Co, int Ci, int CP, float* dw, void* stream);
/* All convolution weights of a step re-laid-out in ONE launch (they only change in the optimizer step, and a launch costs
 * ~5 us whatever its size): jobs[i] is one rtts_conv_w_perm problem. */
#define RTTS_CONV_PERM_MAX_GROUP 8
typedef struct {
    const float* w;    /* (Co, Ci, 5) fp32 master */
    void* wp;          /* (>= Co, 5*CP) bf16 */
    int32_t Co, Ci, CP, reserved;
} rtts_conv_perm_job;
int rtts_conv_w_perm_grouped(const rtts_conv_perm_job* jobs, int n, void* stream);
/* The adjoint for the gradients, likewise grouped: jobs[i].w = dwp (Co_pad, 5*CP) fp32, jobs[i].wp = dw (Co, Ci, 5) fp32,
 * dw[co][ci][k] += dwp[co][k][ci].  Two jobs of one call may not add into overlapping dw (refused: they would race). */
int rtts_conv_dw_unperm_grouped(const rtts_conv_perm_job* jobs, int n, void* stream);
/* The convolution in front of a BatchNorm (reference modules.py:19-54,103-169: Conv1d -> BatchNorm1d): y (M, C_out) fp32 = the forward
 * of rtts_conv1d_k5 (no bias: BatchNorm cancels it) AND, from the same accumulators, the per-channel sums of y and y^2 over the rows that
 * carry data, as rtts_gemm_nt_partial_rows(M, C_out) partial rows of [sum y | sum y^2] (2 C_out floats each) in `partial`.
 * rtts_bn_stats_from_partials finishes them into mean / rstd / running statistics exactly as rtts_bn_stats does (which re-reads y). */
int rtts_conv1d_k5_moments(const void* x, int64_t ldx, const void* wp, int64_t ldw, int M, int C_out, int C_in, void* y, int64_t ldy,
                           int B, int L, int halo, float* partial, void* stream);
int rtts_bn_stats_from_partials(const float* partial, int nrows, int B, int L, int C, float* mean, float* rstd, float* run_mean,
                                float* run_var, const float* mean_shift, int64_t* num_batches, void* stream);
int rtts_bn_stats(const float* y, int B, int L, int halo, int C, float* mean, float* rstd, float* run_mean, float* run_var,
                  const float* mean_shift, int64_t* num_batches, float* partial_ws, void* stream);
int rtts_bn_act_fwd(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                    float drop_p, uint32_t seed, const uint32_t* seed_dev, int B, int L, int halo, int C, void* z, int z_halo,
                    int z_lead, int64_t z_rows, void* stream);
int rtts_bn_act_bwd(const float* y, const void* dz, int dz_halo, const float* mean, const float* rstd, const float* gamma,
                    const float* beta, int act, float drop_p, uint32_t seed, const uint32_t* seed_dev, int B, int L, int halo, int C,
                    void* dy, int dy_lead, int64_t dy_rows, float* dgamma, float* dbeta, float* partial_ws, void* stream);
/* Data-parallel BatchNorm (SyncBN; SURVEY.md 8(e), reference modules.py:29,127 normalise over the whole batch): the two
 * stages of rtts_bn_stats / rtts_bn_act_bwd as separate calls, so that the caller can all-reduce the 2*C floats between them.
 *   rtts_bn_moments        moments[0..C) = sum y, [C..2C) = sum y^2 over this rank's B*L valid rows
 *   rtts_bn_from_moments   mean / rstd (eps 1e-5; running statistics as rtts_bn_stats) from summed moments over `count` rows
 *   rtts_bn_act_bwd_sums   sums[0..C) = sum g, [C..2C) = sum g*yhat (g = dz through act and dropout); dgamma, dbeta accumulate
 *                          the LOCAL sums (the gradient all-reduce adds the ranks)
 *   rtts_bn_act_bwd_apply  dy from (all-reduced) sums over `count` rows
 * count = 0 in rtts_bn_from_moments / rtts_bn_act_bwd_apply: the row count is read from element [2*C] of moments / sums -- the
 * caller stores its own B*L there before the all-reduce, so ranks with different batch shapes need no second collective. */
int rtts_bn_moments(const float* y, int B, int L, int halo, int C, float* moments, float* partial_ws, void* stream);
int rtts_bn_from_moments(const float* moments, int64_t count, int C, float* mean, float* rstd, float* run_mean, float* run_var,
                         const float* mean_shift, int64_t* num_batches, void* stream);
int rtts_bn_act_bwd_sums(const float* y, const void* dz, int dz_halo, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, int act, float drop_p, uint32_t seed, const uint32_t* seed_dev, int B, int L, int halo, int C,
                         float* sums, float* dgamma, float* dbeta, float* partial_ws, void* stream);
int rtts_bn_act_bwd_apply(const float* y, const void* dz, int dz_halo, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, int act, float drop_p, uint32_t seed, const uint32_t* seed_dev, int B, int L, int halo, int C,
                          const float* sums, int64_t count, void* dy, int dy_lead, int64_t dy_rows, void* stream);
int rtts_tts_loss(const float* raw, const float* post, int64_t ld_mel, const float* tgt, const float* mask, const float* stop,
                  int64_t ld_stop, const float* tstop, int rows, int NM, int kind, float pos_weight, float w_raw, float w_post,
                  float w_stop, float* d_raw, float* d_post, int64_t ld_grad, float* d_stop, float* losses, float* partial_ws,
                  int padded_len, int valid_len, const float* res, int64_t ld_res, int halo, int dpost_lead, int64_t dpost_rows,
                  int64_t tgt_batch_stride, const int32_t* valid_len_dev, int64_t mask_batch_stride, int64_t tstop_batch_stride,
                  void* stream);
/* tgt_batch_stride: elements between two samples of tgt (0 = valid_len * NM; larger for the view frames [1, L) of the batch).
 * valid_len_dev (may be NULL): the loss length as a device word, 1 <= *valid_len_dev <= valid_len -- a replayed hipGraph whose
 * batch buffers are padded to a fixed length serves batches of any length up to it; valid_len is then the time length of
 * the tgt / mask / tstop buffers only.  mask_batch_stride / tstop_batch_stride: elements between two samples of mask / tstop
 * (0 = valid_len * NM / valid_len).
 * rtts_heads_grad scale_dev (may be NULL): the upstream gradient of the total loss, multiplied into d_raw, d_post, d_stop. */
int rtts_heads_grad(const float* d_raw, const float* d_post, int dpost_lead, const float* dx0, int64_t ld_dx0, const float* d_stop,
                    int B, int L, int halo, int n_mels, int width, float* dheads, const float* scale_dev, void* stream);

/* Up to RTTS_SEGMENTS_MAX flat copies / additions in one launch (per-step refreshes of padded GEMM operands, additions of
 * padded gradient blocks into their parameters' gradients). */
#define RTTS_SEGMENTS_MAX 12
enum { RTTS_SEG_COPY_F32 = 0, RTTS_SEG_COPY_BF16 = 1, RTTS_SEG_ADD_F32 = 2, RTTS_SEG_CAST_F32_BF16 = 3 };
typedef struct {
    void* dst;
    const void* src;
    int64_t count;          /* elements */
    int32_t kind, reserved;
} rtts_segment;
int rtts_segments(const rtts_segment* jobs, int n, void* stream);

/* Scaled positional encoding (reference modules.py:172-192): out = y + alpha * dropout_p(table[t]), the mask shared over the
 * batch; dalpha += sum dy * dropout_p(table).  relu_drop: h = dropout_p(relu(h)) in place (decoder prenet, modules.py:82-100). */
int rtts_pe_add(const void* y, const float* table, const float* alpha, float drop_p, uint32_t seed, const uint32_t* seed_dev,
                int T, int64_t M, int d, float* out, void* stream);
int rtts_pe_dalpha(const float* dy, const float* table, float drop_p, uint32_t seed, const uint32_t* seed_dev, int T, int64_t M,
                   int d, float* dalpha, float* partial_ws, void* stream);
int rtts_relu_drop(void* h, float drop_p, uint32_t seed, const uint32_t* seed_dev, int64_t n, void* stream);

/* What ReformerTTS.forward derives from a batch before its first layer (reference reformer_tts.py:119-125, wrappers.py:60), one
 * launch: pad_phonemes (B, Lp_pad) = phonemes right-padded with 0; phoneme_mask = pad_phonemes != 0 and its inverse (the
 * cross-attention's key_padding_mask); frame_mask (B, Lm_pad) = (mean over the n_mels columns of loss_mask != 0), 0 behind Lm.
 * Masks are one byte per element (torch.bool storage).  Strides in elements. */
int rtts_batch_masks(const int64_t* phonemes, int64_t ph_stride, int B, int Lp, int Lp_pad, const float* loss_mask, int64_t lm_bstride,
                     int64_t lm_rstride, int Lm, int Lm_pad, int n_mels, int64_t* pad_phonemes, uint8_t* phoneme_mask,
                     uint8_t* phoneme_pad_mask, uint8_t* frame_mask, void* stream);

/* nn.Embedding + the Dropout behind it (reference modules.py:17,22,56): out (rows, C) fp32 = dropout_p(E[ids]); backward:
 * dE[id] += sum of (dx * the same keep-scales) over the rows whose id matches; padding_idx skipped.  dE accumulates: it may be
 * the parameter's gradient itself. */
int rtts_embedding_fwd(const int64_t* ids, const float* E, int rows, int C, int n_embeddings, float drop_p, uint32_t seed,
                       const uint32_t* seed_dev, float* out, void* stream);
int rtts_embedding_bwd(const int64_t* ids, const float* dx, int rows, int C, int n_embeddings, int padding_idx, float* dE,
                       float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);
/* the same with dx given as a (B, L, C) VIEW of a larger array (the convolution stack's gradient on its halo rows): batch stride and row
 * stride in floats, rows = B * L */
int rtts_embedding_bwd_strided(const int64_t* ids, const float* dx, int64_t batch_stride, int64_t row_stride, int L, int rows, int C,
                               int n_embeddings, int padding_idx, float* dE, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* stream);

/* ---- weight-gradient GEMM, split over the token dimension ------------------------------------
 * c[N][K] (fp32, stride ldc) (+)= sum_m a[m][N] * b[m][K]   (a, b bf16 with strides lda, ldb)
 * = dW of a Linear layer y = x W^T (reference modules.py:195-207, reformer.py:161-217 via autograd).
 * N % 128 == 0, K % 128 == 0, M % 64 == 0.  slab_ws (>= N*K*16 floats for full split) holds the
 * per-split partial tiles; they are summed in a fixed order by a second small launch (deterministic).
 * (A single-launch variant in which the last workgroup of a tile folds the slabs was measured 6x slower:
 * the agent-scope release fence every workgroup needs writes back a whole XCD L2.)  accumulate=1: += . */
int rtts_gemm_tn(const void* a, int64_t lda, const void* b, int64_t ldb, int M, int N, int K, float* c, int64_t ldc,
                 int accumulate, float* slab_ws, int64_t slab_ws_floats, void* stream);

/* Up to RTTS_GEMM_TN_MAX_GROUP independent weight gradients in ONE pair of launches (the deferred gradients of a
 * reversible layer): the grid holds every problem's tiles, so the split factor -- and with it the slab traffic --
 * drops to what the whole group needs to fill the chip.  A problem's result agrees with its single launch up to the fp32
 * summation order, not bit for bit: the tile size (128 or 256) and each problem's split factor depend on the whole group
 * (its tile count and GFLOP, what is left of slab_ws), and split decides how the token range is summed.  Every group is
 * deterministic run to run.  No two problems of one call may write a common element of C (their workgroups would race on
 * it and lose a contribution): such a call is refused; problems of one ldc that write disjoint column blocks of one matrix
 * are fine, spans of different ldc that interleave are refused too.  Launch overlapping problems one call after the other. */
#define RTTS_GEMM_TN_MAX_GROUP 16
typedef struct {
    const void* a; int64_t lda;    /* dY (M x N) bf16 */
    const void* b; int64_t ldb;    /* X  (M x K) bf16 */
    float* c;      int64_t ldc;    /* dW (N x K) fp32 */
    int32_t M, N, K, accumulate;
} rtts_gemm_tn_problem;
int rtts_gemm_tn_grouped(const rtts_gemm_tn_problem* problems, int n, float* slab_ws, int64_t slab_ws_floats, void* stream);

/* ---- forward / input-gradient GEMM of the stacks' Linear layers ---------------------------------
 * c[M][N] (bf16, stride ldc) = epilogue( a[M][K] (bf16, stride lda) x W ), fp32 accumulation:
 *   w_is_kn = 0: W = w[N][K] (stride ldw)  -> y = x W^T, the forward of nn.Linear: toqk / tov / to_out of the LSH layer
 *                (reformer.py:198-217 via reformer_pytorch), in_proj / out_proj of nn.MultiheadAttention
 *                (reformer.py:161-186), FeedForward net.0 / net.3 (modules.py:195-207)
 *   w_is_kn = 1: W = w[K][N] (stride ldw)  -> dx = dy W, the input gradient autograd derives for the same lines
 * epilogue: 0 none; 1 + bias[N] (fp32); 2 relu(+ bias) (FeedForward's Linear -> ReLU, modules.py:200-201);
 *           3 ReLU gate: c = acc * (gate[M][N] > 0) (bf16, stride ldg) -- the backward of that ReLU -- and, if
 *             colsum_partial != NULL, fp32 partial column sums of c: rtts_gemm_nt_partial_rows(M, N) rows of N floats
 *             (the hidden bias gradient; sum them with rtts_colsum_final_grouped).
 * K % 64 == 0; (M, N) must tile by one of 192x128, 256x128, 96x64, 128x64; a, w 16-byte aligned, lda, ldw % 8 == 0.
 * Replaces the reference's ATen/cuBLAS calls for these layers; parity vs oracle/model_ref.py in tests/test_gemm_hip.py. */
int rtts_gemm_nt(const void* a, int64_t lda, const void* w, int64_t ldw, int w_is_kn, int M, int N, int K, void* c,
                 int64_t ldc, const float* bias, int epilogue, const void* gate, int64_t ldg, float* colsum_partial,
                 void* stream);
int rtts_gemm_nt_partial_rows(int M, int N);
/* Grouped / extended form of rtts_gemm_nt (round 4).  n = 2..4 INDEPENDENT problems of one weight layout and one epilogue run as
 * ONE launch: one grid over all their tiles, a workgroup finds its problem by tile range -- the cross-attention's q and k|v
 * projections of one layer (reformer.py:161-186: two separate in_proj products inside nn.MultiheadAttention) and their
 * input-gradient pair (dxn = dq Wq beside dkeys += dkv Wkv) pay one launch ramp, tail and kernel boundary instead of two.
 * n = 1: one problem, with the epilogues rtts_gemm_nt has no arguments for:
 *   epilogue 4 + accumulate: c is fp32 (rows of ldc floats), c += result (+ bias) -- the gradient of the encoder keys summed over
 *                the decoder layers in the GEMM that produces each layer's share (no separate add launch);
 *   epilogue 5: [K][N] weights only -- the input gradient of to_out / out_proj (c = dout, bf16) AND delta[b*H + h][t] =
 *                sum over the 64 columns of head h of aux[m][.] * dout[m][.] (aux = the attention output, bf16 (M, N) stride
 *                ld_aux; rows m = b*T + t; delta f32 (B*H, T)), i.e. rtts_lsh_bwd_delta folded into the product that makes dout.
 * Epilogues 0, 1, 4 in a group (each problem its own); 0, 1, 4, 5 alone; epilogue 0 with a bias is refused (a group would add it).
 * Shapes: as rtts_gemm_nt (a group needs one tile shape that tiles every problem: 192x128, 96x64 or 128x64).
 * Tested in tests/test_gemm_hip.py against float64 on the same bf16 operands. */
typedef struct {
    const void* a; int64_t lda;
    const void* w; int64_t ldw;
    void* c; int64_t ldc;
    const float* bias;
    const void* aux; int64_t ld_aux;
    float* aux_out;
    int32_t M, N, K, epilogue;
    int32_t T, H, accumulate, reserved;
} rtts_gemm_nt_problem;
#define RTTS_GEMM_NT_MAX_GROUP 4
int rtts_gemm_nt_grouped(const rtts_gemm_nt_problem* problems, int n, int w_is_kn, void* stream);
/* TEST / A-B ONLY, process-wide: forms of the rtts_gemm_nt kernels.
 * 10 / 11 / 12: store form of the bf16 epilogues (8-byte stores / 16-byte stores after a lane-pair exchange /
 * 16-byte write-through stores), 9: the library's pick again.  Results are identical bit for bit in every form.
 * 21 / 22: main loop of the convolutions (rtts_conv1d_k5*): the plain loop, which fetches the input rows once per tap / the convolution
 * form wherever it fits (the rows of all channel blocks stay in LDS and serve the five taps; not for the 256 x 256 tile, nor where the
 * images exceed LDS), 20: the library's pick again.  Same K order: identical bit for bit as well.
 * Every other value is refused (-1, rtts_last_error): 0..3 once chose among launch forms that no longer exist. */
int rtts_debug_set_gemm_mode(int mode);
/* TEST-ONLY, process-wide (one atomic word): tile of rtts_gemm_tn / rtts_gemm_tn_grouped.  0 = the library's pick (the default:
 * what every product call gets), 1 = 128 x 128 tiles for every group, also where the library would take the 256 x 256 ring
 * kernel; anything else is refused (-1, rtts_last_error).  Replaces the RTTS_GEMM_TN_SMALL_TILES environment variable the
 * launch path used to read on every call. */
int rtts_debug_set_gemm_tn_tiles(int small_tiles);
/* FeedForward pair with a 1-bit ReLU gate: the forward GEMM (epilogue 2: bias + ReLU) also writes one 64-bit word per
 * lane and tile -- bit b set <=> the b-th output of that lane is a positive bf16 -- and the input-gradient GEMM of the same
 * (M, N) (epilogue 3, [K][N] weight) reads the words instead of re-reading the (M, N) activation (50 MB at the baseline
 * shapes).  Both calls get the same tile shape for the same (M, N), hence the same lane -> element map; gate_words holds
 * rtts_gemm_nt_gate_words(M, N) words (0: the tile chosen for this shape has no word form -- use rtts_gemm_nt with the
 * activation as `gate`). */
int64_t rtts_gemm_nt_gate_words(int M, int N);
int rtts_gemm_nt_gated(const void* a, int64_t lda, const void* w, int64_t ldw, int w_is_kn, int M, int N, int K, void* c,
                       int64_t ldc, const float* bias, int epilogue, uint64_t* gate_words, float* colsum_partial, void* stream);

/* ---- on-box peak probes (bench.py; not on the training path) --------------------------------------
 * rtts_peak_copy: dst = src, float4 stream copy of `bytes` (multiple of 16) -> achieved HBM rate = 2*bytes / time.
 * rtts_peak_mfma: `workgroups` x 8 waves each issue iters x 8 back-to-back v_mfma_f32_16x16x32_bf16 on random register
 *                 operands -> dense bf16 matrix rate = workgroups*8*iters*8*16384 FLOP / time. */
int rtts_peak_copy(const void* src, void* dst, int64_t bytes, void* stream);
/* Probe, not on the training path: a ring all-reduce as the CUs see it -- `workgroups` resident workgroups (8-32) copy `bytes`
 * (+1 on every word) in 16 KB pieces with write-through stores and sleep `sleep` x ~0.5 us between pieces (pace of a link, not of
 * HBM).  scripts/comm_overlap_probe.py runs it beside the data-parallel chain of hipGraphs. */
int rtts_comm_probe(const void* src, void* dst, int64_t bytes, int workgroups, int sleep, void* stream);
/* TEST / MEASUREMENT ONLY: a one-lane kernel writes the device's 100 MHz wall clock into buf[slot] (uint64).  Capturable: markers inside
 * a replayed hipGraph give the timeline of an UNPROFILED step (scripts/replay_stamps.py). */
int rtts_debug_stamp(void* buf, int slot, void* stream);
int rtts_peak_mfma(float* sink, int workgroups, int iters, void* stream);

/* ---- SqueezeWave vocoder, inference -----------------------------------
 * Activations are channels-last rows; the 1x1 convolutions are GEMMs outside.  Replaces, per WN layer
 * (reference reformer_tts/squeeze_wave/modules.py):
 *   rtts_sw_depthwise_k3  BatchNorm1d(eval, folded into w/bias by the caller) + depthwise Conv1d(k=3, pad 1) (:88-122):
 *                         x fp32 (B,L,C), w (C,3), bias (C) -> y bf16
 *   rtts_sw_gate          fused_add_tanh_sigmoid_multiply (:10-24) of the pointwise output pw (B*L, 2C) and the layer's
 *                         slice [cond_offset, +2C) of the conditioning (B*Lm, ld_cond), nearest-upsampled by `upsample`
 *                         (nn.Upsample, :216-219) -> acts bf16 (B*L, C)
 *   rtts_sw_coupling_inv  a1 = (a1 - b) / exp(s) on channels [half, 2*half) of audio (rows, ld_audio), wn_out = [s | b] (:353-359)
 *   rtts_sw_coupling_inv1x1  the same coupling followed by the inverse invertible 1x1 convolution (:57-85, :360-361) in one
 *                         launch: out (rows, n) fp32 = [a0 | (a1 - b) / exp(s)] @ winv^T, winv (n, n) fp32 row-major = W^-1,
 *                         wn_out = [s | b] with row stride ld_wn (the WN block's end_conv GEMM output, consumed in place);
 *                         n even, <= 128; NOT in place; fp32 FMA arithmetic (the audio path never drops to bf16) */
int rtts_sw_depthwise_k3(const float* x, const float* w, const float* bias, int B, int L, int C, void* y,
                         const float* edge_lo, const float* edge_hi, void* stream);
/* edge_lo / edge_hi (C floats, may be NULL) are subtracted at l = 0 / l = L-1: the share of a folded BatchNorm constant
 * that the zero padding of the reference does not see. */
int rtts_sw_gate(const void* pw, const void* cond, int64_t ld_cond, int cond_offset, int upsample, int B, int L, int Lm, int C,
                 void* acts, void* stream);
int rtts_sw_coupling_inv(float* audio, int64_t ld_audio, const float* wn_out, int64_t rows, int half, void* stream);
/* Ragged batches (SqueezeWave.infer_ragged / capture_ragged): the utterances of a batch laid end to end as rows, each vocoded
 * as the reference vocodes one utterance trimmed at its stop index (cli.py:241 `spectrogram[:, :, :stop]`, then
 * squeeze_wave/modules.py:334-376 per utterance).  moff is a DEVICE int32 table of nseg + 1 non-decreasing mel-frame
 * offsets (1 <= nseg <= 1024), read when the kernel runs: utterance s owns mel rows [moff[s], moff[s+1]) and audio rows
 * [upsample * moff[s], upsample * moff[s+1]).  Rows past upsample * moff[nseg], up to the capacity `rows`, are padding: they
 * are computed, but no real row reads them.
 *   rtts_sw_depthwise_k3_seg  rtts_sw_depthwise_k3 over `rows` packed rows: each segment has its own zero padding, and its
 *                         first / last row gets edge_lo / edge_hi as row 0 / L-1 does in the uniform form (which is the
 *                         same kernel with moff[s] = s * L / upsample, bit for bit)
 *   rtts_sw_gate          needs no table: audio row r of segment s reads conditioning row moff[s] + (r - upsample * moff[s]) /
 *                         upsample = r / upsample, which the uniform entry computes with B = 1, L = rows, Lm = rows / upsample
 *   rtts_sw_pack_mel      dst (rows, ld_dst) fp32 = the packed mel rows the conditioning GEMM reads: row moff[s] + t = frame t
 *                         of mel[s] (B, n_mel, L) read through its element strides, for t < moff[s+1] - moff[s] (and t < L);
 *                         every other row up to `rows` is zero */
int rtts_sw_depthwise_k3_seg(const float* x, const float* w, const float* bias, const int32_t* moff, int nseg, int upsample,
                             int64_t rows, int C, void* y, const float* edge_lo, const float* edge_hi, void* stream);
int rtts_sw_pack_mel(const float* mel, int64_t stride_b, int64_t stride_c, int64_t stride_t, int L, int n_mel, const int32_t* moff,
                     int nseg, int64_t rows, float* dst, int64_t ld_dst, void* stream);
int rtts_sw_coupling_inv1x1(const float* audio, int64_t ld_audio, const float* wn_out, int64_t ld_wn, const float* winv, int n,
                            int64_t rows, float* out, int64_t ld_out, void* stream);
/* The analysis direction, audio -> latent z with its likelihood terms (SqueezeWave.forward, squeeze_wave/modules.py:294-332, in
 * eval mode, and SqueezeWaveLoss, squeeze_wave/loss.py:14-31), over the same channels-last fp32 rows:
 *   rtts_sw_coupling_fwd1x1  one flow boundary, the mirror of rtts_sw_coupling_inv1x1: the previous flow's affine coupling
 *                         c = [x0 | exp(log_s) * x1 + b] (:326-327) with [log_s | b] = wn_out (row stride ld_wn, half = n_in / 2),
 *                         this flow's early output (:312-314: columns [0, n_early) of c -> z[:, z_col : z_col + n_early]) and
 *                         this flow's invertible 1x1 convolution (:53-65, :316) of the remaining n = n_in - n_early columns:
 *                         out (rows, n) = c[:, n_early:] @ w^T, w (n, n) fp32 row-major.  ls_row[row] += sum_c log_s[row][c]
 *                         (fp32, a fixed order per row, no atomics: the caller zeroes it once; :328 and loss.py:23-24).
 *                         wn_out NULL: the first flow, no coupling and ls_row untouched.  w NULL: the tail after the last
 *                         flow, n_early == n_in and everything goes to z (:329-331).  n_in even, <= 128; n_early and n even;
 *                         NOT in place (out != x); fp32 FMA arithmetic
 *   rtts_sw_nll_reduce    out (nseg, 2) FLOAT64 = {sum z^2, sum ls_row} per segment (loss.py:21-28, per utterance): z (rows, C)
 *                         with row stride ld_z; segment s = audio rows [upsample * moff[s], upsample * moff[s+1]) of the device
 *                         offset table, clamped to [0, rows), or rows [s * L, (s + 1) * L) with moff NULL (nseg * L == rows).
 *                         One workgroup per segment, float64 accumulation in a fixed order; rows of no segment are not read;
 *                         an empty segment gives zeros
 *   rtts_sw_pack_audio    dst (rows, C) fp32 contiguous = the packed audio rows (:304-306 `unfold` per utterance, laid end to
 *                         end): utterance s contributes exactly upsample * C * (moff[s+1] - moff[s]) samples, read from
 *                         src[start[s] ...] (start: DEVICE int64 table of nseg first-sample indices into the flat fp32 buffer
 *                         src of n_src samples); elements past the total, or whose source index falls outside src, are zero */
int rtts_sw_coupling_fwd1x1(const float* x, int64_t ld_x, const float* wn_out, int64_t ld_wn, const float* w, int n_in, int n_early,
                            int64_t rows, float* out, int64_t ld_out, float* z, int64_t ld_z, int z_col, float* ls_row, void* stream);
int rtts_sw_nll_reduce(const float* z, int64_t ld_z, int C, const float* ls_row, const int32_t* moff, int nseg, int upsample, int64_t L,
                       int64_t rows, double* out, void* stream);
int rtts_sw_pack_audio(const float* src, int64_t n_src, const int64_t* start, const int32_t* moff, int nseg, int upsample, int C,
                       int64_t rows, float* dst, void* stream);
/* Training (SqueezeWave.nll_backward): the backward of the analysis direction with the BatchNorms on batch statistics
 * (squeeze_wave/modules.py:100-117 DepthwiseSeparableConv1d in .train(), :203-235 WN.forward, :294-332 SqueezeWave.forward,
 * loss.py:14-31; the optimiser step of training/wrappers.py:327-418 differentiates exactly this).  The 1x1 convolutions'
 * gradients are rtts_gemm_nt (w_is_kn = 1) and rtts_gemm_tn; these are the pieces between them.  All are deterministic (no
 * atomics, partial sums added in a fixed order, fp32 accumulation) and validate their arguments before any launch.
 *   rtts_sw_gate_bwd      backward of rtts_sw_gate (:10-24, :216-225): dacts bf16 (B*L, C) -> dpw bf16 (B*L, 2C) = [d_t | d_s],
 *                         d_t = da g (1 - t^2), d_s = da t g (1 - g) with t, g recomputed from pw and cond as the forward did;
 *                         dcond[r][cond_offset : +2C] (bf16, B*Lm rows of stride ld_dcond) = the fp32 sum of [d_t | d_s] over the
 *                         `upsample` audio rows of conditioning row r, rounded once (the backward of nn.Upsample(nearest))
 *   rtts_sw_dwbn_bwd_sums / _apply   backward of BatchNorm1d (batch statistics over the B*L rows) followed by the depthwise k3
 *                         convolution (:100-117, zero padding of bn(h) per utterance): h fp32 (B*L, C) the block's input, dy bf16
 *                         (B*L, C) the gradient of the convolution's output, mean / rstd the batch statistics, gamma / beta the
 *                         BatchNorm's affine, w (C, 3) the depthwise taps; C % 8 == 0, h / dy / dh 16-byte aligned (8 channels per access).  _sums: sums (6, C) fp32 = {d w_0, d w_1, d w_2, d bias,
 *                         d gamma, d beta} (stored, not accumulated) through partial_ws of rtts_sw_dwbn_bwd_partial_floats(B*L, C)
 *                         floats.  _apply: dh (B*L, C) fp32 += gamma rstd (du - sums[5] / m - xhat sums[4] / m), m = B*L
 *   rtts_sw_boundary_bwd  backward of rtts_sw_coupling_fwd1x1 (same x, wn_out, w, n_in, n_early, z, z_col): dout (rows, n) the
 *                         gradient of its `out`; the early columns' gradient is z * z_scale (the loss's sum z^2 / (2 sigma^2 N)).
 *                         dw (n, n) fp32 = dout^T c[:, n_early:] (stored; through partial_ws of rtts_sw_boundary_bwd_blocks(rows)
 *                         * n * n floats); with wn_out: dx (rows, n_in) = [dc_0 | dc_1 exp(log_s)] and dwn (rows, >= n_in) =
 *                         [dc_1 x_1 exp(log_s) - inv_n | dc_1], dc = [z-seed | dout w] (inv_n = 1 / N: the loss's -sum log_s / N).
 *                         wn_out NULL: the first flow (only dw).  w NULL: the tail (n_early == n_in, dc is the z-seed). */
int rtts_sw_gate_bwd(const void* pw, const void* cond, int64_t ld_cond, int cond_offset, int upsample, int B, int L, int Lm, int C,
                     const void* dacts, void* dpw, void* dcond, int64_t ld_dcond, void* stream);
int rtts_sw_dwbn_bwd_partial_floats(int64_t rows, int C);
int rtts_sw_dwbn_bwd_sums(const float* h, const void* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                          const float* w, int B, int L, int C, float* sums, float* partial_ws, void* stream);
int rtts_sw_dwbn_bwd_apply(const float* h, const void* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           const float* w, const float* sums, int B, int L, int C, float* dh, void* stream);
int rtts_sw_boundary_bwd_blocks(int64_t rows);
int rtts_sw_boundary_bwd(const float* x, int64_t ld_x, const float* wn_out, int64_t ld_wn, const float* w, int n_in, int n_early,
                         int64_t rows, const float* dout, int64_t ld_dout, const float* z, int64_t ld_z, int z_col, float z_scale,
                         float inv_n, float* dx, int64_t ld_dx, float* dwn, int64_t ld_dwn, float* dw, float* partial_ws, void* stream);
/* The invertible 1x1 convolutions of a training step factored on the device (replaces torch.logdet(W), squeeze_wave/modules.py:63,
 * and W.inverse(), :79, for ALL flows of a model in ONE launch; csrc/sw_lu.hip):
 *   w[i]      address of W_i, (n[i], n[i]) fp32 row-major, dense;   winv[i]  address of the (n[i], n[i]) fp32 output, W_i^-1
 *   slogdet   DEVICE buffer of 2 * count doubles: matrix i writes {sign_i, log|det W_i|}, sign in {-1, 0, +1}
 * w, n and winv are HOST arrays (of device addresses, of sizes): they are copied by value into the kernel's argument block, no
 * device table is allocated and a captured graph carries the addresses itself.  One workgroup per matrix: W_i widened to
 * float64 in LDS, Gauss-Jordan elimination in place with partial (row) pivoting -- the largest |a| of the column, the LOWEST row
 * on a tie -- entirely in float64; log|det| is the float64 sum of log|pivot| in pivot order, the sign the permutation's parity
 * times the pivots' signs, W^-1 is rounded to fp32 once, at the store.  A pivot that is exactly 0: sign 0, log|det| = -inf and
 * winv[i] all NaN; the other matrices of the launch are unaffected.  No atomics, fixed reduction trees: a matrix comes out bit
 * for bit the same alone and in any batch.  Only the n[i] * n[i] words of winv[i] and the 2 * count doubles are written; winv[i]
 * must not overlap any w[k].  Supported: 1 <= count <= RTTS_SW_FACTOR_MAX_COUNT (a model with more flows calls again), 1 <= n[i] <=
 * RTTS_SW_FACTOR_MAX_N; anything else, or a null pointer, is rejected before any launch with a message that names the argument. */
#define RTTS_SW_FACTOR_MAX_COUNT 16
#define RTTS_SW_FACTOR_MAX_N 128
int rtts_sw_inv1x1_factor(const float* const* w, const int* n, int count, float* const* winv, double* slogdet, void* stream);
/* One training batch drawn from a corpus that lives on the device (csrc/sw_corpus.hip): the fixed-length crop of
 * SpectrogramToSpeechDataset.__getitem__ (reference dataset/interface.py:64-97) for each of the B slots of a batch, written as
 * the rows the training step reads (training/wrappers.py:395-403 hands LitSqueezeWave.training_step the stacked crops), with the
 * utterance and the hop chosen by the kernel: a replayed graph gets a fresh batch and the host does nothing.
 *   audio           the utterances end to end, n_audio samples: in_format 0 = f32, 1 = int16 mono, scaled by 1 / 32768 as
 *                   rtts_resample scales it (exact in f32)
 *   sample_offsets  i64 (n_utt + 1), as rtts_mel_spectrogram takes them: utterance u is samples [so[u], so[u+1]), N = their count
 *   mel, ld_mel, frame_offsets   f32 (n_mel, ld_mel) rows and i64 (n_utt + 1) offsets, exactly what rtts_mel_spectrogram wrote:
 *                   utterance u owns columns [fo[u], fo[u+1]), T_u = fo[u+1] - fo[u]
 *   order           i32 (n_order): the epoch's utterance order;  state  i64[2] = {cursor, epoch_seed}, only read;  seed: host word
 *   picks_in        i32 (B, 2) = {utterance, hop} per slot, or NULL.  Given, it replaces the draw (tests, validation, replaying a
 *                   recorded batch) and order / state may be NULL
 *   B, seg_frames, hop, C   the batch, the crop in mel frames, samples per frame, n_audio_channels; S = seg_frames * hop samples
 * The draw of slot b: i = cursor + b, u = order[i mod n_order]; if N >= S: max_hop = (N - S) / hop and
 *     h = (uint64(rtts_drop_hash(seed + uint32(epoch_seed), uint32(i))) * (max_hop + 1)) >> 32      (max_hop < 2^31)
 * else h = 0 -- a multiply-shift, not a modulo: no rejection loop, bias below (max_hop + 1) / 2^32.  Then, for j < S, t < seg_frames,
 * m < n_mel:
 *     audio_rows[b * S + j]                                = h * hop + j < N ? audio[so[u] + h * hop + j] : 0
 *     mel_rows[(b * seg_frames + t) * ld_mel_rows + m]     = h + t < T_u ? mel[m * ld_mel + fo[u] + h + t] : 0
 * which is the reference's crop for N >= S (every read in range) and its zero padding of audio AND mel for N < S (zeros, not
 * log(clip): torch.nn.functional.pad(..., 'constant')).  audio_rows: f32, B * S contiguous = the (B * S / C, C) rows of the
 * training step; mel_rows: f32 (B * seg_frames, ld_mel_rows) channels-last, columns past n_mel are not touched;
 * picks_out: i32 (B, 2) = the {u, h} used.
 * Every read is held to the utterance's own bounds.  u outside [0, n_utt) -- from order or from picks_in --, a negative hop, or
 * offsets of u that decrease or leave [0, n_audio] / [0, ld_mel], write an all-zero segment and picks_out[b] = {-1, 0}: a bad
 * table entry never becomes a read out of bounds.  No atomics; the kernel writes no word that it reads (the caller advances
 * the cursor with a separate stream-ordered add), so the output depends on the arguments alone.
 * Supported: B in 1..65535, seg_frames, hop, C >= 1 with S % C == 0, 1 <= n_mel <= 128, ld_mel_rows >= n_mel, n_utt >= 1, and
 * n_order >= 1 when the batch is drawn; anything else, or a null pointer, is rejected before any launch by the argument's name. */
int rtts_sw_draw_segments(const void* audio, int in_format, int64_t n_audio, const int64_t* sample_offsets, const float* mel,
                          int64_t ld_mel, const int64_t* frame_offsets, int n_utt, const int32_t* order, int n_order,
                          const int64_t* state, uint32_t seed, const int32_t* picks_in, int B, int seg_frames, int hop, int C,
                          int n_mel, float* audio_rows, float* mel_rows, int64_t ld_mel_rows, int32_t* picks_out, void* stream);
/* One text-to-spectrogram training batch collated from a corpus that lives on the device (csrc/tts_corpus.hip):
 * custom_sequence_padder (reference dataset/utils.py:5-42) for the B utterances `ids` names, and the Gaussian noise on the
 * teacher-forcing input of LitReformerTTS.forward (reference training/wrappers.py:53-63), in one launch, written in the layouts
 * the training step reads.
 *   mel, ld_mel, frame_offsets   f32 (n_mel, ld_mel) rows and i64 (n_utt + 1) offsets, as rtts_mel_spectrogram writes them:
 *                   utterance u owns columns [fo[u], fo[u+1]), len = their count
 *   phoneme_ids, n_phonemes, phoneme_offsets   i32 ids end to end and i64 (n_utt + 1) offsets: utterance u owns [po[u], po[u+1])
 *   ids             i32 (B), DEVICE: the utterances of the batch (the caller passes plan + offset; there is no cursor word)
 *   lm              the batch's longest utterance in frames, as the host knows it: only stored into valid_len
 * Outputs, each nullable (a null one is skipped) and each with its own row count -- the reference's collate layout and the padded
 * buffers of a captured step differ.  With len_b, plen_b the frames and phonemes of ids[b], for c < n_mel:
 *   phonemes            i64 (B, LP)             [b, j]    = j < plen_b ? phoneme_ids[po + j] : 0
 *   spectrogram_input   f32 (B, R_in, n_mel)    [b, t, c] = 1 <= t <= len_b && t < valid_in ? mel[c, fo + t - 1] + noise : 0
 *   spectrogram_target  f32 (B, R_target, n_mel) [b, t, c] = t < len_b ? mel[c, fo + t] : 0
 *   stop_tokens         f32 (B, R_stop)         [b, t]    = t == len_b - 1 ? 1 : 0
 *   loss_mask           f32 (B, R_mask, n_mel)  [b, t, c] = t < len_b ? 1 : 0
 *   valid_len           i32 [1]                 = lm (an ordinary store from one lane)
 * R_in = valid_in = lm + 1 is the reference's `spectrogram` (B, 1 + lm, n_mel) (target = its rows 1.., R_target = lm);
 * R_in = the padded length of a captured step's buffer with valid_in = lm is that buffer as the host path fills it from
 * spectrogram[:, :-1]: the batch's longest utterance loses its last frame, rows >= lm are zero.
 * noise: noise_std <= 0 means none (bit for bit the kernel without the stage).  Otherwise the live input elements get
 * + noise_std * z(b, f = t - 1, c); the start frame, the padding and the target stay untouched.  This is deliberately NOT the
 * reference as written: its walrus (wrappers.py:45) binds std = True, and its in-place write also lands on the target and on the
 * padding.  z is Box-Muller on the counter hash of the dropout sites, keyed by the utterance's own element, not the padded shape:
 *     s_b = rtts_drop_hash(seed, b);  e = f * n_mel + c;  h1 = rtts_drop_hash(s_b, 2e);  h2 = rtts_drop_hash(s_b, 2e + 1)
 *     u1 = ((h1 >> 8) + 1) * 2^-24;  u2 = (h2 >> 8) * 2^-24;  z = sqrtf(-2 logf(u1)) * cosf(6.2831855f * u2)     (|z| <= 5.77)
 * An id outside [0, n_utt), or one whose offsets decrease or leave [0, ld_mel] / [0, n_phonemes], is an utterance of length 0: an
 * all-zero slot with no stop token, never a read out of bounds.  Every word of every non-null output is written exactly once,
 * padding included; no atomics; the output depends on the arguments alone.
 * Supported: B in 1..65535, 1 <= n_mel <= 128, n_utt >= 1, row counts and LP >= 1 for the outputs given, 1 <= valid_in <= R_in;
 * anything else, or a null input pointer, is rejected before any launch by the argument's name. */
int rtts_tts_collate(const float* mel, int64_t ld_mel, const int64_t* frame_offsets, const int32_t* phoneme_ids, int64_t n_phonemes,
                     const int64_t* phoneme_offsets, int n_utt, const int32_t* ids, int B, int n_mel, int lm, int64_t* phonemes, int LP,
                     float* spectrogram_input, int R_in, int valid_in, float* spectrogram_target, int R_target, float* stop_tokens,
                     int R_stop, float* loss_mask, int R_mask, int32_t* valid_len, float noise_std, uint32_t seed, void* stream);
/* B generated spectrograms scored against their truths where both already live (csrc/infer_metrics.hip): the inference_pred_mse
 * and inference_stop_mae of LitReformerTTS.validate_inference (reference training/wrappers.py:188-195) and the per-utterance
 * squared error behind predict_samples' mse_loss and cutoff (reference cli.py:150-152).  Two kernels on `stream`, nothing read back.
 *   gen             f32, element (b, m, t) at gen[b gs_b + m gs_mel + t gs_t], L >= 0 frames (null only with L = 0): ReformerTTS.infer's
 *                   (B, n_mel, L) and the teacher-forced forward's (B, T, n_mel) are both taken as they are
 *   gen_stop        i64 (B), nullable: infer's stop indices
 *   truth           f32, channel m of frame f at truth[m ts_mel + f ts_t], f < truth_frames.  Slot b owns frames [f0_b, f0_b + len_b)
 *                   by exactly ONE of two descriptions:
 *                     corpus        frame_offsets i64 (n_utt + 1) + ids i32 (B), DEVICE; ids null: slot b is utterance b; ids may
 *                                   repeat and come in any order.  f0_b = fo[u], len_b = fo[u + 1] - fo[u]
 *                     padded batch  starts i64 (B) + lengths i32 (B), DEVICE, in frames (a collate batch's spectrogram[:, 1:] viewed
 *                                   as (B (lm + 1), n_mel) rows: starts[b] = b (lm + 1) + 1, ts_t = n_mel, ts_mel = 1)
 *   lm              the batch's longest truth in frames (true_mel.shape[-1] of the reference), a host int >= 1
 *   longest         the longest len_b where the host knows it (must not exceed lm), 0 where it does not
 *   partials        f64 workspace of B * rtts_infer_metrics_tiles(lm) words, overwritten
 * Outputs, f64, with g(b, m, t) = t < L ? gen(b, m, t) : 0 widened to f64 BEFORE the subtraction:
 *   sse[b]      = sum_{t < len_b} sum_m (g(b, m, t) - truth_b(m, t))^2
 *   stop_err[b] = | gen_stop[b] - (len_b - 1) |                     (0 when gen_stop is null)
 *   totals[0]   = sum_b sse[b] / (B n_mel lm)        totals[1] = mean_b stop_err[b]      (0 when gen_stop is null)
 * With gen = infer's spectrogram, totals are wrappers.py:188-195 exactly: the reference divides by the PADDED element count
 * (mse_loss over zeros_like(true_mel)), truth frames past L count against a prediction of zero, and generated frames past an
 * utterance's own stop still count up to len_b; frames at or past len_b are masked on both sides and are not read here, so a NaN
 * there reaches nothing, while one in a counted frame reaches sse[b] and totals[0].  sse[b] / (len_b n_mel) is cli.py:150's B = 1
 * mse_loss of utterance b.
 * Every sum has one fixed order (per-workgroup partials folded by index, no atomics) that depends on (B, n_mel, lm, the lengths)
 * alone -- not on the strides: the same numbers in another layout, and a second call, give the same bits.
 * A slot whose description leaves [0, truth_frames] (or an id outside [0, n_utt)) is never read: its sse and stop_err, and the
 * totals with them, are NaN.
 * Supported: B in 1..65535, 1 <= n_mel <= 128, lm >= 1, L >= 0, every len_b >= 1; anything else, a null pointer, neither or both
 * truth descriptions, or longest > lm is rejected before any launch by the argument's name. */
int rtts_infer_metrics_tiles(int lm);
int rtts_infer_metrics(const float* gen, int64_t gs_b, int64_t gs_mel, int64_t gs_t, int L, const int64_t* gen_stop, const float* truth,
                       int64_t ts_mel, int64_t ts_t, int64_t truth_frames, const int64_t* frame_offsets, int n_utt, const int32_t* ids,
                       const int64_t* starts, const int32_t* lengths, int B, int n_mel, int lm, int longest, double* partials, double* sse,
                       double* stop_err, double* totals, void* stream);
/* B generated spectrograms aligned to their truths by dynamic time warping (csrc/dtw.hip): the path cost and path length behind
 * MCD-DTW, the number that survives a generation running a few frames early, late or at another rate, which the frame-by-frame
 * rtts_infer_metrics above does not.  Not in the reference.  Four kernels on `stream`, nothing read back, no atomics; the call can
 * be captured in a hipGraph.
 *   gen, gen_stop, truth and the two truth descriptions: exactly the arguments of rtts_infer_metrics, with L <= rtts_dtw_max_frames()
 *   slot b          compares its first N_b = min(gen_stop[b], L) generated frames (L when gen_stop is null) with its M_b = len_b truth
 *                   frames; both lengths are read on the device
 *   lm              a host upper bound of every M_b, 1..rtts_dtw_max_frames() (a slot with M_b > lm is not scored)
 *   basis           f32 (n_proj, n_mel) row-major, nullable: every compared frame x becomes p[k] = f32(sum_m f64(basis[k, m]) f64(x[m])),
 *                   m ascending.  Null: the frames are compared as they are, and n_proj must be n_mel.  Which basis makes the result
 *                   a mel-cepstral distortion is the caller's business (evaluation.cepstral_basis)
 *   workspace       rtts_dtw_workspace_bytes(B, L, lm, n_proj) bytes (-1 for sizes the call would reject), overwritten.  It begins
 *                   with the projected generated frames, f32 (B, max(L, 1), n_proj) (tests read them)
 *   phases          RTTS_DTW_ALL.  A subset runs only those kernels on what an earlier call left in the workspace and the
 *                   outputs: for timing the phases one by one, nothing else
 * With d(i, j) = sqrtf(sum_k (p_i[k] - q_j[k])^2) in f32, computed FROM THE DIFFERENCES with k ascending (never as
 * |p|^2 + |q|^2 - 2 p.q, which cancels exactly where a good generation sits; a distance past the f32 range counts as FLT_MAX),
 * and widened to f64:
 *   D(0, 0) = d(0, 0);  D(i, j) = d(i, j) + the first minimal of D(i-1, j-1), D(i-1, j), D(i, j-1) in this order (a later one replaces
 *   an earlier one only when strictly smaller; predecessors outside the table do not exist);  S(i, j) = S of the chosen one + 1,
 *   S(0, 0) = 1
 * Outputs:
 *   cost[b]    f64 = D(N_b - 1, M_b - 1)            steps[b]  i32 = S(N_b - 1, M_b - 1), in [max(N_b, M_b), N_b + M_b - 1]
 *   totals[0]  f64 = mean_b cost[b] / steps[b]      totals[1] f64 = sum_b cost[b] / sum_b steps[b]
 * Every cell has one evaluation and every sum one fixed order: the outputs depend on the arguments alone -- not on the strides,
 * not on which truth description named the frames -- and a second call gives the same bits.
 * A slot with N_b = 0 or M_b > lm, one whose description leaves [0, truth_frames] or is empty, or whose id is outside [0, n_utt),
 * is never read: cost NaN, steps 0.  A non-finite value in a COMPARED frame (or in its projection) is detected while
 * projecting and gives the slot cost NaN, steps 0 as well: the recurrence never orders NaNs; frames at or past N_b / M_b are
 * not read, so a NaN there reaches nothing.  Either case makes both totals NaN.
 * Supported: B in 1..65535, 1 <= n_mel <= 128, 1 <= n_proj <= 128, 0 <= L <= rtts_dtw_max_frames() (2048), 1 <= lm <=
 * rtts_dtw_max_frames(); anything else, a null pointer, neither or both truth descriptions, or a workspace smaller than
 * rtts_dtw_workspace_bytes is rejected before any launch by the argument's name. */
#define RTTS_DTW_PROJECT 1
#define RTTS_DTW_DISTANCES 2
#define RTTS_DTW_RECURRENCE 4
#define RTTS_DTW_FOLD 8
#define RTTS_DTW_ALL 15
int rtts_dtw_max_frames(void);
int64_t rtts_dtw_workspace_bytes(int B, int L, int lm, int n_proj);
int rtts_dtw_align(const float* gen, int64_t gs_b, int64_t gs_mel, int64_t gs_t, int L, const int64_t* gen_stop, const float* truth,
                   int64_t ts_mel, int64_t ts_t, int64_t truth_frames, const int64_t* frame_offsets, int n_utt, const int32_t* ids,
                   const int64_t* starts, const int32_t* lengths, int B, int n_mel, int lm, const float* basis, int n_proj,
                   void* workspace, int64_t workspace_bytes, int phases, double* cost, int32_t* steps, double* totals, void* stream);

/* ---- Audio -> log-mel spectrogram (dataset preprocessing) ---------
 * Replaces the spectrogram creators of reference reformer_tts/dataset/convert.py:86-123 (Tacotron2SpectrogramCreator; :34-84
 * MelSpectrogramCreator is the same call with power 2 and another mel matrix) and spectrogram_to_log_scale, for a RAGGED batch of
 * utterances in one launch: per utterance torch.stft(center=True, pad_mode="reflect") magnitudes ^ power, the mel matrix,
 * log(max(., clip)).  All arithmetic is f32 (v_mfma_f32_32x32x2_f32, bit for bit a k-ordered fmaf chain): an utterance's output is
 * bitwise the same alone and anywhere in a batch.
 *   audio           f32, the utterances end to end: utterance s is samples [sample_offsets[s], sample_offsets[s+1])
 *   sample_offsets  i64 (nseg + 1), frame_offsets i64 (nseg + 1): DEVICE tables the kernel reads, and the same values in
 *                   sample_offsets_host / frame_offsets_host, which the entry point validates and sizes the grid by (1 <= nseg <= 65535)
 *                   The two copies MUST hold the same values: the kernel takes lengths and output columns from the device tables,
 *                   the bounds check and the grid come from the host tables, and nothing can compare them without a host
 *                   synchronisation -- a mismatch is undefined behaviour (reads and stores out of bounds)
 *   utterance s     N_s samples > n_fft / 2 (reflect padding), T_s = rtts_mel_frames(N_s, hop) = N_s / hop + 1 frames, written to
 *                   columns [frame_offsets[s], + T_s); frame_offsets[s+1] - frame_offsets[s] >= T_s, columns past T_s are not touched
 *   dft_basis       f32 (n_fft, n_fft) row-major, row n = sample of the frame, window folded in: column k < n_fft/2 =
 *                   w[n] cos(2 pi n k / n_fft); column n_fft/2 + k = w[n] sin(2 pi n k / n_fft) for 1 <= k < n_fft/2; column n_fft/2 =
 *                   w[n] cos(pi n), the Nyquist bin (the sine of bin 0 is zero).  w = periodic Hann of win_length, centred in n_fft
 *   mel_basis       f32 (n_mels, n_fft/2 + 1) row-major, applied to |X|^power
 *   out             f32 (n_mels, ld_out) rows, ld_out >= frame_offsets[nseg]: columns [frame_offsets[s], + T_s) are the reference's
 *                   (n_mels, T) of utterance s
 * Supported: n_fft in {512, 1024, 2048}, hop = n_fft / 4, 1 <= n_mels <= 128, power 1 (magnitude) or 2, clip > 0.  Anything else, a
 * null pointer, nseg < 1 or an utterance of <= n_fft / 2 samples is rejected before any launch. */
int64_t rtts_mel_frames(int64_t n_samples, int hop);
int rtts_mel_spectrogram(const float* audio, const int64_t* sample_offsets_host, const int64_t* frame_offsets_host,
                         const int64_t* sample_offsets, const int64_t* frame_offsets, int nseg, const float* dft_basis,
                         const float* mel_basis, int n_fft, int hop, int n_mels, int power, float clip, float* out, int64_t ld_out,
                         void* stream);

/* ---- Sample-rate conversion (dataset preprocessing, in front of the log-mel call) -------------
 * Replaces resample_wav of reference reformer_tts/dataset/convert.py:131-146 (torchaudio.transforms.Resample, keep channel 0),
 * for a RAGGED batch of utterances that share (orig, new, channels), in one launch.  With c = 0.99 * min(orig, new) / 2, L = 6,
 * W = L / (2 c), an utterance x[0..N), zero outside, gives M = rtts_resample_len(N, orig, new) = ceil(N * new / orig) samples
 *     out[k] = sum_i x[i] h(i / orig - k / new),   h(d) = (1 + cos(2 pi c d / L)) / 2 * sin(2 pi c d) / (pi d) / orig for |d| < W, else 0
 * (the Hann-windowed sinc of Kaldi's LinearResample = torchaudio's sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).
 * The filter arrives as tables over the reduced ratio orig_red : new_red = orig / g : new / g, g = gcd(orig, new): output
 * k = j * new_red + p is the f32 fmaf chain over t = 0 .. taps-1, in this order, of x[j * orig_red + first[p] + t] * taps_table[t][p].
 * Padded taps and samples outside the utterance take part as zeros, so an utterance's output is bitwise the same alone and anywhere
 * in a batch.
 *   audio           in_format 0: f32 mono, the utterances end to end (channels must be 1).  in_format 1: int16 PCM, `channels`
 *                   interleaved (a WAV payload as it is): channel 0 is read and scaled by 1 / 32768, the other channels are skipped
 *   in_offsets / out_offsets (nseg + 1 non-decreasing int64, in FRAMES = one sample per channel), each given twice: *_host in host
 *                   memory, read by this call; the others in DEVICE memory, read by the kernel when it runs.  The two copies MUST hold
 *                   the same values, as for rtts_mel_spectrogram: the bounds check and the grid come from the host tables
 *   utterance s     owns input frames [in_offsets[s], in_offsets[s+1]), N_s >= 1 of them (shorter than taps is fine), and writes
 *                   out[out_offsets[s] .. + M_s); out_offsets[s+1] - out_offsets[s] >= M_s, samples past M_s are not touched.  `out`
 *                   with out_offsets is exactly the (audio, sample_offsets) input of rtts_mel_spectrogram
 *   first           int32 (new_red), device: ceil(p * orig_red / new_red - W * orig), negative for small p, non-decreasing in p with
 *                   first[p + new_red] = first[p] + orig_red
 *   taps_table      f32 (taps, new_red) row-major, device: row t, column p = h((first[p] + t) / orig - p / new), zero where a
 *                   phase has fewer than `taps` coefficients.  Built in float64 on the host and rounded once
 *                   (dataset/audio.py resample_tables)
 * A workgroup computes RTTS_RESAMPLE_TILE consecutive outputs of one utterance from one LDS image of the inputs they share.
 * Supported: orig_red != new_red, both >= 1; taps in 1..RTTS_RESAMPLE_MAX_TAPS; new_red * taps <= RTTS_RESAMPLE_MAX_TABLE; a tile's
 * inputs, ceil((RTTS_RESAMPLE_TILE - 1) * orig_red / new_red) + 1 + taps words, plus min(new_red, RTTS_RESAMPLE_TILE) words must fit
 * 64 KB of LDS (downsampling by up to about 15 : 1; upsampling is not limited by it); 1 <= channels <= 8 (int16), channels = 1
 * (f32); nseg in 1..65535.  Anything else, a null pointer, offsets that decrease, an empty utterance or an output slot smaller
 * than M_s is rejected before any launch. */
#define RTTS_RESAMPLE_TILE 1024
#define RTTS_RESAMPLE_MAX_TAPS 256
#define RTTS_RESAMPLE_MAX_TABLE (1 << 22)
int64_t rtts_resample_len(int64_t n_samples, int orig, int new_);
int rtts_resample(const void* audio, int in_format, int channels, const int64_t* in_offsets_host, const int64_t* out_offsets_host,
                  const int64_t* in_offsets, const int64_t* out_offsets, int nseg, const int32_t* first, const float* taps_table,
                  int orig_red, int new_red, int taps, float* out, void* stream);

/* ---- Vocoder denoiser (the last stage of synthesis in the WaveGlow / SqueezeWave family) -------
 * Subtracts the vocoder's bias spectrum from the STFT magnitudes of generated audio and resynthesises with the original phase, for
 * a RAGGED batch of utterances in one launch.  One utterance x of n samples, n_fft = 1024, hop = 256, w = periodic Hann of n_fft,
 * T = rtts_mel_frames(n, hop) frames, xpad = x reflect-padded by n_fft / 2 on both sides (so n > n_fft / 2):
 *     X[k][t] = sum_m w[m] xpad[t hop + m] exp(-2 pi i k m / n_fft)                        k = 0 .. n_fft / 2
 *     g[k][t] = max(|X[k][t]| - strength * bias[k], 0) / |X[k][t]|                         (0 where |X| = 0)
 *     f[t][m] = irfft(g[.][t] X[.][t])[m]
 *     y[p]    = sum_t w[q - t hop] f[t][q - t hop] / sum_t w[q - t hop]^2,   q = p + n_fft / 2,   p = 0 .. n - 1
 * both sums over the frames 0 <= t < T that cover q, in ascending t: torch.istft(torch.stft(x, center=True, pad_mode="reflect") * g,
 * center=True, length=n).  All arithmetic is f32 (v_mfma_f32_32x32x2_f32, bit for bit a k-ordered fmaf chain, then one fixed-order
 * sum per sample): an utterance's output is bitwise the same alone and anywhere in a batch, and from call to call.
 *   audio, out      f32, the utterances end to end over the SAME offsets: utterance s is samples [sample_offsets[s], sample_offsets[s+1])
 *                   of both (what rtts_resample writes, rtts_mel_spectrogram reads and the ragged vocoder returns).  out must not
 *                   overlap audio (a workgroup reads the input of its neighbours' samples); samples outside the offsets are
 *                   neither read nor written
 *   sample_offsets  i64 (nseg + 1): the DEVICE table the kernel reads, and the same values in sample_offsets_host, which the entry
 *                   point validates and sizes the grid by.  The two copies MUST hold the same values, as for rtts_mel_spectrogram
 *   dft_basis       f32 (n_fft, n_fft), the basis of rtts_mel_spectrogram (analysis window folded in; column 0 is the window)
 *   idft_basis      f32 (n_fft, n_fft) row-major, its inverse with the synthesis window folded in: row = column of dft_basis,
 *                   column m = sample of the frame: w[m] / n_fft for bin 0, w[m] cos(pi m) / n_fft for the Nyquist row n_fft / 2,
 *                   2 w[m] cos(2 pi k m / n_fft) / n_fft and 2 w[m] sin(2 pi k m / n_fft) / n_fft for rows k and n_fft / 2 + k
 *                   (dataset/audio.py idft_basis: float64 on the host, rounded once)
 *   bias            f32 (n_fft / 2 + 1), the vocoder's bias magnitudes per bin, device
 * Supported: n_fft = 1024, hop = 256, 1 <= nseg <= 65535, strength finite and >= 0, every utterance longer than n_fft / 2.  Anything
 * else, a null pointer or an out that overlaps audio is rejected before any launch. */
int rtts_denoise(const float* audio, const int64_t* sample_offsets_host, const int64_t* sample_offsets, int nseg,
                 const float* dft_basis, const float* idft_basis, const float* bias /* n_fft/2+1 */, float strength, int n_fft,
                 int hop, float* out, void* stream);

/* ---- Griffin-Lim vocoding: log-mel spectrogram -> audio without a trained vocoder ---------------
 * For a RAGGED batch of utterances, n_fft = 1024, hop = 256, w = periodic Hann of n_fft.  One utterance of L mel frames gives
 * n = hop L samples (the vocoder's contract) and T = L + 1 STFT frames; STFT and iSTFT are those of rtts_denoise
 * (torch.stft(center=True, pad_mode="reflect") / torch.istft(center=True, length=n)).
 *   1. magnitudes   A[k][t] = max(0, sum_m P[k][m] exp(mel[m][t])),  t < L,  P = pinv(mel matrix) (n_fft/2 + 1, n_mels), float64 on the
 *                   host, rounded once to f32;  M[k][t] = A[k][t]^(1/power), power = 1 (magnitude mels) or 2 (power mels);
 *                   column L repeats column L - 1, so M is (n_fft/2 + 1, L + 1)
 *   2. start        x_0 = iSTFT(M e^{i phi});  phase 1 ("hash"): phi[k][t] = 2 pi (rtts_drop_hash(seed, t (n_fft/2 + 1) + k) >> 8) / 2^24
 *                   with t the utterance's OWN frame index (the counter hash of the dropout masks, csrc/rtts_common.h; the index in
 *                   uint32 arithmetic);  phase 0 ("zero"): phi = 0.  The imaginary part of bins 0 and n_fft/2 is dropped, as irfft does
 *   3. iteration    k = 0 .. n_iter - 1, beta = momentum / (1 + momentum):   R = STFT(x_k - beta x_{k-1})   (no beta term at k = 0)
 *                   x_{k+1} = iSTFT(M R / |R|),  R / |R| = 1 where |R| = 0.  momentum 0 is the classic loop, 0.99 the fast one
 *                   (by linearity the momentum term needs no spectrogram kept between the iterations)
 *   4. an utterance of fewer than 3 frames (n <= n_fft / 2) cannot be reflect-padded: its samples are written as zeros
 * All arithmetic is f32: M is one ascending-m fmaf chain per value; init and step are the launch of rtts_denoise with another gain
 * (v_mfma_f32_32x32x2_f32, bit for bit a k-ordered fmaf chain, then one fixed-order sum per sample).  An utterance's output is
 * bitwise the same alone and anywhere in a batch, and from call to call; no atomics.
 *   mel             f32, read in place: frame t, channel m of utterance s is mel[s stride_b + m stride_c + (mel_start[s] + t) stride_t]
 *                   (element strides).  A (B, n_mels, L) tensor: its strides and mel_start = 0; a packed (n_mels, sum L) one:
 *                   stride_b = 0 and mel_start = the utterances' first columns.  mel_start: i64 (nseg), DEVICE
 *   mag             f32 (n_fft/2 + 1, ld_mag) bin-major: utterance s owns columns [col_offsets[s], col_offsets[s+1]), L_s + 1 of them --
 *                   the frame offsets of rtts_mel_spectrogram for lengths hop L_s.  col_offsets[nseg] <= ld_mag
 *   sample_offsets  utterance s is samples [sample_offsets[s], sample_offsets[s+1]) of cur, prev and out: hop L_s of them
 *   col_offsets, sample_offsets   i64 (nseg + 1): the DEVICE tables the kernels read, and the same values in the _host copies, which
 *                   the entry points validate and size the grid by.  The two copies MUST hold the same values
 *   pinv            f32 (n_fft/2 + 1, n_mels) row-major, device;  dft_basis, idft_basis: those of rtts_denoise
 *   cur, prev, out  f32 over the same sample offsets.  prev may be null (and is not read when beta = 0).  out may overlap neither
 *                   cur nor prev (a workgroup reads the input of its neighbours' samples); samples outside the offsets are neither
 *                   read nor written
 * Supported: n_fft = 1024, hop = 256, 1 <= nseg <= 65535, 1 <= n_mels <= 128, power 1 or 2, 0 <= beta < 1, phase 0 or 1.  Anything
 * else, a null pointer (but prev), offsets that do not step as stated or an out that overlaps an input is rejected before any
 * launch. */
int rtts_gl_magnitudes(const float* mel, int64_t stride_b, int64_t stride_c, int64_t stride_t, const int64_t* mel_start,
                       const int64_t* col_offsets_host, const int64_t* col_offsets, int nseg, const float* pinv, int n_mels, int power,
                       int n_fft, float* mag, int64_t ld_mag, void* stream);
int rtts_gl_init(const float* mag, int64_t ld_mag, const int64_t* col_offsets_host, const int64_t* col_offsets,
                 const int64_t* sample_offsets_host, const int64_t* sample_offsets, int nseg, const float* dft_basis,
                 const float* idft_basis, int phase, uint32_t seed, int n_fft, int hop, float* out, void* stream);
int rtts_gl_step(const float* cur, const float* prev, float beta, const float* mag, int64_t ld_mag, const int64_t* col_offsets_host,
                 const int64_t* col_offsets, const int64_t* sample_offsets_host, const int64_t* sample_offsets, int nseg,
                 const float* dft_basis, const float* idft_basis, int n_fft, int hop, float* out, void* stream);

/* ---- F0 tracking and pitch-error counts (evaluation; not in the reference) ---------------------
 * rtts_pitch_yin: the F0 contour of a RAGGED batch of utterances on the frame grid of rtts_mel_spectrogram, one launch: YIN
 * (de Cheveigne and Kawahara 2002, steps 2 to 5) with the integration window W = 1024 and lags 0 .. RTTS_PITCH_MAX_LAG = 512.
 * One utterance x[0..N), zero outside, frame t, s_t = t hop - (W + 512) / 2:
 *     d_t(tau)  = sum_{j=0..W-1} (x[s_t + j] - x[s_t + j + tau])^2                           tau = 0 .. 512
 *     d'_t(0)   = 1,   d'_t(tau) = d_t(tau) tau / sum_{j=1..tau} d_t(j),  1 where that sum is 0
 *     pick      the smallest tau in [tau_min, tau_max] with d'(tau) < threshold; then, while tau + 1 <= tau_max and
 *               d'(tau + 1) < d'(tau), tau + 1.  None: the frame is unvoiced, f0 = 0, aperiodicity = min d' over [tau_min, tau_max]
 *     voiced    a, b, c = d'(tau - 1), d'(tau), d'(tau + 1);  off = 0.5 (a - c) / (a - 2 b + c) if a > b and c >= b, else 0;
 *               f0 = sample_rate / (tau + off),  aperiodicity = b
 * All arithmetic is f32, and d is summed in the direct squared-difference form (never as energies minus twice a correlation,
 * which cancels exactly at the period): with block k = samples [k hop - 768, + hop), P_k(tau) is one fmaf chain over the block's
 * j in ascending order, P = fmaf(e, e, P) with e the rounded difference; d_t = P_t + P_{t+1} + ... + P_{t + W / hop - 1}, left to
 * right; the running sum of lag tau = 8 l + i (i = 1..8) is (the totals of the groups of eight lags before l, combined by a
 * 64-wide Hillis-Steele scan, distances 1, 2, .. 32) + (d(8 l + 1) + ... + d(tau), left to right).  The order depends on hop alone:
 * an utterance's outputs are bitwise the same alone and anywhere in a batch, and from call to call.  No atomics; the call can be
 * captured in a hipGraph.
 *   audio           f32, the utterances end to end: utterance s is samples [sample_offsets[s], sample_offsets[s+1]), N_s >= 1 of
 *                   them (shorter than the window is fine)
 *   sample_offsets  i64 (nseg + 1), frame_offsets i64 (nseg + 1): DEVICE tables the kernel reads, and the same values in
 *                   sample_offsets_host / frame_offsets_host, which the entry point validates and sizes the grid by (1 <= nseg <= 65535).
 *                   The two copies MUST hold the same values, as for rtts_mel_spectrogram
 *   f0, aperiodicity   f32, one value per frame: utterance s owns [frame_offsets[s], + T_s), T_s = rtts_mel_frames(N_s, hop);
 *                   frame_offsets[s+1] - frame_offsets[s] >= T_s, slots past T_s are not touched
 *   cmnd            nullable; f32 (frame_offsets[nseg], RTTS_PITCH_MAX_LAG + 1) row-major: row frame_offsets[s] + t = d'_t(0 .. 512)
 *   a frame that touches a non-finite sample (one in [s_t, s_t + W + 512)) gives NaN in f0 and aperiodicity; its cmnd row holds
 *   what the arithmetic gave
 * A workgroup computes RTTS_PITCH_TILE_FRAMES consecutive frames of one utterance from one LDS image of the samples they share,
 * and every hop block's partial sums once for the frames that overlap it.
 * Supported: hop in {128, 256, 512}, 2 <= tau_min <= tau_max <= 511, 0 < threshold < 1, sample_rate > 0.  Anything else, a null
 * pointer (but cmnd), an offset that decreases, an empty utterance or a frame slot smaller than T_s is rejected before any launch.
 *
 * rtts_f0_compare: contour a against the reference contour b, one launch, nothing read on the host.  Each contour is packed f32
 * with its own DEVICE i64 (nseg + 1) frame-offset table; utterance s is compared over its first n_s = min(T_a, T_b) frames, T =
 * the difference of its offsets.  A frame is voiced where its value is > 0.  table is f64 (nseg + 1, 5) row-major, row s:
 *     [0] n_s      [1] frames voiced in both      [2] sum over those of (1200 log2(fa / fb))^2, in f64
 *     [3] those with |fa / fb - 1| > gross          [4] frames voiced in exactly one contour
 * and row nseg = the column sums over s in ascending order.  Fixed order, no atomics: lane l of a wave adds frames l, l + 64, ..
 * in ascending order, the 64 partial sums are folded by halving distances.  A NaN among the compared frames of either contour
 * makes the utterance's row and the last row NaN (the rule of rtts_dtw_align).
 * Supported: nseg in 1..65535, 0 < gross < 1; anything else or a null pointer is rejected before the launch. */
#define RTTS_PITCH_MAX_LAG 512
#define RTTS_PITCH_TILE_FRAMES 16
int rtts_pitch_yin(const float* audio, const int64_t* sample_offsets_host, const int64_t* frame_offsets_host,
                   const int64_t* sample_offsets, const int64_t* frame_offsets, int nseg, int hop, int tau_min, int tau_max,
                   float threshold, float sample_rate, float* f0, float* aperiodicity, float* cmnd, void* stream);
int rtts_f0_compare(const float* f0_a, const int64_t* frame_offsets_a, const float* f0_b, const int64_t* frame_offsets_b, int nseg,
                    double gross, double* table, void* stream);

/* ---- Alignment scores and phoneme durations from attention matrices (evaluation; not in the reference) ----
 * Whether the decoder's encoder-decoder attention has learnt a text-to-speech alignment, as numbers instead of the reference's
 * pictures (plot_attention_matrix, wrappers.py:137-150), and the phoneme durations such an alignment implies.  csrc/align.hip.
 * Both entries read the same operand where it lies and nothing on the host; no floating-point atomics; both can be captured in a
 * hipGraph; a second call gives the same bits, and a slot's outputs do not depend on the batch around it.
 *   a               f32, n_mat matrices of (B, Tq, Tk): element (m, b, t, k) at a[m sm + b sb + t st + k], strides in elements.  The
 *                   base must be 16-byte aligned and sm, sb, st multiples of 4, st >= Tk, and no two slots may overlap (a slot
 *                   spans Tq st elements: sb >= Tq st and sm >= (B - 1) sb + Tq st, or the two the other way round): the
 *                   per-layer outputs of rtts_xattn_probs_mean, stacked or written into one (L, B, T, Tk) buffer
 *   n_frames, n_keys  i32 (B,) ON THE DEVICE: slot b uses frames t < T = n_frames[b] and keys k < K = n_keys[b] of every matrix;
 *                   nothing at or past them is read
 *   a slot is UNSCORABLE when T is outside 1..Tq, K outside 1..Tk, or a value inside its region is not finite: its f64 outputs
 *   are NaN and its integer outputs 0 (arg-max and path -1), and it makes the totals row NaN; it is never read out of range, and
 *   every other slot keeps its bits
 * Supported: 1 <= n_mat <= 64, 1 <= B <= 65535, 1 <= Tq <= 4096, 1 <= Tk <= 2048, no multiple-of requirement.  Anything else, a
 * null pointer (but path), an unaligned base or stride, a short workspace, sigma <= 0 or floor <= 0 is rejected before any launch
 * by the argument's name.
 *
 * rtts_align_stats: the arg-max track and the sums behind the usual alignment scores.
 *   argmax      i32 (n_mat, B, Tq): the key with the largest a[t, .] over k < K, the lowest index on a tie; -1 for t >= T
 *   dur_argmax  i32 (n_mat, B, Tk): the number of frames whose arg-max is k
 *   table       f64 (n_mat, B + 1, 8), row b of matrix m:
 *                   [0] T   [1] K   [2] sum_t sum_k a   [3] sum_t max_k a   [4] sum_t (-sum_k a ln a over a > 0)
 *                   [5] sum_t sum_k a w(t, k),  w = 1 - exp(-(k / K - t / T)^2 / (2 sigma^2)), in f64 from the f32 values
 *                   [6] #{t >= 1 : argmax[t] >= argmax[t-1]}   [7] #{k : dur_argmax[k] > 0}
 *               and row B = the column sums over the slots in ascending order.  [3] / T is FastSpeech's focus rate, [5] / T
 *               the guided-attention weight of Tachibana et al. ("mass off the diagonal")
 *   A frame's sums have one fixed order that depends on K alone (lane l of a wave adds columns 4 l .. 4 l + 3, 4 l + 256 .., ascending;
 *   the 64 lanes are folded by halving distances), frames are added in frame order within tiles of 16 and the tiles in order.
 *   workspace   rtts_align_stats_workspace(n_mat, B, Tq, Tk) bytes (-1 outside the envelope), overwritten
 *
 * rtts_align_mas: monotonic alignment search (Glow-TTS): the path k(t) with k(0) = 0, k(T-1) = K-1 and steps of 0 or 1 that
 * maximises sum_t log a[t, k(t)].  With c[t, k] = log(max((double)a[t, k], floor)) and every Q in f64:
 *   Q[0, 0] = c[0, 0],  Q[0, k > 0] = -inf,  Q[t, k] = c[t, k] + max(Q[t-1, k], Q[t-1, k-1]), on an exact tie the path STAYS (k);
 *   back-tracked from (T-1, K-1).
 *   durations   i32 (n_mat, B, Tk): #{t : k(t) = k}; >= 1 for k < K, summing to T, 0 for k >= K
 *   path        nullable; i32 (n_mat, B, Tq): k(t), -1 for t >= T
 *   scores      f64 (n_mat, B + 1, 2): [Q[T-1, K-1], sum_t a[t, k(t)] added in frame order]; row B = the sums over the slots
 *   T < K also makes a slot unscorable here (no monotonic path visits every key); rtts_align_stats still scores it.
 *   workspace   rtts_align_mas_workspace(n_mat, B, Tq, Tk) bytes (-1 outside the envelope): the one-bit back-pointers when
 *               (Tq, Tk) bits do not fit in LDS */
int64_t rtts_align_stats_workspace(int n_mat, int B, int Tq, int Tk);
int rtts_align_stats(const float* a, int64_t sm, int64_t sb, int64_t st, int n_mat, int B, int Tq, int Tk, const int32_t* n_frames,
                     const int32_t* n_keys, double sigma, int32_t* argmax, int32_t* dur_argmax, double* table, void* workspace,
                     int64_t workspace_bytes, void* stream);
int64_t rtts_align_mas_workspace(int n_mat, int B, int Tq, int Tk);
int rtts_align_mas(const float* a, int64_t sm, int64_t sb, int64_t st, int n_mat, int B, int Tq, int Tk, const int32_t* n_frames,
                   const int32_t* n_keys, double floor, int32_t* durations, int32_t* path, double* scores, void* workspace,
                   int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTTS_H */
