// Dense encoder-decoder ("cross") attention, forward and backward, for short key sequences
// (T_k = 128 or 256 keys held entirely on chip; the text side of Reformer-TTS is padded to 256).
// Head width DH is a template parameter: 64 (num_heads 8 at embedding_dim 512) and 128 (num_heads 4: the reference's
// config/legacy/attention-depth-3-heads-4.yml and attention-depth-3-heads-3.yml).
//
// Replaces nn.MultiheadAttention as wrapped by MultiheadAttentionWrapper
// (reformer_tts/model/reformer.py:161-186): scores = (q W_q)(k W_k)^T / sqrt(dh),
// key_padding_mask -> -inf, softmax, P V, per head; the four projections stay GEMMs outside.
//
// Same MFMA dataflow as the LSH chunk kernels (lsh_attn_fwd.hip / lsh_attn_bwd.hip):
//   forward : lane = query, S^T = K Q^T, in-register softmax over all keys, O^T = V^T P^T
//   backward: lane = key, wave w owns keys [32w, 32w+32) of the chunk: dV, dK complete in registers for the
//             workgroup's 128 queries; dS^T crosses LDS once for dQ^T = K^T dS^T.  dK/dV of the
//             T_q/128 query blocks are written as partial slabs and summed by rtts_sum_slabs
//             (deterministic, no atomics).
#include "rtts_common.h"
#include "attn_tile.h"
#include <float.h>

#define XA_QB 128     // queries per workgroup
#ifndef XA_UNROLL
#define XA_UNROLL 1   // query-tile loop of the backward
#endif

// ------------------------------------------------------------------------------ forward
// LDS images of the backward (and the forward's V image): attn_tile.h's row images (at_off) and its dS^T image [key][128
// queries] (at_ds_off<128>); the bank arithmetic is written out there.
//
// DH = 128 (256-byte rows).  A row is NOT stored as 256 contiguous bytes: every image is DH / 64 PLANES, plane p = columns
// [64 p, 64 p + 64) of every row as a [rows][128 B] image of its own, swizzled by at_off.  The bank arithmetic:
// a bank is (byte address / 4) mod 64, i.e. the address mod 256; a plane is rows x 128 B with rows a multiple of 128, so every
// plane starts at a multiple of 16 KB and address mod 256 of (plane, row, piece) equals that of (row, piece) in the 64 kernels.
// Every LDS instruction of these kernels addresses ONE plane (a 32x32x16 MFMA fragment is 16 or 8 consecutive dh values, which
// never straddle a multiple of 64; a DMA wave-instruction fills 8 half-rows of one plane; the staging image holds 64 columns at a
// time), so each instruction sees the bank pattern derived for 128-byte rows: ds_read_b128 of one piece from 16 rows, the
// transposed read of 4 rows x 64 B, the 8-byte staging stores and 16-byte staging reads are all conflict free (degree 1), as at
// DH = 64.  (Contiguous 256-byte rows start every row at bank 0: an unswizzled piece from 16 rows would be a 16-way conflict and the
// 3-bit at_sw cannot spread 16 rows over the 16 pieces of such a row; the planes keep the derivation that is already tested.)
// The dS^T image [key][128 queries] does not depend on DH.  On the global side a half-row is one full 128-byte line, so the DMA
// loads stay line-sized.
// Row staging of the epilogues: attn_tile.h's at_store_rows, once per 64-column plane at DH = 128.
// (Round 4 also tried the forward with TWO passes over the key tiles -- maximum first, then Q K^T again, exp, row sum, P V --
//  so that a query's 256 logits need not sit in registers: 168 instead of 288 registers, two workgroups per CU instead of one,
//  bit-identical, and SLOWER: 25.2 against 22.2 us.  The kernel is bound by its vector work, not by exposed latency.)
// (and a vector-instruction diet of the same kernel -- padding-only key tiles skipped, all-valid tiles unmasked, scale and maximum in
//  one fma: 22.1 against 22.0 us.  With one four-wave workgroup per CU the kernel's time is the serial chain "64 KB of K and V
//  rows arrive (every CU at once: ~3 us) -> products and softmax (~2.5 us) -> rows leave"; neither fewer instructions nor more
//  resident waves shorten it.  A third variant -- a workgroup loads the K / V images once and works TWO query blocks -- was 29.7
//  against 21.9 us: the load is not what a block's 7.3 us are spent on either.  All three removed again; profiles/r04_xattn_ab.log.)

// score scale 1 / sqrt(DH), applied in fp32
template <int DH> struct xa_dh {
    static_assert(DH == 64 || DH == 128, "head width 64 or 128");
    static constexpr float scale = DH == 64 ? 0.125f : 0.08838834764831845f;
    static constexpr int NP = DH / 64;       // 64-column planes of an LDS image
    static constexpr int NKS = DH / 16;      // 16-wide k steps of a Q K^T product
    static constexpr int NDT = DH / 32;      // 32-wide dh tiles of an output
};

// XA_PLANES(NP, statements): the statements once per 64-column plane, `pl` a constant.  Written without a loop (and the second
// plane under `if constexpr`) so that the DH = 64 instantiations stay, statement for statement, the kernels they were before
// the head width became a template parameter: their optimized IR is identical to the pre-template kernels'.
#define XA_PLANES(NP_, ...)                  \
    do {                                     \
        {                                    \
            constexpr int pl = 0;            \
            __VA_ARGS__                      \
        }                                    \
        if constexpr ((NP_) == 2) {          \
            constexpr int pl = 1;            \
            __VA_ARGS__                      \
        }                                    \
    } while (0)

// LDS per workgroup: 2 x TK x 2 DH bytes (K, V) + 4 TK (validity words): 33 / 66 KB at DH = 64 (TK = 128 / 256), 66 / 129 KB at
// DH = 128, of the CU's 160 KB.  DH = 128 holds 256 keys only in the single-pass form (T_k = 256: 156 VGPRs + 128 AGPRs); its
// chunk-walking form is instantiated for 128 keys alone (xa_fwd_chunk), where it needs no scratch (247 + 112 registers)
template <int DH, int TK, bool MULTI>
__global__ __launch_bounds__(256) void xattn_fwd_kernel(const bf16_t* __restrict__ q, int64_t ld_q, const bf16_t* __restrict__ kv,
                                                        int64_t ld_kv, const uint8_t* __restrict__ kvalid, int H, int Tq, int TKtot_,
                                                        bf16_t* __restrict__ o, int64_t ld_o, float* __restrict__ lse,
                                                        uint32_t seed, const uint32_t* __restrict__ seed_dev, uint32_t thresh,
                                                        float dscale) {
    // TK = keys held on chip at a time; TKtot (a multiple of TK) keys are walked chunk by chunk with a running maximum and
    // normaliser.  MULTI = false: TKtot == TK is a compile-time fact -- the loop below runs once, the running state folds away
    // and the kernel is the single-pass softmax (two waves per SIMD; the general form needs one wave's worth of registers more)
    const int TKtot = MULTI ? TKtot_ : TK;
    constexpr int NKT = TK / 32;
    constexpr int NP = xa_dh<DH>::NP, NKS = xa_dh<DH>::NKS, PLANE = TK * 128;
    constexpr float SC = xa_dh<DH>::scale;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* Ks = smem;                       // [NP][TK][128] swizzled (at_off), like V
    unsigned char* Vs = Ks + NP * PLANE;
    int* kval = reinterpret_cast<int*>(Vs + NP * PLANE);

    const int nqb = Tq / XA_QB;
    const uint32_t wi = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = wi / nqb, qb = wi % nqb;
    const int b = bh / H, h = bh % H;
    const int d = H * DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;

    // Q fragments straight from global: lane (r, hh) holds Q[q0 + r][16 ks + 8 hh .. +8]
    const int qrow = qb * XA_QB + wave * 32 + r;
    const bf16_t* qptr = q + ((size_t)b * Tq + qrow) * ld_q + (size_t)h * DH;
    bf16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qptr + ks * 16 + 8 * hh);
    if (thresh && seed_dev) seed += seed_dev[0];

    float m_run = -FLT_MAX, l_run = 0.f;
    f32x16 oacc[NP][2] = {};
    const int trq = (lane & 15) >> 2, trp = lane & 3, trc = (lane >> 4) & 1;
#pragma unroll 1
    for (int c0 = 0; c0 < TKtot; c0 += TK) {
        const bf16_t* kbase = kv + ((size_t)b * TKtot + c0) * ld_kv + (size_t)h * DH;
        const bf16_t* vbase = kbase + d;
        if (c0) __syncthreads();        // every wave is done with the previous chunk's images
        // K and V rows go global -> LDS by DMA (no staging registers, no ds_write pass): one wave-instruction fills 8 consecutive
        // 128-byte rows (of one plane) in lane order, so the swizzle goes on the SOURCE side (lsh_attn_bwd.hip's gather)
        constexpr int ITERS = TK * 8 / 256;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int rowb = it * 32 + wave * 8;                     // wave-uniform: first row of this instruction
            const int row = rowb + (lane >> 3);
            const int lp = (lane & 7) ^ at_sw(row);
            XA_PLANES(NP,
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kbase + pl * 64 + (size_t)row * ld_kv + lp * 8),
                                                 (RTTS_LDS void*)(Ks + pl * PLANE + rowb * 128), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vbase + pl * 64 + (size_t)row * ld_kv + lp * 8),
                                                 (RTTS_LDS void*)(Vs + pl * PLANE + rowb * 128), 16, 0, 0););
        }
        for (int j = tid; j < TK; j += 256) kval[j] = kvalid ? (int)kvalid[(size_t)b * TKtot + c0 + j] : 1;
        __syncthreads();

        f32x16 s[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            f32x16 acc = {0};
            XA_PLANES(NP,
                _Pragma("unroll")
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + pl * PLANE + at_off(kt * 32 + r, ks * 2 + hh));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[pl * 4 + ks], acc, 0, 0, 0);
                });
            s[kt] = acc;
        }
        float m = -FLT_MAX;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int4 kvv = *reinterpret_cast<const int4*>(kval + kt * 32 + 8 * g + 4 * hh);
                const int vv[4] = {kvv.x, kvv.y, kvv.z, kvv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = vv[j] ? s[kt][4 * g + j] * SC : -FLT_MAX;
                    s[kt][4 * g + j] = x;
                    m = fmaxf(m, x);
                }
            }
        m = fmaxf(rtts_xhalf_max(m), m_run);
        // rescale what the earlier chunks left (first chunk: m_run = -FLT_MAX, l_run = 0, oacc = 0; a chunk of masked keys only
        // leaves m = m_run and alpha = 1)
        const float alpha = (m_run == -FLT_MAX) ? 0.f : __expf(m_run - m);
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = s[kt][i] == -FLT_MAX ? 0.f : __expf(s[kt][i] - m);
                s[kt][i] = p;
                l += p;
            }
        l_run = l_run * alpha + rtts_xhalf_sum(l);
        m_run = m;
        if (c0) {
            XA_PLANES(NP,
                _Pragma("unroll")
                for (int dt = 0; dt < 2; ++dt)
                    _Pragma("unroll")
                    for (int i = 0; i < 16; ++i) oacc[pl][dt][i] *= alpha;);
        }
        if (thresh) {
            // nn.MultiheadAttention(dropout=p): dropout on the NORMALISED probabilities; the normaliser is the full one, the
            // keep-scale of element (head, query, key) multiplies the unnormalised p before P V
            const uint32_t base = ((uint32_t)bh * (uint32_t)Tq + (uint32_t)qrow) * (uint32_t)TKtot + (uint32_t)c0;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    s[kt][i] *= rtts_drop_keep(seed, base + (uint32_t)(kt * 32 + 8 * (i >> 2) + 4 * hh + (i & 3)), thresh, dscale);
        }
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int o8 = 8 * s2;
                const bf16x8 pf = cvt_bf16x8(s[kt][o8], s[kt][o8 + 1], s[kt][o8 + 2], s[kt][o8 + 3], s[kt][o8 + 4], s[kt][o8 + 5],
                                             s[kt][o8 + 6], s[kt][o8 + 7]);
                XA_PLANES(NP,
                    _Pragma("unroll")
                    for (int dt = 0; dt < 2; ++dt) {
                        const int blk = (kt * 32 + 16 * s2) * 128;
                        const int t0 = at_off(4 * hh + trq, dt * 4 + 2 * trc + (trp >> 1)) + 8 * (trp & 1);
                        const int t1 = at_off(4 * hh + trq, (dt ^ 1) * 4 + 2 * trc + (trp >> 1)) + 8 * (trp & 1);   /* row + 8: sw flips bit 2 */
                        const bf16x8 vf = rtts_tr_frag(Vs + pl * PLANE + blk + t0, Vs + pl * PLANE + blk + 8 * 128 + t1);
                        oacc[pl][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, oacc[pl][dt], 0, 0, 0);
                    });
            }
    }
    const float inv_l = 1.f / l_run;
    __syncthreads();                 // every wave is done with the K image: it becomes the waves' row staging (4 KB each)
    XA_PLANES(NP, at_store_rows(Ks + wave * 4096, oacc[pl], inv_l,
                                o + ((size_t)b * Tq + qb * XA_QB + wave * 32) * ld_o + (size_t)h * DH + pl * 64, ld_o, lane););
    if (hh == 0) lse[(size_t)bh * Tq + qrow] = m_run + logf(l_run);
}

// ------------------------------------------------------------------------------ backward
// One wave per 32 keys (two per SIMD at TK = 256): the decomposition of lsh_attn_bwd.hip, and like there the one-trip `k2` loops
// and [KT2] arrays are kept as statements (as scalars: the same program, other instructions).
// DH = 128 is instantiated for TK = 128 only (rtts_xattn_bwd_key_chunks): four waves of 32 keys hold dK and dV in 2 x 64 fp32 per
// lane, the accumulator count of a 64-key wave at DH = 64, and the images are K 32 KB + Q, dout 2 x 32 KB + dS^T 32 KB + 1 KB of
// lse / delta = 129 KB of the CU's 160 KB (TK = 256 would need 64 + 64 + 64 KB).  DH = 64: 65 KB (TK = 128), 129 KB (TK = 256).
//
// GUIDE (training with a guided attention loss, rtts_xattn_bwd_guided): the loss c sum P o W is linear in P, so its gradient is
// one more term of the dS line, dS = P o (keep o dP + c W - (delta + c rows)) / sqrt(dh), with rows = rowsum(P o W) from
// rtts_xattn_guide_rows and c from rtts_xattn_guide_fold.  GUIDE = false compiles every guided statement away under `if constexpr`
// and its argument is an empty struct: the unguided kernels keep their statements and their register, LDS and occupancy figures.
template <bool GUIDE> struct XaGuide {};
template <> struct XaGuide<true> {     // arguments of the guided form only
    const float* __restrict__ rows;    // (B * H, Tq) rowsum(P o W)
    const float* __restrict__ c_dev;   // c = coef / (H sum_b T_b)
    const int32_t* __restrict__ n_frames;   // T_b
    const int32_t* __restrict__ n_keys;     // K_b
    float g;                           // 1 / (sqrt(2) sigma): w = 1 - exp(-((k / K - t / T) g)^2)
};
// does slot b count?  T_b in 1..Tq and K_b in 1..Tk
__device__ __forceinline__ bool xg_slot(const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_keys, int b, int Tq, int Tk,
                                        int& T, int& K) {
    T = n_frames[b];
    K = n_keys[b];
    return T >= 1 && T <= Tq && K >= 1 && K <= Tk;
}
// w(t, k) = 1 - exp(-y), y = (k g / K - t g / T)^2, from kk = k g / K, t and sT = g / T: one fma and one exp2.  Near the diagonal
// (y < 1/4) 1 - exp(-y) cancels -- its absolute error stays 2^-24 while w goes to 0, and a sharp, well aligned row is all such
// cells -- so there the series y - y^2/2 + ... - y^6/720 stands in (next term y^7/5040: 2^-24 relative at y = 1/4).  The rows
// kernel and the backward share this function: c (W - rows) must cancel to the last bit where a row is one-hot.
__device__ __forceinline__ float xg_w(float kk, float t, float sT) {
    const float dd = __builtin_fmaf(t, -sT, kk);
    const float y = dd * dd;
    const float far = 1.f - __builtin_amdgcn_exp2f(y * -1.4426950408889634f);
    float near = __builtin_fmaf(y, -1.f / 720.f, 1.f / 120.f);
    near = __builtin_fmaf(y, near, -1.f / 24.f);
    near = __builtin_fmaf(y, near, 1.f / 6.f);
    near = __builtin_fmaf(y, near, -0.5f);
    near = __builtin_fmaf(y, near, 1.f);
    return y < 0.25f ? y * near : far;
}

template <int DH, int TK, bool DROP, bool GUIDE>
__global__ __launch_bounds__(TK * 2) void xattn_bwd_kernel(const bf16_t* __restrict__ q, int64_t ld_q, const bf16_t* __restrict__ kv,
                                                       int64_t ld_kv, const uint8_t* __restrict__ kvalid,
                                                       const bf16_t* __restrict__ dout, int64_t ld_do, const float* __restrict__ lse,
                                                       const float* __restrict__ delta, int H, int Tq, int TKtot, bf16_t* __restrict__ dq,
                                                       int64_t ld_dq, size_t dq_chunk_stride, bf16_t* __restrict__ dkv_part, int B,
                                                       uint32_t seed, const uint32_t* __restrict__ seed_dev, uint32_t thresh,
                                                       float dscale, const XaGuide<GUIDE> gd) {
    // blockIdx.y = key chunk: this workgroup owns keys [kc0, kc0 + TK) of TKtot.  P = exp(s - lse) needs only the forward's
    // global lse, so the chunks are independent: dK/dV of the chunk are complete for this query block, dQ is the chunk's
    // share (dq_chunk_stride elements between the chunks' partial dQ arrays; one chunk: dq itself)
    const int kc0 = blockIdx.y * TK;
    dq += (size_t)blockIdx.y * dq_chunk_stride;
    constexpr int KT2 = 1;
    constexpr int NTHR = TK * 2;             // one wave per 32 keys
    constexpr int NW = NTHR / 64;
    if (DROP && seed_dev) seed += seed_dev[0];
    constexpr int DSROW = XA_QB * 2;
    constexpr int NP = xa_dh<DH>::NP, NKS = xa_dh<DH>::NKS, NDT = xa_dh<DH>::NDT, KPL = TK * 128, QPL = XA_QB * 128;
    constexpr float SC = xa_dh<DH>::scale;
    static_assert(DH == 64 || TK == 128, "DH = 128 works in 128-key chunks");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* Ks = smem;                        // [NP][TK][128]   swizzled
    unsigned char* Qs = Ks + NP * KPL;               // [NP][128][128]  swizzled
    unsigned char* Os = Qs + NP * QPL;               // [NP][128][128]  swizzled
    unsigned char* Ds = Os + NP * QPL;               // [TK][256]   dS^T (already * scale), swizzled
    float* qlse = reinterpret_cast<float*>(Ds + TK * DSROW);
    float* qdel = qlse + XA_QB;

    const int nqb = Tq / XA_QB;
    const uint32_t wi = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = wi / nqb, qb = wi % nqb;
    const int b = bh / H, h = bh % H;
    const int d = H * DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;

    const bf16_t* kbase = kv + ((size_t)b * TKtot + kc0) * ld_kv + (size_t)h * DH;
    const bf16_t* vbase = kbase + d;
    const bf16_t* qbase = q + ((size_t)b * Tq + (size_t)qb * XA_QB) * ld_q + (size_t)h * DH;
    const bf16_t* dobase = dout + ((size_t)b * Tq + (size_t)qb * XA_QB) * ld_do + (size_t)h * DH;

    // images by LDS-DMA (one wave-instruction = 8 rows of 128 B of one plane in lane order, the swizzle on the SOURCE side)
    {
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
        for (int it = 0; it < TK * 8 / NTHR; ++it) {
            const int rowb = it * (NTHR / 8) + wv * 8, row = rowb + (lane >> 3);
            const int lp = (lane & 7) ^ at_sw(row);
            XA_PLANES(NP,
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kbase + pl * 64 + (size_t)row * ld_kv + lp * 8),
                                                 (RTTS_LDS void*)(Ks + pl * KPL + rowb * 128), 16, 0, 0););
        }
        for (int rowb = wv * 8; rowb < XA_QB; rowb += NTHR / 8) {
            const int row = rowb + (lane >> 3);
            const int lp = (lane & 7) ^ at_sw(row);
            XA_PLANES(NP,
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(qbase + pl * 64 + (size_t)row * ld_q + lp * 8),
                                                 (RTTS_LDS void*)(Qs + pl * QPL + rowb * 128), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(dobase + pl * 64 + (size_t)row * ld_do + lp * 8),
                                                 (RTTS_LDS void*)(Os + pl * QPL + rowb * 128), 16, 0, 0););
        }
    }
    // GUIDE: this sample's T_b, K_b and c (0 for a slot that does not count: every guided term is then exactly 0)
    float gc = 0.f, gsT = 0.f, gsK = 0.f;
    int gT = 0, gK = 0;
    if constexpr (GUIDE) {
        if (xg_slot(gd.n_frames, gd.n_keys, b, Tq, TKtot, gT, gK)) {
            gc = gd.c_dev[0];
            gsT = gd.g / (float)gT;
            gsK = gd.g / (float)gK;
        } else {
            gT = gK = 0;
        }
    }
    for (int j = tid; j < XA_QB; j += NTHR) {
        qlse[j] = lse[(size_t)bh * Tq + qb * XA_QB + j] * 1.4426950408889634f;   // base-2 softmax: exp2(s * c - lse * log2 e)
        if constexpr (GUIDE) qdel[j] = delta[(size_t)bh * Tq + qb * XA_QB + j] + gc * gd.rows[(size_t)bh * Tq + qb * XA_QB + j];
        else qdel[j] = delta[(size_t)bh * Tq + qb * XA_QB + j];
    }
    int myrow[KT2];
#pragma unroll
    for (int k2 = 0; k2 < KT2; ++k2) myrow[k2] = (wave * KT2 + k2) * 32 + r;
    bf16x8 vf[KT2][NKS], kf[KT2][NKS];
    int kvl[KT2];
#pragma unroll
    for (int k2 = 0; k2 < KT2; ++k2) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            vf[k2][ks] = *reinterpret_cast<const bf16x8*>(vbase + (size_t)myrow[k2] * ld_kv + ks * 16 + 8 * hh);
            kf[k2][ks] = *reinterpret_cast<const bf16x8*>(kbase + (size_t)myrow[k2] * ld_kv + ks * 16 + 8 * hh);
        }
        kvl[k2] = kvalid ? (int)kvalid[(size_t)b * TKtot + kc0 + myrow[k2]] : 1;
    }
    // GUIDE: the lane's key is a constant of the kernel: k g / K_b, and c (0 for a key at or past K_b)
    float gkk[KT2], gck[KT2];
    if constexpr (GUIDE) {
#pragma unroll
        for (int k2 = 0; k2 < KT2; ++k2) {
            gkk[k2] = (float)(kc0 + myrow[k2]) * gsK;
            gck[k2] = (kc0 + myrow[k2]) < gK ? gc : 0.f;
        }
    }
    const float gt0 = (float)(qb * XA_QB + 4 * hh);      // GUIDE: first query of the lane's register groups
    const int gtn = gT - qb * XA_QB - 4 * hh;            // GUIDE: queries below this count (t < T_b)
    __syncthreads();

    f32x16 dvacc[KT2][NP][2], gacc[KT2][NP][2];
#pragma unroll
    for (int a = 0; a < KT2; ++a)
        XA_PLANES(NP,
            _Pragma("unroll")
            for (int c2 = 0; c2 < 2; ++c2) {
                dvacc[a][pl][c2] = (f32x16){0};
                gacc[a][pl][c2] = (f32x16){0};
            });
    const int trq = (lane & 15) >> 2, trp = lane & 3, trc = (lane >> 4) & 1;
    int fro[4], tro[2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fro[ks] = at_off(r, ks * 2 + hh);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) tro[dt] = at_off(4 * hh + trq, dt * 4 + 2 * trc + (trp >> 1)) + 8 * (trp & 1);
    int dso[KT2][4];
#pragma unroll
    for (int k2 = 0; k2 < KT2; ++k2)
#pragma unroll
        for (int g = 0; g < 4; ++g) dso[k2][g] = at_ds_off<128>((wave * KT2 + k2) * 32 + r, 2 * g + hh);

#pragma unroll XA_UNROLL
    for (int qt = 0; qt < XA_QB / 32; ++qt) {
        bf16x8 qf[NKS], dof[NKS];
        XA_PLANES(NP,
            _Pragma("unroll")
            for (int ks = 0; ks < 4; ++ks) {
                qf[pl * 4 + ks] = *reinterpret_cast<const bf16x8*>(Qs + pl * QPL + qt * (32 * 128) + fro[ks]);
                dof[pl * 4 + ks] = *reinterpret_cast<const bf16x8*>(Os + pl * QPL + qt * (32 * 128) + fro[ks]);
            });
        bf16x8 qtf[2][NDT], dotf[2][NDT];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
            XA_PLANES(NP,
                _Pragma("unroll")
                for (int dt = 0; dt < 2; ++dt) {
                    const int blk = (qt * 32 + 16 * s2) * 128;     /* second read: 8 rows on, where sw flips the piece bit dt toggles */
                    qtf[s2][pl * 2 + dt] = rtts_tr_frag(Qs + pl * QPL + blk + tro[dt], Qs + pl * QPL + blk + 8 * 128 + tro[dt ^ 1]);
                    dotf[s2][pl * 2 + dt] = rtts_tr_frag(Os + pl * QPL + blk + tro[dt], Os + pl * QPL + blk + 8 * 128 + tro[dt ^ 1]);
                });
#pragma unroll
        for (int k2 = 0; k2 < KT2; ++k2) {
            f32x16 sacc = {0}, pacc = {0};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], kf[k2][ks], sacc, 0, 0, 0);
                pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof[ks], vf[k2][ks], pacc, 0, 0, 0);
            }
            float pp[16], ds[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int q0 = qt * 32 + 8 * g + 4 * hh;
                const float4 l4 = *reinterpret_cast<const float4*>(qlse + q0);
                const float4 d4 = *reinterpret_cast<const float4*>(qdel + q0);
                const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 4 * g + j;
                    const float p = kvl[k2] ? __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[i], SC * 1.4426950408889634f, -lv[j])) : 0.f;
                    // dropout on P: O = (D*P) V  =>  dV += (D*P)^T dO,  dS = P * (D*dP - delta)   (delta = O.dO as ever);
                    // DROP is a template parameter: nn.MultiheadAttention's dropout is 0 in config/baseline.yml
                    const float keep = DROP ? rtts_drop_keep(seed, ((uint32_t)bh * (uint32_t)Tq + (uint32_t)(qb * XA_QB + q0 + j)) *
                                                                         (uint32_t)TKtot + (uint32_t)(kc0 + myrow[k2]), thresh, dscale)
                                              : 1.f;
                    pp[i] = p * keep;
                    if constexpr (GUIDE) {
                        // + c W[t, k]; the guided term is not dropped out (the loss reads P before the dropout)
                        const int tq = qt * 32 + 8 * g + j;
                        const float gw = tq < gtn ? gck[k2] * xg_w(gkk[k2], gt0 + (float)tq, gsT) : 0.f;
                        ds[i] = p * ((pacc[i] * keep + gw) - dl[j]) * SC;
                    } else {
                        ds[i] = p * (pacc[i] * keep - dl[j]) * SC;
                    }
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const float* pq = pp + 8 * s2;
                const float* dq_ = ds + 8 * s2;
                const bf16x8 pb = cvt_bf16x8(pq[0], pq[1], pq[2], pq[3], pq[4], pq[5], pq[6], pq[7]);
                const bf16x8 db = cvt_bf16x8(dq_[0], dq_[1], dq_[2], dq_[3], dq_[4], dq_[5], dq_[6], dq_[7]);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    XA_PLANES(NP,
                        dvacc[k2][pl][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf[s2][pl * 2 + dt], pb, dvacc[k2][pl][dt], 0, 0, 0);
                        gacc[k2][pl][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf[s2][pl * 2 + dt], db, gacc[k2][pl][dt], 0, 0, 0););
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 pk;
                pk.x = pack_bf16x2(ds[4 * g], ds[4 * g + 1]);
                pk.y = pack_bf16x2(ds[4 * g + 2], ds[4 * g + 3]);
                *reinterpret_cast<uint2*>(Ds + (dso[k2][g] ^ (qt << 6))) = pk;
            }
        }
    }

    // dK | dV partial slab of this query block: layout (nqb, B, TKtot, 2d)
    bf16_t* slab = dkv_part + (((size_t)qb * B + b) * TKtot + kc0) * (size_t)(2 * d) + (size_t)h * DH;
    __syncthreads();                 // every dS^T tile is in Ds; nobody reads the Q / dout images any more: they become the row staging
    {
        static_assert(2 * NP * QPL >= NW * 4096, "the Q and dout images must hold a 4 KB staging per wave");
        unsigned char* stg = Qs + wave * 4096;
#pragma unroll
        for (int k2 = 0; k2 < KT2; ++k2) {
            // rows of this wave's 32-key tile are consecutive keys: myrow[k2] = first key + r
            bf16_t* dkp = slab + (size_t)(myrow[k2] - r) * (2 * d);
            XA_PLANES(NP, at_store_rows(stg, gacc[k2][pl], 1.f, dkp + pl * 64, 2 * d, lane););
            XA_PLANES(NP, at_store_rows(stg, dvacc[k2][pl], 1.f, dkp + d + pl * 64, 2 * d, lane););
        }
    }

    // dQ^T[dh][q] = K^T dS^T: the 8 (DH = 128: 16) (query tile, 32-wide dh tile) outputs are dealt over the waves
    constexpr int NOUT = (XA_QB / 32) * NDT;
    for (int oi = wave; oi < NOUT; oi += NW) {
        const int qt = oi >> NP, dt = oi & 1, dpl = NP == 2 ? (oi >> 1) & 1 : 0;      // plane dpl, 32-wide tile dt of the plane
        f32x16 dqa = {0};
        const int rl = 8 * hh + trq;                       // key row inside a 16-key step (second read: +4)
        const int gq = qt * 8 + 4 * trc + trp;             // 8-byte granule of the dS^T row
        const int do0 = at_ds_off<128>(rl, gq), do1 = at_ds_off<128>(rl + 4, gq);
        const int kpc = dt * 4 + 2 * trc + (trp >> 1);
        const unsigned char* Kp = Ks + dpl * KPL;
        const int ko0 = at_off(rl, kpc) + 8 * (trp & 1), ko1 = at_off(rl + 4, kpc) + 8 * (trp & 1);
#pragma unroll
        for (int kb = 0; kb < TK; kb += 16) {
            const bf16x8 bfrag = rtts_tr_frag(Ds + kb * DSROW + do0, Ds + kb * DSROW + do1);
            const bf16x8 afrag = rtts_tr_frag(Kp + kb * 128 + ko0, Kp + kb * 128 + ko1);
            dqa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, bfrag, dqa, 0, 0, 0);
        }
        bf16_t* dqp = dq + ((size_t)b * Tq + (size_t)qb * XA_QB + qt * 32 + r) * ld_dq + (size_t)h * DH;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 pk;
            pk.x = pack_bf16x2(dqa[4 * g], dqa[4 * g + 1]);
            pk.y = pack_bf16x2(dqa[4 * g + 2], dqa[4 * g + 3]);
            *reinterpret_cast<uint2*>(dqp + dpl * 64 + dt * 32 + 8 * g + 4 * hh) = pk;
        }
    }
}

// out = sum over slabs (bf16 in, fp32 accumulate, bf16 out), 8 elements per thread
__global__ __launch_bounds__(256) void sum_slabs_kernel(const bf16_t* __restrict__ part, int nslabs, size_t n8,
                                                        bf16_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int s = 0; s < nslabs; ++s) {
            const uint4 t = reinterpret_cast<const uint4*>(part)[(size_t)s * n8 + i];
            const uint32_t u[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[2 * j] += __uint_as_float(u[j] << 16);
                acc[2 * j + 1] += __uint_as_float(u[j] & 0xffff0000u);
            }
        }
        uint4 o;
        o.x = pack_bf16x2(acc[0], acc[1]);
        o.y = pack_bf16x2(acc[2], acc[3]);
        o.z = pack_bf16x2(acc[4], acc[5]);
        o.w = pack_bf16x2(acc[6], acc[7]);
        reinterpret_cast<uint4*>(out)[i] = o;
    }
}

static RttsLdsState g_xa_lds[2][4][2];   // [dh == 128][kernel][chunk == 256]
static RttsLdsState g_xp_lds;
static RttsLdsState g_xg_lds[2][2][2];   // guided backward: [dh == 128][dropout][chunk == 256]
extern "C" int rtts_sum_slabs(const void* part, int nslabs, int64_t n, void* out, void* stream);

static int xa_check(const char* fn, int B, int H, int Tq, int Tk, int dh, int64_t ld_q, int64_t ld_kv) {
    RTTS_REQUIRE(dh == 64 || dh == 128, "%s: dh=%d unsupported (this build: 64 or 128)", fn, dh);
    RTTS_REQUIRE(Tk >= 128 && Tk % 128 == 0 && Tk <= 2048, "%s: T_k=%d unsupported (a multiple of 128 up to 2048)", fn, Tk);
    RTTS_REQUIRE(Tq > 0 && Tq % XA_QB == 0, "%s: T_q=%d must be a multiple of 128", fn, Tq);
    RTTS_REQUIRE(B > 0 && H > 0, "%s: bad B/H", fn);
    RTTS_REQUIRE(ld_q >= (int64_t)H * dh && ld_q % 8 == 0 && ld_kv >= (int64_t)2 * H * dh && ld_kv % 8 == 0, "%s: bad row strides", fn);
    return 0;
}

// keys held on chip at a time: 256 when T_k is a multiple of it, else 128; the backward at dh = 128 always works 128 (its
// Q, dout and dS^T images leave room for 32 KB of K rows)
static inline int xa_chunk(int Tk) { return Tk % 256 == 0 ? 256 : 128; }
static inline int xa_bwd_chunk(int Tk, int dh) { return dh == 128 ? 128 : xa_chunk(Tk); }
// the forward at dh = 128 holds 256 keys only when they are all there are (the single-pass kernel: 156 + 128 registers); its
// chunk-walking form with 256 keys' logits, the running state and 64 output accumulators would spill, so longer T_k walk 128
static inline int xa_fwd_chunk(int Tk, int dh) { return dh == 128 ? (Tk == 256 ? 256 : 128) : xa_chunk(Tk); }
extern "C" int rtts_xattn_key_chunks(int Tk) { return (Tk >= 128 && Tk % 128 == 0) ? Tk / xa_chunk(Tk) : -1; }
extern "C" int rtts_xattn_bwd_key_chunks(int Tk, int dh) {
    return (Tk >= 128 && Tk % 128 == 0 && Tk <= 2048 && (dh == 64 || dh == 128)) ? Tk / xa_bwd_chunk(Tk, dh) : -1;
}

extern "C" int rtts_xattn_fwd(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid, int B, int H, int Tq,
                              int Tk, int dh, void* o, int64_t ld_o, float* lse, float drop_p, uint32_t seed, const uint32_t* seed_dev,
                              void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(q && kv && o && lse && drop_p >= 0.f && drop_p < 1.f, "rtts_xattn_fwd: bad arguments");
    if (xa_check("rtts_xattn_fwd", B, H, Tq, Tk, dh, ld_q, ld_kv)) return -1;
    RTTS_REQUIRE(ld_o >= (int64_t)H * dh && ld_o % 8 == 0, "rtts_xattn_fwd: bad ld_o");
    RTTS_REQUIRE((((uintptr_t)q | (uintptr_t)kv | (uintptr_t)o) & 15) == 0, "rtts_xattn_fwd: buffers must be 16-byte aligned");
    const dim3 grid(B * H * (Tq / XA_QB));
    const int chunk = xa_fwd_chunk(Tk, dh);
    const size_t lds = 2 * (size_t)chunk * (2 * dh) + (size_t)chunk * 4;
#define GO(DH_, TK_)                                                                                                      \
    do {                                                                                                                  \
        auto kern = Tk == TK_ ? xattn_fwd_kernel<DH_, TK_, false> : xattn_fwd_kernel<DH_, TK_, true>;                     \
        RTTS_ENSURE_LDS("rtts_xattn_fwd", kern, lds, g_xa_lds[DH_ == 128][Tk == TK_ ? 0 : 3][TK_ == 256]);                \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q, ld_q, (const bf16_t*)kv, ld_kv, \
                           kvalid, H, Tq, Tk, (bf16_t*)o, ld_o, lse, seed, seed_dev, rtts_drop_thresh(drop_p), 1.f / (1.f - drop_p)); \
    } while (0)
#define GO1(DH_, TK_)                                                                                                     \
    do {                                                                                                                  \
        auto kern = xattn_fwd_kernel<DH_, TK_, false>;                                                                    \
        RTTS_ENSURE_LDS("rtts_xattn_fwd", kern, lds, g_xa_lds[DH_ == 128][0][TK_ == 256]);                                \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q, ld_q, (const bf16_t*)kv, ld_kv, \
                           kvalid, H, Tq, Tk, (bf16_t*)o, ld_o, lse, seed, seed_dev, rtts_drop_thresh(drop_p), 1.f / (1.f - drop_p)); \
    } while (0)
    if (dh == 128) { if (chunk == 256) GO1(128, 256); else GO(128, 128); }
    else { if (chunk == 256) GO(64, 256); else GO(64, 128); }
#undef GO1
#undef GO
    RTTS_LAUNCH_CHECK("rtts_xattn_fwd");
    return 0;
}

// rtts_xattn_bwd (gd == nullptr) and rtts_xattn_bwd_guided: one set of checks, one grid, one LDS size
static int xa_bwd_launch(const char* fn, const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid, const void* dout,
                         int64_t ld_dout, const float* lse, const float* delta, int B, int H, int Tq, int Tk, int dh, void* dq,
                         int64_t ld_dq, void* dkv_part, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* dq_chunks,
                         const XaGuide<true>* gd, void* stream) {
    RTTS_REQUIRE(q && kv && dout && lse && delta && dq && dkv_part && drop_p >= 0.f && drop_p < 1.f, "%s: bad arguments", fn);
    if (xa_check(fn, B, H, Tq, Tk, dh, ld_q, ld_kv)) return -1;
    RTTS_REQUIRE(ld_dout >= (int64_t)H * dh && ld_dout % 8 == 0 && ld_dq >= (int64_t)H * dh && ld_dq % 8 == 0, "%s: bad strides", fn);
    RTTS_REQUIRE((((uintptr_t)q | (uintptr_t)kv | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dkv_part) & 15) == 0,
                 "%s: buffers must be 16-byte aligned", fn);
    const int chunk = xa_bwd_chunk(Tk, dh), nchunks = Tk / chunk;
    // more than one key chunk: each chunk's workgroups write their share of dQ to dq_chunks (nchunks, B*Tq, H*dh) bf16 and
    // the shares are summed into dq (compact rows) by the slab-sum kernel
    RTTS_REQUIRE(nchunks == 1 || (dq_chunks && ld_dq == (int64_t)H * dh && ((uintptr_t)dq_chunks & 15) == 0),
                 "%s: T_k=%d is worked in %d key chunks: needs dq_chunks (%d x B*T_q x H*dh bf16) and ld_dq == H*dh", fn, Tk, nchunks,
                 nchunks);
    const dim3 grid(B * H * (Tq / XA_QB), nchunks);
    const size_t dq_stride = nchunks > 1 ? (size_t)B * Tq * H * dh : 0;
    bf16_t* dq_dst = (bf16_t*)(nchunks > 1 ? dq_chunks : dq);
    const size_t lds = (size_t)chunk * (2 * dh) + 2 * (size_t)XA_QB * (2 * dh) + (size_t)chunk * (XA_QB * 2) + XA_QB * 8;
#define GO(DH_, TK_)                                                                                                      \
    do {                                                                                                                  \
        if (gd) {                                                                                                         \
            auto kern = drop_p > 0.f ? xattn_bwd_kernel<DH_, TK_, true, true> : xattn_bwd_kernel<DH_, TK_, false, true>;  \
            RTTS_ENSURE_LDS(fn, kern, lds, g_xg_lds[DH_ == 128][drop_p > 0.f][TK_ == 256]);                               \
            hipLaunchKernelGGL(kern, grid, dim3(TK_ * 2), lds, (hipStream_t)stream, (const bf16_t*)q, ld_q, (const bf16_t*)kv, ld_kv, \
                               kvalid, (const bf16_t*)dout, ld_dout, lse, delta, H, Tq, Tk, dq_dst, ld_dq, dq_stride, (bf16_t*)dkv_part, B, \
                               seed, seed_dev, rtts_drop_thresh(drop_p), 1.f / (1.f - drop_p), *gd);                                 \
        } else {                                                                                                          \
            auto kern = drop_p > 0.f ? xattn_bwd_kernel<DH_, TK_, true, false> : xattn_bwd_kernel<DH_, TK_, false, false>; \
            RTTS_ENSURE_LDS(fn, kern, lds, g_xa_lds[DH_ == 128][1 + (drop_p > 0.f)][TK_ == 256]);                         \
            hipLaunchKernelGGL(kern, grid, dim3(TK_ * 2), lds, (hipStream_t)stream, (const bf16_t*)q, ld_q, (const bf16_t*)kv, ld_kv, \
                               kvalid, (const bf16_t*)dout, ld_dout, lse, delta, H, Tq, Tk, dq_dst, ld_dq, dq_stride, (bf16_t*)dkv_part, B, \
                               seed, seed_dev, rtts_drop_thresh(drop_p), 1.f / (1.f - drop_p), XaGuide<false>{});        \
        }                                                                                                                 \
    } while (0)
    if (dh == 128) GO(128, 128); else if (chunk == 256) GO(64, 256); else GO(64, 128);
#undef GO
    RTTS_LAUNCH_CHECK(fn);
    if (nchunks > 1) return rtts_sum_slabs(dq_chunks, nchunks, (int64_t)dq_stride, dq, stream);
    return 0;
}

extern "C" int rtts_xattn_bwd(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid, const void* dout,
                              int64_t ld_dout, const float* lse, const float* delta, int B, int H, int Tq, int Tk, int dh, void* dq,
                              int64_t ld_dq, void* dkv_part, float drop_p, uint32_t seed, const uint32_t* seed_dev, void* dq_chunks,
                              void* stream) {
    RTTS_ENTER(stream);
    return xa_bwd_launch("rtts_xattn_bwd", q, ld_q, kv, ld_kv, kvalid, dout, ld_dout, lse, delta, B, H, Tq, Tk, dh, dq, ld_dq, dkv_part,
                         drop_p, seed, seed_dev, dq_chunks, nullptr, stream);
}

// ------------------------------------------------------------------------------ guided attention loss (training)
// loss = sum_{b,h,t} rows / (H sum_b T_b), rows[b,h,t] = sum_k P[b,h,t,k] W[b,t,k]: the guided-attention weight of Tachibana et
// al. that rtts_align_stats reports (table column [5]), as a term of the training loss.  Not in the reference, whose
// MultiheadAttentionWrapper (reformer_tts/model/reformer.py:161-186) only collects the matrices in eval mode.
//
// rows: the forward's dataflow (lane = query, S^T = K Q^T, P = exp2(s c - lse log2 e)), one workgroup per (b, h, 128-query block),
// the 128-key chunks walked in ascending order (K of chunk c + 1 arrives by DMA while chunk c is worked); a lane adds its keys in
// ascending order and the two half-waves fold once at the end: one fixed order, no atomics.  Chunks wholly past K_b are skipped.
// LDS: 2 x 128 keys x 2 DH bytes + 1 KB of validity words: 33 KB at DH = 64, 65 KB at DH = 128.
#define XG_KC 128
template <int DH>
__global__ __launch_bounds__(256) void xattn_guide_rows_kernel(const bf16_t* __restrict__ q, int64_t ld_q, const bf16_t* __restrict__ kv,
                                                               int64_t ld_kv, const uint8_t* __restrict__ kvalid, const float* __restrict__ lse,
                                                               const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_keys,
                                                               int H, int Tq, int Tk, float g, float* __restrict__ rows) {
    constexpr int NKT = XG_KC / 32;
    constexpr int NP = xa_dh<DH>::NP, NKS = xa_dh<DH>::NKS, PLANE = XG_KC * 128;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // 2 x [NP][XG_KC][128 B] swizzled (at_off), 2 x kval
    const int nqb = Tq / XA_QB;
    const uint32_t wi = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = wi / nqb, qb = wi % nqb;
    const int b = bh / H, h = bh % H;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int qrow = qb * XA_QB + wave * 32 + r;
    float* out = rows + (size_t)bh * Tq + qrow;
    int T, K;
    if (!xg_slot(n_frames, n_keys, b, Tq, Tk, T, K) || qb * XA_QB >= T) {     // the whole workgroup: nothing to add up
        if (hh == 0) *out = 0.f;
        return;
    }
    const int nkc = (K + XG_KC - 1) / XG_KC;
    const bf16_t* kbase = kv + (size_t)b * Tk * ld_kv + (size_t)h * DH;
    int* kval = reinterpret_cast<int*>(smem + 2 * NP * PLANE);

    auto stage_k = [&](int c, int buf) {
        constexpr int ITERS = XG_KC * 8 / 256;
        unsigned char* dst = smem + buf * (NP * PLANE);
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int rowb = it * 32 + wave * 8;
            const int row = rowb + (lane >> 3);
            const int lp = (lane & 7) ^ at_sw(row);
            XA_PLANES(NP,
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kbase + pl * 64 + (size_t)(c * XG_KC + row) * ld_kv + lp * 8),
                                                 (RTTS_LDS void*)(dst + pl * PLANE + rowb * 128), 16, 0, 0););
        }
        for (int j = tid; j < XG_KC; j += 256) kval[buf * XG_KC + j] = kvalid ? (int)kvalid[(size_t)b * Tk + c * XG_KC + j] : 1;
    };
    stage_k(0, 0);

    constexpr float kLog2e = 1.4426950408889634f;
    bf16x8 qf[NKS];
    const bf16_t* qptr = q + ((size_t)b * Tq + qrow) * ld_q + (size_t)h * DH;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qptr + ks * 16 + 8 * hh);
    // P = exp2((s c - lse) log2 e) with the difference taken FIRST and c the forward's own fp32 scale (its lse is the normaliser of
    // exactly those logits): at logits near 80 the one-fma form exp2(s c log2 e - lse log2 e) rounds the exponent at the size of
    // lse log2 e (2^-18 absolute, 3e-6 of P), which a sum of P itself, unlike P V rounded to bf16, would show
    const float lrow = lse[(size_t)bh * Tq + qrow];
    const float sT = g / (float)T, sK = g / (float)K;
    const float tq = (float)qrow;
    float acc = 0.f;
#pragma unroll 1
    for (int c = 0; c < nkc; ++c) {
        __syncthreads();            // K of chunk c is in LDS, and every wave is done with the buffer chunk c - 1 read
        if (c + 1 < nkc) stage_k(c + 1, (c + 1) & 1);
        const unsigned char* Ks = smem + (c & 1) * (NP * PLANE);
        const int* kvc = kval + (c & 1) * XG_KC;
        const int k0 = c * XG_KC + 4 * hh;               // the lane's first key of the chunk
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            f32x16 s = {0};
            XA_PLANES(NP,
                _Pragma("unroll")
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + pl * PLANE + at_off(kt * 32 + r, ks * 2 + hh));
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[pl * 4 + ks], s, 0, 0, 0);
                });
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int4 kvv = *reinterpret_cast<const int4*>(kvc + kt * 32 + 8 * g4 + 4 * hh);
                const int vv[4] = {kvv.x, kvv.y, kvv.z, kvv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = k0 + kt * 32 + 8 * g4 + j;
                    const float ex = __builtin_fmaf(s[4 * g4 + j], xa_dh<DH>::scale, -lrow);
                    const float p = (vv[j] && key < K) ? __builtin_amdgcn_exp2f(ex * kLog2e) : 0.f;
                    acc = __builtin_fmaf(p, xg_w((float)key * sK, tq, sT), acc);
                }
            }
        }
    }
    acc = rtts_xhalf_sum(acc);
    if (hh == 0) *out = qrow < T ? acc : 0.f;
}

// out[b] = sum_{h,t} rows / (H T_b) (0 for a slot that does not count), out[B] = the loss, c_dev = coef / (H sum_b T_b).  One
// workgroup: thread i adds elements i, i + 1024, ... of a sample in f64, the 1024 sums fold in a fixed tree, the samples in order.
#define XG_FOLD_THREADS 1024
__global__ __launch_bounds__(XG_FOLD_THREADS) void xattn_guide_fold_kernel(const float* __restrict__ rows, const int32_t* __restrict__ n_frames,
                                                                          const int32_t* __restrict__ n_keys, int B, int H, int Tq, int Tk,
                                                                          double coef, double* __restrict__ out, float* __restrict__ c_dev) {
    __shared__ double red[XG_FOLD_THREADS];
    const int tid = threadIdx.x;
    double total = 0.0, frames = 0.0;
    for (int b = 0; b < B; ++b) {
        int T, K;
        const bool ok = xg_slot(n_frames, n_keys, b, Tq, Tk, T, K);
        double s = 0.0;
        if (ok)
            for (int i = tid; i < H * T; i += XG_FOLD_THREADS) s += (double)rows[((size_t)b * H + i / T) * Tq + i % T];
        red[tid] = s;
        __syncthreads();
        for (int o = XG_FOLD_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            out[b] = ok ? red[0] / ((double)H * T) : 0.0;
            if (ok) {
                total += red[0];
                frames += (double)T;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[B] = frames > 0.0 ? total / ((double)H * frames) : 0.0;
        c_dev[0] = frames > 0.0 ? (float)(coef / ((double)H * frames)) : 0.f;
    }
}

static RttsLdsState g_xg_rows_lds;
// 1 / (sqrt(2) sigma): w = 1 - exp(-x^2 / (2 sigma^2)) = 1 - exp(-(x g)^2)
static inline float xg_g(double sigma) { return (float)(0.7071067811865476 / sigma); }
#define XG_NAMED(fn, p) RTTS_REQUIRE((p) != nullptr, "%s: %s is a null pointer", fn, #p)

extern "C" int rtts_xattn_guide_rows(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid, const float* lse,
                                     const int32_t* n_frames, const int32_t* n_keys, int B, int H, int Tq, int Tk, int dh, double sigma,
                                     float* rows, void* stream) {
    RTTS_ENTER(stream);
    const char* fn = "rtts_xattn_guide_rows";
    XG_NAMED(fn, q); XG_NAMED(fn, kv); XG_NAMED(fn, lse); XG_NAMED(fn, n_frames); XG_NAMED(fn, n_keys); XG_NAMED(fn, rows);
    RTTS_REQUIRE(sigma > 0.0 && sigma <= 1.7e308, "%s: sigma must be positive and finite (got %g)", fn, sigma);
    if (xa_check(fn, B, H, Tq, Tk, dh, ld_q, ld_kv)) return -1;
    RTTS_REQUIRE((((uintptr_t)q | (uintptr_t)kv) & 15) == 0, "%s: q and kv must be 16-byte aligned", fn);
    const size_t nwg = (size_t)B * H * (Tq / XA_QB);
    RTTS_REQUIRE(nwg <= 0x7fffffff, "%s: grid too large", fn);
    const size_t lds = 2 * (size_t)XG_KC * (2 * dh) + 2 * XG_KC * 4;
    if (dh == 128) {
        RTTS_ENSURE_LDS(fn, xattn_guide_rows_kernel<128>, lds, g_xg_rows_lds);
        hipLaunchKernelGGL(xattn_guide_rows_kernel<128>, dim3((unsigned)nwg), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q, ld_q,
                           (const bf16_t*)kv, ld_kv, kvalid, lse, n_frames, n_keys, H, Tq, Tk, xg_g(sigma), rows);
    } else {
        hipLaunchKernelGGL(xattn_guide_rows_kernel<64>, dim3((unsigned)nwg), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q, ld_q,
                           (const bf16_t*)kv, ld_kv, kvalid, lse, n_frames, n_keys, H, Tq, Tk, xg_g(sigma), rows);
    }
    RTTS_LAUNCH_CHECK(fn);
    return 0;
}

extern "C" int rtts_xattn_guide_fold(const float* rows, const int32_t* n_frames, const int32_t* n_keys, int B, int H, int Tq, int Tk,
                                     double coef, double* out, float* c_dev, void* stream) {
    RTTS_ENTER(stream);
    const char* fn = "rtts_xattn_guide_fold";
    XG_NAMED(fn, rows); XG_NAMED(fn, n_frames); XG_NAMED(fn, n_keys); XG_NAMED(fn, out); XG_NAMED(fn, c_dev);
    RTTS_REQUIRE(coef == coef && coef >= -1.7e308 && coef <= 1.7e308, "%s: coef must be finite (got %g)", fn, coef);
    if (xa_check(fn, B, H, Tq, Tk, 64, (int64_t)H * 64, (int64_t)2 * H * 64)) return -1;      // the shape part of the envelope
    hipLaunchKernelGGL(xattn_guide_fold_kernel, dim3(1), dim3(XG_FOLD_THREADS), 0, (hipStream_t)stream, rows, n_frames, n_keys, B, H, Tq, Tk,
                       coef, out, c_dev);
    RTTS_LAUNCH_CHECK(fn);
    return 0;
}

extern "C" int rtts_xattn_bwd_guided(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid, const void* dout,
                                     int64_t ld_dout, const float* lse, const float* delta, int B, int H, int Tq, int Tk, int dh, void* dq,
                                     int64_t ld_dq, void* dkv_part, float drop_p, uint32_t seed, const uint32_t* seed_dev,
                                     void* dq_chunks, const float* guide_rows, const float* c_dev, const int32_t* n_frames,
                                     const int32_t* n_keys, double sigma, void* stream) {
    RTTS_ENTER(stream);
    const char* fn = "rtts_xattn_bwd_guided";
    XG_NAMED(fn, q); XG_NAMED(fn, kv); XG_NAMED(fn, dout); XG_NAMED(fn, lse); XG_NAMED(fn, delta); XG_NAMED(fn, dq); XG_NAMED(fn, dkv_part);
    XG_NAMED(fn, guide_rows); XG_NAMED(fn, c_dev); XG_NAMED(fn, n_frames); XG_NAMED(fn, n_keys);
    RTTS_REQUIRE(sigma > 0.0 && sigma <= 1.7e308, "%s: sigma must be positive and finite (got %g)", fn, sigma);
    const XaGuide<true> gd{guide_rows, c_dev, n_frames, n_keys, xg_g(sigma)};
    return xa_bwd_launch(fn, q, ld_q, kv, ld_kv, kvalid, dout, ld_dout, lse, delta, B, H, Tq, Tk, dh, dq, ld_dq, dkv_part, drop_p, seed,
                         seed_dev, dq_chunks, &gd, stream);
}

// ------------------------------------------------------------------------------ head-averaged probabilities (eval)
// a[b, i, j] = (1/H) sum_h exp(s_h(i, j) - lse_h(i)), s_h = q_h . k_h / sqrt(dh); masked keys exactly 0.  What
// nn.MultiheadAttention returns as its (head-averaged, fp32) weights and MultiheadAttentionWrapper collects in eval mode
// (reference reformer_tts/model/reformer.py:161-186).  The forward's lse (full-key log-normaliser) makes every key chunk
// independent: workgroup = (b, 128-query block, 128-key chunk), four waves of 32 queries, the H heads walked inside so the head
// sum stays in registers (no atomics, no cross-workgroup reduction).  K of head h + 1 arrives in LDS (DMA, double buffer) while
// head h is worked; Q fragments and lse come straight from global (each wave reads only its own queries).
// Layout as the forward's S^T = K Q^T: lane (r, hh) = query r, register 4 g + j = key 8 g + 4 hh + j of a 32-key tile, so a
// register group is 4 consecutive keys of one row of `a` = one 16-byte store; the 4 groups of a tile complete 32 rows x 128 B.
// LDS: 2 x 128 keys x 2 DH bytes + 512: 33 KB at DH = 64, 65 KB at DH = 128 (planes of 64 columns as in the kernels above).
#define XP_KC 128     // keys per workgroup
template <int DH>
__global__ __launch_bounds__(256) void xattn_probs_mean_kernel(const bf16_t* __restrict__ q, int64_t ld_q, const bf16_t* __restrict__ kv,
                                                               int64_t ld_kv, const uint8_t* __restrict__ kvalid, const float* __restrict__ lse,
                                                               int H, int Tq, int Tk, float* __restrict__ a, int64_t ld_a) {
    constexpr int NKT = XP_KC / 32;
    constexpr int NP = xa_dh<DH>::NP, NKS = xa_dh<DH>::NKS, PLANE = XP_KC * 128;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // 2 x [NP][XP_KC][128 B] swizzled (at_off), kval
    const int nqb = Tq / XA_QB, nkc = Tk / XP_KC;
    const uint32_t wi = xcd_remap(blockIdx.x, gridDim.x);       // (b, query block, key chunk), key chunk fastest: the chunks of a
    const int kc = wi % nkc, qb = (wi / nkc) % nqb, b = wi / (nkc * nqb);   // query block share its Q rows in one XCD's L2
    const int c0 = kc * XP_KC;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int qrow = qb * XA_QB + wave * 32 + r;
    const bf16_t* kbase = kv + ((size_t)b * Tk + c0) * ld_kv;

    auto stage_k = [&](int h, unsigned char* dst) {
        constexpr int ITERS = XP_KC * 8 / 256;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int rowb = it * 32 + wave * 8;
            const int row = rowb + (lane >> 3);
            const int lp = (lane & 7) ^ at_sw(row);
            XA_PLANES(NP,
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kbase + pl * 64 + (size_t)row * ld_kv + h * DH + lp * 8),
                                                 (RTTS_LDS void*)(dst + pl * PLANE + rowb * 128), 16, 0, 0););
        }
    };
    stage_k(0, smem);

    int* kval = reinterpret_cast<int*>(smem + 2 * NP * PLANE);  // key validity of the chunk (the head loop's first barrier publishes it)
    for (int j = tid; j < XP_KC; j += 256) kval[j] = kvalid ? (int)kvalid[(size_t)b * Tk + c0 + j] : 1;

    constexpr float kLog2e = 1.4426950408889634f;
    const float c = xa_dh<DH>::scale * kLog2e;                  // 1 / sqrt(DH), in the exp2 domain
    f32x16 acc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) acc[kt] = f32x16{0};
    const bf16_t* qptr = q + ((size_t)b * Tq + qrow) * ld_q;
#pragma unroll 1
    for (int h = 0; h < H; ++h) {
        bf16x8 qf[NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qptr + h * DH + ks * 16 + 8 * hh);
        const float l2 = lse[((size_t)b * H + h) * Tq + qrow] * kLog2e;
        __syncthreads();            // K of head h is in LDS, and every wave is done with the buffer head h - 1 read
        if (h + 1 < H) stage_k(h + 1, smem + ((h + 1) & 1) * (NP * PLANE));
        const unsigned char* Ks = smem + (h & 1) * (NP * PLANE);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            f32x16 s = {0};
            XA_PLANES(NP,
                _Pragma("unroll")
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + pl * PLANE + at_off(kt * 32 + r, ks * 2 + hh));
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[pl * 4 + ks], s, 0, 0, 0);
                });
            // exp(s / sqrt(DH) - lse) as one fma and v_exp_f32 (2^x); masked keys are zeroed at the store, whatever they sum to here
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[kt][i] += __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, -l2));
        }
    }

    const float inv_h = 1.f / (float)H;
    float* arow = a + ((size_t)b * Tq + qrow) * ld_a + c0 + 4 * hh;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int4 vv = *reinterpret_cast<const int4*>(kval + kt * 32 + 8 * g + 4 * hh);
            uint4 v;
            v.x = __float_as_uint(vv.x ? acc[kt][4 * g] * inv_h : 0.f);
            v.y = __float_as_uint(vv.y ? acc[kt][4 * g + 1] * inv_h : 0.f);
            v.z = __float_as_uint(vv.z ? acc[kt][4 * g + 2] * inv_h : 0.f);
            v.w = __float_as_uint(vv.w ? acc[kt][4 * g + 3] * inv_h : 0.f);
            rtts_store16_out(arow + kt * 32 + 8 * g, v);
        }
}

extern "C" int rtts_xattn_probs_mean(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid, const float* lse,
                                     int B, int H, int Tq, int Tk, int dh, float* a, int64_t ld_a, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(q && kv && lse && a, "rtts_xattn_probs_mean: q, kv, lse and a must not be NULL");
    if (xa_check("rtts_xattn_probs_mean", B, H, Tq, Tk, dh, ld_q, ld_kv)) return -1;
    RTTS_REQUIRE(ld_a >= Tk && ld_a % 4 == 0, "rtts_xattn_probs_mean: ld_a=%lld must be >= T_k=%d and a multiple of 4", (long long)ld_a, Tk);
    RTTS_REQUIRE((((uintptr_t)q | (uintptr_t)kv | (uintptr_t)a) & 15) == 0, "rtts_xattn_probs_mean: q, kv and a must be 16-byte aligned");
    const size_t nwg = (size_t)B * (Tq / XA_QB) * (Tk / XP_KC);
    RTTS_REQUIRE(nwg <= 0x7fffffff, "rtts_xattn_probs_mean: grid too large");
    const size_t lds = 2 * (size_t)XP_KC * (2 * dh) + XP_KC * 4;
    if (dh == 128) {
        RTTS_ENSURE_LDS("rtts_xattn_probs_mean", xattn_probs_mean_kernel<128>, lds, g_xp_lds);
        hipLaunchKernelGGL(xattn_probs_mean_kernel<128>, dim3((unsigned)nwg), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q, ld_q,
                           (const bf16_t*)kv, ld_kv, kvalid, lse, H, Tq, Tk, a, ld_a);
    } else {
        hipLaunchKernelGGL(xattn_probs_mean_kernel<64>, dim3((unsigned)nwg), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q, ld_q,
                           (const bf16_t*)kv, ld_kv, kvalid, lse, H, Tq, Tk, a, ld_a);
    }
    RTTS_LAUNCH_CHECK("rtts_xattn_probs_mean");
    return 0;
}

extern "C" int rtts_sum_slabs(const void* part, int nslabs, int64_t n, void* out, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(part && out && nslabs > 0 && n > 0 && n % 8 == 0, "rtts_sum_slabs: n must be a positive multiple of 8");
    size_t blocks = ((size_t)n / 8 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sum_slabs_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)part, nslabs,
                       (size_t)n / 8, (bf16_t*)out);
    RTTS_LAUNCH_CHECK("rtts_sum_slabs");
    return 0;
}
