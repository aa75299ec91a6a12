// Dense shared-QK attention, forward and backward: what reformer_pytorch's LSHSelfAttention computes when `use_full_attn` is set
// or T <= full_attn_thres (FullQKAttention; the layer is built at reference reformer_tts/model/reformer.py:198-217).
// Per (batch, head), rows qk_i, v_i of 64 bf16 in the [qk | v] layout the projection GEMM writes (common row stride ld):
//   s_ij = (qk_i . qk_j) / (8 max(|qk_j|, 1e-12));  s_ii = -5e4;  then s_ij = -FLT_MAX unless mask_i and mask_j;  then (causal)
//   s_ij = -FLT_MAX for j > i;  P = softmax_j(s);  o_i = sum_j P_ij keep_ij v_j.
// The fills are applied in THIS order, so a query with mask_i = 0 has every logit equal: P_ij = 1 / T over ALL T keys (padding,
// the diagonal and the causal future included) and o_i = mean(v).  The logit is taken as in lsh_attn_fwd.hip: the raw bf16 MFMA
// product times an fp32 column scale.
//
// One tile size everywhere: a workgroup of two waves owns 64 rows (lane = owner row, 32 per wave) and streams the other side in
// tiles of 64 rows through LDS (16 KB: two [64][128 B] images, swizzled like xattn.hip's), so T is not bounded by the chip.
//   forward      : owner = query.  S^T = K Q^T per tile, online softmax (running maximum and normaliser), O^T += V^T P^T.
//   backward (K) : owner = key.    Streams (q, dout, lse, delta) tiles: dV^T += dO^T P, G^T += Q^T dS; the key-role gradient
//                  (g - k^ (k^ . g)) / |k| goes to an fp32 workspace (B*H, T, 64), dV is final.
//   backward (Q) : owner = query.  Streams (k, v) tiles: dQ^T += K^T (dS * column scale); adds the workspace row and writes dqk.
// Both backward passes rebuild S and dP (7 MFMA products instead of 5) and in exchange need no partial slabs, no atomics and no
// reduce launch: every output row is written exactly once, by one lane pair, in a fixed order -- two runs are bit-identical.
// A query with mask_i = 0 has lse = -FLT_MAX (written exactly so by the forward): the backward never rebuilds its P from lse
// (exp(-FLT_MAX + FLT_MAX) would be 1) but takes P_ij = 1 / T and dS = 0; such rows still feed dV of every key, so a causal
// pass may skip the tiles beyond the diagonal only where they hold no such row.
// The backward kernels are held to two waves per SIMD (a few spilled registers in the dropout and causal key-pass variants), and
// a causal grid hands out the long blocks of a (batch, head) first: together 261 -> 182 us at B 12, H 8, T 1024.
#include "rtts_common.h"
#include "attn_tile.h"   // the swizzled [row][128 B] images (at_off) and the row staging of the epilogues (at_store_rows)
#include <float.h>

#define FA_TILE 64
#define FA_MAX_T 4096

// 64 rows of 64 bf16 (row stride ld) -> a swizzled [64][128 B] image, by LDS-DMA: one wave-instruction fills 8 rows in lane order,
// the swizzle goes on the source side.  128 threads.
__device__ __forceinline__ void fa_stage(unsigned char* img, const bf16_t* base, int64_t ld, int wave, int lane) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int rowb = it * 16 + wave * 8;
        const int row = rowb + (lane >> 3);
        const int lp = (lane & 7) ^ at_sw(row);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + (size_t)row * ld + lp * 8),
                                         (RTTS_LDS void*)(img + rowb * 128), 16, 0, 0);
    }
}
// column scale 1 / (8 max(|k|, 1e-12)) of 64 rows: two threads per row, 32 elements each (fixed order: every kernel gets the
// same bits for the same row)
__device__ __forceinline__ void fa_col_scale(float* cs, const bf16_t* base, int64_t ld, int tid) {
    const int row = tid >> 1, half = tid & 1;
    const uint4* p = reinterpret_cast<const uint4*>(base + (size_t)row * ld + half * 32);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 t = p[i];
        const uint32_t u[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = __uint_as_float(u[j] << 16), c = __uint_as_float(u[j] & 0xffff0000u);
            ss = __builtin_fmaf(a, a, ss);
            ss = __builtin_fmaf(c, c, ss);
        }
    }
    ss += __shfl_xor(ss, 1);
    if (half == 0) cs[row] = 0.125f * __builtin_amdgcn_rsqf(fmaxf(ss, 1e-24f));
}

// ------------------------------------------------------------------------------ forward
template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(128) void full_attn_fwd_kernel(const bf16_t* __restrict__ qk, const bf16_t* __restrict__ v, int64_t ld,
                                                            const uint8_t* __restrict__ mask, int H, int T, bf16_t* __restrict__ o,
                                                            int64_t ld_o, float* __restrict__ lse, uint32_t seed,
                                                            const uint32_t* __restrict__ seed_dev, uint32_t thresh, float dscale) {
    __shared__ __attribute__((aligned(16))) unsigned char Ks[FA_TILE * 128];
    __shared__ __attribute__((aligned(16))) unsigned char Vs[FA_TILE * 128];
    __shared__ __attribute__((aligned(16))) float cs[FA_TILE];
    __shared__ __attribute__((aligned(16))) int kvl[FA_TILE];

    const int nqb = T / FA_TILE;
    const uint32_t wi = xcd_remap(blockIdx.x, gridDim.x);
    // causal: a block's work grows with qb -- the long blocks of a (batch, head) are dispatched first, the short ones fill the tail
    const int bh = wi / nqb, qb = CAUSAL ? nqb - 1 - (int)(wi % nqb) : (int)(wi % nqb);
    const int b = bh / H, h = bh % H;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int qrow = qb * FA_TILE + wave * 32 + r;
    const bf16_t* qptr = qk + ((size_t)b * T + qrow) * ld + (size_t)h * 64;
    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qptr + ks * 16 + 8 * hh);
    const int qv = mask ? (int)(mask[(size_t)b * T + qrow] != 0) : 1;
    if (DROP && seed_dev) seed += seed_dev[0];
    // a causal block stops at its diagonal tile -- unless it holds a query with mask 0, whose row is the mean over all T keys
    int kend = T;
    if (CAUSAL) kend = __syncthreads_or(!qv) ? T : (qb + 1) * FA_TILE;

    float m_run = -FLT_MAX, l_run = 0.f;
    f32x16 oacc[2] = {};
    const int trq = (lane & 15) >> 2, trp = lane & 3, trc = (lane >> 4) & 1;
#pragma unroll 1
    for (int j0 = 0; j0 < kend; j0 += FA_TILE) {
        const bf16_t* kbase = qk + ((size_t)b * T + j0) * ld + (size_t)h * 64;
        const bf16_t* vbase = v + ((size_t)b * T + j0) * ld + (size_t)h * 64;
        if (j0) __syncthreads();            // every wave is done with the previous tile's images
        fa_stage(Ks, kbase, ld, wave, lane);
        fa_stage(Vs, vbase, ld, wave, lane);
        fa_col_scale(cs, kbase, ld, tid);
        if (tid < FA_TILE) kvl[tid] = mask ? (int)(mask[(size_t)b * T + j0 + tid] != 0) : 1;
        __syncthreads();

        f32x16 s[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f32x16 acc = {0};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + at_off(kt * 32 + r, ks * 2 + hh));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
            }
            s[kt] = acc;
        }
        float m = -FLT_MAX;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int4 kvv = *reinterpret_cast<const int4*>(kvl + kt * 32 + 8 * g + 4 * hh);
                const float4 c4 = *reinterpret_cast<const float4*>(cs + kt * 32 + 8 * g + 4 * hh);
                const int vv[4] = {kvv.x, kvv.y, kvv.z, kvv.w};
                const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = j0 + kt * 32 + 8 * g + 4 * hh + j;
                    // selects, not branches: (a) self, then (b) padding on either side and (c) the future overwrite it
                    const int live = qv & vv[j] & (CAUSAL ? (int)(key <= qrow) : 1);
                    float x = s[kt][4 * g + j] * cc[j];
                    x = key == qrow ? AT_SELF : x;
                    x = live ? x : -FLT_MAX;
                    s[kt][4 * g + j] = x;
                    m = fmaxf(m, x);
                }
            }
        m = fmaxf(rtts_xhalf_max(m), m_run);
        // m_run = -FLT_MAX while only filled logits were seen: they all count 1 (a row that stays so is the uniform row of a
        // masked query); the first finite logit gives alpha = exp(-FLT_MAX - m) = 0 and wipes them
        const float alpha = __expf(m_run - m);
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = __expf(s[kt][i] - m);
                s[kt][i] = p;
                l += p;
            }
        l_run = l_run * alpha + rtts_xhalf_sum(l);
        m_run = m;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
        if (DROP) {
            const uint32_t base = ((uint32_t)bh * (uint32_t)T + (uint32_t)qrow) * (uint32_t)T + (uint32_t)j0;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    s[kt][i] *= rtts_drop_keep(seed, base + (uint32_t)(kt * 32 + 8 * (i >> 2) + 4 * hh + (i & 3)), thresh, dscale);
        }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int o8 = 8 * s2;
                const bf16x8 pf = cvt_bf16x8(s[kt][o8], s[kt][o8 + 1], s[kt][o8 + 2], s[kt][o8 + 3], s[kt][o8 + 4], s[kt][o8 + 5],
                                             s[kt][o8 + 6], s[kt][o8 + 7]);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const int blk = (kt * 32 + 16 * s2) * 128;
                    const int t0 = at_off(4 * hh + trq, dt * 4 + 2 * trc + (trp >> 1)) + 8 * (trp & 1);
                    const int t1 = at_off(4 * hh + trq, (dt ^ 1) * 4 + 2 * trc + (trp >> 1)) + 8 * (trp & 1);   // row + 8: sw flips bit 2
                    const bf16x8 vf = rtts_tr_frag(Vs + blk + t0, Vs + blk + 8 * 128 + t1);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, oacc[dt], 0, 0, 0);
                }
            }
    }
    const float inv_l = 1.f / l_run;
    __syncthreads();                 // the K image becomes the waves' row staging (4 KB each)
    at_store_rows(Ks + wave * 4096, oacc, inv_l, o + ((size_t)b * T + qb * FA_TILE + wave * 32) * ld_o + (size_t)h * 64, ld_o, lane);
    if (hh == 0) lse[(size_t)bh * T + qrow] = (m_run == -FLT_MAX) ? -FLT_MAX : m_run + logf(l_run);
}

// ------------------------------------------------------------------------------ backward
// KEYPASS: owner rows are keys, the streamed tiles are queries (images: q rows, dout rows).  Otherwise owner rows are queries and
// the streamed tiles are keys (images: k rows, v rows).  In both the products are laid out [streamed row in registers][owner in
// the lane], as in xattn.hip's backward: register 4 g + j of lane (r, hh) = streamed row 8 g + 4 hh + j of a 32-row sub-tile.
template <bool KEYPASS, bool CAUSAL, bool DROP>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) void full_attn_bwd_kernel(const bf16_t* __restrict__ qk, const bf16_t* __restrict__ v, int64_t ld,
                                                            const uint8_t* __restrict__ mask, const bf16_t* __restrict__ dout,
                                                            int64_t ld_do, const float* __restrict__ lse, const float* __restrict__ delta,
                                                            int H, int T, bf16_t* __restrict__ dst, int64_t ld_d, float* __restrict__ ws,
                                                            uint32_t seed, const uint32_t* __restrict__ seed_dev, uint32_t thresh,
                                                            float dscale) {
    __shared__ __attribute__((aligned(16))) unsigned char X1[FA_TILE * 128];     // streamed qk rows
    __shared__ __attribute__((aligned(16))) unsigned char X2[FA_TILE * 128];     // streamed dout (KEYPASS) / v rows
    __shared__ __attribute__((aligned(16))) float sa[FA_TILE];                   // KEYPASS: lse of the streamed queries; else column scale
    __shared__ __attribute__((aligned(16))) float sb[FA_TILE];                   // KEYPASS: delta of the streamed queries; else the owners' scale scratch
    __shared__ __attribute__((aligned(16))) int svl[FA_TILE];                    // validity of the streamed rows

    const int nb = T / FA_TILE;
    const uint32_t wi = xcd_remap(blockIdx.x, gridDim.x);
    // causal: a key block's work shrinks with ob, a query block's grows: the long blocks of a (batch, head) go first
    const int bh = wi / nb, ob = (CAUSAL && !KEYPASS) ? nb - 1 - (int)(wi % nb) : (int)(wi % nb);
    const int b = bh / H, h = bh % H;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int own = ob * FA_TILE + wave * 32 + r;
    const size_t rowoff = ((size_t)b * T + own) * ld + (size_t)h * 64;
    if (DROP && seed_dev) seed += seed_dev[0];
    const float inv_t = 1.f / (float)T;

    bf16x8 a1[4], a2[4];
    {
        const bf16_t* p1 = qk + rowoff;
        const bf16_t* p2 = KEYPASS ? v + rowoff : dout + ((size_t)b * T + own) * ld_do + (size_t)h * 64;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            a1[ks] = *reinterpret_cast<const bf16x8*>(p1 + ks * 16 + 8 * hh);
            a2[ks] = *reinterpret_cast<const bf16x8*>(p2 + ks * 16 + 8 * hh);
        }
    }
    const int ov = mask ? (int)(mask[(size_t)b * T + own] != 0) : 1;
    float o_cs = 0.f, o_lse = 0.f, o_del = 0.f;
    if (KEYPASS) {
        fa_col_scale(sb, qk + ((size_t)b * T + ob * FA_TILE) * ld + (size_t)h * 64, ld, tid);
        __syncthreads();
        o_cs = sb[wave * 32 + r];
        __syncthreads();
    } else {
        o_lse = lse[(size_t)bh * T + own];
        o_del = delta[(size_t)bh * T + own];
    }

    f32x16 acc1[2] = {}, acc2[2] = {};      // KEYPASS: dV^T, G^T; else dQ^T (acc2 unused)
    const int trq = (lane & 15) >> 2, trp = lane & 3, trc = (lane >> 4) & 1;
    int fro[4], tro[2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fro[ks] = at_off(r, ks * 2 + hh);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) tro[dt] = at_off(4 * hh + trq, dt * 4 + 2 * trc + (trp >> 1)) + 8 * (trp & 1);

    // causal: a key block meets the queries from its own tile on (and earlier tiles only where they hold a masked query, whose
    // uniform row feeds dV of every key); a query block meets the keys up to its own tile
    const int tend = (!KEYPASS && CAUSAL) ? (ob + 1) * FA_TILE : T;
    bool staged = false;
#pragma unroll 1
    for (int t0 = 0; t0 < tend; t0 += FA_TILE) {
        if (KEYPASS && CAUSAL && t0 < ob * FA_TILE) {
            if (!mask) continue;
            const int bad = tid < FA_TILE ? !mask[(size_t)b * T + t0 + tid] : 0;
            if (!__syncthreads_or(bad)) continue;
        }
        const size_t toff = ((size_t)b * T + t0) * ld + (size_t)h * 64;
        if (staged) __syncthreads();
        staged = true;
        fa_stage(X1, qk + toff, ld, wave, lane);
        if (KEYPASS) {
            fa_stage(X2, dout + ((size_t)b * T + t0) * ld_do + (size_t)h * 64, ld_do, wave, lane);
            if (tid < FA_TILE) {
                sa[tid] = lse[(size_t)bh * T + t0 + tid];
                sb[tid] = delta[(size_t)bh * T + t0 + tid];
            }
        } else {
            fa_stage(X2, v + toff, ld, wave, lane);
            fa_col_scale(sa, qk + toff, ld, tid);
        }
        if (tid < FA_TILE) svl[tid] = mask ? (int)(mask[(size_t)b * T + t0 + tid] != 0) : 1;
        __syncthreads();

#pragma unroll
        for (int st = 0; st < 2; ++st) {
            f32x16 sacc = {0}, pacc = {0};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(X1 + st * (32 * 128) + fro[ks]);
                const bf16x8 x2 = *reinterpret_cast<const bf16x8*>(X2 + st * (32 * 128) + fro[ks]);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1, a1[ks], sacc, 0, 0, 0);
                pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2, a2[ks], pacc, 0, 0, 0);
            }
            float pp[16], ds[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int s0 = st * 32 + 8 * g + 4 * hh;
                const float4 a4 = *reinterpret_cast<const float4*>(sa + s0);
                const float4 b4 = *reinterpret_cast<const float4*>(sb + s0);
                const int4 v4 = *reinterpret_cast<const int4*>(svl + s0);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
                const int vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 4 * g + j;
                    const int srow = t0 + s0 + j;
                    const int qi = KEYPASS ? srow : own, kj = KEYPASS ? own : srow;
                    const int vq = KEYPASS ? vv[j] : ov, vk = KEYPASS ? ov : vv[j];
                    const float l_i = KEYPASS ? av[j] : o_lse, d_i = KEYPASS ? bv[j] : o_del, c_j = KEYPASS ? o_cs : av[j];
                    const float keep = DROP ? rtts_drop_keep(seed, ((uint32_t)bh * (uint32_t)T + (uint32_t)qi) * (uint32_t)T + (uint32_t)kj,
                                                             thresh, dscale)
                                            : 1.f;
                    // selects, not branches.  A filled pair of a valid query: P = 0 (the -5e4 diagonal: P = exp(-5e4 - lse), 1 for a row
                    // with nothing else) and no gradient; a masked query: uniform over all T keys, no logit depends on qk (its
                    // lse = -FLT_MAX would rebuild P = inf or 1: whatever the exp gives is discarded by the select)
                    const int live = vk & (CAUSAL ? (int)(kj <= qi) : 1);
                    const float sl = qi == kj ? AT_SELF : sacc[i] * c_j;
                    float p = __expf(sl - l_i);
                    p = live ? p : 0.f;
                    float dsv = (live & (int)(qi != kj)) ? p * (pacc[i] * keep - d_i) : 0.f;
                    p = vq ? p : inv_t;
                    dsv = vq ? dsv : 0.f;
                    pp[i] = p * keep;
                    ds[i] = KEYPASS ? dsv : dsv * c_j;           // query role: dS_ij k_j / (8 |k_j|)
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const float* dq_ = ds + 8 * s2;
                const bf16x8 db = cvt_bf16x8(dq_[0], dq_[1], dq_[2], dq_[3], dq_[4], dq_[5], dq_[6], dq_[7]);
                const int blk = (st * 32 + 16 * s2) * 128;
                if (KEYPASS) {
                    const float* pq = pp + 8 * s2;
                    const bf16x8 pb = cvt_bf16x8(pq[0], pq[1], pq[2], pq[3], pq[4], pq[5], pq[6], pq[7]);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const bf16x8 dotf = rtts_tr_frag(X2 + blk + tro[dt], X2 + blk + 8 * 128 + tro[dt ^ 1]);
                        const bf16x8 qtf = rtts_tr_frag(X1 + blk + tro[dt], X1 + blk + 8 * 128 + tro[dt ^ 1]);
                        acc1[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf, pb, acc1[dt], 0, 0, 0);
                        acc2[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, db, acc2[dt], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const bf16x8 ktf = rtts_tr_frag(X1 + blk + tro[dt], X1 + blk + 8 * 128 + tro[dt ^ 1]);
                        acc1[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf, db, acc1[dt], 0, 0, 0);
                    }
                }
            }
        }
    }

    // workspace row of the owner: fp32 (B*H, T, 64); lane (r, hh) holds dh = 32 dt + 8 g + 4 hh + {0..3}
    float* wrow = ws + ((size_t)bh * T + own) * 64;
    if (KEYPASS) {
        // key role through the normalisation: (g - k^ (k^ . g)) / max(|k|, 1e-12), g = G / 8, k^ = k / max(|k|, 1e-12)
        const float inv_n = o_cs * 8.f;
        const bf16_t* kp = qk + rowoff;
        float kh[2][16];
        float dot = 0.f;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint2 u = *reinterpret_cast<const uint2*>(kp + 32 * dt + 8 * g + 4 * hh);
                kh[dt][4 * g] = __uint_as_float(u.x << 16) * inv_n;
                kh[dt][4 * g + 1] = __uint_as_float(u.x & 0xffff0000u) * inv_n;
                kh[dt][4 * g + 2] = __uint_as_float(u.y << 16) * inv_n;
                kh[dt][4 * g + 3] = __uint_as_float(u.y & 0xffff0000u) * inv_n;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc2[dt][4 * g + j] *= 0.125f;
                    dot = __builtin_fmaf(kh[dt][4 * g + j], acc2[dt][4 * g + j], dot);
                }
            }
        dot = rtts_xhalf_sum(dot);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 w;
                w.x = (acc2[dt][4 * g] - kh[dt][4 * g] * dot) * inv_n;
                w.y = (acc2[dt][4 * g + 1] - kh[dt][4 * g + 1] * dot) * inv_n;
                w.z = (acc2[dt][4 * g + 2] - kh[dt][4 * g + 2] * dot) * inv_n;
                w.w = (acc2[dt][4 * g + 3] - kh[dt][4 * g + 3] * dot) * inv_n;
                *reinterpret_cast<float4*>(wrow + 32 * dt + 8 * g + 4 * hh) = w;
            }
    } else {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 w = *reinterpret_cast<const float4*>(wrow + 32 * dt + 8 * g + 4 * hh);
                acc1[dt][4 * g] += w.x;
                acc1[dt][4 * g + 1] += w.y;
                acc1[dt][4 * g + 2] += w.z;
                acc1[dt][4 * g + 3] += w.w;
            }
    }
    __syncthreads();                 // the first image becomes the waves' row staging (4 KB each)
    at_store_rows(X1 + wave * 4096, acc1, 1.f, dst + ((size_t)b * T + ob * FA_TILE + wave * 32) * ld_d + (size_t)h * 64, ld_d, lane);
}

// ------------------------------------------------------------------------------ entry points
extern "C" int rtts_full_attn_max_t(int dh) { return dh == 64 ? FA_MAX_T : -1; }

static int fa_check(const char* fn, int B, int H, int T, int dh, int64_t ld) {
    RTTS_REQUIRE(dh == 64, "%s: dh=%d unsupported (this build: 64)", fn, dh);
    RTTS_REQUIRE(T >= FA_TILE && T % FA_TILE == 0 && T <= FA_MAX_T, "%s: T=%d unsupported (a multiple of 64 from 64 to %d)", fn, T, FA_MAX_T);
    RTTS_REQUIRE(B > 0 && H > 0 && (int64_t)B * H * (T / FA_TILE) <= 0x7fffffff, "%s: bad B/H", fn);
    RTTS_REQUIRE(ld >= (int64_t)H * dh && ld % 8 == 0, "%s: row stride ld=%lld must be >= H*dh and a multiple of 8", fn, (long long)ld);
    return 0;
}

extern "C" int rtts_full_attn_fwd(const void* qk, const void* v, int64_t ld, const uint8_t* mask, int B, int H, int T, int dh, int causal,
                                  void* out, int64_t ld_out, float* lse, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev,
                                  void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(qk && v && out && lse && drop_p >= 0.f && drop_p < 1.f, "rtts_full_attn_fwd: bad arguments (qk, v, out and lse must not be NULL)");
    if (fa_check("rtts_full_attn_fwd", B, H, T, dh, ld)) return -1;
    RTTS_REQUIRE(ld_out >= (int64_t)H * dh && ld_out % 8 == 0, "rtts_full_attn_fwd: bad ld_out");
    RTTS_REQUIRE((((uintptr_t)qk | (uintptr_t)v | (uintptr_t)out) & 15) == 0, "rtts_full_attn_fwd: buffers must be 16-byte aligned");
    const dim3 grid((unsigned)(B * H * (T / FA_TILE)));
    const uint32_t thresh = rtts_drop_thresh(drop_p);
#define GO(C_, D_)                                                                                                                 \
    hipLaunchKernelGGL((full_attn_fwd_kernel<C_, D_>), grid, dim3(128), 0, (hipStream_t)stream, (const bf16_t*)qk, (const bf16_t*)v, ld, \
                       mask, H, T, (bf16_t*)out, ld_out, lse, drop_seed, seed_dev, thresh, 1.f / (1.f - drop_p))
    if (causal) { if (thresh) GO(true, true); else GO(true, false); }
    else { if (thresh) GO(false, true); else GO(false, false); }
#undef GO
    RTTS_LAUNCH_CHECK("rtts_full_attn_fwd");
    return 0;
}

extern "C" int64_t rtts_full_attn_bwd_workspace(int B, int H, int T, int dh) {
    if (dh != 64 || B <= 0 || H <= 0 || T < FA_TILE || T % FA_TILE || T > FA_MAX_T) return -1;
    return (int64_t)B * H * T * dh * 4;
}

extern "C" int rtts_full_attn_bwd(const void* qk, const void* v, int64_t ld, const uint8_t* mask, const void* dout, int64_t ld_dout,
                                  const float* lse, const float* delta, int B, int H, int T, int dh, int causal, void* dqk, void* dv,
                                  int64_t ld_d, void* workspace, float drop_p, uint32_t drop_seed, const uint32_t* seed_dev, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(qk && v && dout && lse && delta && dqk && dv && workspace && drop_p >= 0.f && drop_p < 1.f,
                 "rtts_full_attn_bwd: bad arguments (no pointer but mask and seed_dev may be NULL)");
    if (fa_check("rtts_full_attn_bwd", B, H, T, dh, ld)) return -1;
    RTTS_REQUIRE(ld_dout >= (int64_t)H * dh && ld_dout % 8 == 0 && ld_d >= (int64_t)H * dh && ld_d % 8 == 0, "rtts_full_attn_bwd: bad strides");
    RTTS_REQUIRE((((uintptr_t)qk | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)dqk | (uintptr_t)dv | (uintptr_t)workspace) & 15) == 0,
                 "rtts_full_attn_bwd: buffers must be 16-byte aligned");
    const dim3 grid((unsigned)(B * H * (T / FA_TILE)));
    const uint32_t thresh = rtts_drop_thresh(drop_p);
#define GO(K_, C_, D_, DST_)                                                                                                       \
    hipLaunchKernelGGL((full_attn_bwd_kernel<K_, C_, D_>), grid, dim3(128), 0, (hipStream_t)stream, (const bf16_t*)qk, (const bf16_t*)v, \
                       ld, mask, (const bf16_t*)dout, ld_dout, lse, delta, H, T, (bf16_t*)(DST_), ld_d, (float*)workspace, drop_seed,    \
                       seed_dev, thresh, 1.f / (1.f - drop_p))
#define GO2(K_, DST_)                                                                  \
    do {                                                                               \
        if (causal) { if (thresh) GO(K_, true, true, DST_); else GO(K_, true, false, DST_); }   \
        else { if (thresh) GO(K_, false, true, DST_); else GO(K_, false, false, DST_); }        \
    } while (0)
    GO2(true, dv);          // dV, key-role rows -> workspace
    RTTS_LAUNCH_CHECK("rtts_full_attn_bwd");
    GO2(false, dqk);        // query role + workspace -> dqk
#undef GO2
#undef GO
    RTTS_LAUNCH_CHECK("rtts_full_attn_bwd");
    return 0;
}
