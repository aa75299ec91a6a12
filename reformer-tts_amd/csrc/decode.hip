// Single-query attention for incremental generation: one new decoder position per utterance against what earlier positions left
// behind.  Two entry points, one kernel template in two modes:
//   self  (rtts_decode_self_attn) : row p of full_attn.hip's causal forward with every position valid.  The new [qk | v] row is
//                                   appended to a (B, cap, 2*H*64) cache at the DEVICE position p = *pos and attends to the p rows
//                                   already there:  s_j = (q . k_j) / (8 max(|k_j|, 1e-12)) for j < p, s_p = -5e4, softmax over
//                                   j <= p, o = sum_j P_j v_j.  Key and value of position p come from the row itself, never from
//                                   the cache, so nothing depends on when the append lands.
//   cross (rtts_decode_cross_attn): one query per (batch, head) against the projected encoder keys, s_j = q . k_j / sqrt(dh),
//                                   keys with kvalid = 0 skipped (P exactly 0), a sample without any valid key gets o = NaN.
// M = 1 leaves the matrix pipe nothing to do: these are VALU kernels bounded by the HBM read of the keys and values.  A key row
// (dh bf16) is read by dh / 8 neighbouring lanes, 16 bytes each, straight to registers; the lanes of a key share its dot product by
// three or four shuffles and each keeps the running maximum, the normaliser and 8 fp32 accumulator columns of ITS keys (P and the
// P V sum stay in fp32).  A workgroup of four waves folds its 32 (dh 64) or 16 (dh 128) lane groups through LDS in a fixed order.
// SPLITS.  B * H is 8 at batch 1 for 256 compute units, so a (batch, head) is worked by `splits` workgroups: key tiles of 64 are
// dealt round-robin (split s takes tiles s, s + S, ...: balanced for every p without the host knowing p), every split leaves
// (maximum, normaliser, dh accumulators) in an fp32 workspace and a second small launch folds them in split order.  A split that
// got no key leaves (-FLT_MAX, 0, 0...), which the fold weighs with exactly 0.  No atomics: two calls give the same bits.
// The position is read on the device, so ONE captured launch serves every frame; p outside [0, cap) writes nothing to the cache
// and sets every o to NaN.
#include "rtts_common.h"
#include "attn_tile.h"   // AT_SELF
#include <float.h>

#define DA_TILE 64
#define DA_THREADS 256
#define DA_MAX_SPLITS 64
#define DA_MAX_T 4096
#define DA_HDR 4                       // floats in front of a partial's accumulators: running maximum, normaliser, two unused
#define DA_NAN2 0x7fc07fc0u            // two bf16 NaN

// columns c0, c0 + 1 of one (batch, head): `n` partials (maximum, normaliser, accumulators) at `part`, `stride` floats apart, folded
// in index order
__device__ __forceinline__ void da_fold(const float* part, int stride, int n, int c0, float& M, float& L, float& a0, float& a1) {
    M = -FLT_MAX;
    for (int i = 0; i < n; ++i) M = fmaxf(M, part[(size_t)i * stride]);
    L = 0.f, a0 = 0.f, a1 = 0.f;
    for (int i = 0; i < n; ++i) {
        const float* pi = part + (size_t)i * stride;
        const float w = __expf(pi[0] - M);         // an empty partial: exp(-FLT_MAX - M) = 0, or 1 times its zeros when all are empty
        L = __builtin_fmaf(pi[1], w, L);
        a0 = __builtin_fmaf(pi[DA_HDR + c0], w, a0);
        a1 = __builtin_fmaf(pi[DA_HDR + c0 + 1], w, a1);
    }
}

__device__ __forceinline__ void da_store_o(bf16_t* o, int c0, float L, float a0, float a1) {
    // L = 0: no key at all (cross mode, kvalid all 0) -> NaN, as rtts_xattn_fwd documents
    const float inv = 1.f / L;
    *reinterpret_cast<uint32_t*>(o + c0) = L > 0.f ? pack_bf16x2(a0 * inv, a1 * inv) : DA_NAN2;
}

template <int DH, bool SELF>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_kernel(const bf16_t* __restrict__ q, int64_t ld_q, const bf16_t* kv, int64_t ld_kv,
                                                                 int64_t kv_batch_stride, bf16_t* cache, const uint8_t* __restrict__ kvalid,
                                                                 const int32_t* __restrict__ pos, int H, int T, bf16_t* __restrict__ o,
                                                                 int64_t ld_o, int splits, float* __restrict__ ws) {
    constexpr int LPK = DH / 8;                 // lanes per key
    constexpr int GPW = 64 / LPK;               // keys of a wave per pass
    constexpr int KPP = 4 * GPW;                // keys of the workgroup per pass = its lane groups
    constexpr int NPASS = DA_TILE / KPP;
    constexpr int PS = DH + DA_HDR;             // floats of one partial
    __shared__ __attribute__((aligned(16))) float part[KPP * PS];

    const int bh = blockIdx.x / splits, s = blockIdx.x % splits;
    const int b = bh / H, h = bh % H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane % LPK, g = lane / LPK;
    bf16_t* orow = o + (size_t)b * ld_o + (size_t)h * DH;

    int n = T, p = 0;
    if (SELF) {
        p = pos[0];
        if (p < 0 || p >= T) {                  // outside the cache: nothing is appended, o = NaN (written by the fold when there is one)
            if (splits == 1 && tid < DH / 2) *reinterpret_cast<uint32_t*>(orow + 2 * tid) = DA_NAN2;
            return;
        }
        n = p;
    }
    const bf16_t* qrow = q + (size_t)b * ld_q + (size_t)h * DH;
    const bf16_t* kb = kv + (size_t)b * kv_batch_stride + (size_t)h * DH + li * 8;
    const size_t voff = (size_t)H * DH;
    if (SELF && s == 0 && tid < 16) {           // the append: this head's 128 bytes of qk and of v, once
        const size_t off = (size_t)(tid >> 3) * voff + (size_t)h * DH + (tid & 7) * 8;
        *reinterpret_cast<uint4*>(cache + (size_t)b * kv_batch_stride + (size_t)p * ld_kv + off) =
            *reinterpret_cast<const uint4*>(q + (size_t)b * ld_q + off);
    }
    float qf[8];
    rtts_unpack8(*reinterpret_cast<const uint4*>(qrow + li * 8), qf);
    const float scale = DH == 64 ? 0.125f : 0.08838834764831845f;

    float m = -FLT_MAX, l = 0.f, acc[8] = {};
#pragma unroll 1
    for (int t = s; t * DA_TILE < n; t += splits) {
        uint4 kk[NPASS], vv[NPASS];
        bool live[NPASS];
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int j = t * DA_TILE + i * KPP + wave * GPW + g;
            live[i] = j < n && (SELF || !kvalid || kvalid[(size_t)b * T + j] != 0);
            kk[i] = vv[i] = uint4{0, 0, 0, 0};
            if (live[i]) {                       // rows at or beyond n are never read
                kk[i] = *reinterpret_cast<const uint4*>(kb + (size_t)j * ld_kv);
                vv[i] = *reinterpret_cast<const uint4*>(kb + (size_t)j * ld_kv + voff);
            }
        }
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            float kf[8], vf[8];
            rtts_unpack8(kk[i], kf);
            rtts_unpack8(vv[i], vf);
            float dot = 0.f, ss = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                dot = __builtin_fmaf(qf[c], kf[c], dot);
                if (SELF) ss = __builtin_fmaf(kf[c], kf[c], ss);
            }
#pragma unroll
            for (int sh = 1; sh < LPK; sh <<= 1) {
                dot += __shfl_xor(dot, sh);
                if (SELF) ss += __shfl_xor(ss, sh);
            }
            const float x = SELF ? dot * (0.125f * __builtin_amdgcn_rsqf(fmaxf(ss, 1e-24f))) : dot * scale;
            // selects, not branches: a key that is not live leaves (m, l, acc) as they are
            const float mn = live[i] ? fmaxf(m, x) : m;
            const float alpha = __expf(m - mn);
            const float pr = live[i] ? __expf(x - mn) : 0.f;
            l = __builtin_fmaf(l, alpha, pr);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = __builtin_fmaf(acc[c], alpha, pr * vf[c]);
            m = mn;
        }
    }
    float* mine = part + (wave * GPW + g) * PS;
    if (li == 0) {
        mine[0] = m;
        mine[1] = l;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) mine[DA_HDR + li * 8 + c] = acc[c];
    __syncthreads();
    if (tid >= DH / 2) return;
    const int c0 = 2 * tid;
    float M, L, a0, a1;
    da_fold(part, PS, KPP, c0, M, L, a0, a1);
    if (SELF && s == 0) {                        // position p itself: logit -5e4, value from the new row
        const uint32_t u = *reinterpret_cast<const uint32_t*>(q + (size_t)b * ld_q + voff + (size_t)h * DH + c0);
        const float mn = fmaxf(M, AT_SELF);
        const float alpha = __expf(M - mn), pr = __expf(AT_SELF - mn);
        L = __builtin_fmaf(L, alpha, pr);
        a0 = __builtin_fmaf(a0, alpha, pr * __uint_as_float(u << 16));
        a1 = __builtin_fmaf(a1, alpha, pr * __uint_as_float(u & 0xffff0000u));
        M = mn;
    }
    if (splits == 1) {
        da_store_o(orow, c0, L, a0, a1);
        return;
    }
    float* wr = ws + ((size_t)bh * splits + s) * PS;
    if (tid == 0) {
        wr[0] = M;
        wr[1] = L;
    }
    *reinterpret_cast<float2*>(wr + DA_HDR + c0) = float2{a0, a1};
}

template <int DH, bool SELF>
__global__ __launch_bounds__(64) void decode_attn_fold_kernel(const float* __restrict__ ws, const int32_t* __restrict__ pos, int H, int T,
                                                              bf16_t* __restrict__ o, int64_t ld_o, int splits) {
    const int bh = blockIdx.x, tid = threadIdx.x;
    if (tid >= DH / 2) return;
    const int c0 = 2 * tid;
    bf16_t* orow = o + (size_t)(bh / H) * ld_o + (size_t)(bh % H) * DH;
    if (SELF) {
        const int p = pos[0];
        if (p < 0 || p >= T) {                  // the splits wrote nothing
            *reinterpret_cast<uint32_t*>(orow + c0) = DA_NAN2;
            return;
        }
    }
    float M, L, a0, a1;
    da_fold(ws + (size_t)bh * splits * (DH + DA_HDR), DH + DA_HDR, splits, c0, M, L, a0, a1);
    da_store_o(orow, c0, L, a0, a1);
}

// im2col rows of the postnet tail (model/incremental.py).  The window is the R = 2 n + 1 positions p - (R - 1) ... p of one
// utterance (n convolutions, window index w <-> position a = p - (R - 1) + w); layer k reads window rows >= 2 k and writes rows
// >= 2 k + 2.  dst row b * nr + i (window row r = r0 + i), tap t, channel c  =  src at window row w = r + t - 2, or zero where the
// row is absent: w outside the window (beyond p: the sequence ends there) or a < 0 (in front of the first frame), at EVERY layer.
// src: abs = 1, fp32 (B, cap, C) indexed by the position a (the mel history); abs = 0, bf16 plain rows (b * src_nr + w - src_r0).
__global__ __launch_bounds__(256) void decode_tail_im2col_kernel(const void* __restrict__ src, int src_abs, int64_t ld_src,
                                                                 int64_t src_batch_stride, int src_r0, int C, const int32_t* __restrict__ pos,
                                                                 int cap, int R, int r0, int nr, int CP, bf16_t* __restrict__ dst, int64_t total8) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total8) return;
    const int per_tap = CP / 8, per_row = 5 * per_tap;
    const int row = (int)(idx / per_row), rem = (int)(idx % per_row);
    const int tap = rem / per_tap, c = (rem % per_tap) * 8;
    const int b = row / nr, w = r0 + row % nr + tap - 2;
    const int p = pos[0];
    const int a = p - (R - 1) + w;
    const bool ok = p >= 0 && p < cap && w >= 0 && w < R && a >= 0 && c < C && (src_abs || w >= src_r0);
    uint4 out = {0, 0, 0, 0};
    if (ok) {
        if (src_abs) {
            const float* sp = reinterpret_cast<const float*>(src) + (size_t)b * src_batch_stride + (size_t)a * ld_src + c;
            const float4 x0 = *reinterpret_cast<const float4*>(sp), x1 = *reinterpret_cast<const float4*>(sp + 4);
            out = uint4{pack_bf16x2(x0.x, x0.y), pack_bf16x2(x0.z, x0.w), pack_bf16x2(x1.x, x1.y), pack_bf16x2(x1.z, x1.w)};
        } else {
            out = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(src) + (size_t)b * src_batch_stride +
                                                  (size_t)(w - src_r0) * ld_src + c);
        }
    }
    *reinterpret_cast<uint4*>(dst + (size_t)row * (5 * CP) + (size_t)tap * CP + c) = out;
}

// ------------------------------------------------------------------------------ entry points
extern "C" int rtts_decode_attn_splits(int BH, int T) {
    if (BH <= 0 || T < DA_TILE || T % DA_TILE || T > DA_MAX_T) return -1;
    // about two workgroups per compute unit, never more splits than key tiles
    int s = 512 / BH;
    const int tiles = T / DA_TILE;
    s = s > tiles ? tiles : s;
    s = s > DA_MAX_SPLITS ? DA_MAX_SPLITS : s;
    return s < 1 ? 1 : s;
}

extern "C" int64_t rtts_decode_attn_workspace(int BH, int splits, int dh) {
    if (BH <= 0 || splits < 1 || splits > DA_MAX_SPLITS || (dh != 64 && dh != 128)) return -1;
    return (int64_t)BH * splits * (dh + DA_HDR) * 4;
}

static int da_common(const char* fn, int B, int H, int T, int& splits, const void* workspace) {
    RTTS_REQUIRE(B > 0 && H > 0 && (int64_t)B * H * DA_MAX_SPLITS <= 0x7fffffff, "%s: bad B/H", fn);
    RTTS_REQUIRE(splits >= 0 && splits <= DA_MAX_SPLITS, "%s: splits=%d unsupported (0 = the library's pick, else 1 to %d)", fn, splits, DA_MAX_SPLITS);
    if (splits == 0) splits = rtts_decode_attn_splits(B * H, T);
    RTTS_REQUIRE(splits == 1 || (workspace && ((uintptr_t)workspace & 15) == 0),
                 "%s: workspace must not be NULL (16-byte aligned, rtts_decode_attn_workspace bytes) with more than one split", fn);
    return 0;
}

extern "C" int rtts_decode_self_attn(const void* row, int64_t ld_row, void* cache, int64_t ld_cache, int64_t cache_batch_stride,
                                     const int32_t* pos, int B, int H, int cap, int dh, void* o, int64_t ld_o, int splits, void* workspace,
                                     void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(row && cache && pos && o, "rtts_decode_self_attn: row, cache, pos and o must not be NULL");
    RTTS_REQUIRE(dh == 64, "rtts_decode_self_attn: dh=%d unsupported (this build: 64)", dh);
    RTTS_REQUIRE(cap >= DA_TILE && cap % DA_TILE == 0 && cap <= rtts_full_attn_max_t(64),
                 "rtts_decode_self_attn: cap=%d unsupported (a multiple of 64 from 64 to %d)", cap, rtts_full_attn_max_t(64));
    if (da_common("rtts_decode_self_attn", B, H, cap, splits, workspace)) return -1;
    const int64_t wide = 2 * (int64_t)H * dh;
    RTTS_REQUIRE(ld_row >= wide && ld_row % 8 == 0, "rtts_decode_self_attn: ld_row=%lld must be >= 2*H*dh and a multiple of 8", (long long)ld_row);
    RTTS_REQUIRE(ld_cache >= wide && ld_cache % 8 == 0, "rtts_decode_self_attn: ld_cache=%lld must be >= 2*H*dh and a multiple of 8", (long long)ld_cache);
    RTTS_REQUIRE(cache_batch_stride >= (int64_t)cap * ld_cache && cache_batch_stride % 8 == 0,
                 "rtts_decode_self_attn: cache_batch_stride=%lld must be >= cap*ld_cache and a multiple of 8", (long long)cache_batch_stride);
    RTTS_REQUIRE(ld_o >= (int64_t)H * dh && ld_o % 2 == 0, "rtts_decode_self_attn: ld_o=%lld must be >= H*dh and even", (long long)ld_o);
    RTTS_REQUIRE((((uintptr_t)row | (uintptr_t)cache) & 15) == 0 && ((uintptr_t)o & 3) == 0 && ((uintptr_t)pos & 3) == 0,
                 "rtts_decode_self_attn: row and cache must be 16-byte aligned, o and pos 4-byte aligned");
    hipLaunchKernelGGL((decode_attn_kernel<64, true>), dim3((unsigned)(B * H * splits)), dim3(DA_THREADS), 0, (hipStream_t)stream,
                       (const bf16_t*)row, ld_row, (const bf16_t*)cache, ld_cache, cache_batch_stride, (bf16_t*)cache, (const uint8_t*)nullptr, pos, H,
                       cap, (bf16_t*)o, ld_o, splits, (float*)workspace);
    RTTS_LAUNCH_CHECK("rtts_decode_self_attn");
    if (splits > 1) {
        hipLaunchKernelGGL((decode_attn_fold_kernel<64, true>), dim3((unsigned)(B * H)), dim3(64), 0, (hipStream_t)stream,
                           (const float*)workspace, pos, H, cap, (bf16_t*)o, ld_o, splits);
        RTTS_LAUNCH_CHECK("rtts_decode_self_attn");
    }
    return 0;
}

extern "C" int rtts_decode_cross_attn(const void* q, int64_t ld_q, const void* kv, int64_t ld_kv, const uint8_t* kvalid, int B, int H, int Tk,
                                      int dh, void* o, int64_t ld_o, int splits, void* workspace, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(q && kv && o, "rtts_decode_cross_attn: q, kv and o must not be NULL");
    RTTS_REQUIRE(dh == 64 || dh == 128, "rtts_decode_cross_attn: dh=%d unsupported (64 or 128)", dh);
    RTTS_REQUIRE(Tk >= 128 && Tk % 128 == 0 && Tk <= 2048, "rtts_decode_cross_attn: Tk=%d unsupported (a multiple of 128 up to 2048)", Tk);
    if (da_common("rtts_decode_cross_attn", B, H, Tk, splits, workspace)) return -1;
    RTTS_REQUIRE(ld_q >= (int64_t)H * dh && ld_q % 8 == 0, "rtts_decode_cross_attn: ld_q=%lld must be >= H*dh and a multiple of 8", (long long)ld_q);
    RTTS_REQUIRE(ld_kv >= 2 * (int64_t)H * dh && ld_kv % 8 == 0, "rtts_decode_cross_attn: ld_kv=%lld must be >= 2*H*dh and a multiple of 8",
                 (long long)ld_kv);
    RTTS_REQUIRE(ld_o >= (int64_t)H * dh && ld_o % 2 == 0, "rtts_decode_cross_attn: ld_o=%lld must be >= H*dh and even", (long long)ld_o);
    RTTS_REQUIRE((((uintptr_t)q | (uintptr_t)kv) & 15) == 0 && ((uintptr_t)o & 3) == 0,
                 "rtts_decode_cross_attn: q and kv must be 16-byte aligned, o 4-byte aligned");
    const dim3 grid((unsigned)(B * H * splits));
#define GO(DH_)                                                                                                                              \
    do {                                                                                                                                     \
        hipLaunchKernelGGL((decode_attn_kernel<DH_, false>), grid, dim3(DA_THREADS), 0, (hipStream_t)stream, (const bf16_t*)q, ld_q,         \
                           (const bf16_t*)kv, ld_kv, (int64_t)Tk * ld_kv, (bf16_t*)nullptr, kvalid, (const int32_t*)nullptr, H, Tk, (bf16_t*)o, \
                           ld_o, splits, (float*)workspace);                                                                                 \
        RTTS_LAUNCH_CHECK("rtts_decode_cross_attn");                                                                                         \
        if (splits > 1)                                                                                                                      \
            hipLaunchKernelGGL((decode_attn_fold_kernel<DH_, false>), dim3((unsigned)(B * H)), dim3(64), 0, (hipStream_t)stream,             \
                               (const float*)workspace, (const int32_t*)nullptr, H, Tk, (bf16_t*)o, ld_o, splits);                           \
    } while (0)
    if (dh == 64) GO(64); else GO(128);
#undef GO
    RTTS_LAUNCH_CHECK("rtts_decode_cross_attn");
    return 0;
}

extern "C" int rtts_decode_tail_im2col(const void* src, int src_abs, int64_t ld_src, int64_t src_batch_stride, int src_r0, int C,
                                       const int32_t* pos, int cap, int B, int R, int r0, int nr, int CP, void* dst, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(src && pos && dst, "rtts_decode_tail_im2col: src, pos and dst must not be NULL");
    RTTS_REQUIRE(B > 0 && R >= 1 && R % 2 == 1 && r0 >= 0 && nr >= 1 && r0 + nr == R && src_r0 >= 0 && src_r0 <= r0 && cap >= 1,
                 "rtts_decode_tail_im2col: bad window (R odd, rows r0 ... R - 1, src_r0 <= r0)");
    RTTS_REQUIRE(CP > 0 && CP % 8 == 0 && C > 0 && C % 8 == 0 && C <= CP, "rtts_decode_tail_im2col: C and CP must be multiples of 8, C <= CP");
    RTTS_REQUIRE(ld_src >= C && ld_src % (src_abs ? 4 : 8) == 0 && src_batch_stride % (src_abs ? 4 : 8) == 0 && ((uintptr_t)src & 15) == 0 &&
                     ((uintptr_t)dst & 15) == 0,
                 "rtts_decode_tail_im2col: src rows must be 16-byte aligned (ld_src >= C)");
    RTTS_REQUIRE(src_batch_stride >= (src_abs ? (int64_t)cap : (int64_t)(R - src_r0)) * ld_src,
                 "rtts_decode_tail_im2col: src_batch_stride smaller than one utterance's rows");
    const int64_t total8 = (int64_t)B * nr * 5 * (CP / 8);
    RTTS_REQUIRE(total8 <= 0x7fffffff, "rtts_decode_tail_im2col: too many rows");
    hipLaunchKernelGGL(decode_tail_im2col_kernel, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, src_abs, ld_src,
                       src_batch_stride, src_r0, C, pos, cap, R, r0, nr, CP, (bf16_t*)dst, total8);
    RTTS_LAUNCH_CHECK("rtts_decode_tail_im2col");
    return 0;
}
