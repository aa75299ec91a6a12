// The tile the STFT -> gain -> inverse STFT launches share (denoise.hip, griffin_lim.hip): n_fft = 1024, hop = 256, 32 frames of one
// utterance per workgroup of 8 waves, both transforms as GEMMs on v_mfma_f32_32x32x2_f32 with the bases streamed from L2.
#pragma once
#include "rtts_common.h"

#define DN_THREADS 512
#define DN_NFFT 1024
#define DN_HOP 256
#define DN_LOG_HOP 8
#define DN_FT 32                                                  // frames of a workgroup
#define DN_STRIDE 29                                              // hops a workgroup completes: FT - (n_fft / hop - 1)
#define DN_SPAN ((DN_FT - 1) * DN_HOP + DN_NFFT)                  // samples the frames of a tile cover
#define DN_FR_LD (DN_NFFT + 1)                                    // row stride of the resynthesised frames: 32 frames on 32 banks
#define DN_W2_AT (DN_FT * DN_FR_LD)                               // the squared window sits behind every image
#ifndef DN_U
#define DN_U 8                                                    // k-pairs per block of the A operand (two blocks in registers)
#endif
#define DN_LDS_BYTES ((size_t)(DN_W2_AT + DN_NFFT) * sizeof(float))

static_assert(DN_SPAN + DN_SPAN / DN_HOP + 4 <= DN_W2_AT && DN_NFFT * DN_FT <= DN_W2_AT, "the span and the spectrum lie below the window");
static_assert(DN_LDS_BYTES <= 160 * 1024, "a tile's images must fit the 160 KB of LDS");

// acc[i] += A (32 rows x K) * B (K x 32 frames) over K = n_fft for 4 row tiles at once.  A[k][row]: ap + k * n_fft + aoff[i] (row =
// lane & 31 and the k parity lane >> 5 are already in ap), streamed from L2; B: the word of k-pair kp (k = 2 kp + h) is bword(kp).
// Two register sets take turns: while the products of one block of DN_U k-pairs run, the loads of the next block are issued BETWEEN
// them, one load per product (sched_group_barrier), so each wave keeps a rolling window of one block of loads in flight and never
// drains it.  (Loading a whole block in front of its products and copying it over at the loop head -- the log-mel launch's form --
// left the L2 reads and the products of the one workgroup a CU holds here almost unoverlapped: 0.84 against 0.61 ms on 16 utterances.)
// The order of the products, and so every bit of the result, is the same in both forms.
template <typename BWord>
__device__ __forceinline__ void dn_gemm(f32x16 (&acc)[4], const float* __restrict__ ap, const int (&aoff)[4], BWord bword) {
    constexpr int U = DN_U, NBLK = DN_NFFT / 2 / U;
    static_assert(NBLK % 2 == 0, "two blocks per trip");
    float a0[U][4], a1[U][4], b0[U], b1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a0[u][i] = ap[(size_t)u * 2 * DN_NFFT + aoff[i]];
        b0[u] = bword(u);
    }
    for (int blk = 0; blk < NBLK; blk += 2) {
        const float* an = ap + (size_t)(blk + 1) * U * 2 * DN_NFFT;
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a1[u][i] = an[(size_t)u * 2 * DN_NFFT + aoff[i]];
            b1[u] = bword((blk + 1) * U + u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u][i], b0[u], acc[i], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        const int nb = blk + 2 < NBLK ? blk + 2 : blk;                   // the last trip loads a block again
        const float* am = ap + (size_t)nb * U * 2 * DN_NFFT;
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a0[u][i] = am[(size_t)u * 2 * DN_NFFT + aoff[i]];
            b0[u] = bword(nb * U + u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u][i], b1[u], acc[i], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
