// The tile of the STFT -> gain -> inverse STFT launches (denoise.hip, griffin_lim.hip): n_fft = 1024, hop = 256, everything f32.
// stft_tile_walk is the whole program of such a launch; a launch supplies a sample source and a gain, nothing else.
//
// A workgroup (8 waves) takes DN_FT = 32 consecutive frames of ONE utterance, frames t0 = 29 * tile .. t0 + 31:
//   1. (FORWARD) stages the span the frames share, reflect-padded per utterance, in LDS once (frame t is span[t * hop, + n_fft)),
//      and the squared window (column 0 of the forward basis is the window itself);
//   2. (FORWARD) short-time DFT as a GEMM on v_mfma_f32_32x32x2_f32, as the log-mel launch does it: D[col][frame] = sum_n
//      basis[n][col] * span[frame * hop + n], the basis streamed from L2 into the A operand, the frames read from LDS as the B
//      operand.  A wave owns two tiles of 32 bins, cosine and sine accumulators side by side, so a bin never leaves its lane;
//   3. in the accumulators: the gain maps a bin's (re, im) to what goes to LDS as [column][frame] rows, 1024 x 32 words = 128 KB,
//      over the span, which nobody reads any more.  Without FORWARD (re, im) are zeros and the gain makes the spectrum up;
//   4. inverse DFT as a second GEMM on the same instruction: f[m][frame] = sum_col idft[col][m] * Z[col][frame], the inverse basis
//      (synthesis window folded in) streamed from L2 as A, Z read from LDS as B.  A wave owns 128 samples x 32 frames = 4 tiles;
//   5. the frames go back to LDS as [frame][sample] rows (stride n_fft + 1) over Z, and every output sample is the sum of its
//      at most four covering frames IN ASCENDING FRAME ORDER divided by the sum of w^2 over the same frames, in the same order.
// Tiles overlap by three frames: a tile completes the 29 hops whose four covering frames it holds (the first tile of an utterance
// also the hops in front of them), so every output sample is written by exactly one workgroup -- no atomics, no shared address.
// Every spectrum value and every frame sample is ONE k-ordered fmaf chain (the instruction is bit for bit that chain), every
// output sample one fixed-order sum of them.  Samples of no utterance are neither read nor written.
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
#define DN_U 8                                                    // k-pairs per block of the A operand (two blocks in registers)
#define DN_LDS_BYTES ((size_t)(DN_W2_AT + DN_NFFT) * sizeof(float))

static_assert(DN_SPAN + DN_SPAN / DN_HOP + 4 <= DN_W2_AT && DN_NFFT * DN_FT <= DN_W2_AT, "the span and the spectrum lie below the window");
static_assert(DN_LDS_BYTES <= 160 * 1024, "a tile's images must fit the 160 KB of LDS");

// torch.stft's reflect padding (also the log-mel launch's): s, a sample index of an utterance of n samples that may lie in front
// of or behind it, becomes the sample it mirrors.  n > n_fft / 2: one reflection reaches every sample of a real frame; false for
// the samples of frames past the last one, which read as zero.
__device__ __forceinline__ bool stft_reflect(int64_t n, int64_t& s) {
    if (s < 0) s = -s;
    if (s >= n) s = 2 * (n - 1) - s;
    return s >= 0 && s < n;
}

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

// One tile of utterance blockIdx.y (samples soff[y] .. soff[y + 1] of the packed audio), tile blockIdx.x; lds: DN_LDS_BYTES.
//   sample(s)                                     the staged value of ABSOLUTE sample s of the packed audio (FORWARD only)
//   gain.pair(t0, c, live, bin, re, im, z0, z1)   bin = 0: bins 0 and n_fft/2 of frame t0 + c, which are real and share the column
//                                                 pair: (re, im) are their two values, z0 / z1 what their cosine columns get
//   gain.bin(t0, c, live, bin, re, im, zr, zi)    every other bin: zr / zi go to its cosine / sine column
// live: frame t0 + c exists.  Frames past the utterance's last one are never summed.
template <bool FORWARD, typename Sample, typename Gain>
__device__ __forceinline__ void stft_tile_walk(float* lds, const int64_t* __restrict__ soff, const float* __restrict__ basis,
                                               const float* __restrict__ ibasis, float* __restrict__ out, Sample sample, Gain gain) {
    float* xs = lds;                                              // the span: sample p at p + p / hop
    float* zs = lds;                                              // after the forward DFT: [column][frame]
    float* fr = lds;                                              // after the inverse DFT: [frame][sample], stride DN_FR_LD
    float* w2 = lds + DN_W2_AT;

    const int seg = blockIdx.y;
    const int64_t s0 = soff[seg];
    const int64_t n = soff[seg + 1] - s0;
    const int64_t frames = n / DN_HOP + 1;
    const int64_t u_max = (n + DN_NFFT / 2 - 1) / DN_HOP;         // hop of the last output sample (padded position n - 1 + n_fft / 2)
    const int64_t t0 = (int64_t)blockIdx.x * DN_STRIDE;
    if (blockIdx.x > 0 && t0 + 3 > u_max) return;                 // the grid is sized for the longest utterance of the call

    const int tid = threadIdx.x;
    if (FORWARD)
        for (int p = tid; p < DN_SPAN; p += DN_THREADS) {
            int64_t s = t0 * DN_HOP - DN_NFFT / 2 + p;
            xs[p + (p >> DN_LOG_HOP)] = stft_reflect(n, s) ? sample(s0 + s) : 0.f;
        }
    for (int m = tid; m < DN_NFFT; m += DN_THREADS) {
        const float wm = basis[(size_t)m * DN_NFFT];
        w2[m] = wm * wm;
    }
    __syncthreads();

    const int w = tid >> 6, l = tid & 63, c = l & 31, h = l >> 5;
    const bool live = t0 + c < frames;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x16{0};
    if (FORWARD) {
        // accumulators 2j / 2j+1: cosine / sine columns of bins 32 * (2 w + j) ..
        const int aoff[4] = {0, DN_NFFT / 2, 32, DN_NFFT / 2 + 32};
        const float* bp = xs + c * (DN_HOP + 1) + h;
        // samples 2 kp + h of frame c: the padded image skips a word at every multiple of hop
        dn_gemm(acc, basis + (size_t)h * DN_NFFT + w * 64 + c, aoff,
                [&](int kp) { return bp[(kp >> (DN_LOG_HOP - 1)) * (DN_HOP + 1) + (kp & (DN_HOP / 2 - 1)) * 2]; });
        __syncthreads();                                          // every wave has read its last sample: the span becomes the spectrum
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int bin = (w * 2 + j) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float re = acc[2 * j][r], im = acc[2 * j + 1][r];
            float zr, zi;
            if (bin == 0) {                                       // bins 0 and n_fft/2 are real: they share the column pair
                gain.pair(t0, c, live, bin, re, im, zr, zi);
                zs[c] = zr;
                zs[(DN_NFFT / 2) * DN_FT + c] = zi;
            } else {
                gain.bin(t0, c, live, bin, re, im, zr, zi);
                zs[bin * DN_FT + c] = zr;
                zs[(DN_NFFT / 2 + bin) * DN_FT + c] = zi;
            }
        }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x16{0};
    {
        const int aoff[4] = {0, 32, 64, 96};                      // accumulator j: samples 128 w + 32 j ..
        const float* bp = zs + h * DN_FT + c;
        dn_gemm(acc, ibasis + (size_t)h * DN_NFFT + w * 128 + c, aoff, [&](int kp) { return bp[2 * kp * DN_FT]; });
    }
    __syncthreads();                                              // every wave has read its last column: the spectrum becomes the frames
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) fr[c * DN_FR_LD + w * 128 + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = acc[j][r];
    __syncthreads();

    // hops t0 + ul of this tile: ul = 3 .. 31 have their four frames here; the first tile also owns the hops in front of them
    // (hop 2 holds output sample 0).  Frames past the utterance's last one do not exist.
    const int ul_lo = blockIdx.x == 0 ? 2 : 3;
    const int64_t ul_end = u_max - t0 + 1;
    const int ul_hi = ul_end < DN_FT ? (int)ul_end : DN_FT;       // exclusive
    float* op = out + s0;
    for (int idx = ul_lo * DN_HOP + tid; idx < ul_hi * DN_HOP; idx += DN_THREADS) {
        const int ul = idx >> DN_LOG_HOP, i = idx & (DN_HOP - 1);
        const int tl_lo = ul >= 3 ? ul - 3 : 0;
        const int64_t last = frames - 1 - t0;
        const int tl_hi = last < ul ? (int)last : ul;             // inclusive
        float sum = 0.f, env = 0.f;
        for (int tl = tl_lo; tl <= tl_hi; ++tl) {
            const int m = ((ul - tl) << DN_LOG_HOP) + i;
            sum += fr[tl * DN_FR_LD + m];
            env += w2[m];
        }
        const int64_t p = t0 * DN_HOP + idx - DN_NFFT / 2;
        if (p >= 0 && p < n) op[p] = sum / env;
    }
}

// The host side of a tile launch; who is the entry point's name.  Every helper returns -1 with the error set, as RTTS_REQUIRE does.
static inline int stft_tile_check_shape(const char* who, int n_fft, int hop, int nseg) {
    RTTS_REQUIRE(n_fft == DN_NFFT, "%s: n_fft must be %d (got %d)", who, DN_NFFT, n_fft);
    RTTS_REQUIRE(hop == DN_HOP, "%s: hop must be %d (got %d)", who, DN_HOP, hop);
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "%s: nseg must be in 1..65535 (got %d)", who, nseg);
    return 0;
}

// u_longest: the last hop of the longest utterance.  Utterances of at most n_fft / 2 samples cannot be reflect-padded: they are
// refused (refuse_short) or left to the kernel, which launches no tile for them; a transformed one ends in hop 4 at least.
static inline int stft_tile_longest(const char* who, const int64_t* soff, int nseg, bool refuse_short, int64_t* u_longest) {
    *u_longest = 4;
    for (int s = 0; s < nseg; ++s) {
        const int64_t n = soff[s + 1] - soff[s];
        if (refuse_short)
            RTTS_REQUIRE(soff[s] >= 0 && n > DN_NFFT / 2, "%s: utterance %d has %lld samples; reflect padding needs more than n_fft / 2 = %d",
                         who, s, (long long)n, DN_NFFT / 2);
        const int64_t u_max = (n + DN_NFFT / 2 - 1) / DN_HOP;
        if (n > DN_NFFT / 2 && u_max > *u_longest) *u_longest = u_max;
    }
    return 0;
}

static inline int stft_tile_count(const char* who, int64_t u_longest, unsigned* tiles) {
    const int64_t t = (u_longest - 3) / DN_STRIDE + 1;
    RTTS_REQUIRE(t <= 0x7fffffff, "%s: an utterance of %lld hops is too long for one launch", who, (long long)u_longest);
    *tiles = (unsigned)t;
    return 0;
}

// a tile reads its neighbours' input: do the utterances of a (null: no) and of b, packed by soff, share an address?
static inline bool stft_tile_overlap(const float* a, const float* b, const int64_t* soff, int nseg) {
    if (!a || !b || soff[nseg] == soff[0]) return false;
    return !(b + soff[nseg] <= a + soff[0] || a + soff[nseg] <= b + soff[0]);
}
