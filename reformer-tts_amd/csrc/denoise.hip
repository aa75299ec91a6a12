// Vocoder denoiser for a ragged batch of utterances, one launch (rtts_denoise of include/rtts.h): STFT, subtract the vocoder's bias
// spectrum from the magnitudes, inverse STFT with the original phase.
//
// A workgroup (8 waves) takes DN_FT = 32 consecutive frames of ONE utterance, frames t0 = 29 * tile .. t0 + 31:
//   1. stages the audio span the frames share, reflect-padded per utterance, in LDS once (frame t is span[t * hop, + n_fft)), and
//      the squared window (column 0 of the forward basis is the window itself);
//   2. short-time DFT as a GEMM on v_mfma_f32_32x32x2_f32, as the log-mel launch does it: D[col][frame] = sum_n basis[n][col] *
//      span[frame * hop + n], the basis streamed from L2 into the A operand, the frames read from LDS as the B operand.  A wave owns
//      two tiles of 32 bins, cosine and sine accumulators side by side, so a bin's magnitude never leaves its lane;
//   3. in the accumulators: |X|, gain = max(|X| - strength * bias, 0) / |X| (0 where |X| = 0), and gain * (cosine, sine) to LDS as
//      [column][frame] rows, 1024 x 32 words = 128 KB, over the span, which nobody reads any more;
//   4. inverse DFT as a second GEMM on the same instruction: f[m][frame] = sum_col idft[col][m] * Z[col][frame], the inverse basis
//      (synthesis window folded in) streamed from L2 as A, Z read from LDS as B.  A wave owns 128 samples x 32 frames = 4 tiles;
//   5. the frames go back to LDS as [frame][sample] rows (stride n_fft + 1) over Z, and every output sample is the sum of its
//      at most four covering frames IN ASCENDING FRAME ORDER divided by the sum of w^2 over the same frames, in the same order.
// Tiles overlap by three frames: a tile completes the 29 hops whose four covering frames it holds (the first tile of an utterance
// also the hops in front of them), so every output sample is written by exactly one workgroup -- no atomics, no shared address.
//
// Invariants: everything is f32.  Every spectrum value and every frame sample is ONE k-ordered fmaf chain (the instruction is bit
// for bit that chain), every output sample one fixed-order sum of them: an utterance's output bits depend on its own samples, the
// bias and the strength only -- not on its slot in the batch, the other utterances or the grid size -- and two calls give the
// same bits.  Samples of no utterance are neither read nor written.
#include "stft_tile.h"

#include <math.h>

__global__ __launch_bounds__(DN_THREADS) void denoise_kernel(const float* __restrict__ audio, const int64_t* __restrict__ soff,
                                                             const float* __restrict__ basis, const float* __restrict__ ibasis,
                                                             const float* __restrict__ bias, float strength, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float dn_lds[];
    float* xs = dn_lds;                                           // the span: sample p at p + p / hop
    float* zs = dn_lds;                                           // after the forward DFT: [column][frame]
    float* fr = dn_lds;                                           // after the inverse DFT: [frame][sample], stride DN_FR_LD
    float* w2 = dn_lds + DN_W2_AT;

    const int seg = blockIdx.y;
    const int64_t s0 = soff[seg];
    const int64_t n = soff[seg + 1] - s0;
    const int64_t frames = n / DN_HOP + 1;
    const int64_t u_max = (n + DN_NFFT / 2 - 1) / DN_HOP;         // hop of the last output sample (padded position n - 1 + n_fft / 2)
    const int64_t t0 = (int64_t)blockIdx.x * DN_STRIDE;
    if (blockIdx.x > 0 && t0 + 3 > u_max) return;                 // the grid is sized for the longest utterance of the call

    const int tid = threadIdx.x;
    const float* x = audio + s0;
    for (int p = tid; p < DN_SPAN; p += DN_THREADS) {
        int64_t s = t0 * DN_HOP - DN_NFFT / 2 + p;
        if (s < 0) s = -s;
        if (s >= n) s = 2 * (n - 1) - s;                          // n > n_fft / 2: one reflection reaches every sample of a real frame
        xs[p + (p >> DN_LOG_HOP)] = (s >= 0 && s < n) ? x[s] : 0.f;   // frames past the last one: never summed
    }
    for (int m = tid; m < DN_NFFT; m += DN_THREADS) {
        const float wm = basis[(size_t)m * DN_NFFT];
        w2[m] = wm * wm;
    }
    __syncthreads();

    const int w = tid >> 6, l = tid & 63, c = l & 31, h = l >> 5;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x16{0};
    {
        // accumulators 2j / 2j+1: cosine / sine columns of bins 32 * (2 w + j) ..
        const int aoff[4] = {0, DN_NFFT / 2, 32, DN_NFFT / 2 + 32};
        const float* bp = xs + c * (DN_HOP + 1) + h;
        // samples 2 kp + h of frame c: the padded image skips a word at every multiple of hop
        dn_gemm(acc, basis + (size_t)h * DN_NFFT + w * 64 + c, aoff,
                [&](int kp) { return bp[(kp >> (DN_LOG_HOP - 1)) * (DN_HOP + 1) + (kp & (DN_HOP / 2 - 1)) * 2]; });
    }
    __syncthreads();                                              // every wave has read its last sample: the span becomes the spectrum
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int bin = (w * 2 + j) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float re = acc[2 * j][r], im = acc[2 * j + 1][r];
            if (bin == 0) {                                       // bins 0 and n_fft/2 are real: they share the column pair
                const float m0 = fabsf(re), m1 = fabsf(im);
                const float g0 = m0 > 0.f ? fmaxf(m0 - strength * bias[0], 0.f) / m0 : 0.f;
                const float g1 = m1 > 0.f ? fmaxf(m1 - strength * bias[DN_NFFT / 2], 0.f) / m1 : 0.f;
                zs[c] = g0 * re;
                zs[(DN_NFFT / 2) * DN_FT + c] = g1 * im;
            } else {
                const float mag = sqrtf(re * re + im * im);
                const float g = mag > 0.f ? fmaxf(mag - strength * bias[bin], 0.f) / mag : 0.f;
                zs[bin * DN_FT + c] = g * re;
                zs[(DN_NFFT / 2 + bin) * DN_FT + c] = g * im;
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

static RttsLdsState g_denoise_lds;

extern "C" int rtts_denoise(const float* audio, const int64_t* sample_offsets_host, const int64_t* sample_offsets, int nseg,
                            const float* dft_basis, const float* idft_basis, const float* bias, float strength, int n_fft, int hop,
                            float* out, void* stream) {
    RTTS_REQUIRE(audio && sample_offsets_host && sample_offsets && dft_basis && idft_basis && bias && out,
                 "rtts_denoise: null pointer argument");
    RTTS_REQUIRE(n_fft == DN_NFFT, "rtts_denoise: n_fft must be %d (got %d)", DN_NFFT, n_fft);
    RTTS_REQUIRE(hop == DN_HOP, "rtts_denoise: hop must be %d (got %d)", DN_HOP, hop);
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "rtts_denoise: nseg must be in 1..65535 (got %d)", nseg);
    RTTS_REQUIRE(isfinite(strength) && strength >= 0.f, "rtts_denoise: strength must be finite and >= 0 (got %g)", (double)strength);
    int64_t u_longest = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t n = sample_offsets_host[s + 1] - sample_offsets_host[s];
        RTTS_REQUIRE(sample_offsets_host[s] >= 0 && n > n_fft / 2,
                     "rtts_denoise: utterance %d has %lld samples; reflect padding needs more than n_fft / 2 = %d", s, (long long)n, n_fft / 2);
        const int64_t u_max = (n + n_fft / 2 - 1) / hop;
        if (u_max > u_longest) u_longest = u_max;
    }
    {
        const float* a_lo = audio + sample_offsets_host[0];
        const float* a_hi = audio + sample_offsets_host[nseg];
        const float* o_lo = out + sample_offsets_host[0];
        const float* o_hi = out + sample_offsets_host[nseg];
        RTTS_REQUIRE(o_hi <= a_lo || a_hi <= o_lo, "rtts_denoise: out must not overlap audio (a tile reads its neighbours' input)");
    }
    const int64_t tiles = (u_longest - 3) / DN_STRIDE + 1;        // n > n_fft / 2: the last hop is at least 4
    RTTS_REQUIRE(tiles <= 0x7fffffff, "rtts_denoise: an utterance of %lld hops is too long for one launch", (long long)u_longest);
    RTTS_ENTER(stream);
    RTTS_ENSURE_LDS("rtts_denoise", denoise_kernel, DN_LDS_BYTES, g_denoise_lds);
    hipLaunchKernelGGL(denoise_kernel, dim3((unsigned)tiles, (unsigned)nseg), dim3(DN_THREADS), DN_LDS_BYTES, (hipStream_t)stream, audio,
                       sample_offsets, dft_basis, idft_basis, bias, strength, out);
    RTTS_LAUNCH_CHECK("rtts_denoise");
    return 0;
}
