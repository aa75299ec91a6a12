// Griffin-Lim vocoding for a ragged batch of utterances (rtts_gl_magnitudes / rtts_gl_init / rtts_gl_step of include/rtts.h): from a
// log-mel spectrogram to audio without a trained vocoder.
//
//   rtts_gl_magnitudes  M[k][t] = max(0, sum_m P[k][m] exp(mel[m][t]))^(1/power), P the pseudo-inverse of the mel matrix: a small f32
//                       product (513 x n_mels per frame), one ascending-m fmaf chain per value, on the vector units.
//   rtts_gl_init        x_0 = iSTFT(M e^{i phi}), phi from the counter hash or zero.
//   rtts_gl_step        x_{k+1} = iSTFT(M R / |R|), R = STFT(x_k - beta x_{k-1}).
//
// init and step are the denoiser's launch (denoise.hip, stft_tile.h) with another gain.  A workgroup (8 waves) takes DN_FT = 32
// consecutive frames of ONE utterance, frames t0 = 29 * tile .. t0 + 31:
//   1. (step) stages cur[s] - beta * prev[s] over the span the frames share, reflect-padded per utterance, in LDS;
//   2. (step) short-time DFT as a GEMM on v_mfma_f32_32x32x2_f32, a bin's cosine and sine accumulators side by side in one lane;
//   3. in the accumulators: M[bin][frame] * R / |R| (M where |R| = 0) to LDS as [column][frame] rows over the span; M is read from
//      global memory here, the lanes of one bin reading consecutive frames.  init writes M (cos phi, -sin phi) instead -- the sine
//      columns of the bases hold +sum w x sin = -Im X -- and M alone at bins 0 and n_fft/2, whose imaginary part irfft drops;
//   4. inverse DFT as a second GEMM, the frames back to LDS as [frame][sample] rows;
//   5. every output sample is the sum of its at most four covering frames IN ASCENDING FRAME ORDER divided by the sum of w^2 over
//      the same frames, in the same order, written by exactly one workgroup (tiles overlap by three frames) -- no atomics.
// Frames of a tile past the utterance's last one get a zero spectrum; they are never summed and M is not read for them.
//
// Invariants: everything is f32.  An utterance's output bits depend on its own mel, the seed and the options only -- the hash is
// indexed by the utterance's OWN frame index -- not on its slot in the batch, the other utterances or the grid size, and two calls
// give the same bits.  Samples of no utterance are neither read nor written.  An utterance of at most n_fft / 2 samples (fewer than
// three mel frames) cannot be reflect-padded: its samples are written as zeros.
#include "stft_tile.h"

#include <math.h>

#define GL_BINS (DN_NFFT / 2 + 1)
#define GL_MAG_THREADS 256
#define GL_MAG_FT 32                                              // columns of M a workgroup of rtts_gl_magnitudes writes
#define GL_MAX_MELS 128

// M for GL_MAG_FT consecutive columns of one utterance.  exp(mel) of the columns' frames is staged once in LDS ([mel][column]:
// the 32 lanes of a bin read 32 banks); column L repeats frame L - 1.  A thread owns one column and every eighth bin.
__global__ __launch_bounds__(GL_MAG_THREADS) void gl_magnitudes_kernel(const float* __restrict__ mel, int64_t sb, int64_t sc, int64_t st,
                                                                       const int64_t* __restrict__ mel_start, const int64_t* __restrict__ coff,
                                                                       const float* __restrict__ pinv, int n_mels, int power,
                                                                       float* __restrict__ mag, int64_t ld_mag) {
    __shared__ float es[GL_MAX_MELS * GL_MAG_FT];
    const int seg = blockIdx.y;
    const int64_t c0 = coff[seg];
    const int64_t cols = coff[seg + 1] - c0;                      // L + 1
    const int64_t L = cols - 1;
    const int64_t t0 = (int64_t)blockIdx.x * GL_MAG_FT;
    if (t0 >= cols) return;                                       // the grid is sized for the longest utterance of the call
    const int tid = threadIdx.x;
    const float* src = mel + (int64_t)seg * sb + mel_start[seg] * st;
    for (int i = tid; i < n_mels * GL_MAG_FT; i += GL_MAG_THREADS) {
        const int m = i / GL_MAG_FT, c = i % GL_MAG_FT;
        int64_t t = t0 + c;
        if (t > L - 1) t = L - 1;
        es[i] = (t >= 0 && t0 + c < cols) ? expf(src[(int64_t)m * sc + t * st]) : 0.f;   // L = 0: the one column is zero
    }
    __syncthreads();
    const int c = tid & (GL_MAG_FT - 1);
    if (t0 + c >= cols) return;
    for (int bin = tid / GL_MAG_FT; bin < GL_BINS; bin += GL_MAG_THREADS / GL_MAG_FT) {
        const float* p = pinv + (size_t)bin * n_mels;
        float a = 0.f;
        for (int m = 0; m < n_mels; ++m) a = fmaf(p[m], es[m * GL_MAG_FT + c], a);
        a = fmaxf(a, 0.f);
        mag[(int64_t)bin * ld_mag + c0 + t0 + c] = power == 2 ? sqrtf(a) : a;
    }
}

// (cos phi, sin phi) of bin k, frame t of an utterance: phi = 2 pi (hash >> 8) / 2^24, the 24 bits exact in f32
__device__ __forceinline__ void gl_phase(uint32_t seed, int64_t t, int bin, float& co, float& si) {
    const uint32_t h = rtts_drop_hash(seed, (uint32_t)t * (uint32_t)GL_BINS + (uint32_t)bin);
    sincospif(2.f * ((float)(h >> 8) * 0x1p-24f), &si, &co);
}

// INIT: no input audio and no forward DFT, the spectrum image is M (cos phi, -sin phi) (phase 1: the hash, 0: zero phases)
template <bool INIT>
__global__ __launch_bounds__(DN_THREADS) void gl_tile_kernel(const float* __restrict__ cur, const float* __restrict__ prev, float beta,
                                                             const float* __restrict__ mag, int64_t ld_mag, const int64_t* __restrict__ coff,
                                                             const int64_t* __restrict__ soff, const float* __restrict__ basis,
                                                             const float* __restrict__ ibasis, int phase, uint32_t seed,
                                                             float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float gl_lds[];
    float* xs = gl_lds;                                           // the span: sample p at p + p / hop
    float* zs = gl_lds;                                           // the spectrum: [column][frame]
    float* fr = gl_lds;                                           // after the inverse DFT: [frame][sample], stride DN_FR_LD
    float* w2 = gl_lds + DN_W2_AT;

    const int seg = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t s0 = soff[seg];
    const int64_t n = soff[seg + 1] - s0;
    float* op = out + s0;
    if (n <= DN_NFFT / 2) {                                       // fewer than three frames: zeros, written by the first tile
        if (blockIdx.x == 0)
            for (int64_t p = tid; p < n; p += DN_THREADS) op[p] = 0.f;
        return;
    }
    const int64_t frames = n / DN_HOP + 1;
    const int64_t u_max = (n + DN_NFFT / 2 - 1) / DN_HOP;         // hop of the last output sample (padded position n - 1 + n_fft / 2)
    const int64_t t0 = (int64_t)blockIdx.x * DN_STRIDE;
    if (blockIdx.x > 0 && t0 + 3 > u_max) return;                 // the grid is sized for the longest utterance of the call
    const float* mg = mag + coff[seg] + t0;                       // M[bin][t0 + c] at mg[bin * ld_mag + c], c < frames - t0

    if (!INIT) {
        const float* x = cur + s0;
        const float* xp = prev ? prev + s0 : nullptr;
        for (int p = tid; p < DN_SPAN; p += DN_THREADS) {
            int64_t s = t0 * DN_HOP - DN_NFFT / 2 + p;
            if (s < 0) s = -s;
            if (s >= n) s = 2 * (n - 1) - s;                      // n > n_fft / 2: one reflection reaches every sample of a real frame
            float v = 0.f;                                        // frames past the last one: never summed
            if (s >= 0 && s < n) v = xp ? fmaf(-beta, xp[s], x[s]) : x[s];
            xs[p + (p >> DN_LOG_HOP)] = v;
        }
    }
    for (int m = tid; m < DN_NFFT; m += DN_THREADS) {
        const float wm = basis[(size_t)m * DN_NFFT];
        w2[m] = wm * wm;
    }
    __syncthreads();

    const int w = tid >> 6, l = tid & 63, c = l & 31, h = l >> 5;
    const bool live = t0 + c < frames;                            // this lane's frame exists
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x16{0};
    if (!INIT) {
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
            const float m = live ? mg[(int64_t)bin * ld_mag + c] : 0.f;
            if (bin == 0) {                                       // bins 0 and n_fft/2 are real: they share the column pair
                const float m1 = live ? mg[(int64_t)(DN_NFFT / 2) * ld_mag + c] : 0.f;
                float u0 = 1.f, u1 = 1.f;
                if (INIT) {
                    if (phase) {
                        float si;
                        gl_phase(seed, t0 + c, 0, u0, si);
                        gl_phase(seed, t0 + c, DN_NFFT / 2, u1, si);
                    }
                } else {
                    u0 = acc[0][r] < 0.f ? -1.f : 1.f;            // R / |R| of a real bin, 1 where R = 0
                    u1 = acc[1][r] < 0.f ? -1.f : 1.f;
                }
                zs[c] = m * u0;
                zs[(DN_NFFT / 2) * DN_FT + c] = m1 * u1;
            } else {
                float zr = m, zi = 0.f;                           // R / |R| = 1 where |R| = 0; zero phases
                if (INIT) {
                    if (phase) {
                        float co, si;
                        gl_phase(seed, t0 + c, bin, co, si);
                        zr = m * co;
                        zi = -(m * si);
                    }
                } else {
                    const float re = acc[2 * j][r], im = acc[2 * j + 1][r];
                    const float a = sqrtf(re * re + im * im);
                    if (a > 0.f) {
                        const float g = m / a;
                        zr = g * re;
                        zi = g * im;
                    }
                }
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

static RttsLdsState g_gl_init_lds, g_gl_step_lds;

// The offsets of a call, validated on the host copies: utterance s has n_s = 256 L_s samples and L_s + 1 columns of M.
static int gl_check_offsets(const char* who, const int64_t* soff, const int64_t* coff, int nseg, int64_t ld_mag, int hop, int64_t* u_longest) {
    RTTS_REQUIRE(soff[0] >= 0 && coff[0] >= 0, "%s: offsets must not be negative", who);
    *u_longest = 4;
    for (int s = 0; s < nseg; ++s) {
        const int64_t n = soff[s + 1] - soff[s], cols = coff[s + 1] - coff[s];
        RTTS_REQUIRE(n >= 0 && n % hop == 0, "%s: utterance %d has %lld samples; sample_offsets must step by multiples of hop = %d", who, s,
                     (long long)n, hop);
        RTTS_REQUIRE(cols == n / hop + 1, "%s: utterance %d of %lld samples owns %lld columns of mag; col_offsets must step by frames + 1 = %lld",
                     who, s, (long long)n, (long long)cols, (long long)(n / hop + 1));
        const int64_t u_max = (n + DN_NFFT / 2 - 1) / hop;
        if (n > DN_NFFT / 2 && u_max > *u_longest) *u_longest = u_max;
    }
    RTTS_REQUIRE(coff[nseg] <= ld_mag, "%s: col_offsets end at %lld, past ld_mag = %lld", who, (long long)coff[nseg], (long long)ld_mag);
    return 0;
}

static bool gl_overlap(const float* a, const float* b, const int64_t* soff, int nseg) {
    if (!a || !b || soff[nseg] == soff[0]) return false;
    return !(b + soff[nseg] <= a + soff[0] || a + soff[nseg] <= b + soff[0]);
}

extern "C" int rtts_gl_magnitudes(const float* mel, int64_t stride_b, int64_t stride_c, int64_t stride_t, const int64_t* mel_start,
                                  const int64_t* col_offsets_host, const int64_t* col_offsets, int nseg, const float* pinv, int n_mels,
                                  int power, int n_fft, float* mag, int64_t ld_mag, void* stream) {
    RTTS_REQUIRE(mel && mel_start && col_offsets_host && col_offsets && pinv && mag, "rtts_gl_magnitudes: null pointer argument");
    RTTS_REQUIRE(n_fft == DN_NFFT, "rtts_gl_magnitudes: n_fft must be %d (got %d)", DN_NFFT, n_fft);
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "rtts_gl_magnitudes: nseg must be in 1..65535 (got %d)", nseg);
    RTTS_REQUIRE(n_mels >= 1 && n_mels <= GL_MAX_MELS, "rtts_gl_magnitudes: n_mels must be in 1..%d (got %d)", GL_MAX_MELS, n_mels);
    RTTS_REQUIRE(power == 1 || power == 2, "rtts_gl_magnitudes: power must be 1 or 2 (got %d)", power);
    RTTS_REQUIRE(col_offsets_host[0] >= 0, "rtts_gl_magnitudes: col_offsets must not be negative");
    int64_t longest = 1;
    for (int s = 0; s < nseg; ++s) {
        const int64_t cols = col_offsets_host[s + 1] - col_offsets_host[s];
        RTTS_REQUIRE(cols >= 1, "rtts_gl_magnitudes: utterance %d owns %lld columns of mag; col_offsets must step by frames + 1 >= 1", s,
                     (long long)cols);
        if (cols > longest) longest = cols;
    }
    RTTS_REQUIRE(col_offsets_host[nseg] <= ld_mag, "rtts_gl_magnitudes: col_offsets end at %lld, past ld_mag = %lld",
                 (long long)col_offsets_host[nseg], (long long)ld_mag);
    const int64_t tiles = (longest + GL_MAG_FT - 1) / GL_MAG_FT;
    RTTS_REQUIRE(tiles <= 0x7fffffff, "rtts_gl_magnitudes: an utterance of %lld frames is too long for one launch", (long long)longest);
    RTTS_ENTER(stream);
    hipLaunchKernelGGL(gl_magnitudes_kernel, dim3((unsigned)tiles, (unsigned)nseg), dim3(GL_MAG_THREADS), 0, (hipStream_t)stream, mel, stride_b,
                       stride_c, stride_t, mel_start, col_offsets, pinv, n_mels, power, mag, ld_mag);
    RTTS_LAUNCH_CHECK("rtts_gl_magnitudes");
    return 0;
}

extern "C" int rtts_gl_init(const float* mag, int64_t ld_mag, const int64_t* col_offsets_host, const int64_t* col_offsets,
                            const int64_t* sample_offsets_host, const int64_t* sample_offsets, int nseg, const float* dft_basis,
                            const float* idft_basis, int phase, uint32_t seed, int n_fft, int hop, float* out, void* stream) {
    RTTS_REQUIRE(mag && col_offsets_host && col_offsets && sample_offsets_host && sample_offsets && dft_basis && idft_basis && out,
                 "rtts_gl_init: null pointer argument");
    RTTS_REQUIRE(n_fft == DN_NFFT, "rtts_gl_init: n_fft must be %d (got %d)", DN_NFFT, n_fft);
    RTTS_REQUIRE(hop == DN_HOP, "rtts_gl_init: hop must be %d (got %d)", DN_HOP, hop);
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "rtts_gl_init: nseg must be in 1..65535 (got %d)", nseg);
    RTTS_REQUIRE(phase == 0 || phase == 1, "rtts_gl_init: phase must be 0 (zero) or 1 (hash) (got %d)", phase);
    int64_t u_longest;
    if (gl_check_offsets("rtts_gl_init", sample_offsets_host, col_offsets_host, nseg, ld_mag, hop, &u_longest)) return -1;
    const int64_t tiles = (u_longest - 3) / DN_STRIDE + 1;
    RTTS_REQUIRE(tiles <= 0x7fffffff, "rtts_gl_init: an utterance of %lld hops is too long for one launch", (long long)u_longest);
    RTTS_ENTER(stream);
    RTTS_ENSURE_LDS("rtts_gl_init", gl_tile_kernel<true>, DN_LDS_BYTES, g_gl_init_lds);
    hipLaunchKernelGGL(gl_tile_kernel<true>, dim3((unsigned)tiles, (unsigned)nseg), dim3(DN_THREADS), DN_LDS_BYTES, (hipStream_t)stream,
                       (const float*)nullptr, (const float*)nullptr, 0.f, mag, ld_mag, col_offsets, sample_offsets, dft_basis, idft_basis, phase,
                       seed, out);
    RTTS_LAUNCH_CHECK("rtts_gl_init");
    return 0;
}

extern "C" int rtts_gl_step(const float* cur, const float* prev, float beta, const float* mag, int64_t ld_mag, const int64_t* col_offsets_host,
                            const int64_t* col_offsets, const int64_t* sample_offsets_host, const int64_t* sample_offsets, int nseg,
                            const float* dft_basis, const float* idft_basis, int n_fft, int hop, float* out, void* stream) {
    RTTS_REQUIRE(cur && mag && col_offsets_host && col_offsets && sample_offsets_host && sample_offsets && dft_basis && idft_basis && out,
                 "rtts_gl_step: null pointer argument (only prev may be null)");
    RTTS_REQUIRE(n_fft == DN_NFFT, "rtts_gl_step: n_fft must be %d (got %d)", DN_NFFT, n_fft);
    RTTS_REQUIRE(hop == DN_HOP, "rtts_gl_step: hop must be %d (got %d)", DN_HOP, hop);
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "rtts_gl_step: nseg must be in 1..65535 (got %d)", nseg);
    RTTS_REQUIRE(isfinite(beta) && beta >= 0.f && beta < 1.f, "rtts_gl_step: beta must be in [0, 1) (got %g)", (double)beta);
    int64_t u_longest;
    if (gl_check_offsets("rtts_gl_step", sample_offsets_host, col_offsets_host, nseg, ld_mag, hop, &u_longest)) return -1;
    RTTS_REQUIRE(!gl_overlap(out, cur, sample_offsets_host, nseg), "rtts_gl_step: out must not overlap cur (a tile reads its neighbours' input)");
    RTTS_REQUIRE(!gl_overlap(out, prev, sample_offsets_host, nseg), "rtts_gl_step: out must not overlap prev (a tile reads its neighbours' input)");
    const int64_t tiles = (u_longest - 3) / DN_STRIDE + 1;
    RTTS_REQUIRE(tiles <= 0x7fffffff, "rtts_gl_step: an utterance of %lld hops is too long for one launch", (long long)u_longest);
    RTTS_ENTER(stream);
    RTTS_ENSURE_LDS("rtts_gl_step", gl_tile_kernel<false>, DN_LDS_BYTES, g_gl_step_lds);
    hipLaunchKernelGGL(gl_tile_kernel<false>, dim3((unsigned)tiles, (unsigned)nseg), dim3(DN_THREADS), DN_LDS_BYTES, (hipStream_t)stream, cur,
                       beta > 0.f ? prev : (const float*)nullptr, beta, mag, ld_mag, col_offsets, sample_offsets, dft_basis, idft_basis, 0, 0u,
                       out);
    RTTS_LAUNCH_CHECK("rtts_gl_step");
    return 0;
}
