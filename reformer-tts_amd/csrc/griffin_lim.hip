// Griffin-Lim vocoding for a ragged batch of utterances (rtts_gl_magnitudes / rtts_gl_init / rtts_gl_step of include/rtts.h): from a
// log-mel spectrogram to audio without a trained vocoder.
//
//   rtts_gl_magnitudes  M[k][t] = max(0, sum_m P[k][m] exp(mel[m][t]))^(1/power), P the pseudo-inverse of the mel matrix: a small f32
//                       product (513 x n_mels per frame), one ascending-m fmaf chain per value, on the vector units.
//   rtts_gl_init        x_0 = iSTFT(M e^{i phi}), phi from the counter hash or zero.
//   rtts_gl_step        x_{k+1} = iSTFT(M R / |R|), R = STFT(x_k - beta x_{k-1}).
//
// init and step are the tile walk of stft_tile.h: init without its forward half, on a spectrum M e^{i phi} that its gain makes
// up; step on x_k - beta x_{k-1} with the gain M R / |R|.  M is read from global memory in the gain, and only for the frames of a
// tile that exist: the others get a zero spectrum and are never summed.
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

// M[bin][frame] of an utterance whose first column is mg: read only for the frames that exist, the lanes of one bin reading
// consecutive frames
struct GlMag {
    const float* __restrict__ mg;
    int64_t ld_mag;
    __device__ __forceinline__ float at(int64_t t0, int c, bool live, int bin) const { return live ? (mg + t0)[(int64_t)bin * ld_mag + c] : 0.f; }
};

// rtts_gl_init: M (cos phi, -sin phi) -- the sine columns of the bases hold +sum w x sin = -Im X -- and M cos phi at bins 0 and
// n_fft/2, whose imaginary part irfft drops (phase 1: the hash, 0: zero phases)
struct GlInitGain {
    GlMag M;
    int phase;
    uint32_t seed;
    __device__ __forceinline__ void pair(int64_t t0, int c, bool live, int bin, float, float, float& z0, float& z1) const {
        const float m = M.at(t0, c, live, bin), m1 = M.at(t0, c, live, DN_NFFT / 2);
        float u0 = 1.f, u1 = 1.f;
        if (phase) {
            float si;
            gl_phase(seed, t0 + c, 0, u0, si);
            gl_phase(seed, t0 + c, DN_NFFT / 2, u1, si);
        }
        z0 = m * u0;
        z1 = m1 * u1;
    }
    __device__ __forceinline__ void bin(int64_t t0, int c, bool live, int bin, float, float, float& zr, float& zi) const {
        const float m = M.at(t0, c, live, bin);
        zr = m, zi = 0.f;
        if (phase) {
            float co, si;
            gl_phase(seed, t0 + c, bin, co, si);
            zr = m * co;
            zi = -(m * si);
        }
    }
};

// rtts_gl_step: M R / |R|, M where |R| = 0
struct GlStepGain {
    GlMag M;
    __device__ __forceinline__ void pair(int64_t t0, int c, bool live, int bin, float re, float im, float& z0, float& z1) const {
        const float m = M.at(t0, c, live, bin), m1 = M.at(t0, c, live, DN_NFFT / 2);
        z0 = m * (re < 0.f ? -1.f : 1.f);                          // R / |R| of a real bin, 1 where R = 0
        z1 = m1 * (im < 0.f ? -1.f : 1.f);
    }
    __device__ __forceinline__ void bin(int64_t t0, int c, bool live, int bin, float re, float im, float& zr, float& zi) const {
        const float m = M.at(t0, c, live, bin);
        zr = m, zi = 0.f;
        const float a = sqrtf(re * re + im * im);
        if (a > 0.f) {
            const float g = m / a;
            zr = g * re;
            zi = g * im;
        }
    }
};

// INIT: no input audio and no forward DFT; else the walk runs on cur - beta * prev (prev null: on cur)
template <bool INIT>
__global__ __launch_bounds__(DN_THREADS) void gl_tile_kernel(const float* __restrict__ cur, const float* __restrict__ prev, float beta,
                                                             const float* __restrict__ mag, int64_t ld_mag, const int64_t* __restrict__ coff,
                                                             const int64_t* __restrict__ soff, const float* __restrict__ basis,
                                                             const float* __restrict__ ibasis, int phase, uint32_t seed,
                                                             float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float gl_lds[];
    const int seg = blockIdx.y;
    const int64_t s0 = soff[seg];
    const int64_t n = soff[seg + 1] - s0;
    if (n <= DN_NFFT / 2) {                                       // fewer than three frames: zeros, written by the first tile
        if (blockIdx.x == 0)
            for (int64_t p = threadIdx.x; p < n; p += DN_THREADS) out[s0 + p] = 0.f;
        return;
    }
    const auto sample = [=](int64_t s) { return prev ? fmaf(-beta, prev[s], cur[s]) : cur[s]; };
    const GlMag M{mag + coff[seg], ld_mag};
    if constexpr (INIT)
        stft_tile_walk<false>(gl_lds, soff, basis, ibasis, out, sample, GlInitGain{M, phase, seed});
    else
        stft_tile_walk<true>(gl_lds, soff, basis, ibasis, out, sample, GlStepGain{M});
}

static RttsLdsState g_gl_init_lds, g_gl_step_lds;

// The offsets of a call, validated on the host copies: utterance s has n_s = 256 L_s samples and L_s + 1 columns of M.
static int gl_check_offsets(const char* who, const int64_t* soff, const int64_t* coff, int nseg, int64_t ld_mag, int hop, int64_t* u_longest) {
    RTTS_REQUIRE(soff[0] >= 0 && coff[0] >= 0, "%s: offsets must not be negative", who);
    for (int s = 0; s < nseg; ++s) {
        const int64_t n = soff[s + 1] - soff[s], cols = coff[s + 1] - coff[s];
        RTTS_REQUIRE(n >= 0 && n % hop == 0, "%s: utterance %d has %lld samples; sample_offsets must step by multiples of hop = %d", who, s,
                     (long long)n, hop);
        RTTS_REQUIRE(cols == n / hop + 1, "%s: utterance %d of %lld samples owns %lld columns of mag; col_offsets must step by frames + 1 = %lld",
                     who, s, (long long)n, (long long)cols, (long long)(n / hop + 1));
    }
    RTTS_REQUIRE(coff[nseg] <= ld_mag, "%s: col_offsets end at %lld, past ld_mag = %lld", who, (long long)coff[nseg], (long long)ld_mag);
    return stft_tile_longest(who, soff, nseg, false, u_longest);
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
    if (stft_tile_check_shape("rtts_gl_init", n_fft, hop, nseg)) return -1;
    RTTS_REQUIRE(phase == 0 || phase == 1, "rtts_gl_init: phase must be 0 (zero) or 1 (hash) (got %d)", phase);
    int64_t u_longest;
    if (gl_check_offsets("rtts_gl_init", sample_offsets_host, col_offsets_host, nseg, ld_mag, hop, &u_longest)) return -1;
    unsigned tiles;
    if (stft_tile_count("rtts_gl_init", u_longest, &tiles)) return -1;
    RTTS_ENTER(stream);
    RTTS_ENSURE_LDS("rtts_gl_init", gl_tile_kernel<true>, DN_LDS_BYTES, g_gl_init_lds);
    hipLaunchKernelGGL(gl_tile_kernel<true>, dim3(tiles, (unsigned)nseg), dim3(DN_THREADS), DN_LDS_BYTES, (hipStream_t)stream,
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
    if (stft_tile_check_shape("rtts_gl_step", n_fft, hop, nseg)) return -1;
    RTTS_REQUIRE(isfinite(beta) && beta >= 0.f && beta < 1.f, "rtts_gl_step: beta must be in [0, 1) (got %g)", (double)beta);
    int64_t u_longest;
    if (gl_check_offsets("rtts_gl_step", sample_offsets_host, col_offsets_host, nseg, ld_mag, hop, &u_longest)) return -1;
    RTTS_REQUIRE(!stft_tile_overlap(out, cur, sample_offsets_host, nseg), "rtts_gl_step: out must not overlap cur (a tile reads its neighbours' input)");
    RTTS_REQUIRE(!stft_tile_overlap(out, prev, sample_offsets_host, nseg), "rtts_gl_step: out must not overlap prev (a tile reads its neighbours' input)");
    unsigned tiles;
    if (stft_tile_count("rtts_gl_step", u_longest, &tiles)) return -1;
    RTTS_ENTER(stream);
    RTTS_ENSURE_LDS("rtts_gl_step", gl_tile_kernel<false>, DN_LDS_BYTES, g_gl_step_lds);
    hipLaunchKernelGGL(gl_tile_kernel<false>, dim3(tiles, (unsigned)nseg), dim3(DN_THREADS), DN_LDS_BYTES, (hipStream_t)stream, cur,
                       beta > 0.f ? prev : (const float*)nullptr, beta, mag, ld_mag, col_offsets, sample_offsets, dft_basis, idft_basis, 0, 0u,
                       out);
    RTTS_LAUNCH_CHECK("rtts_gl_step");
    return 0;
}
