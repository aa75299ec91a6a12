// Vocoder denoiser for a ragged batch of utterances, one launch (rtts_denoise of include/rtts.h): STFT, subtract the vocoder's bias
// spectrum from the magnitudes, inverse STFT with the original phase.  The launch is the tile walk of stft_tile.h on the audio
// itself, with the gain max(|X| - strength * bias, 0) / |X| (0 where |X| = 0) on every bin.
//
// Invariants: everything is f32.  An utterance's output bits depend on its own samples, the bias and the strength only -- not on
// its slot in the batch, the other utterances or the grid size -- and two calls give the same bits.
#include "stft_tile.h"

#include <math.h>

struct DenoiseGain {
    const float* __restrict__ bias;
    float strength;
    __device__ __forceinline__ void pair(int64_t, int, bool, int, float re, float im, float& z0, float& z1) const {
        const float m0 = fabsf(re), m1 = fabsf(im);
        const float g0 = m0 > 0.f ? fmaxf(m0 - strength * bias[0], 0.f) / m0 : 0.f;
        const float g1 = m1 > 0.f ? fmaxf(m1 - strength * bias[DN_NFFT / 2], 0.f) / m1 : 0.f;
        z0 = g0 * re;
        z1 = g1 * im;
    }
    __device__ __forceinline__ void bin(int64_t, int, bool, int bin, float re, float im, float& zr, float& zi) const {
        const float mag = sqrtf(re * re + im * im);
        const float g = mag > 0.f ? fmaxf(mag - strength * bias[bin], 0.f) / mag : 0.f;
        zr = g * re;
        zi = g * im;
    }
};

__global__ __launch_bounds__(DN_THREADS) void denoise_kernel(const float* __restrict__ audio, const int64_t* __restrict__ soff,
                                                             const float* __restrict__ basis, const float* __restrict__ ibasis,
                                                             const float* __restrict__ bias, float strength, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float dn_lds[];
    stft_tile_walk<true>(dn_lds, soff, basis, ibasis, out, [=](int64_t s) { return audio[s]; }, DenoiseGain{bias, strength});
}

static RttsLdsState g_denoise_lds;

extern "C" int rtts_denoise(const float* audio, const int64_t* sample_offsets_host, const int64_t* sample_offsets, int nseg,
                            const float* dft_basis, const float* idft_basis, const float* bias, float strength, int n_fft, int hop,
                            float* out, void* stream) {
    RTTS_REQUIRE(audio && sample_offsets_host && sample_offsets && dft_basis && idft_basis && bias && out,
                 "rtts_denoise: null pointer argument");
    if (stft_tile_check_shape("rtts_denoise", n_fft, hop, nseg)) return -1;
    RTTS_REQUIRE(isfinite(strength) && strength >= 0.f, "rtts_denoise: strength must be finite and >= 0 (got %g)", (double)strength);
    int64_t u_longest;
    if (stft_tile_longest("rtts_denoise", sample_offsets_host, nseg, true, &u_longest)) return -1;
    RTTS_REQUIRE(!stft_tile_overlap(out, audio, sample_offsets_host, nseg),
                 "rtts_denoise: out must not overlap audio (a tile reads its neighbours' input)");
    unsigned tiles;
    if (stft_tile_count("rtts_denoise", u_longest, &tiles)) return -1;
    RTTS_ENTER(stream);
    RTTS_ENSURE_LDS("rtts_denoise", denoise_kernel, DN_LDS_BYTES, g_denoise_lds);
    hipLaunchKernelGGL(denoise_kernel, dim3(tiles, (unsigned)nseg), dim3(DN_THREADS), DN_LDS_BYTES, (hipStream_t)stream, audio,
                       sample_offsets, dft_basis, idft_basis, bias, strength, out);
    RTTS_LAUNCH_CHECK("rtts_denoise");
    return 0;
}
