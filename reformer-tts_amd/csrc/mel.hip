// Audio -> log-mel spectrogram for a ragged batch of utterances, one launch (rtts_mel_spectrogram of include/rtts.h).
//
// A workgroup (8 waves) takes MEL_FT consecutive frames of ONE utterance:
//   1. stages the audio span the frames share, reflect-padded per utterance (stft_reflect of stft_tile.h), in LDS once (frame t
//      is span[t * hop, + n_fft));
//   2. short-time DFT as a GEMM on v_mfma_f32_32x32x2_f32: D[bin][frame] = sum_n basis[n][col] * span[frame * hop + n], the
//      basis (window folded in) streamed from L2 straight into the A operand, the frames read from LDS as the B operand.  The
//      real DFT of n_fft samples has exactly n_fft independent real outputs, so the basis is square: columns [0, n_fft/2) are the
//      cosines of bins 0 .. n_fft/2-1, columns [n_fft/2, n_fft) the sines of the same bins -- except column n_fft/2, whose
//      sine (of bin 0) is identically zero and which holds the cosine of the Nyquist bin instead.  A wave owns n_fft/512
//      tiles of 32 bins, cosine and sine accumulators side by side, so a bin's magnitude never leaves its lane;
//   3. |X|^power goes to LDS as [bin][frame] rows (n_fft/2 + 1 bins and one zero row: the mel product walks k in pairs), over the
//      span, which nobody reads any more;
//   4. mel = M (n_mels, n_fft/2+1) x magnitudes on the same instruction, one 32-row tile of M per wave, A from global memory;
//   5. log(max(., clip)) and the store, 32 consecutive frames of a mel row per half wave.
// Everything is f32, and every output element is ONE k-ordered fmaf chain over n (then over bins): the instruction is bit for bit
// that chain, so a frame's values do not depend on its place in the tile, the utterance or the batch.
#include "stft_tile.h"                                            // stft_reflect

#define MEL_THREADS 512
#define MEL_WAVES 8

template <int NFFT>
struct MelShape {
    static constexpr int HOP = NFFT / 4;
    static constexpr int LOG_HOP = NFFT == 512 ? 7 : NFFT == 1024 ? 8 : 9;
    static constexpr int NB = NFFT / 2 + 1;                       // bins
    static constexpr int FT = NFFT == 2048 ? 16 : 32;             // frames of a workgroup (the magnitudes of 32 do not fit at 2048)
    static constexpr int NBT = NFFT / 2 / 32 / MEL_WAVES;         // 32-bin tiles of a wave
    static constexpr int SPAN = (FT - 1) * HOP + NFFT;            // samples the frames of a tile cover
    // sample p of the span lives at p + p / HOP: frame t starts at t * (HOP + 1), so the 32 frames of a B-operand read sit on 32 banks
    static constexpr int SPAN_LDS = (SPAN + SPAN / HOP + 4) & ~3;
    static constexpr int MAG_LDS = (NB + 1) * FT;
    // the magnitudes overwrite the span once every wave is through with it: two workgroups fit a CU at n_fft <= 1024
    static constexpr size_t LDS_BYTES = (size_t)(SPAN_LDS > MAG_LDS ? SPAN_LDS : MAG_LDS) * sizeof(float);
};

template <int NFFT>
__global__ __launch_bounds__(MEL_THREADS) void mel_kernel(const float* __restrict__ audio, const int64_t* __restrict__ soff,
                                                          const int64_t* __restrict__ foff, const float* __restrict__ basis,
                                                          const float* __restrict__ melw, int n_mels, int power, float clip,
                                                          float* __restrict__ out, int64_t ld_out) {
    using S = MelShape<NFFT>;
    constexpr int HOP = S::HOP, NB = S::NB, FT = S::FT, NBT = S::NBT, NC = 2 * NBT;
    extern __shared__ __attribute__((aligned(16))) float mel_lds[];
    float* xs = mel_lds;
    float* mag = mel_lds;                                         // after the barrier that ends the DFT

    const int seg = blockIdx.y;
    const int64_t s0 = soff[seg];
    const int64_t n = soff[seg + 1] - s0;
    const int64_t frames = n / HOP + 1;
    const int64_t t0 = (int64_t)blockIdx.x * FT;
    if (t0 >= frames) return;                                     // the grid is sized for the longest utterance of the call

    const int tid = threadIdx.x;
    const float* x = audio + s0;
    for (int p = tid; p < S::SPAN; p += MEL_THREADS) {
        int64_t s = t0 * HOP - NFFT / 2 + p;
        xs[p + (p >> S::LOG_HOP)] = stft_reflect(n, s) ? x[s] : 0.f;
    }
    __syncthreads();

    const int w = tid >> 6, l = tid & 63, c = l & 31, h = l >> 5;
    const int tcol = c & (FT - 1);                                // FT = 16: columns 16-31 repeat 0-15 and are dropped
    {
        constexpr int U = NBT >= 4 ? 2 : 4;                       // k-steps (of two samples) per prefetched block
        constexpr int NBLK = NFFT / 2 / U, BPQ = HOP / 2 / U;
        f32x16 acc[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) acc[i] = f32x16{0};
        const float* ap = basis + (size_t)h * NFFT + w * NBT * 32 + c;
        const float* bp = xs + tcol * (HOP + 1) + h;
        float a_cur[U][NC], a_nxt[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < NBT; ++j) {
                a_cur[u][2 * j] = ap[(size_t)u * 2 * NFFT + j * 32];
                a_cur[u][2 * j + 1] = ap[(size_t)u * 2 * NFFT + NFFT / 2 + j * 32];
            }
        for (int blk = 0; blk < NBLK; ++blk) {
            const float* an = ap + (size_t)(blk + 1 < NBLK ? blk + 1 : blk) * U * 2 * NFFT;      // the last block is loaded twice
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < NBT; ++j) {
                    a_nxt[u][2 * j] = an[(size_t)u * 2 * NFFT + j * 32];
                    a_nxt[u][2 * j + 1] = an[(size_t)u * 2 * NFFT + NFFT / 2 + j * 32];
                }
            // samples n0 + h, n0 = 2 * U * blk: a block never straddles a multiple of HOP, where the padded image skips a word
            const float* b0 = bp + (blk / BPQ) * (HOP + 1) + (blk % BPQ) * 2 * U;
            float b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) b[u] = b0[2 * u];
            // the next block's loads stay in front of this block's products (left alone, the scheduler sinks them to the end of the
            // body, and every block then waits out a full L2 round trip)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int i = 0; i < NC; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[u][i], b[u], acc[i], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int i = 0; i < NC; ++i) a_cur[u][i] = a_nxt[u][i];
        }
        __syncthreads();                                          // every wave has read its last sample: the span becomes the magnitudes
        if (tid < FT) mag[NB * FT + tid] = 0.f;
        // acc[2j][r] / acc[2j+1][r]: real / imaginary part of bin 32 * (w * NBT + j) + (r & 3) + 8 * (r >> 2) + 4 * h, frame c
        if (c < FT) {
#pragma unroll
            for (int j = 0; j < NBT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int bin = (w * NBT + j) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float re = acc[2 * j][r], im = acc[2 * j + 1][r];
                    if (bin == 0) {                               // bins 0 and n_fft/2 are real: they share the column pair
                        mag[c] = power == 2 ? re * re : fabsf(re);
                        mag[(NFFT / 2) * FT + c] = power == 2 ? im * im : fabsf(im);
                    } else {
                        const float p2 = re * re + im * im;
                        mag[bin * FT + c] = power == 2 ? p2 : sqrtf(p2);
                    }
                }
        }
    }
    __syncthreads();

    if (w * 32 >= n_mels) return;
    const int m = w * 32 + c;                                     // row of M this lane feeds
    const float* mp = melw + (size_t)(m < n_mels ? m : n_mels - 1) * NB;
    const float* bm = mag + h * FT + tcol;
    f32x16 o = f32x16{0};
    // k = 2 p + h in pairs p: n_fft / 4 pairs in blocks of MU (M's values loaded a block ahead of their products, unconditionally, so
    // that they travel together), then the pair (Nyquist bin, zero row)
    constexpr int MU = 8;
    const bool mrow = m < n_mels;
    for (int p0 = 0; p0 < NFFT / 4; p0 += MU) {
        float a[MU];
#pragma unroll
        for (int u = 0; u < MU; ++u) a[u] = mp[2 * (p0 + u) + h];
#pragma unroll
        for (int u = 0; u < MU; ++u) o = __builtin_amdgcn_mfma_f32_32x32x2f32(mrow ? a[u] : 0.f, bm[2 * (p0 + u) * FT], o, 0, 0, 0);
    }
    {
        const float a = mp[NFFT / 2];                             // h = 1 pairs with the zero row
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(mrow && h == 0 ? a : 0.f, bm[(NFFT / 2) * FT], o, 0, 0, 0);
    }
    const int64_t t = t0 + c;
    if (c < FT && t < frames) {
        float* op = out + foff[seg] + t;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = w * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row < n_mels) op[(int64_t)row * ld_out] = logf(fmaxf(o[r], clip));
        }
    }
}

static RttsLdsState g_mel_lds[3];

extern "C" int64_t rtts_mel_frames(int64_t n_samples, int hop) {
    if (n_samples < 1 || hop < 1) {
        rtts_set_error("rtts_mel_frames: n_samples and hop must be positive (got %lld, %d)", (long long)n_samples, hop);
        return -1;
    }
    return n_samples / hop + 1;
}

template <int NFFT>
static int mel_launch(int slot, const float* audio, const int64_t* soff, const int64_t* foff, int nseg, int64_t max_frames,
                      const float* basis, const float* melw, int n_mels, int power, float clip, float* out, int64_t ld_out, void* stream) {
    using S = MelShape<NFFT>;
    static_assert(S::LDS_BYTES <= 160 * 1024, "a tile's audio span and magnitudes must fit the 160 KB of LDS");
    RTTS_ENSURE_LDS("rtts_mel_spectrogram", mel_kernel<NFFT>, S::LDS_BYTES, g_mel_lds[slot]);
    const int64_t tiles = (max_frames + S::FT - 1) / S::FT;
    RTTS_REQUIRE(tiles <= 0x7fffffff, "rtts_mel_spectrogram: an utterance of %lld frames is too long for one launch", (long long)max_frames);
    hipLaunchKernelGGL(mel_kernel<NFFT>, dim3((unsigned)tiles, (unsigned)nseg), dim3(MEL_THREADS), S::LDS_BYTES, (hipStream_t)stream, audio,
                       soff, foff, basis, melw, n_mels, power, clip, out, ld_out);
    RTTS_LAUNCH_CHECK("rtts_mel_spectrogram");
    return 0;
}

extern "C" int rtts_mel_spectrogram(const float* audio, const int64_t* sample_offsets_host, const int64_t* frame_offsets_host,
                                    const int64_t* sample_offsets, const int64_t* frame_offsets, int nseg, const float* dft_basis,
                                    const float* mel_basis, int n_fft, int hop, int n_mels, int power, float clip, float* out,
                                    int64_t ld_out, void* stream) {
    RTTS_REQUIRE(audio && sample_offsets_host && frame_offsets_host && sample_offsets && frame_offsets && dft_basis && mel_basis && out,
                 "rtts_mel_spectrogram: null pointer argument");
    RTTS_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "rtts_mel_spectrogram: n_fft must be 512, 1024 or 2048 (got %d)", n_fft);
    RTTS_REQUIRE(hop == n_fft / 4, "rtts_mel_spectrogram: hop must be n_fft / 4 = %d (got %d)", n_fft / 4, hop);
    RTTS_REQUIRE(n_mels >= 1 && n_mels <= 128, "rtts_mel_spectrogram: n_mels must be in 1..128 (got %d)", n_mels);
    RTTS_REQUIRE(power == 1 || power == 2, "rtts_mel_spectrogram: power must be 1 (magnitude) or 2 (squared magnitude), got %d", power);
    RTTS_REQUIRE(clip > 0.f, "rtts_mel_spectrogram: clip must be positive (got %g)", (double)clip);
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "rtts_mel_spectrogram: nseg must be in 1..65535 (got %d)", nseg);
    int64_t max_frames = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t n = sample_offsets_host[s + 1] - sample_offsets_host[s];
        RTTS_REQUIRE(sample_offsets_host[s] >= 0 && n > n_fft / 2,
                     "rtts_mel_spectrogram: utterance %d has %lld samples; reflect padding needs more than n_fft / 2 = %d", s, (long long)n,
                     n_fft / 2);
        const int64_t frames = n / hop + 1;
        RTTS_REQUIRE(frame_offsets_host[s] >= 0 && frame_offsets_host[s + 1] - frame_offsets_host[s] >= frames,
                     "rtts_mel_spectrogram: utterance %d has %lld frames, its slot in frame_offsets holds %lld", s, (long long)frames,
                     (long long)(frame_offsets_host[s + 1] - frame_offsets_host[s]));
        if (frames > max_frames) max_frames = frames;
    }
    RTTS_REQUIRE(ld_out >= frame_offsets_host[nseg], "rtts_mel_spectrogram: ld_out %lld is shorter than the %lld frames of frame_offsets",
                 (long long)ld_out, (long long)frame_offsets_host[nseg]);
    RTTS_ENTER(stream);
    switch (n_fft) {
        case 512: return mel_launch<512>(0, audio, sample_offsets, frame_offsets, nseg, max_frames, dft_basis, mel_basis, n_mels, power, clip, out, ld_out, stream);
        case 1024: return mel_launch<1024>(1, audio, sample_offsets, frame_offsets, nseg, max_frames, dft_basis, mel_basis, n_mels, power, clip, out, ld_out, stream);
        default: return mel_launch<2048>(2, audio, sample_offsets, frame_offsets, nseg, max_frames, dft_basis, mel_basis, n_mels, power, clip, out, ld_out, stream);
    }
}
