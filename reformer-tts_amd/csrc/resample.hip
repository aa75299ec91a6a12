// Sample-rate conversion of a ragged batch of utterances, one launch (rtts_resample of include/rtts.h): the windowed-sinc
// polyphase filter of torchaudio's Resample (lowpass_filter_width 6, rolloff 0.99, Hann window), which the reference runs on every
// clip before it makes a spectrogram (dataset/convert.py:131-146).
//
// With the rates reduced to orig_red : new_red, output k = j * new_red + p of an utterance is
//     out[k] = sum_t x[j * orig_red + first[p] + t] * w[t][p],    t = 0 .. taps-1,    x = 0 outside [0, N)
// (first and w: dataset/audio.py resample_tables, float64 on the host, rounded once).  A workgroup takes RS_TILE consecutive outputs
// of ONE utterance:
//   1. the inputs they share -- [start(k0), start(k0 + RS_TILE - 1) + taps), start(k) = j * orig_red + first[p] is non-decreasing in
//      k -- go to LDS once, zero filled outside the utterance; 16-bit interleaved PCM is converted here (channel 0, * 2^-15);
//   2. the RS_TILE (or all new_red, if fewer) phases of first[] and, when they fit beside the span, of w go to LDS as well; w is stored
//      [tap][phase] in memory and in LDS, so the lanes of a wave (consecutive outputs = consecutive phases) read consecutive words.
//      A slice that does not fit is read from global memory in the same pattern: the table is read-only, shared by every workgroup,
//      and stays in L2;
//   3. lane l computes outputs k0 + l, k0 + 256 + l, ...: one fmaf chain over t in ascending order, padded taps and samples outside
//      the utterance taking part as zeros, then one store -- a wave writes 256 consecutive bytes.
// The chain of an output depends on nothing but its utterance's samples: not on the tile, not on the utterance's place in the batch.
#include "rtts_common.h"

#define RS_THREADS 256
#define RS_LDS_WORDS 16384                                        // 64 KB: span + first[] slice (+ coefficient slice)

static_assert(RTTS_RESAMPLE_TILE % RS_THREADS == 0, "a lane owns RTTS_RESAMPLE_TILE / RS_THREADS outputs");

template <int FMT>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const void* __restrict__ audio, int channels, const int64_t* __restrict__ ioff,
                                                              const int64_t* __restrict__ ooff, const int32_t* __restrict__ first,
                                                              const float* __restrict__ wt, int orig_r, int new_r, int taps, int span,
                                                              int pw, int coef_lds, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* xs = rs_lds;                                           // span samples
    int* fs = reinterpret_cast<int*>(rs_lds + span);              // pw entries of first[]
    float* cs = rs_lds + span + pw;                               // taps rows of pw coefficients, if coef_lds

    const int seg = blockIdx.y;
    const int64_t i0 = ioff[seg];
    const int64_t n = ioff[seg + 1] - i0;
    const int64_t m = (n * new_r + orig_r - 1) / orig_r;
    const int64_t k0 = (int64_t)blockIdx.x * RTTS_RESAMPLE_TILE;
    if (k0 >= m) return;                                          // the grid is sized for the longest utterance of the call

    const int tid = threadIdx.x;
    const int64_t j0 = k0 / new_r;
    const int p0 = (int)(k0 - j0 * new_r);
    const int f0 = first[p0];
    const int64_t lo = j0 * orig_r + f0;                          // first input of the tile's first output: the span starts here
    const bool whole = new_r <= RTTS_RESAMPLE_TILE;               // the slices hold every phase, at its own index

    for (int i = tid; i < span; i += RS_THREADS) {
        const int64_t s = lo + i;
        float v = 0.f;
        if (s >= 0 && s < n) {
            if (FMT == 0)
                v = static_cast<const float*>(audio)[i0 + s];
            else
                v = (float)static_cast<const int16_t*>(audio)[(i0 + s) * channels] * (1.f / 32768.f);
        }
        xs[i] = v;
    }
    for (int q = tid; q < pw; q += RS_THREADS) {
        int p = q;
        if (!whole) {                                             // slot q = phase of output k0 + q
            p = p0 + q;
            if (p >= new_r) p -= new_r;
        }
        fs[q] = first[p];
        if (coef_lds)
            for (int t = 0; t < taps; ++t) cs[t * pw + q] = wt[(size_t)t * new_r + p];
    }
    __syncthreads();

    float* o = out + ooff[seg] + k0;
    const int last = span - taps;
#pragma unroll
    for (int r = 0; r < RTTS_RESAMPLE_TILE / RS_THREADS; ++r) {
        const int q = r * RS_THREADS + tid;
        if (k0 + q >= m) break;
        const int pp = p0 + q;
        const int dj = pp / new_r;
        const int p = pp - dj * new_r;
        const int slot = whole ? p : q;
        // start(k0 + q) - start(k0): in [0, span - taps] by the monotonicity above; the clamp keeps a `first` that breaks the contract
        // inside the span
        int b = dj * orig_r + fs[slot] - f0;
        b = b < 0 ? 0 : (b > last ? last : b);
        const float* x = xs + b;
        float acc = 0.f;
        if (coef_lds) {
            const float* c = cs + slot;
#pragma unroll 4
            for (int t = 0; t < taps; ++t) acc = fmaf(x[t], c[t * pw], acc);
        } else {
            const float* c = wt + p;
#pragma unroll 4
            for (int t = 0; t < taps; ++t) acc = fmaf(x[t], c[(size_t)t * new_r], acc);
        }
        o[q] = acc;
    }
}

static int rs_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

extern "C" int64_t rtts_resample_len(int64_t n_samples, int orig, int new_) {
    if (n_samples < 1 || orig < 1 || new_ < 1) {
        rtts_set_error("rtts_resample_len: n_samples and the rates must be positive (got %lld, %d, %d)", (long long)n_samples, orig, new_);
        return -1;
    }
    const int g = rs_gcd(orig, new_);
    const int64_t o = orig / g, w = new_ / g;
    if (n_samples > (INT64_MAX - o) / w) {
        rtts_set_error("rtts_resample_len: n_samples * new / gcd overflows 64 bits (got %lld, %d, %d)", (long long)n_samples, orig, new_);
        return -1;
    }
    return (n_samples * w + o - 1) / o;
}

extern "C" int rtts_resample(const void* audio, int in_format, int channels, const int64_t* in_offsets_host, const int64_t* out_offsets_host,
                             const int64_t* in_offsets, const int64_t* out_offsets, int nseg, const int32_t* first, const float* taps_table,
                             int orig_red, int new_red, int taps, float* out, void* stream) {
    RTTS_REQUIRE(audio && in_offsets_host && out_offsets_host && in_offsets && out_offsets && first && taps_table && out,
                 "rtts_resample: null pointer argument");
    RTTS_REQUIRE(in_format == 0 || in_format == 1, "rtts_resample: in_format must be 0 (f32 mono) or 1 (int16 interleaved), got %d", in_format);
    RTTS_REQUIRE(in_format == 0 ? channels == 1 : (channels >= 1 && channels <= 8),
                 "rtts_resample: channels must be 1 for f32 input and 1..8 for int16 input (got %d)", channels);
    RTTS_REQUIRE(orig_red >= 1 && new_red >= 1 && orig_red != new_red,
                 "rtts_resample: orig_red and new_red must be positive and different (got %d, %d)", orig_red, new_red);
    RTTS_REQUIRE(taps >= 1 && taps <= RTTS_RESAMPLE_MAX_TAPS, "rtts_resample: taps must be in 1..%d (got %d)", RTTS_RESAMPLE_MAX_TAPS, taps);
    RTTS_REQUIRE((int64_t)new_red * taps <= RTTS_RESAMPLE_MAX_TABLE, "rtts_resample: the table of new_red * taps = %lld coefficients exceeds %d",
                 (long long)new_red * taps, RTTS_RESAMPLE_MAX_TABLE);
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "rtts_resample: nseg must be in 1..65535 (got %d)", nseg);
    // inputs the RTTS_RESAMPLE_TILE outputs of a workgroup share, and the phases it keeps beside them
    const int64_t span = ((int64_t)(RTTS_RESAMPLE_TILE - 1) * orig_red + new_red - 1) / new_red + 1 + taps;
    const int pw = new_red < RTTS_RESAMPLE_TILE ? new_red : RTTS_RESAMPLE_TILE;
    RTTS_REQUIRE(span + pw <= RS_LDS_WORDS,
                 "rtts_resample: orig_red / new_red = %d / %d with %d taps: the %lld input samples of a tile of %d outputs exceed the LDS budget "
                 "of %d words", orig_red, new_red, taps, (long long)span, RTTS_RESAMPLE_TILE, RS_LDS_WORDS - pw);
    const int coef_lds = span + pw + (int64_t)pw * taps <= RS_LDS_WORDS;
    int64_t max_out = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t n = in_offsets_host[s + 1] - in_offsets_host[s];
        RTTS_REQUIRE(in_offsets_host[s] >= 0 && n >= 1 && n <= ((int64_t)1 << 40),
                     "rtts_resample: in_offsets must start at >= 0 and increase: utterance %d has %lld frames (1..2^40)", s, (long long)n);
        const int64_t m = (n * new_red + orig_red - 1) / orig_red;
        RTTS_REQUIRE(out_offsets_host[s] >= 0 && out_offsets_host[s + 1] - out_offsets_host[s] >= m,
                     "rtts_resample: utterance %d gives %lld samples, its slot in out_offsets holds %lld", s, (long long)m,
                     (long long)(out_offsets_host[s + 1] - out_offsets_host[s]));
        if (m > max_out) max_out = m;
    }
    const int64_t tiles = (max_out + RTTS_RESAMPLE_TILE - 1) / RTTS_RESAMPLE_TILE;
    RTTS_REQUIRE(tiles <= 0x7fffffff, "rtts_resample: an utterance of %lld output samples is too long for one launch", (long long)max_out);
    RTTS_ENTER(stream);
    const size_t lds = (size_t)(span + pw + (coef_lds ? (int64_t)pw * taps : 0)) * sizeof(float);
    const dim3 grid((unsigned)tiles, (unsigned)nseg), block(RS_THREADS);
    if (in_format == 0)
        hipLaunchKernelGGL(resample_kernel<0>, grid, block, lds, (hipStream_t)stream, audio, channels, in_offsets, out_offsets, first,
                           taps_table, orig_red, new_red, taps, (int)span, pw, coef_lds, out);
    else
        hipLaunchKernelGGL(resample_kernel<1>, grid, block, lds, (hipStream_t)stream, audio, channels, in_offsets, out_offsets, first,
                           taps_table, orig_red, new_red, taps, (int)span, pw, coef_lds, out);
    RTTS_LAUNCH_CHECK("rtts_resample");
    return 0;
}
