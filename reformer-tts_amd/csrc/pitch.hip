// F0 contours of a ragged batch of utterances by YIN, one launch (rtts_pitch_yin of include/rtts.h), and the comparison of two
// contours, one launch (rtts_f0_compare).  Not in the reference.
//
// rtts_pitch_yin.  A workgroup (8 waves) takes RTTS_PITCH_TILE_FRAMES consecutive frames of ONE utterance:
//   1. stages the samples the frames share, zero outside the utterance, in LDS once: frame t reads x[t hop - 768, + 1536), so a
//      tile of FT frames reads (FT - 1) hop + 1536 samples -- a whole number of hop blocks.  While staging, a block that holds a
//      non-finite sample raises its flag (plain stores of the same value: no atomics);
//   2. hop-block partial sums.  The window of frame t is the W / hop hop blocks t .. t + W / hop - 1 (block b = samples
//      [b hop - 768, + hop)), and neighbouring frames share all but one of them, so the tile computes
//          P_b(tau) = sum_{j in block b} (x[j] - x[j + tau])^2,    tau = 1 .. 512,
//      once per block, FT - 1 + W / hop blocks in all, each as ONE fmaf chain over ascending j: P = fmaf(e, e, P), e the rounded
//      difference.  The direct form: every term is a square, nothing cancels (the energy form r(0) + r_tau(0) - 2 r(tau) is a
//      small difference of large numbers exactly at the period, where the decision falls).
//      Lanes own lags: lane g of 128 (two waves) owns the four lags 1 + 4 g .. 4 + 4 g and walks the block four samples at a time.
//      A step holds x[j + 1 + 4 g .. + 8) in registers -- two 16-byte LDS reads at consecutive 16-byte slots across the lanes
//      (conflict-free), one of them kept from the step before -- and reads x[j .. j + 4) as broadcasts (every lane the same
//      address): five LDS reads feed 16 subtractions and 16 fmaf.  The image is stored three words in, so that sample
//      j + 1 + 4 g sits on a 16-byte boundary for j a multiple of four.  The four wave pairs take the blocks round robin;
//   3. per frame (a wave takes frames w and w + 8 of the tile): d(tau) = P_t(tau) + P_{t+1}(tau) + ... left to right; lane l owns
//      the eight lags 1 + 8 l .. 8 + 8 l, sums them in ascending order, the 64 lane totals go through a Hillis-Steele scan
//      (distances 1, 2, .. 32), and the running sum of a lag is (sum of the lanes before) + (the lane's own partial sum);
//      d'(tau) = d(tau) * tau / that, goes to LDS (and to cmnd when asked), then the threshold search (ballot), the descent to the
//      local minimum, the three-point interpolation and the two stores.
// Every sum has one order that depends on hop alone: an utterance's outputs are bitwise the same alone and anywhere in a batch,
// and from call to call.  No atomics, nothing read back.
//
// rtts_f0_compare.  One workgroup; wave w takes utterances w, w + 4, ...: lanes stride over the frames in f64, the 64 partial
// rows are folded by halving distances, lane 0 stores the row.  Then the five columns are summed over the utterances in
// ascending order by five threads.
#include "score_common.h"

#define PITCH_THREADS 512
#define PITCH_WAVES 8
#define PITCH_W 1024                                              // integration window
#define PITCH_L RTTS_PITCH_MAX_LAG
#define PITCH_FT RTTS_PITCH_TILE_FRAMES
#define PITCH_REACH (PITCH_W + PITCH_L)                           // samples a frame reads

static_assert(PITCH_L == 512 && PITCH_FT == 2 * PITCH_WAVES, "the lane mappings below are written for 512 lags and 16 frames");

template <int HOP>
struct PitchShape {
    static constexpr int NBW = PITCH_W / HOP;                     // hop blocks of a window
    static constexpr int NB = PITCH_FT - 1 + NBW;                 // hop blocks whose partial sums a tile needs
    static constexpr int NBF = PITCH_FT - 1 + PITCH_REACH / HOP;  // hop blocks a tile reads
    static constexpr int SPAN = NBF * HOP;
    static constexpr int XS = SPAN + 4;                           // the image sits three words in
    static constexpr int DP = PITCH_L + 4;                        // d'(0 .. 512) of one wave's frame
    static constexpr size_t LDS_BYTES = (size_t)(XS + NB * PITCH_L + PITCH_WAVES * DP + 32) * sizeof(float);
};

template <int HOP>
__global__ __launch_bounds__(PITCH_THREADS) void pitch_yin_kernel(const float* __restrict__ audio, const int64_t* __restrict__ soff,
                                                                  const int64_t* __restrict__ foff, int tau_min, int tau_max,
                                                                  float threshold, float sample_rate, float* __restrict__ f0,
                                                                  float* __restrict__ aper, float* __restrict__ cmnd) {
    using S = PitchShape<HOP>;
    extern __shared__ __attribute__((aligned(16))) float pitch_lds[];
    float* xs = pitch_lds;                                        // S::XS
    float* part = xs + S::XS;                                     // NB x 512, lag tau at [tau - 1]
    float* dps = part + S::NB * PITCH_L;                          // 8 x DP
    int* bad = reinterpret_cast<int*>(dps + PITCH_WAVES * S::DP); // NBF <= 27 flags

    const int seg = blockIdx.y;
    const int64_t s0 = soff[seg];
    const int64_t n = soff[seg + 1] - s0;
    const int64_t frames = n / HOP + 1;
    const int64_t t0 = (int64_t)blockIdx.x * PITCH_FT;
    if (t0 >= frames) return;                                     // the grid is sized for the longest utterance of the call

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const float* x = audio + s0;
    if (tid < 32) bad[tid] = 0;
    if (tid < 3) xs[tid] = 0.f;
    if (tid == 3) xs[S::XS - 1] = 0.f;
    __syncthreads();
    const int64_t first = t0 * HOP - PITCH_REACH / 2;
    for (int p = tid; p < S::SPAN; p += PITCH_THREADS) {
        const int64_t s = first + p;
        const float v = (s >= 0 && s < n) ? x[s] : 0.f;
        xs[p + 3] = v;
        if (!(fabsf(v) <= 3.402823466e38f)) bad[p / HOP] = 1;
    }
    __syncthreads();

    {
        const int g = (w & 1) * 64 + l;                           // lags 1 + 4 g + r
        for (int b = w >> 1; b < S::NB; b += PITCH_WAVES / 2) {
            const float* xb = xs + b * HOP + 3;                   // sample j of the block
            const f32x4* xl = reinterpret_cast<const f32x4*>(xs + b * HOP + 4 + 4 * g);      // samples j + 1 + 4 g ..
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            f32x4 lo = xl[0];
#pragma unroll 4
            for (int j = 0; j < HOP; j += 4) {
                const f32x4 hi = xl[j / 4 + 1];
                const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float xi = xb[j + i];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = xi - v[i + r];
                        acc[r] = fmaf(e, e, acc[r]);
                    }
                }
                lo = hi;
            }
            *reinterpret_cast<f32x4*>(part + b * PITCH_L + 4 * g) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        }
    }
    __syncthreads();

    float* dp = dps + w * S::DP;
    for (int k = 0; k < PITCH_FT / PITCH_WAVES; ++k) {            // the same trip count in every wave: the barriers below are uniform
        const int f = w + k * PITCH_WAVES;
        const int64_t t = t0 + f;
        float d[8], c[8];
        {
            const f32x4* p0 = reinterpret_cast<const f32x4*>(part + f * PITCH_L + 8 * l);
            const f32x4 a0 = p0[0], a1 = p0[1];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                d[i] = a0[i];
                d[4 + i] = a1[i];
            }
#pragma unroll
            for (int q = 1; q < S::NBW; ++q) {
                const f32x4 b0 = p0[q * (PITCH_L / 4)], b1 = p0[q * (PITCH_L / 4) + 1];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    d[i] += b0[i];
                    d[4 + i] += b1[i];
                }
            }
        }
        c[0] = d[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) c[i] = c[i - 1] + d[i];
        float tot = c[7];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float up = __shfl_up(tot, off);
            if (l >= off) tot += up;
        }
        float before = __shfl_up(tot, 1);
        if (l == 0) before = 0.f;
        float dv[8];
        float lowest = __int_as_float(0x7f800000);
        int hit = 0x7fffffff;
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            const int tau = 1 + 8 * l + i;
            const float run = before + c[i];
            dv[i] = run == 0.f ? 1.f : d[i] * (float)tau / run;
            if (tau >= tau_min && tau <= tau_max) {
                lowest = fminf(lowest, dv[i]);
                if (dv[i] < threshold) hit = tau;
            }
        }
        __syncthreads();                                          // the d' of this wave's previous frame has been read
        if (l == 0) dp[0] = 1.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) dp[1 + 8 * l + i] = dv[i];
        __syncthreads();
        if (cmnd && t < frames) {
            float* row = cmnd + (foff[seg] + t) * (int64_t)(PITCH_L + 1);
            for (int i = l; i <= PITCH_L; i += 64) row[i] = dp[i];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) lowest = fminf(lowest, __shfl_xor(lowest, off));
        const unsigned long long any = __ballot(hit != 0x7fffffff);
        float freq = 0.f, ap = lowest;
        if (any) {
            int tau = __shfl(hit, __ffsll((long long)any) - 1);   // the lowest lane holds the smallest lag
            while (tau + 1 <= tau_max && dp[tau + 1] < dp[tau]) ++tau;
            const float a = dp[tau - 1], bq = dp[tau], cq = dp[tau + 1];
            float shift = 0.f;
            if (a > bq && cq >= bq) shift = 0.5f * (a - cq) / (a - 2.f * bq + cq);
            freq = sample_rate / ((float)tau + shift);
            ap = bq;
        }
        int touched = 0;
#pragma unroll
        for (int q = 0; q < PITCH_REACH / HOP; ++q) touched |= bad[f + q];
        if (touched) freq = ap = __int_as_float(0x7fc00000);
        if (l == 0 && t < frames) {
            f0[foff[seg] + t] = freq;
            aper[foff[seg] + t] = ap;
        }
    }
}

static RttsLdsState g_pitch_lds[3];

template <int HOP>
static int pitch_launch(int slot, const float* audio, const int64_t* soff, const int64_t* foff, int nseg, int64_t max_frames, int tau_min,
                        int tau_max, float threshold, float sample_rate, float* f0, float* aper, float* cmnd, void* stream) {
    using S = PitchShape<HOP>;
    static_assert(S::LDS_BYTES <= 160 * 1024 && S::NBF <= 32, "a tile's samples, partial sums and flags must fit the LDS");
    RTTS_ENSURE_LDS("rtts_pitch_yin", pitch_yin_kernel<HOP>, S::LDS_BYTES, g_pitch_lds[slot]);
    const int64_t tiles = (max_frames + PITCH_FT - 1) / PITCH_FT;
    RTTS_REQUIRE(tiles <= 0x7fffffff, "rtts_pitch_yin: an utterance of %lld frames is too long for one launch", (long long)max_frames);
    hipLaunchKernelGGL(pitch_yin_kernel<HOP>, dim3((unsigned)tiles, (unsigned)nseg), dim3(PITCH_THREADS), S::LDS_BYTES, (hipStream_t)stream,
                       audio, soff, foff, tau_min, tau_max, threshold, sample_rate, f0, aper, cmnd);
    RTTS_LAUNCH_CHECK("rtts_pitch_yin");
    return 0;
}

extern "C" int rtts_pitch_yin(const float* audio, const int64_t* sample_offsets_host, const int64_t* frame_offsets_host,
                              const int64_t* sample_offsets, const int64_t* frame_offsets, int nseg, int hop, int tau_min, int tau_max,
                              float threshold, float sample_rate, float* f0, float* aperiodicity, float* cmnd, void* stream) {
    RTTS_REQUIRE(audio && sample_offsets_host && frame_offsets_host && sample_offsets && frame_offsets && f0 && aperiodicity,
                 "rtts_pitch_yin: null pointer argument");
    RTTS_REQUIRE(hop == 128 || hop == 256 || hop == 512, "rtts_pitch_yin: hop must be 128, 256 or 512 (got %d)", hop);
    RTTS_REQUIRE(tau_min >= 2 && tau_min <= tau_max && tau_max <= PITCH_L - 1,
                 "rtts_pitch_yin: tau_min and tau_max must satisfy 2 <= tau_min <= tau_max <= %d (got %d, %d)", PITCH_L - 1, tau_min, tau_max);
    RTTS_REQUIRE(threshold > 0.f && threshold < 1.f, "rtts_pitch_yin: threshold must lie strictly between 0 and 1 (got %g)", (double)threshold);
    RTTS_REQUIRE(sample_rate > 0.f && sample_rate <= 3.402823466e38f, "rtts_pitch_yin: sample_rate must be positive and finite (got %g)",
                 (double)sample_rate);
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "rtts_pitch_yin: nseg must be in 1..65535 (got %d)", nseg);
    int64_t max_frames = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t n = sample_offsets_host[s + 1] - sample_offsets_host[s];
        RTTS_REQUIRE(sample_offsets_host[s] >= 0 && n >= 1,
                     "rtts_pitch_yin: sample_offsets must start at >= 0 and increase: utterance %d has %lld samples", s, (long long)n);
        const int64_t frames = n / hop + 1;
        RTTS_REQUIRE(frame_offsets_host[s] >= 0 && frame_offsets_host[s + 1] - frame_offsets_host[s] >= frames,
                     "rtts_pitch_yin: utterance %d has %lld frames, its slot in frame_offsets holds %lld", s, (long long)frames,
                     (long long)(frame_offsets_host[s + 1] - frame_offsets_host[s]));
        if (frames > max_frames) max_frames = frames;
    }
    RTTS_ENTER(stream);
    switch (hop) {
        case 128: return pitch_launch<128>(0, audio, sample_offsets, frame_offsets, nseg, max_frames, tau_min, tau_max, threshold, sample_rate, f0, aperiodicity, cmnd, stream);
        case 256: return pitch_launch<256>(1, audio, sample_offsets, frame_offsets, nseg, max_frames, tau_min, tau_max, threshold, sample_rate, f0, aperiodicity, cmnd, stream);
        default: return pitch_launch<512>(2, audio, sample_offsets, frame_offsets, nseg, max_frames, tau_min, tau_max, threshold, sample_rate, f0, aperiodicity, cmnd, stream);
    }
}

#define F0C_THREADS 256
#define F0C_COLS 5

__global__ __launch_bounds__(F0C_THREADS) void f0_compare_kernel(const float* __restrict__ fa, const int64_t* __restrict__ oa,
                                                                 const float* __restrict__ fb, const int64_t* __restrict__ ob, int nseg,
                                                                 double gross, double* __restrict__ table) {
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const double nan = rtts_nan64();
    for (int s = w; s < nseg; s += F0C_THREADS / 64) {
        const int64_t a0 = oa[s], b0 = ob[s];
        const int64_t ta = oa[s + 1] - a0, tb = ob[s + 1] - b0;
        const int64_t cnt = ta < tb ? ta : tb;
        double both = 0.0, cents2 = 0.0, far = 0.0, flips = 0.0;
        int broken = 0;
        for (int64_t t = l; t < cnt; t += 64) {
            const double va = (double)fa[a0 + t], vb = (double)fb[b0 + t];
            if (va != va || vb != vb) broken = 1;
            const bool ha = va > 0.0, hb = vb > 0.0;
            if (ha && hb) {
                const double ratio = va / vb, c = 1200.0 * log2(ratio);
                both += 1.0;
                cents2 += c * c;
                if (fabs(ratio - 1.0) > gross) far += 1.0;
            } else if (ha != hb) {
                flips += 1.0;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            both += __shfl_down(both, off);
            cents2 += __shfl_down(cents2, off);
            far += __shfl_down(far, off);
            flips += __shfl_down(flips, off);
        }
        broken = __any(broken);
        if (l == 0) {
            double* row = table + (int64_t)s * F0C_COLS;
            row[0] = broken ? nan : (double)(cnt > 0 ? cnt : 0);
            row[1] = broken ? nan : both;
            row[2] = broken ? nan : cents2;
            row[3] = broken ? nan : far;
            row[4] = broken ? nan : flips;
        }
    }
    __threadfence();
    __syncthreads();
    if (tid < F0C_COLS) {
        double sum = 0.0;
        for (int s = 0; s < nseg; ++s) sum += table[(int64_t)s * F0C_COLS + tid];
        table[(int64_t)nseg * F0C_COLS + tid] = sum;
    }
}

extern "C" int rtts_f0_compare(const float* f0_a, const int64_t* frame_offsets_a, const float* f0_b, const int64_t* frame_offsets_b, int nseg,
                               double gross, double* table, void* stream) {
    RTTS_REQUIRE(f0_a && frame_offsets_a && f0_b && frame_offsets_b && table, "rtts_f0_compare: null pointer argument");
    RTTS_REQUIRE(nseg >= 1 && nseg <= 65535, "rtts_f0_compare: nseg must be in 1..65535 (got %d)", nseg);
    RTTS_REQUIRE(gross > 0.0 && gross < 1.0, "rtts_f0_compare: gross must lie strictly between 0 and 1 (got %g)", gross);
    RTTS_ENTER(stream);
    hipLaunchKernelGGL(f0_compare_kernel, dim3(1), dim3(F0C_THREADS), 0, (hipStream_t)stream, f0_a, frame_offsets_a, f0_b, frame_offsets_b, nseg,
                       gross, table);
    RTTS_LAUNCH_CHECK("rtts_f0_compare");
    return 0;
}
