// What the evaluation kernels share (infer_metrics.hip, dtw.hip, align.hip, pitch.hip): which truth frames slot b of a generated
// batch is scored against, the argument checks of that description, and a few wave and workgroup helpers.
#pragma once
#include "rtts_common.h"

#define RTTS_SCORE_MAX_MEL 128    // n_mel of a scored batch: the staging tiles of its users are sized by it

__device__ __forceinline__ double rtts_nan64() { return __longlong_as_double(0x7ff8000000000000LL); }

// sum over a workgroup of THREADS in a fixed order: lanes by halving distances, then the waves by index; valid in thread 0
template <int THREADS>
__device__ __forceinline__ double rtts_block_sum(double v, double* wsum) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    const int tid = threadIdx.x;
    __syncthreads();                                               // wsum may still be read from a previous call
    if ((tid & 63) == 0) wsum[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (tid == 0)
        for (int w = 0; w < THREADS / 64; ++w) s += wsum[w];
    return s;
}

// lane l takes `v` of lane l - 1 and lane 0 keeps `own` (v_mov_b32 with DPP wave_shr:1, no LDS round trip)
__device__ __forceinline__ int rtts_wave_shr1(int own, int v) { return __builtin_amdgcn_update_dpp(own, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ double rtts_wave_shr1(double own, double v) {
    return __hiloint2double(rtts_wave_shr1(__double2hiint(own), __double2hiint(v)), rtts_wave_shr1(__double2loint(own), __double2loint(v)));
}
// lane l takes `v` of lane l + 1 (DPP wave_shl:1); lane 63 keeps its own
__device__ __forceinline__ int rtts_wave_shl1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x130, 0xf, 0xf, false); }
__device__ __forceinline__ double rtts_wave_shl1(double v) {
    return __hiloint2double(rtts_wave_shl1(__double2hiint(v)), rtts_wave_shl1(__double2loint(v)));
}

static inline int64_t rtts_align256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

// Where the truths of a batch lie: the corpus description (fo = frame_offsets of n_utt utterances, slot b is utterance ids[b], or
// b without ids) or the padded-batch one (fo null: slot b is `lengths[b]` frames from frame `starts[b]`), in a buffer of
// truth_frames frames.  Passed to the kernels by value; the fields stand in the order the kernels took them as loose arguments.
struct RttsTruth {
    int64_t truth_frames;
    const int64_t* fo;
    int n_utt;
    const int32_t* ids;
    const int64_t* starts;
    const int32_t* lengths;
};

struct RttsTruthPick {
    int64_t f0, len;              // first truth frame of the slot and its frame count
    bool ok;                      // false: the id is out of range or the frames are not inside [0, truth_frames]
};

// The slot's truth frames, by the same scalar reads in every workgroup of every kernel: they agree without talking to each other.
// A ZERO-LENGTH truth is ok here, and the two users differ on it: infer_metrics.hip scores it as 0 frames (sse 0, stop_err
// |gen_stop + 1|), dtw.hip has no path through an empty table and treats the slot as unscorable (dtw_shape: cost NaN, steps 0).
__device__ __forceinline__ RttsTruthPick rtts_truth_pick(int b, const RttsTruth& tr) {
    RttsTruthPick p = {0, 0, false};
    int64_t c0, c1;
    if (tr.fo) {
        const int64_t u = tr.ids ? (int64_t)tr.ids[b] : (int64_t)b;
        if (u < 0 || u >= tr.n_utt) return p;
        c0 = tr.fo[u];
        c1 = tr.fo[u + 1];
    } else {
        c0 = tr.starts[b];
        c1 = c0 + (int64_t)tr.lengths[b];
    }
    if (c0 < 0 || c1 < c0 || c1 > tr.truth_frames) return p;
    p.f0 = c0;
    p.len = c1 - c0;
    p.ok = true;
    return p;
}

// the argument checks every entry point with these operands makes; `who` is its name
static inline int rtts_check_scored(const char* who, const float* gen, int L, const float* truth, const int64_t* frame_offsets, int n_utt,
                                    const int32_t* ids, const int64_t* starts, const int32_t* lengths, int B, int n_mel, int64_t truth_frames) {
    RTTS_REQUIRE(gen || L == 0, "%s: gen is a null pointer (and L = %d frames are to be read)", who, L);
    RTTS_REQUIRE(truth, "%s: truth is a null pointer", who);
    const bool corpus = frame_offsets != nullptr, padded = starts != nullptr || lengths != nullptr;
    RTTS_REQUIRE(corpus || padded, "%s: no truth description: give frame_offsets (+ ids), or starts + lengths", who);
    RTTS_REQUIRE(!(corpus && padded), "%s: two truth descriptions: give frame_offsets (+ ids) OR starts + lengths", who);
    RTTS_REQUIRE(corpus || (starts && lengths), "%s: the padded-batch description needs both starts and lengths", who);
    RTTS_REQUIRE(corpus || !ids, "%s: ids belong to the corpus description (frame_offsets is a null pointer)", who);
    RTTS_REQUIRE(!corpus || n_utt >= 1, "%s: n_utt must be positive (got %d)", who, n_utt);
    RTTS_REQUIRE(!corpus || ids || B <= n_utt, "%s: without ids slot b is utterance b: B = %d exceeds n_utt = %d", who, B, n_utt);
    RTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in 1..65535 (got %d)", who, B);
    RTTS_REQUIRE(n_mel >= 1 && n_mel <= RTTS_SCORE_MAX_MEL, "%s: n_mel must be in 1..%d (got %d)", who, RTTS_SCORE_MAX_MEL, n_mel);
    RTTS_REQUIRE(truth_frames >= 0, "%s: truth_frames must not be negative (got %lld)", who, (long long)truth_frames);
    return 0;
}
