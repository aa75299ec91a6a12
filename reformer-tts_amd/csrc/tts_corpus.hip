// One text-to-spectrogram training batch collated from a device-resident corpus, one launch (rtts_tts_collate of include/rtts.h):
// custom_sequence_padder (reference dataset/utils.py:5-42) for the B utterances `ids` names, written either in the reference's
// collate layout or in the padded buffers a captured step reads, with the Gaussian input noise of training/wrappers.py:53-63
// applied on the way (to the valid input frames only).
//
// Grid (tiles, B): the workgroups of slot b repeat the same scalar reads (the id, its two offset pairs) and agree on the
// utterance's bounds without talking to each other; nothing a workgroup reads is written by the launch.  Tile k owns rows
// [64 k, 64 k + 64) of EVERY mel-shaped output, each held to its own row count:
//   mel    the transpose of csrc/sw_corpus.hip: source (n_mel, ld_mel) is contiguous along frames, the outputs along channels.  A
//          wave reads 64 consecutive frames of one channel (256 contiguous bytes, 4-byte loads: a column starts at any element),
//          the tile goes through LDS with an odd row pitch -- the 32 lanes of a ds_write group (32 frames, one channel) and of a
//          ds_read group (consecutive channels) both fall on 32 different banks -- and leaves as consecutive words of the output
//          rows.  The input is the target one row later, so the tile holds 65 frames: frame 64 k - 1 in front (one strided read
//          per channel) serves the first input row;
//   rest   stop tokens and loss mask follow from the row index and the length; the first tile of a slot also writes its phonemes.
// No atomics; every word of every non-null output is written exactly once and depends on the arguments alone.
#include "rtts_common.h"

#define TC_THREADS 256
#define TC_TILE 64                // rows of one workgroup: one wave's width (DS_MEL_TILE of sw_corpus.hip)
#define TC_MAX_MEL 128

struct TcPick {
    int64_t f0, len;     // first column of the utterance in `mel`, its frames (0: nothing to read, the slot is zeros)
    int64_t p0, plen;    // first phoneme id in `phoneme_ids`, their count
};

// the bounds every read of slot b is held to
__device__ __forceinline__ TcPick tc_pick(int b, const int32_t* __restrict__ ids, int n_utt, int64_t ld_mel, const int64_t* __restrict__ fo,
                                          int64_t n_phonemes, const int64_t* __restrict__ po) {
    TcPick p = {0, 0, 0, 0};
    const int64_t u = ids[b];
    if (u < 0 || u >= n_utt) return p;
    const int64_t c0 = fo[u], c1 = fo[u + 1], q0 = po[u], q1 = po[u + 1];
    // tables that point outside the buffers are treated like an utterance that does not exist (ds_pick of sw_corpus.hip)
    if (c0 < 0 || c1 < c0 || c1 > ld_mel || q0 < 0 || q1 < q0 || q1 > n_phonemes) return p;
    p.f0 = c0;
    p.len = c1 - c0;
    p.p0 = q0;
    p.plen = q1 - q0;
    return p;
}

// z(b, f, c) of include/rtts.h: Box-Muller on two words of the counter hash, keyed by the element of the UTTERANCE
__device__ __forceinline__ float tc_gauss(uint32_t s_b, uint32_t e) {
    const uint32_t h1 = rtts_drop_hash(s_b, 2u * e), h2 = rtts_drop_hash(s_b, 2u * e + 1u);
    const float u1 = (float)((h1 >> 8) + 1u) * 5.9604644775390625e-8f;        // (0, 1], exact
    const float u2 = (float)(h2 >> 8) * 5.9604644775390625e-8f;               // [0, 1), exact
    return sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
}

template <bool NOISE>
__global__ __launch_bounds__(TC_THREADS) void tts_collate_kernel(
    const float* __restrict__ mel, int64_t ld_mel, const int64_t* __restrict__ fo, const int32_t* __restrict__ phoneme_ids,
    int64_t n_phonemes, const int64_t* __restrict__ po, int n_utt, const int32_t* __restrict__ ids, int n_mel, int lm,
    int64_t* __restrict__ phonemes, int LP, float* __restrict__ spec_in, int R_in, int valid_in, float* __restrict__ spec_tgt, int R_tgt,
    float* __restrict__ stop, int R_stop, float* __restrict__ mask, int R_mask, int32_t* __restrict__ valid_len, float noise_std,
    uint32_t seed) {
    __shared__ float tile[(TC_TILE + 1) * (TC_MAX_MEL + 1)];       // row j = frame t0 - 1 + j
    const int b = blockIdx.y, tid = threadIdx.x;
    const TcPick p = tc_pick(b, ids, n_utt, ld_mel, fo, n_phonemes, po);
    const int t0 = (int)blockIdx.x * TC_TILE;

    if (blockIdx.x == 0) {
        if (b == 0 && tid == 0 && valid_len) valid_len[0] = lm;
        if (phonemes) {
            int64_t* dst = phonemes + (int64_t)b * LP;
            for (int j = tid; j < LP; j += TC_THREADS) dst[j] = j < p.plen ? (int64_t)phoneme_ids[p.p0 + j] : 0;
        }
    }
    if (stop && tid < TC_TILE && t0 + tid < R_stop) stop[(int64_t)b * R_stop + t0 + tid] = (int64_t)(t0 + tid) == p.len - 1 ? 1.f : 0.f;

    const bool want_in = spec_in && t0 < R_in, want_tgt = spec_tgt && t0 < R_tgt, want_mask = mask && t0 < R_mask;
    if (!(want_in || want_tgt || want_mask)) return;               // uniform over the workgroup
    const int pitch = n_mel | 1;
    if (want_in || want_tgt) {
        const int lane = tid & 63, wave = tid >> 6;
        const bool live = t0 + lane < p.len;
        const float* src = mel + p.f0 + t0 + lane;
        for (int m = wave; m < n_mel; m += TC_THREADS / 64) tile[(lane + 1) * pitch + m] = live ? src[(int64_t)m * ld_mel] : 0.f;
        if (tid < n_mel) tile[tid] = (t0 >= 1 && t0 - 1 < p.len) ? mel[(int64_t)tid * ld_mel + p.f0 + t0 - 1] : 0.f;
        __syncthreads();
    }
    const uint32_t s_b = NOISE ? rtts_drop_hash(seed, (uint32_t)b) : 0u;
    const int count = TC_TILE * n_mel;
    for (int e = tid; e < count; e += TC_THREADS) {
        const int t = e / n_mel, m = e - t * n_mel, r = t0 + t;
        if (want_tgt && r < R_tgt) spec_tgt[((int64_t)b * R_tgt + r) * n_mel + m] = tile[(t + 1) * pitch + m];
        if (want_mask && r < R_mask) mask[((int64_t)b * R_mask + r) * n_mel + m] = r < p.len ? 1.f : 0.f;
        if (want_in && r < R_in) {
            float v = 0.f;
            if (r >= 1 && r <= p.len && r < valid_in) {
                v = tile[t * pitch + m];
                if (NOISE) v += noise_std * tc_gauss(s_b, (uint32_t)(r - 1) * (uint32_t)n_mel + (uint32_t)m);
            }
            spec_in[((int64_t)b * R_in + r) * n_mel + m] = v;
        }
    }
}

extern "C" int rtts_tts_collate(const float* mel, int64_t ld_mel, const int64_t* frame_offsets, const int32_t* phoneme_ids, int64_t n_phonemes,
                                const int64_t* phoneme_offsets, int n_utt, const int32_t* ids, int B, int n_mel, int lm, int64_t* phonemes,
                                int LP, float* spectrogram_input, int R_in, int valid_in, float* spectrogram_target, int R_target,
                                float* stop_tokens, int R_stop, float* loss_mask, int R_mask, int32_t* valid_len, float noise_std,
                                uint32_t seed, void* stream) {
    RTTS_REQUIRE(mel, "rtts_tts_collate: mel is a null pointer");
    RTTS_REQUIRE(frame_offsets, "rtts_tts_collate: frame_offsets is a null pointer");
    RTTS_REQUIRE(phoneme_ids, "rtts_tts_collate: phoneme_ids is a null pointer");
    RTTS_REQUIRE(phoneme_offsets, "rtts_tts_collate: phoneme_offsets is a null pointer");
    RTTS_REQUIRE(ids, "rtts_tts_collate: ids is a null pointer");
    RTTS_REQUIRE(phonemes || spectrogram_input || spectrogram_target || stop_tokens || loss_mask || valid_len,
                 "rtts_tts_collate: every output is a null pointer");
    RTTS_REQUIRE(B >= 1 && B <= 65535, "rtts_tts_collate: B must be in 1..65535 (got %d)", B);
    RTTS_REQUIRE(n_mel >= 1 && n_mel <= TC_MAX_MEL, "rtts_tts_collate: n_mel must be in 1..%d (got %d)", TC_MAX_MEL, n_mel);
    RTTS_REQUIRE(n_utt >= 1, "rtts_tts_collate: n_utt must be positive (got %d)", n_utt);
    RTTS_REQUIRE(ld_mel >= 0, "rtts_tts_collate: ld_mel must not be negative (got %lld)", (long long)ld_mel);
    RTTS_REQUIRE(n_phonemes >= 0, "rtts_tts_collate: n_phonemes must not be negative (got %lld)", (long long)n_phonemes);
    RTTS_REQUIRE(lm >= 0, "rtts_tts_collate: lm must not be negative (got %d)", lm);
    RTTS_REQUIRE(!phonemes || LP >= 1, "rtts_tts_collate: LP must be positive (got %d)", LP);
    RTTS_REQUIRE(!spectrogram_input || R_in >= 1, "rtts_tts_collate: R_in must be positive (got %d)", R_in);
    RTTS_REQUIRE(!spectrogram_input || (valid_in >= 1 && valid_in <= R_in),
                 "rtts_tts_collate: valid_in must be in 1..R_in = %d (got %d)", R_in, valid_in);
    RTTS_REQUIRE(!spectrogram_target || R_target >= 1, "rtts_tts_collate: R_target must be positive (got %d)", R_target);
    RTTS_REQUIRE(!stop_tokens || R_stop >= 1, "rtts_tts_collate: R_stop must be positive (got %d)", R_stop);
    RTTS_REQUIRE(!loss_mask || R_mask >= 1, "rtts_tts_collate: R_mask must be positive (got %d)", R_mask);
    int rows = 1;
    if (spectrogram_input && R_in > rows) rows = R_in;
    if (spectrogram_target && R_target > rows) rows = R_target;
    if (stop_tokens && R_stop > rows) rows = R_stop;
    if (loss_mask && R_mask > rows) rows = R_mask;
    RTTS_REQUIRE(rows <= (1 << 30), "rtts_tts_collate: %d rows are too many for one launch", rows);
    const int tiles = (rows + TC_TILE - 1) / TC_TILE;
    RTTS_ENTER(stream);
    const dim3 grid((unsigned)tiles, (unsigned)B), block(TC_THREADS);
    if (noise_std > 0.f)
        hipLaunchKernelGGL(tts_collate_kernel<true>, grid, block, 0, (hipStream_t)stream, mel, ld_mel, frame_offsets, phoneme_ids, n_phonemes,
                           phoneme_offsets, n_utt, ids, n_mel, lm, phonemes, LP, spectrogram_input, R_in, valid_in, spectrogram_target, R_target,
                           stop_tokens, R_stop, loss_mask, R_mask, valid_len, noise_std, seed);
    else
        hipLaunchKernelGGL(tts_collate_kernel<false>, grid, block, 0, (hipStream_t)stream, mel, ld_mel, frame_offsets, phoneme_ids, n_phonemes,
                           phoneme_offsets, n_utt, ids, n_mel, lm, phonemes, LP, spectrogram_input, R_in, valid_in, spectrogram_target, R_target,
                           stop_tokens, R_stop, loss_mask, R_mask, valid_len, noise_std, seed);
    RTTS_LAUNCH_CHECK("rtts_tts_collate");
    return 0;
}
