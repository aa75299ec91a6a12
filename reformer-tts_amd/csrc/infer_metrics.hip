// B generated spectrograms scored against their truths where both already live (rtts_infer_metrics of include/rtts.h): the
// inference_pred_mse / inference_stop_mae of LitReformerTTS.validate_inference (reference training/wrappers.py:188-195) and the
// per-utterance squared error behind predict_samples' mse_loss (reference cli.py:150), nothing read back.
//
// Two kernels on the caller's stream:
//   tiles  grid (tiles, B).  Workgroup (k, b) owns the frame tiles k, k + tiles, ... of slot b, IM_TILE = 32 frames by all n_mel
//          channels each, and writes ONE f64 partial, partials[b * tiles + k].  The workgroups of a slot repeat the same scalar
//          reads (the id, its offsets or start / length: rtts_truth_pick of score_common.h) and agree on the utterance's bounds
//          without talking to each other.
//   fold   one workgroup: sse[b] = the slot's partials added by index, stop_err[b], and the two means, again by index.
// No atomics: every sum has one fixed order, which depends on (B, n_mel, lm, the lengths) and on nothing else -- not on the
// strides either.  That is why there is ONE compute mapping: thread tid always owns frame (tid & 31) of the tile and the channels
// (tid >> 5) + 8 i, so the same numbers in another layout give the same bits.
//
// Operand reads.  An operand whose frames are contiguous (stride_t == 1: what ReformerTTS.infer returns, the packed corpus) is read
// directly in the compute mapping: the 32 lanes of a half-wave read 32 consecutive frames of one channel, 128 contiguous bytes.
// An operand laid out the other way (the teacher-forced forward's (B, T, n_mel), a padded collate batch) is staged first:
//   tile[t * pitch + m],  t < 32 frames, m < n_mel,  pitch = n_mel | 1 words (odd), one tile per operand, f32 as loaded.
// Staging walks e = t * n_mel + m over the workgroup's threads: consecutive lanes read consecutive channels of a frame from
// global memory (contiguous where stride_mel == 1) and write consecutive LDS words (pitch - n_mel <= 1 word skipped at a row
// end): ds_write_b32 banks are word % 32 per 32-lane half, so no two lanes of a half meet on a bank.  The compute mapping then
// reads tile[(lane & 31) * pitch + m]: 32 lanes, 32 multiples of an odd pitch, 32 different banks (ds_read_b32, same rule).
// Two tiles of 32 x 129 words are 33 KB: four workgroups fit the 160 KB of a CU's LDS.  Frames at or past L read as generated zeros;
// frames at or past len_b are not read at all, so a NaN there reaches nothing, while one in a counted frame reaches its slot's sse.
#include "score_common.h"

#define IM_THREADS 256
#define IM_TILE 32
#define IM_MAX_MEL RTTS_SCORE_MAX_MEL
#define IM_MAX_TILES 256          // partials per slot: longer batches stride over their tiles

__global__ __launch_bounds__(IM_THREADS) void infer_metrics_tiles_kernel(
    const float* __restrict__ gen, int64_t gs_b, int64_t gs_mel, int64_t gs_t, int L, const float* __restrict__ truth, int64_t ts_mel,
    int64_t ts_t, RttsTruth tr, int n_mel, int tiles, double* __restrict__ partials) {
    __shared__ float tile_g[IM_TILE * (IM_MAX_MEL + 1)];
    __shared__ float tile_t[IM_TILE * (IM_MAX_MEL + 1)];
    __shared__ double wsum[IM_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const RttsTruthPick p = rtts_truth_pick(b, tr);
    const bool stage_g = gs_t != 1, stage_t = ts_t != 1;           // uniform over the launch
    const int pitch = n_mel | 1;
    const int ft = tid & (IM_TILE - 1), ph = tid / IM_TILE;
    const float* gen_b = gen + (int64_t)b * gs_b;                  // never dereferenced when L == 0 (gen may be null then)
    const int64_t ntile = (p.len + IM_TILE - 1) / IM_TILE;
    double acc = 0.0;
    bool staged = false;
    for (int64_t k = blockIdx.x; k < ntile; k += tiles) {          // uniform over the workgroup: p is
        const int64_t t0 = k * IM_TILE;
        if (stage_g || stage_t) {
            if (staged) __syncthreads();                           // the previous tile has been read
            for (int e = tid; e < IM_TILE * n_mel; e += IM_THREADS) {
                const int t = e / n_mel, m = e - t * n_mel;
                const int64_t r = t0 + t;
                if (stage_g) tile_g[t * pitch + m] = (r < p.len && r < L) ? gen_b[(int64_t)m * gs_mel + r * gs_t] : 0.f;
                if (stage_t) tile_t[t * pitch + m] = r < p.len ? truth[(int64_t)m * ts_mel + (p.f0 + r) * ts_t] : 0.f;
            }
            __syncthreads();
            staged = true;
        }
        const int64_t r = t0 + ft;
        if (r < p.len) {
            for (int m = ph; m < n_mel; m += IM_THREADS / IM_TILE) {
                const float g = stage_g ? tile_g[ft * pitch + m] : (r < L ? gen_b[(int64_t)m * gs_mel + r * gs_t] : 0.f);
                const float y = stage_t ? tile_t[ft * pitch + m] : truth[(int64_t)m * ts_mel + (p.f0 + r) * ts_t];
                const double d = (double)g - (double)y;
                acc += d * d;
            }
        }
    }
    const double s = rtts_block_sum<IM_THREADS>(acc, wsum);
    if (tid == 0) partials[(int64_t)b * tiles + blockIdx.x] = p.ok ? s : rtts_nan64();
}

__global__ __launch_bounds__(IM_THREADS) void infer_metrics_fold_kernel(
    const double* __restrict__ partials, int tiles, const int64_t* __restrict__ gen_stop, RttsTruth tr, int B, int n_mel, int lm,
    double* __restrict__ sse, double* __restrict__ stop_err, double* __restrict__ totals) {
    __shared__ double wsum[IM_THREADS / 64];
    const int tid = threadIdx.x;
    double a_sse = 0.0, a_stop = 0.0;
    for (int b = tid; b < B; b += IM_THREADS) {
        const RttsTruthPick p = rtts_truth_pick(b, tr);
        double s = 0.0;
        for (int k = 0; k < tiles; ++k) s += partials[(int64_t)b * tiles + k];
        double e = 0.0;
        if (gen_stop) {
            const int64_t d = gen_stop[b] - (p.len - 1);
            e = p.ok ? (double)(d < 0 ? -d : d) : rtts_nan64();
        }
        sse[b] = s;
        stop_err[b] = e;
        a_sse += s;
        a_stop += e;
    }
    const double t_sse = rtts_block_sum<IM_THREADS>(a_sse, wsum);
    const double t_stop = rtts_block_sum<IM_THREADS>(a_stop, wsum);
    if (tid == 0) {
        totals[0] = t_sse / ((double)B * (double)n_mel * (double)lm);
        totals[1] = t_stop / (double)B;
    }
}

extern "C" int rtts_infer_metrics_tiles(int lm) {
    const int64_t t = ((int64_t)(lm < 1 ? 1 : lm) + IM_TILE - 1) / IM_TILE;
    return (int)(t > IM_MAX_TILES ? IM_MAX_TILES : t);
}

extern "C" int rtts_infer_metrics(const float* gen, int64_t gs_b, int64_t gs_mel, int64_t gs_t, int L, const int64_t* gen_stop,
                                  const float* truth, int64_t ts_mel, int64_t ts_t, int64_t truth_frames, const int64_t* frame_offsets,
                                  int n_utt, const int32_t* ids, const int64_t* starts, const int32_t* lengths, int B, int n_mel, int lm,
                                  int longest, double* partials, double* sse, double* stop_err, double* totals, void* stream) {
    RTTS_REQUIRE(L >= 0, "rtts_infer_metrics: L must not be negative (got %d)", L);
    if (rtts_check_scored("rtts_infer_metrics", gen, L, truth, frame_offsets, n_utt, ids, starts, lengths, B, n_mel, truth_frames)) return -1;
    RTTS_REQUIRE(partials, "rtts_infer_metrics: partials is a null pointer");
    RTTS_REQUIRE(sse, "rtts_infer_metrics: sse is a null pointer");
    RTTS_REQUIRE(stop_err, "rtts_infer_metrics: stop_err is a null pointer");
    RTTS_REQUIRE(totals, "rtts_infer_metrics: totals is a null pointer");
    RTTS_REQUIRE(lm >= 1, "rtts_infer_metrics: lm must be positive (got %d)", lm);
    RTTS_REQUIRE(longest >= 0 && longest <= lm, "rtts_infer_metrics: lm = %d is smaller than the longest truth, %d frames", lm, longest);
    const RttsTruth tr = {truth_frames, frame_offsets, n_utt, ids, starts, lengths};
    const int tiles = rtts_infer_metrics_tiles(lm);
    RTTS_ENTER(stream);
    hipLaunchKernelGGL(infer_metrics_tiles_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(IM_THREADS), 0, (hipStream_t)stream, gen, gs_b, gs_mel,
                       gs_t, L, truth, ts_mel, ts_t, tr, n_mel, tiles, partials);
    RTTS_LAUNCH_CHECK("rtts_infer_metrics (tiles)");
    hipLaunchKernelGGL(infer_metrics_fold_kernel, dim3(1), dim3(IM_THREADS), 0, (hipStream_t)stream, partials, tiles, gen_stop, tr, B,
                       n_mel, lm, sse, stop_err, totals);
    RTTS_LAUNCH_CHECK("rtts_infer_metrics (fold)");
    return 0;
}
