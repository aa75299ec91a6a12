// B generated spectrograms aligned to their truths by dynamic time warping (rtts_dtw_align of include/rtts.h): the path cost and
// path length behind MCD-DTW, the timing-invariant sibling of rtts_infer_metrics, with the same addressing (the truth description
// of score_common.h) and nothing read back.
//
// Four kernels on the caller's stream, every one reading the slot's two lengths N (generated frames) and M (truth frames) on the
// device (dtw_shape over rtts_truth_pick of score_common.h):
//   project    grid (frame tiles, B, 2).  32 frames by all n_mel channels staged in LDS (either layout, the staging of
//              infer_metrics.hip), then p[k] = f32(sum_m f64(basis[k, m]) f64(x[m])), m ascending (a product of two f32 is exact
//              in f64, so the sum is the same with and without contraction).  A non-finite x or p sets the frame's flag word.
//              Frames at or past N / M are not read.
//   distances  grid (M tiles, N tiles, B).  64 x 64 cells per workgroup, 4 x 4 per thread: d(i, j) = sqrtf(sum_k (p_i[k] -
//              q_j[k])^2), f32, the DIFFERENCE squared, k ascending.  Cell (i, j) is stored SKEWED, at row j + lane(i) of the
//              slot's table, lane(i) = (i / R) & 63: the recurrence's wave reads one contiguous table row per step.
//   recurrence one workgroup of 16 waves per slot.  Thread t owns the R = 1 or 2 rows t R .. t R + R - 1 (R from L, so that 1024
//              threads cover it); inside a wave lane l works on column sigma - l at the wave's step sigma: the row above is
//              the neighbour lane's result of the step before (one DPP wave_shr:1 move per word, no LDS round trip), the
//              diagonal the one of two steps before (a register).  No barrier inside a wave.  Wave w + 1 takes the last row
//              of wave w through an LDS ring of DTW_RING columns and runs DTW_LAG chunks of DTW_CHUNK steps behind it: lane 63
//              of wave w has written column c at its step c + 63, so DTW_LAG * DTW_CHUNK >= DTW_CHUNK + 63 steps later -- one
//              __syncthreads per chunk in between -- wave w + 1 may read it (a group of columns at a time, moved down to
//              lane 0 one lane per step by a second DPP shift); in one round the writer is at most DTW_LAG * DTW_CHUNK +
//              DTW_CHUNK - 64 columns past the reader's oldest unread one, a fraction of the ring.  That makes
//              (M + 63 + DTW_CHUNK - 1) / DTW_CHUNK + DTW_LAG (waves - 1) barriers instead of N + M - 1.
//              The table row of a step is loaded DTW_AHEAD / R steps before its use (registers), never at the point of use.
//              The loop is bound by VALU issue (four waves per SIMD, every instruction four cycles), so no cell is
//              predicated: see the kernel for why the cells outside the table may compute anything.
//              Each cell has ONE evaluation: f64 add of the widened d to the first minimal predecessor in the order
//              diagonal, above, left (strict <), so the result is independent of the wave schedule.
//   fold       one workgroup: the two means over the slots, by index.
// A slot that is not to be read (N = 0, a bad description or id, M outside 1..lm) or that holds a non-finite compared value
// skips the recurrence: cost NaN, steps 0.  The flags are OR-ed by the recurrence's workgroup before its first step: no atomics.
#include "score_common.h"

#define DTW_MAX_FRAMES 2048
#define DTW_MAX_DIM RTTS_SCORE_MAX_MEL   // n_mel and n_proj
#define DTW_PROJ_THREADS 256
#define DTW_PROJ_TILE 32
#define DTW_DIST_THREADS 256
#define DTW_DIST_TILE 64
#define DTW_DIST_KC 32
#define DTW_THREADS 1024
#define DTW_WAVES (DTW_THREADS / 64)
#define DTW_CHUNK 16
#define DTW_LAG 5
#define DTW_RING 256
#define DTW_AHEAD 16
#define DTW_FOLD_THREADS 256

static_assert(DTW_LAG * DTW_CHUNK >= DTW_CHUNK + 63, "a ring column must be written one barrier before it is read");
static_assert(DTW_RING > DTW_LAG * DTW_CHUNK + DTW_CHUNK - 64 && (DTW_RING & (DTW_RING - 1)) == 0,
              "the ring must hold the writer's lead over the reader");
static_assert(DTW_CHUNK % DTW_AHEAD == 0 && DTW_AHEAD % 2 == 0, "a chunk is a whole number of prefetch groups");

struct DtwShape {
    int64_t f0;                   // first truth frame of the slot
    int n, m;                     // generated and truth frames to compare
    bool ok;                      // false: the slot is not to be read (cost NaN, steps 0)
};

// the slot's bounds on top of the shared truth pick: a truth of 1..lm frames and at least one generated frame, or nothing is read
__device__ __forceinline__ DtwShape dtw_shape(int b, const int64_t* __restrict__ gen_stop, int L, const RttsTruth& tr, int lm) {
    DtwShape s = {0, 0, 0, false};
    const RttsTruthPick p = rtts_truth_pick(b, tr);
    if (!p.ok || (uint64_t)(p.len - 1) >= (uint64_t)lm) return s;  // 1 <= len <= lm in one compare: an ok pick has len >= 0
    int64_t n = gen_stop ? gen_stop[b] : (int64_t)L;
    n = n < (int64_t)L ? n : (int64_t)L;
    if (n < 1) return s;
    s.f0 = p.f0;
    s.n = (int)n;
    s.m = (int)p.len;
    s.ok = true;
    return s;
}

__global__ __launch_bounds__(DTW_PROJ_THREADS) void dtw_project_kernel(
    const float* __restrict__ gen, int64_t gs_b, int64_t gs_mel, int64_t gs_t, int L, const int64_t* __restrict__ gen_stop,
    const float* __restrict__ truth, int64_t ts_mel, int64_t ts_t, RttsTruth tr, int n_mel, int lm, const float* __restrict__ basis,
    int n_proj, float* __restrict__ pg, float* __restrict__ pt, int32_t* __restrict__ fg, int32_t* __restrict__ ft) {
    __shared__ float tile[DTW_PROJ_TILE * (DTW_MAX_DIM + 1)];
    __shared__ int bad[DTW_PROJ_TILE];
    const int b = blockIdx.y, side = blockIdx.z, tid = threadIdx.x;
    const DtwShape s = dtw_shape(b, gen_stop, L, tr, lm);
    const int count = side ? s.m : s.n, cap = side ? lm : L;
    const int t0 = blockIdx.x * DTW_PROJ_TILE;
    if (!s.ok || t0 >= count) return;                              // uniform over the workgroup
    const float* src = side ? truth + s.f0 * ts_t : gen + (int64_t)b * gs_b;
    const int64_t st_m = side ? ts_mel : gs_mel, st_t = side ? ts_t : gs_t;
    const int pitch = n_mel | 1;
    if (tid < DTW_PROJ_TILE) bad[tid] = 0;
    for (int e = tid; e < DTW_PROJ_TILE * n_mel; e += DTW_PROJ_THREADS) {
        // consecutive lanes follow the operand's contiguous direction
        const int t = st_t == 1 ? e % DTW_PROJ_TILE : e / n_mel, m = st_t == 1 ? e / DTW_PROJ_TILE : e % n_mel;
        tile[t * pitch + m] = t0 + t < count ? src[(int64_t)m * st_m + (int64_t)(t0 + t) * st_t] : 0.f;
    }
    __syncthreads();
    const int f = tid & (DTW_PROJ_TILE - 1), ph = tid / DTW_PROJ_TILE;
    const bool live = t0 + f < count;
    bool nonfinite = false;
    for (int m = ph; m < n_mel; m += DTW_PROJ_THREADS / DTW_PROJ_TILE) nonfinite |= !isfinite(tile[f * pitch + m]);
    float* dst = (side ? pt : pg) + ((int64_t)b * cap + t0 + f) * n_proj;
    for (int k = ph; k < n_proj; k += DTW_PROJ_THREADS / DTW_PROJ_TILE) {
        float p;
        if (basis) {
            double acc = 0.0;
            for (int m = 0; m < n_mel; ++m) acc += (double)basis[(int64_t)k * n_mel + m] * (double)tile[f * pitch + m];
            p = (float)acc;
        } else {
            p = tile[f * pitch + k];
        }
        nonfinite |= !isfinite(p);
        if (live) dst[k] = p;
    }
    if (nonfinite && live) bad[f] = 1;                             // every writer stores the same word
    __syncthreads();
    if (tid < DTW_PROJ_TILE && t0 + tid < count) (side ? ft : fg)[(int64_t)b * cap + t0 + tid] = bad[tid];
}

template <int R>
__global__ __launch_bounds__(DTW_DIST_THREADS) void dtw_dist_kernel(
    const float* __restrict__ pg, const float* __restrict__ pt, int L, const int64_t* __restrict__ gen_stop, RttsTruth tr, int lm, int n_proj,
    float* __restrict__ table, int pitch, int64_t slot_words) {
    __shared__ float sp[DTW_DIST_TILE * (DTW_DIST_KC + 1)];
    __shared__ float sq[DTW_DIST_TILE * (DTW_DIST_KC + 1)];
    const int b = blockIdx.z, tid = threadIdx.x;
    const DtwShape s = dtw_shape(b, gen_stop, L, tr, lm);
    const int i0 = blockIdx.y * DTW_DIST_TILE, j0 = blockIdx.x * DTW_DIST_TILE;
    if (!s.ok || i0 >= s.n || j0 >= s.m) return;                   // uniform over the workgroup
    const float* gp = pg + (int64_t)b * L * n_proj;
    const float* tp = pt + (int64_t)b * lm * n_proj;
    const int tx = tid & 15, ty = tid >> 4;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < n_proj; k0 += DTW_DIST_KC) {
        const int kc = n_proj - k0 < DTW_DIST_KC ? n_proj - k0 : DTW_DIST_KC;
        if (k0) __syncthreads();                                   // the previous chunk has been read
        for (int e = tid; e < DTW_DIST_TILE * DTW_DIST_KC; e += DTW_DIST_THREADS) {
            const int r = e / DTW_DIST_KC, k = e % DTW_DIST_KC;
            const bool kin = k < kc;
            sp[r * (DTW_DIST_KC + 1) + k] = kin && i0 + r < s.n ? gp[(int64_t)(i0 + r) * n_proj + k0 + k] : 0.f;
            sq[r * (DTW_DIST_KC + 1) + k] = kin && j0 + r < s.m ? tp[(int64_t)(j0 + r) * n_proj + k0 + k] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            float p[4], q[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                p[a] = sp[(tx + 16 * a) * (DTW_DIST_KC + 1) + k];  // 16 rows of odd pitch: 16 banks; the four ty of a wave broadcast
                q[a] = sq[(ty + 16 * a) * (DTW_DIST_KC + 1) + k];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = p[a] - q[c];
                    acc[a][c] = fmaf(d, d, acc[a][c]);
                }
        }
    }
    float* tab = table + (int64_t)b * slot_words;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + tx + 16 * a, j = j0 + ty + 16 * c;
            // sqrtf is the correctly rounded square root here (hipcc's default for f32 division and square root)
            // a distance past the f32 range counts as the largest f32: the recurrence's +inf stays above every path cost
            if (i < s.n && j < s.m) tab[(int64_t)(j + ((i / R) & 63)) * pitch + i] = fminf(sqrtf(acc[a][c]), 3.402823466e38f);
        }
}

template <int R>
__global__ __launch_bounds__(DTW_THREADS) void dtw_recur_kernel(
    const float* __restrict__ table, int pitch, int64_t slot_words, const int32_t* __restrict__ fg, const int32_t* __restrict__ ft, int L,
    const int64_t* __restrict__ gen_stop, RttsTruth tr, int lm, double* __restrict__ cost, int32_t* __restrict__ steps) {
    __shared__ double ring_d[DTW_WAVES][DTW_RING];
    __shared__ int ring_s[DTW_WAVES][DTW_RING];
    const int b = blockIdx.x, tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // a scalar: the step counters below stay out of the VALU
    const DtwShape s = dtw_shape(b, gen_stop, L, tr, lm);
    int flagged = 0;
    if (s.ok) {
        for (int i = tid; i < s.n; i += DTW_THREADS) flagged |= fg[(int64_t)b * L + i];
        for (int j = tid; j < s.m; j += DTW_THREADS) flagged |= ft[(int64_t)b * lm + j];
    }
    if (!s.ok || __syncthreads_or(flagged)) {                      // uniform over the workgroup
        if (tid == 0) {
            cost[b] = rtts_nan64();
            steps[b] = 0;
        }
        return;
    }
    const int N = s.n, M = s.m;
    const int waves = (N + 64 * R - 1) / (64 * R);                 // waves that own a row
    const int chunks = (M + 63 + DTW_CHUNK - 1) / DTW_CHUNK;       // of one wave: its lane 63 ends at step M - 1 + 63
    const int rounds = chunks + (waves - 1) * DTW_LAG;
    const int row0 = tid * R;
    const float* tab = table + (int64_t)b * slot_words + row0;
    const bool active = w < waves;
    const bool feeds = w + 1 < waves;                              // lane 63's last row is the next wave's row above
    // The steps of a lane run from sigma = 0, i.e. from column -l, to the end of the wave's last chunk, past column M - 1, and
    // rows at or past N run too: NO cell is predicated.  A cell outside the table reads its distance as +inf and so becomes
    // +inf itself, exactly what "this predecessor does not exist" has to look like to the cells inside: no sum of at most 4095
    // f32 distances reaches +inf (the table holds none: the distances kernel clamps to FLT_MAX), so the strict < of the
    // tie-break never picks one while a real predecessor stands beside it -- column 0 takes the cell above, row 0 the cell on
    // the left.  Nothing inside depends on a cell below row N - 1 or right of column M - 1.  The origin alone has no real
    // predecessor: thread 0 starts with 0 / 0 steps on its diagonal, which its first step replaces by +inf like any other.
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const float inf32 = __int_as_float(0x7f800000);
    // cell (N - 1, M - 1): row (N - 1) % R of lane final_lane of wave final_wave, at that wave's step final_lane + M - 1
    const int final_wave = (N - 1) / (64 * R), final_lane = ((N - 1) / R) & 63;
    const int final_step = w == final_wave ? final_lane + M - 1 : -1;
    double left_d[R], last_d = inf, diag_d = tid == 0 ? 0.0 : inf; // D(row, j - 1); D(my last row, j); D(row0 - 1, j - 1)
    int left_s[R], last_s = 0, diag_s = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        left_d[r] = inf;
        left_s[r] = 0;
    }
    constexpr int AHEAD = DTW_AHEAD / R;                           // the same registers for either R
    float ahead[AHEAD][R];
    bool row_in[R];
#pragma unroll
    for (int r = 0; r < R; ++r) row_in[r] = row0 + r < N;

    auto fetch = [&](int sigma0) {                                 // the table rows of steps sigma0 .. sigma0 + AHEAD - 1
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) {
            const bool col_in = (unsigned)(sigma0 + a - l) < (unsigned)M;
#pragma unroll
            for (int r = 0; r < R; ++r) ahead[a][r] = (col_in && row_in[r]) ? tab[(int64_t)(sigma0 + a) * pitch + r] : inf32;
        }
    };

    for (int u = 0; u < rounds; ++u) {
        const int lu = u - w * DTW_LAG;
        if (active && lu >= 0 && lu < chunks) {                    // uniform over the wave
            if (lu == 0) fetch(0);
            for (int g = 0; g < DTW_CHUNK / AHEAD; ++g) {
                const int sigma0 = lu * DTW_CHUNK + g * AHEAD;
                float now[AHEAD][R];
#pragma unroll
                for (int a = 0; a < AHEAD; ++a)
#pragma unroll
                    for (int r = 0; r < R; ++r) now[a][r] = ahead[a][r];
                fetch(sigma0 + AHEAD);                             // in flight while this group computes
                // the row above this wave at the group's columns (lane 0's columns sigma0 + a): lane a reads the ring once, and
                // the values move down one lane per step, so that lane 0 holds the one of the current step
                double above_d = inf;
                int above_s = 0;
                if (w > 0) {
                    above_d = ring_d[w - 1][(sigma0 + l) & (DTW_RING - 1)];
                    above_s = ring_s[w - 1][(sigma0 + l) & (DTW_RING - 1)];
                }
#pragma unroll
                for (int a = 0; a < AHEAD; ++a) {
                    const int sigma = sigma0 + a;
                    // the row above my first row at my column: the neighbour lane's last row of the step before; lane 0: the ring
                    const double up_d = rtts_wave_shr1(above_d, last_d);
                    const int up_s = rtts_wave_shr1(above_s, last_s);
                    above_d = rtts_wave_shl1(above_d);
                    above_s = rtts_wave_shl1(above_s);
                    double ab_d = up_d, dg_d = diag_d;             // above and diagonal of the current row
                    int ab_s = up_s, dg_s = diag_s;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        double best = dg_d;
                        int bs = dg_s;
                        const bool by_up = ab_d < best;
                        best = by_up ? ab_d : best;
                        bs = by_up ? ab_s : bs;
                        const bool by_left = left_d[r] < best;
                        best = by_left ? left_d[r] : best;
                        bs = by_left ? left_s[r] : bs;
                        const double d = best + (double)now[a][r];
                        dg_d = left_d[r];                          // D(row, j - 1) is the next row's diagonal
                        dg_s = left_s[r];
                        left_d[r] = ab_d = d;
                        left_s[r] = ab_s = bs + 1;
                    }
                    last_d = ab_d;
                    last_s = ab_s;
                    diag_d = up_d;
                    diag_s = up_s;
                    if (sigma == final_step && l == final_lane) {  // a scalar test first
                        cost[b] = left_d[(N - 1) & (R - 1)];
                        steps[b] = left_s[(N - 1) & (R - 1)];
                    }
                    if (feeds && l == 63) {
                        ring_d[w][(sigma - 63) & (DTW_RING - 1)] = last_d;
                        ring_s[w][(sigma - 63) & (DTW_RING - 1)] = last_s;
                    }
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(DTW_FOLD_THREADS) void dtw_fold_kernel(const double* __restrict__ cost, const int32_t* __restrict__ steps, int B,
                                                                    double* __restrict__ totals) {
    __shared__ double wsum[DTW_FOLD_THREADS / 64];
    double a_mean = 0.0, a_cost = 0.0, a_steps = 0.0;
    for (int b = threadIdx.x; b < B; b += DTW_FOLD_THREADS) {
        const double c = cost[b], n = (double)steps[b];
        a_mean += c / n;                                           // NaN / 0 of a slot that was not scored stays NaN
        a_cost += c;
        a_steps += n;                                              // exact: at most 65535 * 4095
    }
    const double t_mean = rtts_block_sum<DTW_FOLD_THREADS>(a_mean, wsum);
    const double t_cost = rtts_block_sum<DTW_FOLD_THREADS>(a_cost, wsum);
    const double t_steps = rtts_block_sum<DTW_FOLD_THREADS>(a_steps, wsum);
    if (threadIdx.x == 0) {
        totals[0] = t_mean / (double)B;
        totals[1] = t_cost / t_steps;
    }
}

static inline int dtw_pitch(int L) { return ((L < 1 ? 1 : L) + 63) & ~63; }

struct DtwLayout {
    int64_t pg, pt, fg, ft, table, total, slot_words;
    int pitch;
};

static inline DtwLayout dtw_layout(int B, int L, int lm, int n_proj) {
    DtwLayout w;
    w.pitch = dtw_pitch(L);
    w.slot_words = (int64_t)(lm + 63) * w.pitch;
    w.pg = 0;
    w.pt = w.pg + rtts_align256((int64_t)B * (L < 1 ? 1 : L) * n_proj * 4);
    w.fg = w.pt + rtts_align256((int64_t)B * lm * n_proj * 4);
    w.ft = w.fg + rtts_align256((int64_t)B * (L < 1 ? 1 : L) * 4);
    w.table = w.ft + rtts_align256((int64_t)B * lm * 4);
    w.total = w.table + rtts_align256((int64_t)B * w.slot_words * 4);
    return w;
}

extern "C" int rtts_dtw_max_frames(void) { return DTW_MAX_FRAMES; }

extern "C" int64_t rtts_dtw_workspace_bytes(int B, int L, int lm, int n_proj) {
    if (B < 1 || B > 65535 || L < 0 || L > DTW_MAX_FRAMES || lm < 1 || lm > DTW_MAX_FRAMES || n_proj < 1 || n_proj > DTW_MAX_DIM) return -1;
    return dtw_layout(B, L, lm, n_proj).total;
}

extern "C" int rtts_dtw_align(const float* gen, int64_t gs_b, int64_t gs_mel, int64_t gs_t, int L, const int64_t* gen_stop, const float* truth,
                              int64_t ts_mel, int64_t ts_t, int64_t truth_frames, const int64_t* frame_offsets, int n_utt, const int32_t* ids,
                              const int64_t* starts, const int32_t* lengths, int B, int n_mel, int lm, const float* basis, int n_proj,
                              void* workspace, int64_t workspace_bytes, int phases, double* cost, int32_t* steps, double* totals, void* stream) {
    RTTS_REQUIRE(L >= 0 && L <= DTW_MAX_FRAMES, "rtts_dtw_align: L must be in 0..%d (got %d)", DTW_MAX_FRAMES, L);
    if (rtts_check_scored("rtts_dtw_align", gen, L, truth, frame_offsets, n_utt, ids, starts, lengths, B, n_mel, truth_frames)) return -1;
    RTTS_REQUIRE(workspace, "rtts_dtw_align: workspace is a null pointer");
    RTTS_REQUIRE(cost, "rtts_dtw_align: cost is a null pointer");
    RTTS_REQUIRE(steps, "rtts_dtw_align: steps is a null pointer");
    RTTS_REQUIRE(totals, "rtts_dtw_align: totals is a null pointer");
    RTTS_REQUIRE(lm >= 1 && lm <= DTW_MAX_FRAMES, "rtts_dtw_align: lm must be in 1..%d (got %d)", DTW_MAX_FRAMES, lm);
    RTTS_REQUIRE(n_proj >= 1 && n_proj <= DTW_MAX_DIM, "rtts_dtw_align: n_proj must be in 1..%d (got %d)", DTW_MAX_DIM, n_proj);
    RTTS_REQUIRE(basis || n_proj == n_mel, "rtts_dtw_align: without a basis n_proj must be n_mel = %d (got %d)", n_mel, n_proj);
    RTTS_REQUIRE(phases >= 1 && phases <= RTTS_DTW_ALL, "rtts_dtw_align: phases must be a non-empty subset of RTTS_DTW_ALL (got %d)", phases);
    const DtwLayout w = dtw_layout(B, L, lm, n_proj);
    RTTS_REQUIRE(workspace_bytes >= w.total, "rtts_dtw_align: workspace_bytes = %lld is smaller than rtts_dtw_workspace_bytes = %lld",
                 (long long)workspace_bytes, (long long)w.total);
    char* base = (char*)workspace;
    float* pg = (float*)(base + w.pg);
    float* pt = (float*)(base + w.pt);
    int32_t* fg = (int32_t*)(base + w.fg);
    int32_t* ft = (int32_t*)(base + w.ft);
    float* table = (float*)(base + w.table);
    const int rows = L > DTW_THREADS ? 2 : 1;                      // rows of the table per thread of the recurrence
    const int longer = L > lm ? L : lm;
    const RttsTruth tr = {truth_frames, frame_offsets, n_utt, ids, starts, lengths};
    RTTS_ENTER(stream);
    hipStream_t st = (hipStream_t)stream;
    if (phases & RTTS_DTW_PROJECT) {
        hipLaunchKernelGGL(dtw_project_kernel, dim3((unsigned)((longer + DTW_PROJ_TILE - 1) / DTW_PROJ_TILE), (unsigned)B, 2),
                           dim3(DTW_PROJ_THREADS), 0, st, gen, gs_b, gs_mel, gs_t, L, gen_stop, truth, ts_mel, ts_t, tr, n_mel, lm, basis, n_proj, pg,
                           pt, fg, ft);
        RTTS_LAUNCH_CHECK("rtts_dtw_align (project)");
    }
    if ((phases & RTTS_DTW_DISTANCES) && L > 0) {
        const dim3 grid((unsigned)((lm + DTW_DIST_TILE - 1) / DTW_DIST_TILE), (unsigned)((L + DTW_DIST_TILE - 1) / DTW_DIST_TILE), (unsigned)B);
        if (rows == 1)
            hipLaunchKernelGGL(dtw_dist_kernel<1>, grid, dim3(DTW_DIST_THREADS), 0, st, pg, pt, L, gen_stop, tr, lm, n_proj, table, w.pitch,
                               w.slot_words);
        else
            hipLaunchKernelGGL(dtw_dist_kernel<2>, grid, dim3(DTW_DIST_THREADS), 0, st, pg, pt, L, gen_stop, tr, lm, n_proj, table, w.pitch,
                               w.slot_words);
        RTTS_LAUNCH_CHECK("rtts_dtw_align (distances)");
    }
    if (phases & RTTS_DTW_RECURRENCE) {
        if (rows == 1)
            hipLaunchKernelGGL(dtw_recur_kernel<1>, dim3((unsigned)B), dim3(DTW_THREADS), 0, st, table, w.pitch, w.slot_words, fg, ft, L, gen_stop,
                               tr, lm, cost, steps);
        else
            hipLaunchKernelGGL(dtw_recur_kernel<2>, dim3((unsigned)B), dim3(DTW_THREADS), 0, st, table, w.pitch, w.slot_words, fg, ft, L, gen_stop,
                               tr, lm, cost, steps);
        RTTS_LAUNCH_CHECK("rtts_dtw_align (recurrence)");
    }
    if (phases & RTTS_DTW_FOLD) {
        hipLaunchKernelGGL(dtw_fold_kernel, dim3(1), dim3(DTW_FOLD_THREADS), 0, st, cost, steps, B, totals);
        RTTS_LAUNCH_CHECK("rtts_dtw_align (fold)");
    }
    return 0;
}
