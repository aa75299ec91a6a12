// Alignment scores and phoneme durations from encoder-decoder attention matrices (rtts_align_stats and rtts_align_mas of
// include/rtts.h): n_mat matrices of (B, T_q, T_k) f32 probabilities where they lie, every slot's own frame and key counts read
// on the device, nothing read back, no floating-point atomics.
//
// rtts_align_stats, three kernels on the caller's stream:
//   rows    grid (frame tiles, B, n_mat), ALIGN_ROW_WAVES waves.  A tile is ALIGN_TILE consecutive frames, a wave takes one frame at
//           a time: lane l reads the 16-byte groups l, l + 64, .. of the row (a group that straddles K is read word by word, so
//           nothing at or past K is touched) and keeps, over its own columns in ascending order, the f64 sum, the first largest
//           value, -sum a ln a and sum a w; the 64 lanes are folded by halving distances (the arg-max by "larger value, then lower
//           index").  The frame's arg-max goes straight to the output; the tile's frames are then added IN FRAME ORDER by one
//           thread per column and stored as the tile's partial.  The order of every sum depends on (T, K) alone.
//   fold    one workgroup per (matrix, slot): the tile partials added in tile order, the arg-max track's monotone steps, the
//           arg-max durations (an integer histogram in LDS) and the covered keys.  A slot with a non-finite value in its
//           region is wiped here (table NaN, durations 0, arg-max -1).
//   totals  row B of every matrix: the slots added by index.
// The rows kernel reads every byte once; per value it spends one f64 log, one f64 exp and one f64 division, about 140 f64
// instructions per 4 bytes.  Measured at 3 x 12 x 1024 x 256 the call reaches a fifth to a third of HBM's rate, so
// the reads are not the limit; that the arithmetic is has been reasoned, not measured.
//
// rtts_align_mas, two kernels: the recurrence + back-track, one workgroup per (matrix, slot), and the totals kernel above.
//   The key front lies over the lanes: wave w owns keys [64 R w, 64 R (w + 1)), lane l the R keys 64 (R w + r) + l (R = 2 beyond
//   1024 keys).  Q[t, k] needs Q[t-1, k] (a register) and Q[t-1, k-1]: the neighbour lane's register by one DPP wave_shr:1 move
//   per word (rtts_wave_shr1 of score_common.h, the move of dtw.hip's recurrence); lane 0 takes lane 63's (r = 1: of the same
//   wave, a v_readlane) or, for r = 0, the last key of the wave before, which comes through an LDS ring.  The waves run SKEWED
//   like those of dtw.hip's recurrence: wave w works on frame chunk u - w in round u, so wave w - 1 wrote the ring rows of a
//   chunk one barrier before wave w reads them: ceil(T / 16) + waves - 1 barriers instead of T.
//   A frame's values of a are loaded 16 frames ahead, into the registers the frame just taken leaves free (16 R registers, no
//   second copy of a chunk), so the global latency is off the dependent chain.
//   The decision of a cell (1 = came from k - 1; a tie stays) is one bit: a wave's 64 decisions are one ballot, stored as one
//   64-bit word per (frame, 64 keys) -- in LDS when the whole (T_q, T_k) bit table fits, in the caller's workspace otherwise.
//   Cells right of the diagonal (k > t) come out as -inf by themselves (-inf + c), and the back-track from (T-1, K-1) never leaves
//   the feasible band, so nothing is predicated.  Wave 0 walks the bits back 64 frames at a time: lane j loads frame hi - j's two
//   words that can hold the path (k falls by at most 63 over 64 frames), the walk itself reads them by v_readlane -- no
//   dependent memory access per frame.  sum_t a[t, k(t)] is then added in frame order.
#include "score_common.h"

#define ALIGN_MAX_TQ 4096
#define ALIGN_MAX_TK 2048
#define ALIGN_MAX_MAT 64
#define ALIGN_TILE 16
#define ALIGN_ROW_WAVES 4
#define ALIGN_ROW_THREADS (64 * ALIGN_ROW_WAVES)
#define ALIGN_FOLD_THREADS 256
#define ALIGN_CHUNK 16
#define ALIGN_RING 64
#define ALIGN_MAS_MAX_WAVES 16
#define ALIGN_LDS_BUDGET (160 * 1024 - 1024)   // what one workgroup may take of the CU's 160 KB, static arrays included

static_assert(ALIGN_RING >= 2 * ALIGN_CHUNK + 1 && (ALIGN_RING & (ALIGN_RING - 1)) == 0,
              "the ring holds the chunk being read, its predecessor row and the chunk being written");
static_assert(ALIGN_MAX_TK <= 2 * 64 * ALIGN_MAS_MAX_WAVES, "two keys per lane cover the key envelope");

__device__ __forceinline__ double align_ninf() { return __longlong_as_double(0xfff0000000000000LL); }

struct AlignShape {
    int t, k;
    bool ok;
};

// the slot's bounds, by the same two reads in every workgroup of every kernel
__device__ __forceinline__ AlignShape align_shape(const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_keys, int b, int Tq, int Tk) {
    AlignShape s;
    s.t = n_frames[b];
    s.k = n_keys[b];
    s.ok = s.t >= 1 && s.t <= Tq && s.k >= 1 && s.k <= Tk;
    return s;
}

// ------------------------------------------------------------------------------------------------ statistics
__global__ __launch_bounds__(ALIGN_ROW_THREADS) void align_rows_kernel(const float* __restrict__ a, int64_t sm, int64_t sb, int64_t st, int B, int Tq,
                                                                       int Tk, const int32_t* __restrict__ n_frames,
                                                                       const int32_t* __restrict__ n_keys, double inv_two_sigma2,
                                                                       int32_t* __restrict__ argmax, double* __restrict__ part,
                                                                       int32_t* __restrict__ part_bad, int tiles) {
    __shared__ double rowv[ALIGN_TILE][4];
    __shared__ int rowbad[ALIGN_TILE];
    const int tile = blockIdx.x, b = blockIdx.y, m = blockIdx.z, tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const AlignShape s = align_shape(n_frames, n_keys, b, Tq, Tk);
    const int t0 = tile * ALIGN_TILE;
    int32_t* am = argmax + ((int64_t)m * B + b) * Tq;
    if (!s.ok || t0 >= s.t) {                                      // uniform over the workgroup: no frame of this tile is read
        if (tid < ALIGN_TILE && t0 + tid < Tq) am[t0 + tid] = -1;
        return;
    }
    const int T = s.t, K = s.k;
    const float* base = a + (int64_t)m * sm + (int64_t)b * sb;
    const double dK = (double)K, dT = (double)T;
    for (int r = w; r < ALIGN_TILE; r += ALIGN_ROW_WAVES) {
        const int t = t0 + r;
        if (t >= T) {                                              // uniform over the wave
            if (l == 0) {
                if (t < Tq) am[t] = -1;
                rowbad[r] = 0;
            }
            continue;
        }
        const float* row = base + (int64_t)t * st;
        const double tt = (double)t / dT;
        double sum = 0.0, ent = 0.0, gw = 0.0;
        float mx = __int_as_float(0xff800000);
        int mi = 0x7fffffff;
        bool bad = false;
        for (int c = 4 * l; c < K; c += 256) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            const int n = K - c < 4 ? K - c : 4;
            if (n == 4) {
                const float4 q = *reinterpret_cast<const float4*>(row + c);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (i < n) v[i] = row[c + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < n) {
                    const float x = v[i];
                    const double xd = (double)x;
                    bad |= !isfinite(x);
                    sum += xd;
                    if (x > mx) {
                        mx = x;
                        mi = c + i;
                    }
                    if (x > 0.f) ent -= xd * log(xd);
                    const double d = (double)(c + i) / dK - tt;
                    gw += xd * (1.0 - exp(-(d * d) * inv_two_sigma2));
                }
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            sum += __shfl_down(sum, off);
            ent += __shfl_down(ent, off);
            gw += __shfl_down(gw, off);
            const float ox = __shfl_xor(mx, off);
            const int oi = __shfl_xor(mi, off);
            if (ox > mx || (ox == mx && oi < mi)) {
                mx = ox;
                mi = oi;
            }
        }
        const bool any_bad = __any(bad);
        if (l == 0) {
            rowv[r][0] = sum;
            rowv[r][1] = (double)mx;
            rowv[r][2] = ent;
            rowv[r][3] = gw;
            rowbad[r] = any_bad ? 1 : 0;
            am[t] = any_bad ? -1 : mi;
        }
    }
    __syncthreads();
    if (tid < 4) {
        double acc = 0.0;
        for (int r = 0; r < ALIGN_TILE && t0 + r < T; ++r) acc += rowv[r][tid];      // frame order
        part[(((int64_t)m * B + b) * tiles + tile) * 4 + tid] = acc;
    } else if (tid == 64) {
        int f = 0;
        for (int r = 0; r < ALIGN_TILE; ++r) f |= rowbad[r];
        part_bad[((int64_t)m * B + b) * tiles + tile] = f;
    }
}

__global__ __launch_bounds__(ALIGN_FOLD_THREADS) void align_fold_kernel(int B, int Tq, int Tk, const int32_t* __restrict__ n_frames,
                                                                        const int32_t* __restrict__ n_keys, int32_t* __restrict__ argmax,
                                                                        int32_t* __restrict__ dur, const double* __restrict__ part,
                                                                        const int32_t* __restrict__ part_bad, int tiles,
                                                                        double* __restrict__ table) {
    __shared__ int hist[ALIGN_MAX_TK];
    __shared__ int counts[2];
    const int b = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
    const int64_t slot = (int64_t)m * B + b;
    const AlignShape s = align_shape(n_frames, n_keys, b, Tq, Tk);
    int32_t* am = argmax + slot * Tq;
    int32_t* du = dur + slot * Tk;
    double* row = table + ((int64_t)m * (B + 1) + b) * 8;
    int flagged = 0;
    if (s.ok)
        for (int i = tid; i < (s.t + ALIGN_TILE - 1) / ALIGN_TILE; i += ALIGN_FOLD_THREADS) flagged |= part_bad[slot * tiles + i];
    if (!s.ok || __syncthreads_or(flagged)) {                      // uniform over the workgroup
        for (int t = tid; t < Tq; t += ALIGN_FOLD_THREADS) am[t] = -1;
        for (int k = tid; k < Tk; k += ALIGN_FOLD_THREADS) du[k] = 0;
        if (tid < 8) row[tid] = rtts_nan64();
        return;
    }
    const int T = s.t, K = s.k;
    for (int k = tid; k < Tk; k += ALIGN_FOLD_THREADS) hist[k] = 0;
    if (tid < 2) counts[tid] = 0;
    __syncthreads();
    int mono = 0;
    for (int t = tid; t < T; t += ALIGN_FOLD_THREADS) {
        const int k = am[t];                                       // in [0, K): written by the rows kernel from a finite row
        atomicAdd(&hist[k], 1);                                    // integers: exact in any order
        if (t >= 1 && k >= am[t - 1]) ++mono;
    }
    __syncthreads();
    int cov = 0;
    for (int k = tid; k < Tk; k += ALIGN_FOLD_THREADS) {
        const int d = hist[k];
        du[k] = d;
        cov += d > 0;
    }
    atomicAdd(&counts[0], mono);
    atomicAdd(&counts[1], cov);
    __syncthreads();
    if (tid < 4) {
        double acc = 0.0;
        const double* p = part + slot * tiles * 4 + tid;
        const int n = (T + ALIGN_TILE - 1) / ALIGN_TILE;
        for (int i = 0; i < n; ++i) acc += p[(int64_t)i * 4];     // tile order
        row[2 + tid] = acc;
    } else if (tid == 4) {
        row[0] = (double)T;
        row[1] = (double)K;
        row[6] = (double)counts[0];
        row[7] = (double)counts[1];
    }
}

// row B of every matrix: the column sums over the slots, by index
__global__ void align_totals_kernel(double* __restrict__ table, int B, int cols) {
    const int m = blockIdx.x, c = threadIdx.x;
    if (c >= cols) return;
    double* tab = table + (int64_t)m * (B + 1) * cols;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc += tab[(int64_t)b * cols + c];
    tab[(int64_t)B * cols + c] = acc;
}

// ------------------------------------------------------------------------------------------------ monotonic alignment search
// the value of lane `lane` (uniform), in every lane
__device__ __forceinline__ double align_lane(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ uint64_t align_lane(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

struct AlignMasLds {
    int64_t bits, path, start, total;     // byte offsets into the dynamic LDS; bits < 0: the bit table lies in the workspace
    int words;                            // 64-bit words of one frame's decisions
};

static inline int align_mas_keys_per_lane(int Tk) { return Tk > 64 * ALIGN_MAS_MAX_WAVES ? 2 : 1; }
static inline int align_mas_waves(int Tk) {
    const int per = 64 * align_mas_keys_per_lane(Tk);
    return (Tk + per - 1) / per;
}
static inline AlignMasLds align_mas_lds(int Tq, int Tk) {
    AlignMasLds L;
    L.words = align_mas_keys_per_lane(Tk) * align_mas_waves(Tk);
    const int64_t fixed = (int64_t)ALIGN_MAS_MAX_WAVES * ALIGN_RING * 8 + 64;        // the static arrays of the kernel
    const int64_t bits = (int64_t)Tq * L.words * 8;
    const int64_t path = (int64_t)Tq * 4, start = ((int64_t)Tk + 1) * 4;
    const bool in_lds = fixed + bits + path + start + 16 <= ALIGN_LDS_BUDGET;
    L.bits = in_lds ? 0 : -1;
    L.path = in_lds ? bits : 0;
    L.start = L.path + path;
    L.total = (L.start + start + 15) & ~(int64_t)15;
    return L;
}

template <int R, bool BITS_IN_LDS>
__global__ __launch_bounds__(64 * ALIGN_MAS_MAX_WAVES) void align_mas_kernel(
    const float* __restrict__ a, int64_t sm, int64_t sb, int64_t st, int B, int Tq, int Tk, const int32_t* __restrict__ n_frames,
    const int32_t* __restrict__ n_keys, double floor_, int32_t* __restrict__ durations, int32_t* __restrict__ path_out,
    double* __restrict__ scores, uint64_t* __restrict__ ws_bits, int words, int64_t off_path, int64_t off_start) {
    extern __shared__ __attribute__((aligned(16))) unsigned char align_smem[];
    __shared__ double ring[ALIGN_MAS_MAX_WAVES][ALIGN_RING];
    __shared__ double q_final;
    const int b = blockIdx.x, m = blockIdx.y, tid = threadIdx.x, l = tid & 63, nthreads = blockDim.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t slot = (int64_t)m * B + b;
    const AlignShape s = align_shape(n_frames, n_keys, b, Tq, Tk);
    int32_t* du = durations + slot * Tk;
    int32_t* po = path_out ? path_out + slot * Tq : nullptr;
    double* sc = scores + ((int64_t)m * (B + 1) + b) * 2;
    auto wipe = [&]() {
        for (int k = tid; k < Tk; k += nthreads) du[k] = 0;
        if (po)
            for (int t = tid; t < Tq; t += nthreads) po[t] = -1;
        if (tid < 2) sc[tid] = rtts_nan64();
    };
    if (!s.ok || s.t < s.k) {                                      // uniform over the workgroup: nothing of the slot is read
        wipe();
        return;
    }
    const int T = s.t, K = s.k;
    uint64_t* bits = BITS_IN_LDS ? reinterpret_cast<uint64_t*>(align_smem) : ws_bits + slot * (int64_t)Tq * words;
    int* pathbuf = reinterpret_cast<int*>(align_smem + off_path);
    int* start = reinterpret_cast<int*>(align_smem + off_start);
    const float* base = a + (int64_t)m * sm + (int64_t)b * sb;
    const double ninf = align_ninf();
    for (int i = tid; i < ALIGN_MAS_MAX_WAVES * ALIGN_RING; i += nthreads) (&ring[0][0])[i] = ninf;
    __syncthreads();

    const int waves = (K + 64 * R - 1) / (64 * R);                 // waves that own a key below K
    const int chunks = (T + ALIGN_CHUNK - 1) / ALIGN_CHUNK;
    const int rounds = chunks + waves - 1;
    const bool active = w < waves, feeds = w + 1 < waves;
    int key[R];
    bool key_in[R];
    double q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        key[r] = 64 * (R * w + r) + l;
        key_in[r] = key[r] < K;
        q[r] = ninf;
    }
    float ahead[ALIGN_CHUNK][R];                                   // ahead[i]: the next frame = i (mod 16) this wave comes to
    bool bad = false;
    auto fetch = [&](int i, int t) {                               // the values of frame t at my keys
#pragma unroll
        for (int r = 0; r < R; ++r) ahead[i][r] = (t < T && key_in[r]) ? base[(int64_t)t * st + key[r]] : 1.f;
    };
    for (int u = 0; u < rounds; ++u) {
        const int cu = u - w;
        if (active && cu >= 0 && cu < chunks) {                    // uniform over the wave
            const int t0 = cu * ALIGN_CHUNK;
            if (cu == 0) {
#pragma unroll
                for (int i = 0; i < ALIGN_CHUNK; ++i) fetch(i, i);
            }
            // Q[t - 1, my first key - 1] of the chunk's frames: lane i reads the ring row of frame t0 + i - 1 once
            double edge_all = ninf;
            if (w > 0) edge_all = ring[w - 1][(t0 - 1 + (l & (ALIGN_CHUNK - 1))) & (ALIGN_RING - 1)];
#pragma unroll
            for (int i = 0; i < ALIGN_CHUNK; ++i) {
                const int t = t0 + i;
                if (t < T) {                                       // uniform
                    float x[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) x[r] = ahead[i][r];
                    fetch(i, t + ALIGN_CHUNK);                     // a chunk ahead: in flight while the 16 frames between compute
                    // Q[-1, -1] = 0 makes Q[0, 0] = c[0, 0] and leaves every other cell of frame 0 at -inf
                    const double edge = w > 0 ? align_lane(edge_all, i) : (t == 0 ? 0.0 : ninf);
                    double left[R];
                    left[0] = rtts_wave_shr1(edge, q[0]);
                    if (R == 2) left[R - 1] = rtts_wave_shr1(align_lane(q[0], 63), q[R - 1]);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        bad |= !isfinite(x[r]);
                        const double c = log(fmax((double)x[r], floor_));
                        const bool diag = left[r] > q[r];          // a tie stays
                        q[r] = c + (diag ? left[r] : q[r]);
                        const uint64_t mask = __ballot(diag);
                        if (l == 0) bits[(int64_t)t * words + R * w + r] = mask;
                    }
                    if (feeds && l == 63) ring[w][t & (ALIGN_RING - 1)] = q[R - 1];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (key[r] == K - 1) q_final = q[r];                       // one thread: Q[T - 1, K - 1]
    if (__syncthreads_or(bad ? 1 : 0)) {                           // a non-finite value in the region: every cell was read
        wipe();
        return;
    }
    // back-track, wave 0: k is uniform
    if (w == 0) {
        int k = K - 1;
        for (int hi = T - 1; hi >= 0; hi -= 64) {
            const int t = hi - l;
            const bool in = t >= 0;
            const int kw = k >> 6;
            const uint64_t wa = in ? bits[(int64_t)t * words + kw] : 0;
            const uint64_t wb = (in && kw > 0) ? bits[(int64_t)t * words + kw - 1] : 0;
            const int n = hi + 1 < 64 ? hi + 1 : 64;
            int myk = 0;
            for (int j = 0; j < n; ++j) {
                const uint64_t word = (k >> 6) == kw ? align_lane(wa, j) : align_lane(wb, j);
                if (l == j) myk = k;
                if (hi - j > 0) {
                    k -= (int)((word >> (k & 63)) & 1);
                    k = k < 0 ? 0 : k;
                }
            }
            if (in) pathbuf[t] = myk;
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += nthreads) {
        const int k = pathbuf[t];
        if (t == 0 || pathbuf[t - 1] != k) start[k] = t;           // the path visits every key below K, in order
    }
    if (tid == 0) start[K] = T;
    if (po)
        for (int t = tid; t < Tq; t += nthreads) po[t] = t < T ? pathbuf[t] : -1;
    __syncthreads();
    for (int k = tid; k < Tk; k += nthreads) du[k] = k < K ? start[k + 1] - start[k] : 0;
    if (w == 0) {                                                  // sum_t a[t, k(t)], frame order
        double mass = 0.0;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + l;
            const float v = t < T ? base[(int64_t)t * st + pathbuf[t]] : 0.f;
            const int n = T - t0 < 64 ? T - t0 : 64;
            for (int j = 0; j < n; ++j) mass += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
        }
        if (l == 0) {
            sc[0] = q_final;
            sc[1] = mass;
        }
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static inline bool align_envelope(int n_mat, int B, int Tq, int Tk) {
    return n_mat >= 1 && n_mat <= ALIGN_MAX_MAT && B >= 1 && B <= 65535 && Tq >= 1 && Tq <= ALIGN_MAX_TQ && Tk >= 1 && Tk <= ALIGN_MAX_TK;
}
static inline int align_tiles(int Tq) { return (Tq + ALIGN_TILE - 1) / ALIGN_TILE; }

static int align_check_operand(const char* who, const float* a, int64_t sm, int64_t sb, int64_t st, int n_mat, int B, int Tq, int Tk,
                               const int32_t* n_frames, const int32_t* n_keys) {
    RTTS_REQUIRE(a, "%s: a is a null pointer", who);
    RTTS_REQUIRE(n_frames, "%s: n_frames is a null pointer", who);
    RTTS_REQUIRE(n_keys, "%s: n_keys is a null pointer", who);
    RTTS_REQUIRE(n_mat >= 1 && n_mat <= ALIGN_MAX_MAT, "%s: n_mat must be in 1..%d (got %d)", who, ALIGN_MAX_MAT, n_mat);
    RTTS_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in 1..65535 (got %d)", who, B);
    RTTS_REQUIRE(Tq >= 1 && Tq <= ALIGN_MAX_TQ, "%s: Tq must be in 1..%d (got %d)", who, ALIGN_MAX_TQ, Tq);
    RTTS_REQUIRE(Tk >= 1 && Tk <= ALIGN_MAX_TK, "%s: Tk must be in 1..%d (got %d)", who, ALIGN_MAX_TK, Tk);
    RTTS_REQUIRE(((uintptr_t)a & 15) == 0, "%s: a must be 16-byte aligned (the base pointer is %p)", who, (const void*)a);
    RTTS_REQUIRE(st >= Tk && st % 4 == 0, "%s: the stride st = %lld must be a multiple of 4 and at least Tk = %d", who, (long long)st, Tk);
    RTTS_REQUIRE(sb >= 0 && sb % 4 == 0, "%s: the stride sb = %lld must be a non-negative multiple of 4", who, (long long)sb);
    RTTS_REQUIRE(sm >= 0 && sm % 4 == 0, "%s: the stride sm = %lld must be a non-negative multiple of 4", who, (long long)sm);
    // a slot spans Tq st elements; the slots of a matrix lie inside one step of sm (L, B, ..) or the other way round (B, L, ..)
    const int64_t span = (int64_t)Tq * st, all_b = (int64_t)(B - 1) * sb + span, all_m = (int64_t)(n_mat - 1) * sm + span;
    const bool mat_outer = (B == 1 || sb >= span) && (n_mat == 1 || sm >= all_b);
    const bool slot_outer = (n_mat == 1 || sm >= span) && (B == 1 || sb >= all_m);
    RTTS_REQUIRE(mat_outer || slot_outer,
                 "%s: the strides sm = %lld and sb = %lld make slots overlap: a slot spans Tq st = %lld elements, so either sb >= Tq st and "
                 "sm >= (B - 1) sb + Tq st, or sm >= Tq st and sb >= (n_mat - 1) sm + Tq st",
                 who, (long long)sm, (long long)sb, (long long)span);
    return 0;
}

extern "C" int64_t rtts_align_stats_workspace(int n_mat, int B, int Tq, int Tk) {
    if (!align_envelope(n_mat, B, Tq, Tk)) return -1;
    const int64_t slots = (int64_t)n_mat * B * align_tiles(Tq);
    return rtts_align256(slots * 4 * 8) + rtts_align256(slots * 4);
}

extern "C" int rtts_align_stats(const float* a, int64_t sm, int64_t sb, int64_t st, int n_mat, int B, int Tq, int Tk, const int32_t* n_frames,
                                const int32_t* n_keys, double sigma, int32_t* argmax, int32_t* dur_argmax, double* table, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    if (align_check_operand("rtts_align_stats", a, sm, sb, st, n_mat, B, Tq, Tk, n_frames, n_keys)) return -1;
    RTTS_REQUIRE(argmax, "rtts_align_stats: argmax is a null pointer");
    RTTS_REQUIRE(dur_argmax, "rtts_align_stats: dur_argmax is a null pointer");
    RTTS_REQUIRE(table, "rtts_align_stats: table is a null pointer");
    RTTS_REQUIRE(workspace, "rtts_align_stats: workspace is a null pointer");
    RTTS_REQUIRE(sigma > 0.0 && sigma <= 1.7e308, "rtts_align_stats: sigma must be positive and finite (got %g)", sigma);
    const int64_t need = rtts_align_stats_workspace(n_mat, B, Tq, Tk);
    RTTS_REQUIRE(workspace_bytes >= need, "rtts_align_stats: workspace_bytes = %lld is smaller than rtts_align_stats_workspace = %lld",
                 (long long)workspace_bytes, (long long)need);
    const int tiles = align_tiles(Tq);
    double* part = (double*)workspace;
    int32_t* part_bad = (int32_t*)((char*)workspace + rtts_align256((int64_t)n_mat * B * tiles * 4 * 8));
    RTTS_ENTER(stream);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(align_rows_kernel, dim3((unsigned)tiles, (unsigned)B, (unsigned)n_mat), dim3(ALIGN_ROW_THREADS), 0, s, a, sm, sb, st, B, Tq,
                       Tk, n_frames, n_keys, 1.0 / (2.0 * sigma * sigma), argmax, part, part_bad, tiles);
    RTTS_LAUNCH_CHECK("rtts_align_stats (rows)");
    hipLaunchKernelGGL(align_fold_kernel, dim3((unsigned)B, (unsigned)n_mat), dim3(ALIGN_FOLD_THREADS), 0, s, B, Tq, Tk, n_frames, n_keys, argmax,
                       dur_argmax, part, part_bad, tiles, table);
    RTTS_LAUNCH_CHECK("rtts_align_stats (fold)");
    hipLaunchKernelGGL(align_totals_kernel, dim3((unsigned)n_mat), dim3(64), 0, s, table, B, 8);
    RTTS_LAUNCH_CHECK("rtts_align_stats (totals)");
    return 0;
}

extern "C" int64_t rtts_align_mas_workspace(int n_mat, int B, int Tq, int Tk) {
    if (!align_envelope(n_mat, B, Tq, Tk)) return -1;
    const AlignMasLds L = align_mas_lds(Tq, Tk);
    return L.bits >= 0 ? 256 : rtts_align256((int64_t)n_mat * B * Tq * L.words * 8);
}

static RttsLdsState g_align_lds[2][2];

extern "C" int rtts_align_mas(const float* a, int64_t sm, int64_t sb, int64_t st, int n_mat, int B, int Tq, int Tk, const int32_t* n_frames,
                              const int32_t* n_keys, double floor, int32_t* durations, int32_t* path, double* scores, void* workspace,
                              int64_t workspace_bytes, void* stream) {
    if (align_check_operand("rtts_align_mas", a, sm, sb, st, n_mat, B, Tq, Tk, n_frames, n_keys)) return -1;
    RTTS_REQUIRE(durations, "rtts_align_mas: durations is a null pointer");
    RTTS_REQUIRE(scores, "rtts_align_mas: scores is a null pointer");
    RTTS_REQUIRE(workspace, "rtts_align_mas: workspace is a null pointer");
    RTTS_REQUIRE(floor > 0.0 && floor <= 1.7e308, "rtts_align_mas: floor must be positive and finite (got %g)", floor);
    const int64_t need = rtts_align_mas_workspace(n_mat, B, Tq, Tk);
    RTTS_REQUIRE(workspace_bytes >= need, "rtts_align_mas: workspace_bytes = %lld is smaller than rtts_align_mas_workspace = %lld",
                 (long long)workspace_bytes, (long long)need);
    const AlignMasLds L = align_mas_lds(Tq, Tk);
    const int rk = align_mas_keys_per_lane(Tk), threads = 64 * align_mas_waves(Tk);
    const bool in_lds = L.bits >= 0;
    RTTS_ENTER(stream);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)B, (unsigned)n_mat);
#define ALIGN_MAS_LAUNCH(R_, LDS_)                                                                                                       \
    do {                                                                                                                                 \
        RTTS_ENSURE_LDS("rtts_align_mas", (align_mas_kernel<R_, LDS_>), (size_t)L.total, g_align_lds[R_ - 1][LDS_ ? 1 : 0]);             \
        hipLaunchKernelGGL((align_mas_kernel<R_, LDS_>), grid, dim3((unsigned)threads), (size_t)L.total, s, a, sm, sb, st, B, Tq, Tk,    \
                           n_frames, n_keys, floor, durations, path, scores, (uint64_t*)workspace, L.words, L.path, L.start);            \
    } while (0)
    if (rk == 1 && in_lds) ALIGN_MAS_LAUNCH(1, true);
    else if (rk == 1) ALIGN_MAS_LAUNCH(1, false);
    else if (in_lds) ALIGN_MAS_LAUNCH(2, true);
    else ALIGN_MAS_LAUNCH(2, false);
#undef ALIGN_MAS_LAUNCH
    RTTS_LAUNCH_CHECK("rtts_align_mas (recurrence)");
    hipLaunchKernelGGL(align_totals_kernel, dim3((unsigned)n_mat), dim3(64), 0, s, scores, B, 2);
    RTTS_LAUNCH_CHECK("rtts_align_mas (totals)");
    return 0;
}
